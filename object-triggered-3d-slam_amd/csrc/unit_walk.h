// unit_walk.h — per-unit helpers shared by the volume readers that run one workgroup per unit in key order
// (mc.hip marching cubes, tsdf_cloud.hip point clouds): the block-hash lookup, the workgroup scan and the
// two-array scan of the per-unit counts that mails its totals to the volume's pinned mailbox.
#pragma once

#include "compact.h"
#include "tsdf.h"

namespace ot {

__device__ inline int find_unit(const TsdfDev& d, int x, int y, int z) {
    if (!key_in_range(x, y, z)) return -1;
    const unsigned long long key = pack_key(x, y, z);
    unsigned slot = (unsigned)mix64(key) & (unsigned)d.hash_mask;
    for (int probe = 0; probe <= d.hash_mask; ++probe) {
        const unsigned long long k = d.hkeys[slot];
        if (k == key) {
            const int id = d.hvals[slot];
            return id < d.max_units ? id : -1;
        }
        if (k == KEY_EMPTY) return -1;
        slot = (slot + 1) & (unsigned)d.hash_mask;
    }
    return -1;
}

// exclusive scan over an NT-thread workgroup (every thread of the workgroup must call it: two barriers)
template <int NT>
__device__ inline int block_excl_scan_n(int v, int& total) {
    __shared__ int wsum[NT / 64];
    const int lane = (int)lane_id(), wid = threadIdx.x >> 6;
    const int inc = wave_incl_scan(v);
    if (lane == 63) wsum[wid] = inc;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) {
        const int s = wsum[w];
        if (w < wid) off += s;
        tot += s;
    }
    __syncthreads();
    total = tot;
    return off + inc - v;
}

// the extraction's two exclusive scans (triangle and vertex counts per unit, U of each) in one launch: block 0 scans
// the triangle counts, block 1 the vertex counts, 4096 per round (4 consecutive per thread) with a carried total --
// one ~5 us launch instead of a library scan's two launches per array (U is a few thousand units).  Each block mails
// its array's total (triangles, vertices) to the volume's pinned mailbox, then `seq` to its sequence word (seqw[block]):
// the host spins on those (mail_wait), with no launch or event of its own
static __global__ __launch_bounds__(1024) void k_mc_scan2(const long long* __restrict__ c0, long long* __restrict__ b0,
                                                  const long long* __restrict__ c1, long long* __restrict__ b1,
                                                  int n, long long* __restrict__ totals, unsigned* __restrict__ seqw,
                                                  unsigned seq) {
    const long long* in = blockIdx.x ? c1 : c0;
    long long* out = blockIdx.x ? b1 : b0;
    __shared__ long long wsum[16];
    __shared__ long long s_carry;
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    if (t == 0) s_carry = 0;
    __syncthreads();
    for (int base = 0; base < n; base += 4096) {
        const int i0 = base + 4 * t;
        long long v[4], loc = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[k] = i0 + k < n ? in[i0 + k] : 0;
            loc += v[k];
        }
        long long inc = loc;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const long long o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        long long off = s_carry, tot = 0;
        for (int q = 0; q < 16; ++q) {
            off += q < w ? wsum[q] : 0;
            tot += wsum[q];
        }
        long long run = off + inc - loc;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (i0 + k < n) out[i0 + k] = run;
            run += v[k];
        }
        __syncthreads();
        if (t == 0) s_carry += tot;
        __syncthreads();
    }
    if (t == 0) {
        totals[blockIdx.x] = s_carry;
        __threadfence_system();  // the total reaches the host before the sequence word
        __hip_atomic_store(seqw + blockIdx.x, seq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace ot
