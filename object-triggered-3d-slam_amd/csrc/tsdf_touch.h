// tsdf_touch.h — device text of the TSDF batch touch: the stride samples of a batch's frames, merged per workgroup in
// LDS, set their units' frame-mask bits and list the batch's units.  One text (touch_body) behind k_batch_touch and
// k_batch_touch_split (tsdf_frontend.hip) and the touch half of k_integrate_touch (tsdf_fused.hip).
#pragma once

#include "tsdf_stage.h"

namespace ot {

// floor(RN(a / b)) -- Open3D's LocateVolumeUnit on a float64 quotient -- with one multiply in the common case: v =
// RN(a * RN(1/b)) is within 2^-52 |a/b| of a/b (and RN(a/b) within 2^-53), so when v lies farther than 1e-14 |v| (+ an
// absolute floor far below any unit index) from every integer, floor(v) is floor(RN(a/b)); otherwise the IEEE division.
__device__ inline int floor_div(double a, double b, double inv_b) {
    const double v = a * inv_b;
    const double fv = floor(v);
    const double eps = 1e-14 * fabs(v) + 1e-300;
    if (v - fv > eps && (fv + 1.0) - v > eps) return (int)fv;
    return (int)floor(a / b);
}

// Bits `bits` of the mask word of frame f of `slot`; true: this call lists the slot in bslots (the batch's first touch
// of the unit).  WIDE: the batch has frames in both words, and the first touch of a word draws the slot's claim
// (tsdf.h).  !WIDE (a batch of at most WORD_FRAMES frames: every sharded, split, fused and deferred batch): word 0 alone
// and no claim, the single atomicOr a one-word mask takes.
template <bool WIDE>
__device__ inline bool touch_slot(const TsdfDev& d, int slot, int f, unsigned long long bits) {
    if constexpr (WIDE) {
        if (atomicOr(&d.fmask[(unsigned)slot * FMASK_STRIDE + (f >> 6)], bits) != 0ull) return false;
        return atomicExch(&d.fmask[(unsigned)slot * FMASK_STRIDE + FMASK_CLAIM], 1ull) == 0ull;
    } else {
        return atomicOr(&d.fmask[(unsigned)slot * FMASK_STRIDE], bits) == 0ull;
    }
}

template <bool WIDE>
__device__ inline void touch_unit_batch(const TsdfDev& d, int f, int slot_cap, int pc, int x, int y, int z) {
    if (!key_in_range(x, y, z)) {
        atomicOr(&d.counters[C_HASHERR], 2);
        return;
    }
    const unsigned long long key = pack_key(x, y, z);
    if (!unit_owned(d, key)) return;
    const int slot = hash_insert(d, key);
    if (slot < 0) {
        atomicOr(&d.counters[C_HASHERR], 1);
        return;
    }
    const unsigned long long bit = 1ull << (WIDE ? f & 63 : f);
    // fast path; a stale read only costs the atomic below
    if (d.fmask[(unsigned)slot * FMASK_STRIDE + (WIDE ? f >> 6 : 0)] & bit) return;
    if (touch_slot<WIDE>(d, slot, f, bit)) {
        const int pos = atomicAdd(&d.counters[pc], 1);
        if (pos < slot_cap) d.bslots[pos] = slot;
        else atomicOr(&d.counters[C_HASHERR], 1);
    }
}

// Touch pass with LDS de-duplication.  A workgroup owns a 16x16 tile of stride samples and a group of TF frames;
// each (unit key, frame) hit is first merged into an LDS table (key -> frame bitmask, 64-bit LDS atomics), then
// every distinct unit of the tile does ONE global hash insert + ONE atomicOr of its merged mask.  A key that does
// not fit the LDS table falls back to the direct global path.
constexpr int TT = 16;          // tile edge in samples
// frames per workgroup: 2 since the staging-only workgroups (r05au / r05av, tools/touch_stage_ab.py: unsharded step
// within 0.2 % of 4, a rank of 8 shards 3 % faster -- front end 99 vs 105 us per batch; 8: +10 %); with every touch
// workgroup staging a share first, 4 was 1 % faster than 2 (round 3)
constexpr int TF = 2;
constexpr int LTAB = 1024;   // LDS table entries (16 B each + a 4-B slot in the list of used entries)

// Frame groups: group g is frames g tf ... g tf + tf - 1.  A group's frames lie in one mask word, so a touch workgroup's
// LDS masks stay 64-bit and it merges them with one atomicOr: a batch of more than WORD_FRAMES frames takes a group size
// that divides WORD_FRAMES (touch_group_frames, on the host; TF = 2 does).
inline int touch_group_frames(int tf, int n) {
    while (n > WORD_FRAMES && WORD_FRAMES % tf) --tf;
    return tf;
}

__device__ inline bool lds_merge(unsigned long long* keys, unsigned long long* masks, unsigned short* used, int* nused,
                                 unsigned long long key, unsigned long long bit) {
    unsigned h = (unsigned)mix64(key) & (LTAB - 1);
    for (int probe = 0; probe < 64; ++probe) {
        unsigned long long k = keys[h];
        if (k == KEY_EMPTY) {
            const unsigned long long old = atomicCAS(&keys[h], KEY_EMPTY, key);
            if (old == KEY_EMPTY) used[atomicAdd(nused, 1)] = (unsigned short)h;  // the inserting lane lists the entry
            k = (old == KEY_EMPTY) ? key : old;
        }
        if (k == key) {
            atomicOr(&masks[h], bit);
            return true;
        }
        h = (h + 1) & (LTAB - 1);
    }
    return false;
}

// Staging (every pixel of the batch: HBM streaming) and the touch (stride samples: LDS merges and global hash atomics)
// as separate workgroups: stage_blocks > 0 staging-only workgroups follow each frame group's touch tiles in the grid
// (blockIdx.x >= tiles), so the touches' global atomics are spread over the time the staging streams.  Measured
// (tools/touch_stage_ab.py, front end per 64-frame batch): every touch workgroup staging a share first (stage_blocks 0,
// the round-4 form) 115 us, 1 / 2 / 4 / 8 staging workgroups per tile 120 / 111 / 112 / 122 us (r05aq, r05ar: step
// -1.2 % at 2); all touch workgroups dispatched first and the staging after them 123-128 us (r05as: the touches'
// atomics then contend at once).  The touch reads raw depth itself, so nothing in it waits on the staging stores.
// Every rank of a spatially sharded volume stages every pixel: integrating from the raw frames instead (a u16 depth +
// a multiplier-table gather per voxel visit) made the integrate 1.9x slower per unit (round 4,
// tools/shard_frontend.py), more than the staging it saves.
// REPLAY (settle_batch, after the pool grew): the batch's touch again from its STAGED depths (the caller's frames may be
// gone by then; the staged depth is exactly the value the first pass computed from them), no staging.
// LDS of one touch workgroup (k_batch_touch, and the touch half of k_integrate_touch)
struct TouchLds {
    unsigned long long keys[LTAB];
    unsigned long long masks[LTAB];
    unsigned short used[LTAB];  // 16-bit entry indices: 18 KiB in all, so 8 workgroups fit a CU's 160 KiB
    int nused;
};
// STAGE: the staging code paths (stage_blocks >= 0) are compiled in; the split front end's touch has none (the touch half
// of k_integrate_touch: without them it fits 64 VGPRs instead of 96)
// WIDE: the batch may have more than WORD_FRAMES frames (touch_slot); the host launches that form for such a batch only
template <bool REPLAY, bool STAGE = !REPLAY, bool WIDE = false>
__device__ __forceinline__ void touch_body(const BatchFrame* __restrict__ frames, const BatchTouchParams& p,
                                           const TsdfDev& d, int nframes, TouchLds& L, int tile, int grp) {
    unsigned long long* s_keys = L.keys;
    unsigned long long* s_masks = L.masks;
    unsigned short* s_used = L.used;
    int& s_nused = L.nused;
    const int tid = threadIdx.x;
    if constexpr (STAGE) {
        if (p.stage_blocks > 0 && tile >= p.tiles) {  // block-uniform
            stage_share(frames, p, nframes, grp, tile - p.tiles, p.stage_blocks);
            return;
        }
    }
    for (int e = tid; e < LTAB; e += 256) {
        s_keys[e] = KEY_EMPTY;
        s_masks[e] = 0ull;
    }
    if (tid == 0) s_nused = 0;
    // (stage_blocks 0) this touch workgroup also stages a contiguous 1/tiles of its frames' pixels
    if constexpr (STAGE) {
        if (p.stage_blocks == 0) stage_share(frames, p, nframes, grp, tile, p.tiles);
    }
    __syncthreads();
    const int tiles_x = (p.ws + TT - 1) / TT;
    const int sx = (tile % tiles_x) * TT + (tid & (TT - 1));
    const int sy = (tile / tiles_x) * TT + (tid / TT);
    const int f0 = grp * p.tf;  // (the group's frames share a mask word: touch_group_frames)
    if (sx < p.ws && sy < p.hs) {
        const int r = sy * p.stride, c = sx * p.stride;
        for (int f = f0; f < f0 + p.tf && f < nframes; ++f) {
            const BatchFrame& fr = frames[f];
            const int64_t pix = (int64_t)r * p.W + c;  // the staged depth, computed as the staging does
            const float df = REPLAY           ? __uint_as_float(fr.dc[pix].x)
                             : fr.depth16 ? prep_depth(fr, fr.depth16[pix])
                                          : fr.depthf[pix];
            if constexpr (!REPLAY) {
                if (p.sample_stage) {  // what the staging writes there
                    uint32_t cw = 0u;
                    if (fr.color) {
                        const uint8_t* c = fr.color + pix * 3;
                        cw = (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16);
                    }
                    fr.dc[pix] = make_uint2(__float_as_uint(df), cw);
                }
            }
            if (!(df > 0.0f)) continue;
            const double z = (double)df;
            const double x = ((double)c - p.cx) * z / p.fx;
            const double y = ((double)r - p.cy) * z / p.fy;
            double q[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double a = fr.pose[k * 4 + 0] * x;
                const double b = fr.pose[k * 4 + 1] * y;
                const double cc = fr.pose[k * 4 + 2] * z;
                q[k] = ((a + b) + cc) + fr.pose[k * 4 + 3];
            }
            int lo[3], hi[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                lo[k] = floor_div(q[k] - p.trunc, p.unit_len, p.inv_unit);
                hi[k] = floor_div(q[k] + p.trunc, p.unit_len, p.inv_unit);
            }
            const unsigned long long bit = 1ull << (WIDE ? f & 63 : f);
            for (int ux = lo[0]; ux <= hi[0]; ++ux)
                for (int uy = lo[1]; uy <= hi[1]; ++uy)
                    for (int uz = lo[2]; uz <= hi[2]; ++uz) {
                        if (!key_in_range(ux, uy, uz)) {
                            atomicOr(&d.counters[C_HASHERR], 2);
                            continue;
                        }
                        const unsigned long long key = pack_key(ux, uy, uz);
                        if (!unit_owned(d, key)) continue;
                        if (!lds_merge(s_keys, s_masks, s_used, &s_nused, key, bit))
                            touch_unit_batch<WIDE>(d, f, p.slot_cap, p.pc, ux, uy, uz);
                    }
        }
    }
    __syncthreads();
    // only the entries this tile filled (listed by their inserting lanes), not the whole table
    // The slots this batch touches first get a place in its list through ONE counter atomic per wave (ballot, the
    // first such lane adds the wave's count, each lane takes its rank): a batch's thousands of first touches on one
    // counter word no longer serialise in L2 one lane at a time
    const int nused = s_nused;
    for (int t0 = 0; t0 < nused; t0 += 256) {  // block-uniform trip count: every lane reaches the ballot
        const int t = t0 + tid;
        bool fresh = false;
        int slot = -1;
        if (t < nused) {
            const int e = s_used[t];
            slot = hash_insert(d, s_keys[e]);
            if (slot < 0) {
                atomicOr(&d.counters[C_HASHERR], 1);
            } else {
                // no read of the mask first: another frame group's workgroup set the unit's other bits, so the
                // bits are almost never all present, and the read was one more dependent global round trip on
                // every tile's chain (front end 112 -> 104 us per 64-frame batch, r05ax)
                fresh = touch_slot<WIDE>(d, slot, f0, s_masks[e]);
            }
        }
        int cnt;
        const int rank = wave_excl_count(fresh, cnt);
        if (cnt) {  // wave-uniform
            const int leader = __ffsll((long long)__ballot(fresh)) - 1;
            int base = 0;
            if ((int)lane_id() == leader) base = atomicAdd(&d.counters[p.pc], cnt);
            base = __builtin_amdgcn_readlane(base, leader);
            if (fresh) {
                const int pos = base + rank;
                if (pos < p.slot_cap) d.bslots[pos] = slot;
                else atomicOr(&d.counters[C_HASHERR], 1);
            }
        }
    }
}

}  // namespace ot
