// cluster.hip — PointCloud::ClusterDBSCAN on MI355X ("DBSCAN").
//
// Open3D's sequential loop (index order, a work set per cluster) has a closed form that does not depend on any
// visiting order, and that is what runs here:
//   core[i]  = |{j : d2(i, j) < eps^2}| >= min_points (i itself counts);
//   clusters = the connected components of the core points under d2 < eps^2, numbered 0 .. C-1 by ascending smallest
//              point index among their core members;
//   a non-core point takes the smallest label among the core points within eps of it, -1 when there is none.
// d2 is d2_l2 (grid.h): ((dx dx) + dy dy) + dz dz in float64, no contraction -- ROR's test.
//
// The neighbourhood is ROR's: the grid of cell eps * ROR_CELL_SCALE, one lane per point in sorted (cell) order, the 9
// merged column ranges of its cell's 3x3x3 block.  Launches (all indices below are sorted positions unless said):
//   k_db_core    : neighbour count, stopped at min_points -> core[j]; parent[j] = j, minidx[j] = INT_MAX
//   k_db_hook    : each core j unites itself with its core neighbours k < j.  Union-find, the larger root hooked under
//                  the smaller by compare-and-swap, so parent[x] <= x always, every find is a walk of at most x steps
//                  whatever other lanes do, and a failed compare-and-swap means another lane's hook succeeded.  No lane
//                  waits for another.  The root of a finished component is its smallest sorted position whatever the
//                  interleaving.  Every access to parent[] inside this launch is a relaxed agent-scope atomic (other
//                  workgroups, on other XCDs, write it).
//   k_db_flatten : comp[j] = root of j (nothing writes parent[] any more); minidx[root] = min over the component's core
//                  members of their point index (atomicMin, folded through the wave first: one per wave and root)
//   k_db_flag    : each root flags point minidx[root] in an input-order byte array
//   compact      : the exclusive scan of the flags = the cluster number of each flagged point, and C
//   k_db_corelabel : core j: label = rank[minidx[comp[j]]], kept per sorted position and scattered to input order
//   k_db_border  : non-core j: the smallest label among its core neighbours, else -1, scattered to input order
#include <climits>
#include <cmath>

#include "compact.h"
#include "grid.h"
#include "union_find.h"

namespace ot {

// one lane's walk over the candidates of sorted point j: f(k) for every k in the 9 ranges, until it returns false
template <class F>
__device__ inline void for_block_candidates(const GridDev& g, int64_t j, F f) {
    const int2* rg = g.nbr3 + (int64_t)g.pcell[j] * NBR3;
    for (int t = 0; t < NBR3; ++t) {
        const int2 se = rg[t];
        for (int k = se.x; k < se.y; ++k)
            if (!f(k)) return;
    }
}

__global__ __launch_bounds__(256) void k_db_core(GridDev g, int64_t n, double r2, int min_points,
                                                 unsigned char* __restrict__ core, int* __restrict__ parent,
                                                 int* __restrict__ minidx) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const double q[3] = {g.sxyz[j * 3], g.sxyz[j * 3 + 1], g.sxyz[j * 3 + 2]};
    int cnt = 0;
    if (min_points > 0)
        for_block_candidates(g, j, [&](int k) {
            cnt += d2_l2(q, g.sxyz + (int64_t)k * 3) < r2 ? 1 : 0;
            return cnt < min_points;
        });
    core[j] = cnt >= min_points ? 1 : 0;
    parent[j] = (int)j;
    minidx[j] = INT_MAX;
}

// (uf_load / uf_find / uf_union: union_find.h)
__global__ __launch_bounds__(256) void k_db_hook(GridDev g, int64_t n, double r2,
                                                 const unsigned char* __restrict__ core, int* parent) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n || !core[j]) return;
    const double q[3] = {g.sxyz[j * 3], g.sxyz[j * 3 + 1], g.sxyz[j * 3 + 2]};
    int rj = (int)j;  // an ancestor of j: finds for j start here
    for_block_candidates(g, j, [&](int k) {
        // each edge once, from its larger end (the ranges ascend, but the 9 of them are not in order: no early exit)
        if (k < (int)j && core[k] && d2_l2(q, g.sxyz + (int64_t)k * 3) < r2) rj = uf_union(parent, rj, k);
        return true;
    });
    // shorten j's own path for the lanes that reach it later: rj is an ancestor of j, and of two ancestors the
    // smaller is the nearer to the root, so the minimum is always a valid parent
    if (rj < (int)j) __hip_atomic_fetch_min(parent + j, rj, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ inline int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o, 64));
    return v;
}

__global__ __launch_bounds__(256) void k_db_flatten(int64_t n, const unsigned char* __restrict__ core, int* parent,
                                                    const unsigned* __restrict__ sidx, int* __restrict__ comp,
                                                    int* minidx) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool active = j < n && core[j];
    int r = -1, v = INT_MAX;
    if (active) {
        r = uf_find(parent, (int)j);
        comp[j] = r;
        v = (int)sidx[j];
    }
    // one atomic per (wave, root), not per point: the lanes that share the first pending lane's root fold their
    // indices through the wave first (a cloud that is one component sent every point's atomic to one address: 1.1 ms
    // of a 2.0 ms call at 100 000 points).  At most 64 rounds; the whole wave takes part in every round.
    unsigned long long todo = __ballot(active);
    while (todo) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lr = __shfl(r, leader);
        const bool mine = active && r == lr;
        const int m = wave_min_i(mine ? v : INT_MAX);
        if ((int)lane_id() == leader)
            __hip_atomic_fetch_min(minidx + lr, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        todo &= ~__ballot(mine);
    }
}

__global__ __launch_bounds__(256) void k_db_flag(int64_t n, const unsigned char* __restrict__ core,
                                                 const int* __restrict__ comp, const int* __restrict__ minidx,
                                                 unsigned char* __restrict__ flag) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n || !core[j] || comp[j] != (int)j) return;
    flag[minidx[j]] = 1;
}

struct FlagPred {
    const unsigned char* flag;
    __device__ bool operator()(int64_t i) const { return flag[i] != 0; }
};
struct RankEmit {
    int* rank;
    __device__ void operator()(int64_t i, int64_t pos) const { rank[i] = (int)pos; }
};

__global__ __launch_bounds__(256) void k_db_corelabel(int64_t n, const unsigned char* __restrict__ core,
                                                      const int* __restrict__ comp, const int* __restrict__ minidx,
                                                      const int* __restrict__ rank, const unsigned* __restrict__ sidx,
                                                      int* __restrict__ clabel, int32_t* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n || !core[j]) return;
    const int l = rank[minidx[comp[j]]];
    clabel[j] = l;
    out[sidx[j]] = l;
}

__global__ __launch_bounds__(256) void k_db_border(GridDev g, int64_t n, double r2,
                                                   const unsigned char* __restrict__ core,
                                                   const int* __restrict__ clabel, int32_t* __restrict__ out) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n || core[j]) return;
    const double q[3] = {g.sxyz[j * 3], g.sxyz[j * 3 + 1], g.sxyz[j * 3 + 2]};
    int best = INT_MAX;
    for_block_candidates(g, j, [&](int k) {
        if (core[k] && d2_l2(q, g.sxyz + (int64_t)k * 3) < r2) best = min(best, clabel[k]);
        return true;
    });
    out[g.sidx[j]] = best == INT_MAX ? -1 : best;
}

}  // namespace ot

using namespace ot;

extern "C" {

ot_status ot_cluster_dbscan(const double* xyz, int64_t n, double eps, int32_t min_points, int32_t* out_labels,
                            int32_t* n_clusters_host, void* stream_) {
    hipStream_t stream = S(stream_);
    if (!(eps > 0) || !std::isfinite(eps) || min_points < 0)
        return fail(OT_ERR_INVALID_ARGUMENT, "[ClusterDBSCAN] Illegal input parameters, eps must be positive and "
                                             "finite and min_points must not be negative");
    if (n_clusters_host) *n_clusters_host = 0;
    if (n <= 0) return OT_OK;
    if (!xyz || !out_labels || n > 0x7FFFFFFF) return fail(OT_ERR_INVALID_ARGUMENT, "[ClusterDBSCAN] invalid buffers");
    double mn[3], mx[3];
    ot_status st = bounds_host(xyz, n, stream, mn, mx);
    if (st != OT_OK) return st;
    GridBuild gb;
    st = single_frame_grid(xyz, n, eps * ROR_CELL_SCALE, mn, mx, GRID_NBR3, stream, gb);
    if (st != OT_OK) return st;
    const size_t un = (size_t)n;
    auto [parent, comp, minidx, rank, clabel, core, flag] =
        carve(scratch_of(Slot::OP_WS), Arr<int>{un}, Arr<int>{un}, Arr<int>{un}, Arr<int>{un}, Arr<int>{un},
              Arr<unsigned char>{un}, Arr<unsigned char>{un});
    if (!parent) return fail(OT_ERR_HIP, "scratch allocation failed");
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const double r2 = eps * eps;
    OT_HIP_TRY(hipMemsetAsync(flag, 0, (size_t)n, stream));
    hipLaunchKernelGGL(k_db_core, grid, block, 0, stream, gb.g, n, r2, (int)min_points, core, parent, minidx);
    hipLaunchKernelGGL(k_db_hook, grid, block, 0, stream, gb.g, n, r2, (const unsigned char*)core, parent);
    hipLaunchKernelGGL(k_db_flatten, grid, block, 0, stream, n, (const unsigned char*)core, parent, gb.g.sidx, comp,
                       minidx);
    hipLaunchKernelGGL(k_db_flag, grid, block, 0, stream, n, (const unsigned char*)core, (const int*)comp,
                       (const int*)minidx, flag);
    OT_LAUNCH_CHECK();
    int64_t nc = 0;
    st = compact(n, FlagPred{flag}, RankEmit{rank}, stream, &nc, Slot::OP_COMPACT);
    if (st != OT_OK) return st;
    hipLaunchKernelGGL(k_db_corelabel, grid, block, 0, stream, n, (const unsigned char*)core, (const int*)comp,
                       (const int*)minidx, (const int*)rank, gb.g.sidx, clabel, out_labels);
    hipLaunchKernelGGL(k_db_border, grid, block, 0, stream, gb.g, n, r2, (const unsigned char*)core,
                       (const int*)clabel, out_labels);
    OT_LAUNCH_CHECK();
    OT_HIP_TRY(hipStreamSynchronize(stream));
    if (n_clusters_host) *n_clusters_host = (int32_t)nc;
    return OT_OK;
}

}  // extern "C"
