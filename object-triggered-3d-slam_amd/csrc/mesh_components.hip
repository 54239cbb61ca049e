// mesh_components.hip — TriangleMesh::ClusterConnectedTriangles and the triangle clean-up calls on MI355X
// ("mesh components").
//
// Open3D's loop (tidx ascending, a breadth-first fill from each unlabelled triangle over the triangles that share an
// edge) has a closed form that does not depend on any visiting order, and that is what runs here: the clusters are the
// connected components of "shares an edge key (min, max)", numbered 0 .. C-1 by ascending smallest triangle index.
// With b = the bit width of n_vertices - 1, an edge key is (min << b) | max: both indices in full, 2 b <= 62 bits.
// Launches of the clustering:
//   k_mcc_range    any index outside [0, n_vertices)? (the triangle array alone; the call refuses before going on)
//   k_mcc_edges    the 3T (edge key, corner) pairs; parent[t] = t
//   radix sort     by edge key (sort.h), 2 b key bits
//   k_mcc_hook     each sorted position whose key equals its predecessor's unites the two triangles (union_find.h:
//                  smaller root wins, relaxed agent-scope atomics), then shortens both triangles' paths
//   k_mcc_flatten  comp[t] = root of t (nothing writes parent[] any more); a root is its component's smallest triangle
//                  index, so flag[t] = (comp[t] == t) marks each cluster at the triangle that numbers it
//   compact        the exclusive scan of the flags = the cluster number of each root, and C
//   k_mcc_label    label[t] = rank[comp[t]]; the (label, t) pairs and the triangle areas
//   radix sort     by label, stable: one contiguous segment per cluster, its triangles in ascending index order
//   k_mcc_starts   segment starts, and the areas gathered into sorted order
//   k_mcc_sums     one workgroup per cluster: its size, and its area sum in a fixed association -- lane j adds the
//                  segment's elements j, j + 256, ... in order, the 64 lanes of a wave fold by xor butterflies (32, 16,
//                  ... 1), the four waves as (w0 + w1) + (w2 + w3).  The shape depends on the cluster's size alone and
//                  the order on its triangle indices alone; no floating-point atomics.  (A mesh that is one big
//                  cluster is summed by one workgroup: the call's largest kernel on an extracted mesh, DESIGN.md.)
// Duplicates: one path for every size, two stable sorts over the 96-bit canonical key -- by the third component, then by
// the first two -- so equal keys are adjacent with the earliest triangle at the head of each run.
// Masks to survivors, referenced-vertex flags to a new numbering: compact.h.
#include <climits>

#include "compact.h"
#include "mesh_area.h"
#include "mesh_components.h"
#include "sort.h"
#include "union_find.h"

namespace ot {


int index_bits(int64_t nv) {  // bit width of the largest valid index, nv <= 2^31 - 1
    int b = 1;
    while (b < 31 && ((nv - 1) >> b) != 0) ++b;
    return b;
}

__global__ __launch_bounds__(256) void k_mcc_range(const int32_t* __restrict__ T, int64_t m, int64_t nv, int* bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const bool out = i < m && (unsigned long long)(unsigned)T[i] >= (unsigned long long)nv;  // negative: >= 2^31
    if (__ballot(out) != 0ull && lane_id() == 0) atomicOr(bad, 1);
}

__device__ inline unsigned long long edge_key(int32_t a, int32_t b, int bits) {
    const unsigned lo = (unsigned)(a < b ? a : b), hi = (unsigned)(a < b ? b : a);
    return ((unsigned long long)lo << bits) | (unsigned long long)hi;
}

__global__ __launch_bounds__(256) void k_mcc_edges(const int32_t* __restrict__ T, int64_t nt, int bits,
                                                   unsigned long long* __restrict__ keys, unsigned* __restrict__ vals,
                                                   int* __restrict__ parent) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int32_t a = T[t * 3], b = T[t * 3 + 1], c = T[t * 3 + 2];
    keys[t * 3 + 0] = edge_key(a, b, bits);
    keys[t * 3 + 1] = edge_key(b, c, bits);
    keys[t * 3 + 2] = edge_key(c, a, bits);
    vals[t * 3 + 0] = (unsigned)(t * 3 + 0);
    vals[t * 3 + 1] = (unsigned)(t * 3 + 1);
    vals[t * 3 + 2] = (unsigned)(t * 3 + 2);
    parent[t] = (int)t;
}

__global__ __launch_bounds__(256) void k_mcc_hook(const unsigned long long* __restrict__ skeys,
                                                  const unsigned* __restrict__ svals, int64_t m, int* parent) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < 1 || i >= m || skeys[i] != skeys[i - 1]) return;
    const int ta = (int)(svals[i] / 3u), tb = (int)(svals[i - 1] / 3u);
    if (ta == tb) return;  // two corners of one degenerate triangle
    const int r = uf_union(parent, ta, tb);
    // r is an ancestor of both, and of two ancestors the smaller is the nearer to the root: a valid, shorter parent
    if (r < ta) __hip_atomic_fetch_min(parent + ta, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (r < tb) __hip_atomic_fetch_min(parent + tb, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void k_mcc_flatten(int64_t nt, int* parent, int* __restrict__ comp,
                                                     unsigned char* __restrict__ flag) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int r = uf_find(parent, (int)t);
    comp[t] = r;
    flag[t] = r == (int)t ? 1 : 0;
}

struct ByteSetPred {
    const unsigned char* flag;
    __device__ bool operator()(int64_t i) const { return flag[i] != 0; }
};
struct ByteClearPred {
    const unsigned char* flag;
    __device__ bool operator()(int64_t i) const { return flag[i] == 0; }
};
struct RankOfEmit {
    int* rank;
    __device__ void operator()(int64_t i, int64_t pos) const { rank[i] = (int)pos; }
};

__global__ __launch_bounds__(256) void k_mcc_label(int64_t nt, const int* __restrict__ comp,
                                                   const int* __restrict__ rank, const double* __restrict__ V,
                                                   const int32_t* __restrict__ T, int32_t* __restrict__ out_labels,
                                                   unsigned long long* __restrict__ keys, unsigned* __restrict__ vals,
                                                   double* __restrict__ area) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int l = rank[comp[t]];
    out_labels[t] = l;
    keys[t] = (unsigned long long)(unsigned)l;
    vals[t] = (unsigned)t;
    if (V) area[t] = tri_area(V, T, t);
}

// segment starts, and the areas in sorted (label, triangle) order (sarea nullable: no areas)
__global__ __launch_bounds__(256) void k_mcc_starts(const unsigned long long* __restrict__ skeys,
                                                    const unsigned* __restrict__ svals, int64_t nt, int64_t nc,
                                                    int* __restrict__ start, const double* __restrict__ area,
                                                    double* __restrict__ sarea) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    if (i == 0 || skeys[i] != skeys[i - 1]) start[skeys[i]] = (int)i;  // every label 0 .. nc - 1 occurs
    if (i == 0) start[nc] = (int)nt;
    if (sarea) sarea[i] = area[svals[i]];
}

__global__ __launch_bounds__(256) void k_mcc_sums(const int* __restrict__ start, const double* __restrict__ sarea,
                                                  int64_t nc, int32_t* __restrict__ out_n,
                                                  double* __restrict__ out_area) {
    __shared__ double s_w[4];
    for (int64_t k = blockIdx.x; k < nc; k += gridDim.x) {  // block-uniform
        const int s = start[k], e = start[k + 1];
        if (threadIdx.x == 0) out_n[k] = e - s;
        if (!out_area) continue;  // grid-uniform
        // lane j: x_j, x_{j+256}, ... added in that order; eight loads in flight, the adds still one after another
        double acc = 0.0;
        int i = s + (int)threadIdx.x;
        for (; i + 7 * 256 < e; i += 8 * 256) {
            double x[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) x[u] = sarea[i + u * 256];
#pragma unroll
            for (int u = 0; u < 8; ++u) acc += x[u];
        }
        for (; i < e; i += 256) acc += sarea[i];
        acc = wave_sum(acc);  // xor butterflies 32 .. 1: the same association in every lane
        if (lane_id() == 0) s_w[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) out_area[k] = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ clean-up
__global__ __launch_bounds__(256) void k_mcc_degenerate(const int32_t* __restrict__ T, int64_t nt,
                                                        unsigned char* __restrict__ mask) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int32_t a = T[t * 3], b = T[t * 3 + 1], c = T[t * 3 + 2];
    mask[t] = (a == b || b == c || a == c) ? 1 : 0;
}

// TriangleMesh::RemoveDuplicatedTriangles' key: the rotation Open3D picks (not always the one starting at the minimum:
// (a, b, a) with a < b stays (a, b, a), while (a, a, b) and (b, a, a) both become (a, a, b))
struct Key3 {
    unsigned k0, k1, k2;
};
__device__ inline Key3 canon_key(const int32_t* __restrict__ T, int64_t t) {
    const int32_t t0 = T[t * 3], t1 = T[t * 3 + 1], t2 = T[t * 3 + 2];
    if (t0 <= t1) {
        if (t0 <= t2) return Key3{(unsigned)t0, (unsigned)t1, (unsigned)t2};
        return Key3{(unsigned)t2, (unsigned)t0, (unsigned)t1};
    }
    if (t1 <= t2) return Key3{(unsigned)t1, (unsigned)t2, (unsigned)t0};
    return Key3{(unsigned)t2, (unsigned)t0, (unsigned)t1};
}

__global__ __launch_bounds__(256) void k_mcc_dup_k2(const int32_t* __restrict__ T, int64_t nt,
                                                    unsigned long long* __restrict__ keys, unsigned* __restrict__ vals) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    keys[t] = (unsigned long long)canon_key(T, t).k2;
    vals[t] = (unsigned)t;
}

__global__ __launch_bounds__(256) void k_mcc_dup_k01(const int32_t* __restrict__ T, int64_t nt, int bits,
                                                     const unsigned* __restrict__ svals,
                                                     unsigned long long* __restrict__ keys) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    const Key3 k = canon_key(T, svals[i]);
    keys[i] = ((unsigned long long)k.k0 << bits) | (unsigned long long)k.k1;
}

__global__ __launch_bounds__(256) void k_mcc_dup_flag(const int32_t* __restrict__ T, int64_t nt,
                                                      const unsigned* __restrict__ svals,
                                                      unsigned char* __restrict__ mask) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nt) return;
    const unsigned t = svals[i];
    bool dup = false;
    if (i > 0) {
        const Key3 a = canon_key(T, t), b = canon_key(T, svals[i - 1]);
        dup = a.k0 == b.k0 && a.k1 == b.k1 && a.k2 == b.k2;
    }
    mask[t] = dup ? 1 : 0;  // every triangle sits at exactly one sorted position
}

struct TriEmit {
    const int32_t* in;
    int32_t* out;
    __device__ void operator()(int64_t i, int64_t pos) const {
        out[pos * 3 + 0] = in[i * 3 + 0];
        out[pos * 3 + 1] = in[i * 3 + 1];
        out[pos * 3 + 2] = in[i * 3 + 2];
    }
};

__global__ __launch_bounds__(256) void k_mcc_mark(const int32_t* __restrict__ T, int64_t m,
                                                  unsigned char* __restrict__ flag) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) flag[T[i]] = 1;  // range-checked; concurrent stores all write the same byte value
}
struct KeptVertexEmit {
    int32_t* kept;
    int* newidx;
    __device__ void operator()(int64_t i, int64_t pos) const {
        kept[pos] = (int32_t)i;
        newidx[i] = (int)pos;
    }
};
__global__ __launch_bounds__(256) void k_mcc_renumber(int32_t* __restrict__ T, int64_t m,
                                                      const int* __restrict__ newidx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) T[i] = newidx[T[i]];
}

// ------------------------------------------------------------------------------------------------ host side
static inline dim3 blocks_of(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// sizes every entry refuses before any device work
ot_status check_sizes(const char* who, int64_t nt, int64_t nv) {
    if (nt < 0 || nv < 0) return fail(OT_ERR_INVALID_ARGUMENT, std::string("[") + who + "] negative size");
    if (nt > 0x7FFFFFFF / 3 || nv > 0x7FFFFFFF)
        return fail(OT_ERR_INVALID_ARGUMENT, std::string("[") + who + "] mesh too large (3 n_triangles and n_vertices "
                                                                      "must fit 31 bits)");
    return OT_OK;
}

// the range check over the triangle array alone (synchronises)
ot_status check_indices(const char* who, const int32_t* T, int64_t nt, int64_t nv, hipStream_t stream) {
    if (nt == 0) return OT_OK;
    int* bad = (int*)scratch(64, Slot::MCC_BAD);
    if (!bad) return fail(OT_ERR_HIP, "scratch allocation failed");
    OT_HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), stream));
    hipLaunchKernelGGL(k_mcc_range, blocks_of(nt * 3), dim3(256), 0, stream, T, nt * 3, nv, bad);
    OT_LAUNCH_CHECK();
    int h = 0;
    OT_HIP_TRY(hipMemcpyAsync(&h, bad, sizeof(int), hipMemcpyDeviceToHost, stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));
    if (h) return fail(OT_ERR_INVALID_ARGUMENT, std::string("[") + who + "] triangle index out of range [0, n_vertices)");
    return OT_OK;
}

// the duplicate mask of range-checked triangles (mesh_components.h); queued on the stream, no synchronisation
ot_status flag_duplicated_triangles(const int32_t* triangles, int64_t nt, int64_t n_vertices,
                                    unsigned char* out_remove_mask, hipStream_t stream) {
    const size_t unt = (size_t)nt;
    auto [ka, kb, va, vb] = carve(scratch_of(Slot::MCC_WS), Arr<unsigned long long>{unt}, Arr<unsigned long long>{unt},
                                  Arr<unsigned>{unt}, Arr<unsigned>{unt});
    if (!ka) return fail(OT_ERR_HIP, "scratch allocation failed");
    const int bits = index_bits(n_vertices);
    hipLaunchKernelGGL(k_mcc_dup_k2, blocks_of(nt), dim3(256), 0, stream, triangles, nt, ka, va);
    OT_LAUNCH_CHECK();
    ot_status st = sort_pairs_u64_u32(ka, kb, va, vb, (size_t)nt, bits, stream, Slot::SORT_TMP);  // by the third component
    if (st != OT_OK) return st;
    hipLaunchKernelGGL(k_mcc_dup_k01, blocks_of(nt), dim3(256), 0, stream, triangles, nt, bits, (const unsigned*)vb,
                       ka);
    OT_LAUNCH_CHECK();
    st = sort_pairs_u64_u32(ka, kb, vb, va, (size_t)nt, 2 * bits, stream, Slot::SORT_TMP);  // then by the first two
    if (st != OT_OK) return st;
    hipLaunchKernelGGL(k_mcc_dup_flag, blocks_of(nt), dim3(256), 0, stream, triangles, nt, (const unsigned*)va,
                       out_remove_mask);
    OT_LAUNCH_CHECK();
    return OT_OK;
}

}  // namespace ot

using namespace ot;

extern "C" {

ot_status ot_mesh_cluster_connected_triangles(const int32_t* triangles, int64_t n_triangles, const double* vertices,
                                              int64_t n_vertices, int32_t* out_triangle_clusters,
                                              int32_t* out_cluster_n_triangles, double* out_cluster_area,
                                              int64_t* n_clusters_host, void* stream_) {
    static const char* who = "ClusterConnectedTriangles";
    hipStream_t stream = S(stream_);
    const int64_t nt = n_triangles, nv = n_vertices;
    ot_status st = check_sizes(who, nt, nv);
    if (st != OT_OK) return st;
    if (!n_clusters_host || (nt > 0 && (!triangles || !out_triangle_clusters || !out_cluster_n_triangles)) ||
        ((vertices == nullptr) != (out_cluster_area == nullptr)))
        return fail(OT_ERR_INVALID_ARGUMENT, "[ClusterConnectedTriangles] invalid buffers");
    *n_clusters_host = 0;
    if (nt == 0) return OT_OK;
    st = check_indices(who, triangles, nt, nv, stream);
    if (st != OT_OK) return st;
    const int64_t m = nt * 3;
    const size_t unt = (size_t)nt, um = (size_t)m;
    auto [parent, comp, rank, start, flag, area, sarea_ws, kin, kout, vin, vout] =
        carve(scratch_of(Slot::MCC_WS), Arr<int>{unt}, Arr<int>{unt}, Arr<int>{unt}, Arr<int>{unt + 1},
              Arr<unsigned char>{unt}, Arr<double>{unt}, Arr<double>{unt}, Arr<unsigned long long>{um},
              Arr<unsigned long long>{um}, Arr<unsigned>{um}, Arr<unsigned>{um});
    if (!parent) return fail(OT_ERR_HIP, "scratch allocation failed");
    double* sarea = vertices ? sarea_ws : nullptr;
    const int bits = index_bits(nv);
    hipLaunchKernelGGL(k_mcc_edges, blocks_of(nt), dim3(256), 0, stream, triangles, nt, bits, kin, vin, parent);
    OT_LAUNCH_CHECK();
    st = sort_pairs_u64_u32(kin, kout, vin, vout, (size_t)m, 2 * bits, stream, Slot::SORT_TMP);
    if (st != OT_OK) return st;
    hipLaunchKernelGGL(k_mcc_hook, blocks_of(m), dim3(256), 0, stream, (const unsigned long long*)kout,
                       (const unsigned*)vout, m, parent);
    hipLaunchKernelGGL(k_mcc_flatten, blocks_of(nt), dim3(256), 0, stream, nt, parent, comp, flag);
    OT_LAUNCH_CHECK();
    int64_t nc = 0;
    st = compact(nt, ByteSetPred{flag}, RankOfEmit{rank}, stream, &nc, Slot::MCC_COMPACT);
    if (st != OT_OK) return st;
    hipLaunchKernelGGL(k_mcc_label, blocks_of(nt), dim3(256), 0, stream, nt, (const int*)comp, (const int*)rank,
                       vertices, triangles, out_triangle_clusters, kin, vin, area);
    OT_LAUNCH_CHECK();
    int lbits = 1;
    while (lbits < 31 && ((nc - 1) >> lbits) != 0) ++lbits;
    st = sort_pairs_u64_u32(kin, kout, vin, vout, (size_t)nt, lbits, stream, Slot::SORT_TMP);
    if (st != OT_OK) return st;
    hipLaunchKernelGGL(k_mcc_starts, blocks_of(nt), dim3(256), 0, stream, (const unsigned long long*)kout,
                       (const unsigned*)vout, nt, nc, start, (const double*)area, sarea);
    hipLaunchKernelGGL(k_mcc_sums, dim3((unsigned)std::min<int64_t>(nc, 65536)), dim3(256), 0, stream,
                       (const int*)start, (const double*)sarea, nc, out_cluster_n_triangles, out_cluster_area);
    OT_LAUNCH_CHECK();
    OT_HIP_TRY(hipStreamSynchronize(stream));
    *n_clusters_host = nc;
    return OT_OK;
}

ot_status ot_mesh_flag_degenerate_triangles(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                                            uint8_t* out_remove_mask, void* stream_) {
    static const char* who = "RemoveDegenerateTriangles";
    hipStream_t stream = S(stream_);
    ot_status st = check_sizes(who, n_triangles, n_vertices);
    if (st != OT_OK) return st;
    if (n_triangles > 0 && (!triangles || !out_remove_mask))
        return fail(OT_ERR_INVALID_ARGUMENT, "[RemoveDegenerateTriangles] invalid buffers");
    if (n_triangles == 0) return OT_OK;
    st = check_indices(who, triangles, n_triangles, n_vertices, stream);
    if (st != OT_OK) return st;
    hipLaunchKernelGGL(k_mcc_degenerate, blocks_of(n_triangles), dim3(256), 0, stream, triangles, n_triangles,
                       out_remove_mask);
    OT_LAUNCH_CHECK();
    OT_HIP_TRY(hipStreamSynchronize(stream));
    return OT_OK;
}

ot_status ot_mesh_flag_duplicated_triangles(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                                            uint8_t* out_remove_mask, void* stream_) {
    static const char* who = "RemoveDuplicatedTriangles";
    hipStream_t stream = S(stream_);
    const int64_t nt = n_triangles;
    ot_status st = check_sizes(who, nt, n_vertices);
    if (st != OT_OK) return st;
    if (nt > 0 && (!triangles || !out_remove_mask))
        return fail(OT_ERR_INVALID_ARGUMENT, "[RemoveDuplicatedTriangles] invalid buffers");
    if (nt == 0) return OT_OK;
    st = check_indices(who, triangles, nt, n_vertices, stream);
    if (st != OT_OK) return st;
    st = flag_duplicated_triangles(triangles, nt, n_vertices, out_remove_mask, stream);
    if (st != OT_OK) return st;
    OT_HIP_TRY(hipStreamSynchronize(stream));
    return OT_OK;
}

ot_status ot_mesh_remove_triangles_by_mask(const int32_t* triangles, int64_t n_triangles, const uint8_t* remove_mask,
                                           int32_t* out_triangles, int64_t* n_kept_host, void* stream_) {
    hipStream_t stream = S(stream_);
    ot_status st = check_sizes("RemoveTrianglesByMask", n_triangles, 0);
    if (st != OT_OK) return st;
    if (!n_kept_host || (n_triangles > 0 && (!triangles || !remove_mask || !out_triangles)) ||
        (n_triangles > 0 && triangles == out_triangles))
        return fail(OT_ERR_INVALID_ARGUMENT, "[RemoveTrianglesByMask] invalid buffers");
    *n_kept_host = 0;
    if (n_triangles == 0) return OT_OK;
    return compact(n_triangles, ByteClearPred{remove_mask}, TriEmit{triangles, out_triangles}, stream, n_kept_host,
                   Slot::MCC_COMPACT);
}

ot_status ot_mesh_remove_unreferenced_vertices(int64_t n_vertices, int32_t* triangles, int64_t n_triangles,
                                               int32_t* out_kept_old_index, int64_t* n_kept_host, void* stream_) {
    static const char* who = "RemoveUnreferencedVertices";
    hipStream_t stream = S(stream_);
    const int64_t nt = n_triangles, nv = n_vertices;
    ot_status st = check_sizes(who, nt, nv);
    if (st != OT_OK) return st;
    if (!n_kept_host || (nt > 0 && !triangles) || (nv > 0 && !out_kept_old_index))
        return fail(OT_ERR_INVALID_ARGUMENT, "[RemoveUnreferencedVertices] invalid buffers");
    *n_kept_host = 0;
    st = check_indices(who, triangles, nt, nv, stream);  // (no vertices and a triangle: refused here)
    if (st != OT_OK) return st;
    if (nv == 0 || nt == 0) return OT_OK;  // no triangle references anything
    auto [flag, newidx] = carve(scratch_of(Slot::MCC_WS), Arr<unsigned char>{(size_t)nv}, Arr<int>{(size_t)nv});
    if (!flag) return fail(OT_ERR_HIP, "scratch allocation failed");
    const int64_t m = nt * 3;
    OT_HIP_TRY(hipMemsetAsync(flag, 0, (size_t)nv, stream));
    hipLaunchKernelGGL(k_mcc_mark, blocks_of(m), dim3(256), 0, stream, (const int32_t*)triangles, m, flag);
    OT_LAUNCH_CHECK();
    st = compact(nv, ByteSetPred{flag}, KeptVertexEmit{out_kept_old_index, newidx}, stream, n_kept_host,
                 Slot::MCC_COMPACT);
    if (st != OT_OK) return st;
    hipLaunchKernelGGL(k_mcc_renumber, blocks_of(m), dim3(256), 0, stream, triangles, m, (const int*)newidx);
    OT_LAUNCH_CHECK();
    OT_HIP_TRY(hipStreamSynchronize(stream));
    return OT_OK;
}

}  // extern "C"
