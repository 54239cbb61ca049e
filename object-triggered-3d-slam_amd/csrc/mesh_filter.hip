// mesh_filter.hip — TriangleMesh::ComputeAdjacencyList, FilterSmoothSimple / FilterSmoothLaplacian / FilterSmoothTaubin /
// FilterSharpen and SimplifyVertexClustering (Average) on MI355X ("mesh filters").
//
// Adjacency, as a CSR whose rows are in ascending neighbour order (Open3D: unordered_set order):
//   k_mf_adj_keys   the 6T directed keys (vertex << b) | neighbour, b = the bit width of n_vertices - 1
//   radix sort      by key (sort.h), 2 b bits
//   compact         the first of each run of equal keys: the neighbour list and, beside it, each entry's vertex
//   k_mf_offsets    offsets[v] = the first entry whose vertex is >= v (a binary search per vertex: no atomics, and a
//                   vertex without triangles gets an empty row at no extra cost)
// Filters: one launch per step (k_mf_filter, a Taubin iteration is two), one lane per vertex, 256-thread workgroups of
// four wave64s.  A lane walks its row of the CSR and gathers its neighbours' rows of every filtered attribute, four
// neighbours' loads in flight, and adds them in ascending neighbour order: one left-to-right float64 chain per vertex
// and component, which is what fixes the bits, so a chain is never split across lanes.  (A vertex of degree 4 096 is
// therefore walked by one lane while its wave's other lanes wait: slow, correct, and not what a marching-cubes mesh
// holds -- there the degree is about 6 and neighbouring indices are neighbouring rows, so most gathers hit L2.)
// All of a step's attributes go through the one launch: offsets, indices and Laplacian weights are read once.  Steps
// ping-pong between the caller's output arrays and one scratch buffer, arranged so that the last step writes the
// output; every step reads only its predecessor's values.  No floating-point atomics.
// Vertex clustering: the voxel keys, the stable sort and the in-index-order averages are VoxelDownSample's
// (voxel_keys.h); a voxel's new index is the rank of its smallest old vertex index among all voxels' (flags at those
// vertices, compact.h), which is Open3D's first-appearance numbering; the triangles are mapped, rotated to start at
// their smallest index, and the earliest of each distinct triple survives (mesh_components.h).
#include <climits>

#include "compact.h"
#include "mesh_components.h"
#include "sort.h"
#include "voxel_keys.h"

namespace ot {
namespace {

inline dim3 blocks_of(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

// ------------------------------------------------------------------------------------------------ adjacency
__global__ __launch_bounds__(256) void k_mf_adj_keys(const int32_t* __restrict__ T, int64_t nt, int bits,
                                                     unsigned long long* __restrict__ keys,
                                                     unsigned* __restrict__ vals) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const unsigned long long a = (unsigned)T[t * 3], b = (unsigned)T[t * 3 + 1], c = (unsigned)T[t * 3 + 2];
    unsigned long long* k = keys + t * 6;
    k[0] = (a << bits) | b;
    k[1] = (a << bits) | c;
    k[2] = (b << bits) | a;
    k[3] = (b << bits) | c;
    k[4] = (c << bits) | a;
    k[5] = (c << bits) | b;
#pragma unroll
    for (int j = 0; j < 6; ++j) vals[t * 6 + j] = (unsigned)(t * 6 + j);
}

struct AdjEmit {
    const unsigned long long* keys;
    int bits;
    int32_t* vertex;
    int32_t* neighbour;
    __device__ void operator()(int64_t i, int64_t pos) const {
        const unsigned long long k = keys[i];
        vertex[pos] = (int32_t)(k >> bits);
        neighbour[pos] = (int32_t)(k & ((1ull << bits) - 1ull));
    }
};

// offsets[v] = the number of entries whose vertex is below v, v = 0 .. nv (entry vertices ascending)
__global__ __launch_bounds__(256) void k_mf_offsets(const int32_t* __restrict__ vertex, int64_t ne, int64_t nv,
                                                    int32_t* __restrict__ offsets) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v > nv) return;
    int64_t lo = 0, hi = ne;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)vertex[mid] < v) lo = mid + 1;
        else hi = mid;
    }
    offsets[v] = (int32_t)lo;
}

// a CSR handed to the filters must fit the mesh: offsets 0 .. ne ascending, neighbours inside [0, nv)
__global__ __launch_bounds__(256) void k_mf_csr_check(const int32_t* __restrict__ offsets,
                                                      const int32_t* __restrict__ nbr, int64_t nv, int64_t ne,
                                                      int* bad) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    bool out = false;
    if (i < nv) out = offsets[i] < 0 || offsets[i] > offsets[i + 1];
    if (i == 0) out = out || offsets[0] != 0 || (int64_t)offsets[nv] != ne;
    if (i < ne) out = out || (unsigned long long)(unsigned)nbr[i] >= (unsigned long long)nv;
    if (__ballot(out) != 0ull && lane_id() == 0) atomicOr(bad, 1);
}

// ------------------------------------------------------------------------------------------------ filters
enum { MF_SIMPLE = 0, MF_LAPLACIAN = 1, MF_TAUBIN = 2, MF_SHARPEN = 3 };

struct FilterArgs {
    const double* P;       // the positions the Laplacian weights come from (the previous step's)
    const double* src[3];  // vertices, normals, colours of the previous step; NULL: not filtered
    double* dst[3];
};

template <int KIND>
__global__ __launch_bounds__(256) void k_mf_filter(FilterArgs A, const int32_t* __restrict__ offsets,
                                                   const int32_t* __restrict__ nbr, int64_t nv, double par) {
    const int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (v >= nv) return;
    const int beg = offsets[v], end = offsets[v + 1];
    double x0[3][3], acc[3][3], pv[3] = {0, 0, 0};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            x0[a][d] = A.src[a] ? A.src[a][v * 3 + d] : 0.0;
            acc[a][d] = KIND == MF_SIMPLE ? x0[a][d] : 0.0;
        }
    if (KIND == MF_LAPLACIAN) {
#pragma unroll
        for (int d = 0; d < 3; ++d) pv[d] = A.P[v * 3 + d];
    }
    if (beg == end) {  // no neighbours: the attributes stay as they are (Open3D's Laplacian divides 0 by 0)
#pragma unroll
        for (int a = 0; a < 3; ++a)
            if (A.src[a]) {
#pragma unroll
                for (int d = 0; d < 3; ++d) A.dst[a][v * 3 + d] = x0[a][d];
            }
        return;
    }
    double W = 0.0;
    // neighbours in batches of 4: the batch's index and row loads are all issued before its (in-order) sums
    constexpr int NB = 4;
    for (int j0 = beg; j0 < end; j0 += NB) {
        int64_t w[NB];
#pragma unroll
        for (int k = 0; k < NB; ++k) w[k] = nbr[j0 + k < end ? j0 + k : j0];
        double xp[NB][3], x[NB][3][3];
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            if (KIND == MF_LAPLACIAN) {
#pragma unroll
                for (int d = 0; d < 3; ++d) xp[k][d] = A.P[w[k] * 3 + d];
            }
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int d = 0; d < 3; ++d) x[k][a][d] = A.src[a] ? A.src[a][w[k] * 3 + d] : 0.0;
        }
#pragma unroll
        for (int k = 0; k < NB; ++k) {
            if (j0 + k >= end) break;
            double wt = 1.0;
            if (KIND == MF_LAPLACIAN) {
                const double dx = pv[0] - xp[k][0], dy = pv[1] - xp[k][1], dz = pv[2] - xp[k][2];
                const double dist = sqrt((dx * dx + dy * dy) + dz * dz);
                wt = 1.0 / (dist + 1e-12);
                W += wt;
            }
#pragma unroll
            for (int a = 0; a < 3; ++a)
                if (A.src[a]) {
#pragma unroll
                    for (int d = 0; d < 3; ++d) acc[a][d] += KIND == MF_LAPLACIAN ? wt * x[k][a][d] : x[k][a][d];
                }
        }
    }
    const double n = (double)(end - beg);
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (A.src[a]) {
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                double r;
                if (KIND == MF_SIMPLE) r = acc[a][d] / (1.0 + n);  // 1 + n is exact: the float64 of the integer
                else if (KIND == MF_LAPLACIAN) r = x0[a][d] + par * (acc[a][d] / W - x0[a][d]);
                else r = x0[a][d] * (1.0 + par * n) - par * acc[a][d];
                A.dst[a][v * 3 + d] = r;
            }
        }
}

// ------------------------------------------------------------------------------------------------ clustering
struct FlagSetPred {
    const unsigned char* flag;
    __device__ bool operator()(int64_t i) const { return flag[i] != 0; }
};
struct RankEmit {
    int* rank;
    __device__ void operator()(int64_t i, int64_t pos) const { rank[i] = (int)pos; }
};

// the first vertex of each voxel's segment is its smallest old index (the sort is stable)
__global__ __launch_bounds__(256) void k_mf_first(const unsigned* __restrict__ sidx, const int* __restrict__ heads,
                                                  int64_t K, unsigned char* __restrict__ flag) {
    const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (s < K) flag[sidx[heads[s]]] = 1;
}

// the voxel of sorted position i is seg[i]; its new index is the rank of its first vertex
__global__ __launch_bounds__(256) void k_mf_rows(const unsigned* __restrict__ sidx, const int* __restrict__ heads,
                                                 const int* __restrict__ seg, const int* __restrict__ rank, int64_t nv,
                                                 int* __restrict__ row, int* __restrict__ newidx) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= nv) return;
    const int s = seg[i], h = heads[s];
    const int r = rank[sidx[h]];
    newidx[sidx[i]] = r;
    if (i == h) row[s] = r;
}

// the triangle on the new indices, rotated so that its smallest index comes first; drop[t] = two corners coincide
__global__ __launch_bounds__(256) void k_mf_map_tris(const int32_t* __restrict__ T, int64_t nt,
                                                     const int* __restrict__ newidx, int32_t* __restrict__ M,
                                                     unsigned char* __restrict__ drop) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nt) return;
    const int a = newidx[T[t * 3]], b = newidx[T[t * 3 + 1]], c = newidx[T[t * 3 + 2]];
    int r0 = a, r1 = b, r2 = c;
    if (b < a && b <= c) {
        r0 = b, r1 = c, r2 = a;
    } else if (c < a && c < b) {
        r0 = c, r1 = a, r2 = b;
    }
    M[t * 3 + 0] = r0;
    M[t * 3 + 1] = r1;
    M[t * 3 + 2] = r2;
    drop[t] = (a == b || b == c || a == c) ? 1 : 0;
}

struct KeepTriPred {
    const unsigned char* dup;
    const unsigned char* drop;
    __device__ bool operator()(int64_t i) const { return dup[i] == 0 && drop[i] == 0; }
};
struct TriRowEmit {
    const int32_t* in;
    int32_t* out;
    __device__ void operator()(int64_t i, int64_t pos) const {
        out[pos * 3 + 0] = in[i * 3 + 0];
        out[pos * 3 + 1] = in[i * 3 + 1];
        out[pos * 3 + 2] = in[i * 3 + 2];
    }
};

}  // namespace
}  // namespace ot

using namespace ot;

extern "C" {

ot_status ot_mesh_compute_adjacency(const int32_t* triangles, int64_t n_triangles, int64_t n_vertices,
                                    int32_t* out_offsets, int32_t* out_neighbours, int64_t* n_entries_host,
                                    void* stream_) {
    static const char* who = "ComputeAdjacencyList";
    hipStream_t stream = S(stream_);
    const int64_t nt = n_triangles, nv = n_vertices;
    ot_status st = check_sizes(who, nt, nv);
    if (st != OT_OK) return st;
    if (nt > 0x7FFFFFFF / 6)
        return fail(OT_ERR_INVALID_ARGUMENT, "[ComputeAdjacencyList] mesh too large (6 n_triangles must fit 31 bits)");
    if (!n_entries_host || !out_offsets || (nt > 0 && (!triangles || !out_neighbours)))
        return fail(OT_ERR_INVALID_ARGUMENT, "[ComputeAdjacencyList] invalid buffers");
    *n_entries_host = 0;
    st = check_indices(who, triangles, nt, nv, stream);  // (no vertices and a triangle: refused here)
    if (st != OT_OK) return st;
    if (nt == 0) {
        OT_HIP_TRY(hipMemsetAsync(out_offsets, 0, sizeof(int32_t) * (size_t)(nv + 1), stream));
        OT_HIP_TRY(hipStreamSynchronize(stream));
        return OT_OK;
    }
    const int64_t m = nt * 6;
    const size_t um = (size_t)m;
    auto [kin, kout, vin, vout, vertex] =
        carve(scratch_of(Slot::MF_WS), Arr<unsigned long long>{um}, Arr<unsigned long long>{um}, Arr<unsigned>{um},
              Arr<unsigned>{um}, Arr<int32_t>{um});
    if (!kin) return fail(OT_ERR_HIP, "scratch allocation failed");
    const int bits = index_bits(nv);
    hipLaunchKernelGGL(k_mf_adj_keys, blocks_of(nt), dim3(256), 0, stream, triangles, nt, bits, kin, vin);
    OT_LAUNCH_CHECK();
    st = sort_pairs_u64_u32(kin, kout, vin, vout, um, 2 * bits, stream, Slot::SORT_TMP);
    if (st != OT_OK) return st;
    int64_t ne = 0;
    st = compact(m, SegHeadPred{kout}, AdjEmit{kout, bits, vertex, out_neighbours}, stream, &ne, Slot::MF_COMPACT);
    if (st != OT_OK) return st;
    hipLaunchKernelGGL(k_mf_offsets, blocks_of(nv + 1), dim3(256), 0, stream, (const int32_t*)vertex, ne, nv,
                       out_offsets);
    OT_LAUNCH_CHECK();
    OT_HIP_TRY(hipStreamSynchronize(stream));
    *n_entries_host = ne;
    return OT_OK;
}

ot_status ot_mesh_filter(int32_t kind, const double* vertices, const double* normals, const double* colors,
                         int64_t n_vertices, const int32_t* offsets, const int32_t* neighbours, int64_t n_entries,
                         int32_t iterations, double p0, double p1, int32_t scope, double* out_vertices,
                         double* out_normals, double* out_colors, void* stream_) {
    hipStream_t stream = S(stream_);
    const int64_t nv = n_vertices, ne = n_entries;
    if (kind < MF_SIMPLE || kind > MF_SHARPEN) return fail(OT_ERR_INVALID_ARGUMENT, "[FilterMesh] unknown filter kind");
    if (nv < 0 || nv > 0x7FFFFFFF || ne < 0 || ne > 0x7FFFFFFF)
        return fail(OT_ERR_INVALID_ARGUMENT, "[FilterMesh] negative or too large size");
    if ((scope & ~7) != 0) return fail(OT_ERR_INVALID_ARGUMENT, "[FilterMesh] unknown scope bits");
    if (nv == 0) return OT_OK;
    const double* in[3] = {vertices, normals, colors};
    double* out[3] = {out_vertices, out_normals, out_colors};
    if (!vertices || !out_vertices || !offsets || (ne > 0 && !neighbours))
        return fail(OT_ERR_INVALID_ARGUMENT, "[FilterMesh] invalid buffers");
    for (int a = 0; a < 3; ++a)
        if (in[a] && (!out[a] || out[a] == in[a]))
            return fail(OT_ERR_INVALID_ARGUMENT, "[FilterMesh] invalid buffers (an output is missing or aliases its input)");
    const int64_t steps = iterations <= 0 ? 0 : (kind == MF_TAUBIN ? 2 * (int64_t)iterations : (int64_t)iterations);
    bool filtered[3];
    int nf = 0;
    for (int a = 0; a < 3; ++a) {
        filtered[a] = steps > 0 && in[a] && ((scope >> a) & 1);
        nf += filtered[a] ? 1 : 0;
        if (in[a] && !filtered[a])
            OT_HIP_TRY(hipMemcpyAsync(out[a], in[a], sizeof(double) * 3 * (size_t)nv, hipMemcpyDeviceToDevice, stream));
    }
    if (nf == 0) return OT_OK;
    int* bad = (int*)scratch(64, Slot::MCC_BAD);
    if (!bad) return fail(OT_ERR_HIP, "scratch allocation failed");
    OT_HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), stream));
    hipLaunchKernelGGL(k_mf_csr_check, blocks_of(std::max(nv, ne)), dim3(256), 0, stream, offsets, neighbours, nv, ne,
                       bad);
    OT_LAUNCH_CHECK();
    int h = 0;
    OT_HIP_TRY(hipMemcpyAsync(&h, bad, sizeof(int), hipMemcpyDeviceToHost, stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));
    if (h) return fail(OT_ERR_INVALID_ARGUMENT, "[FilterMesh] the adjacency list does not fit the mesh");
    double* ping = nullptr;
    const size_t row_doubles = 3 * (size_t)nv;
    if (steps > 1) {
        ping = (double*)scratch(sizeof(double) * row_doubles * (size_t)nf, Slot::MF_PING);
        if (!ping) return fail(OT_ERR_HIP, "scratch allocation failed");
    }
    double* tmp[3] = {nullptr, nullptr, nullptr};
    for (int a = 0, k = 0; a < 3; ++a)
        if (filtered[a] && ping) tmp[a] = ping + row_doubles * (size_t)(k++);
    const double* cur[3] = {in[0], in[1], in[2]};
    for (int64_t s = 0; s < steps; ++s) {
        const bool to_out = ((steps - 1 - s) & 1) == 0;  // the last step writes the output
        FilterArgs A;
        A.P = filtered[0] ? cur[0] : vertices;
        for (int a = 0; a < 3; ++a) {
            A.src[a] = filtered[a] ? cur[a] : nullptr;
            A.dst[a] = filtered[a] ? (to_out ? out[a] : tmp[a]) : nullptr;
        }
        const double par = (kind == MF_TAUBIN && (s & 1)) ? p1 : p0;
        if (kind == MF_SIMPLE)
            hipLaunchKernelGGL(k_mf_filter<MF_SIMPLE>, blocks_of(nv), dim3(256), 0, stream, A, offsets, neighbours, nv, par);
        else if (kind == MF_SHARPEN)
            hipLaunchKernelGGL(k_mf_filter<MF_SHARPEN>, blocks_of(nv), dim3(256), 0, stream, A, offsets, neighbours, nv, par);
        else
            hipLaunchKernelGGL(k_mf_filter<MF_LAPLACIAN>, blocks_of(nv), dim3(256), 0, stream, A, offsets, neighbours, nv, par);
        OT_LAUNCH_CHECK();
        for (int a = 0; a < 3; ++a)
            if (filtered[a]) cur[a] = A.dst[a];
    }
    return OT_OK;
}

ot_status ot_mesh_simplify_vertex_clustering(const double* vertices, const double* normals, const double* colors,
                                             int64_t n_vertices, const int32_t* triangles, int64_t n_triangles,
                                             double voxel_size, int32_t contraction, double* out_vertices,
                                             double* out_normals, double* out_colors, int64_t* n_out_vertices_host,
                                             int32_t* out_triangles, int64_t* n_out_triangles_host, void* stream_) {
    static const char* who = "SimplifyVertexClustering";
    hipStream_t stream = S(stream_);
    const int64_t nt = n_triangles, nv = n_vertices;
    if (contraction == 1)
        return fail(OT_ERR_INVALID_ARGUMENT, "[SimplifyVertexClustering] SimplificationContraction.Quadric is not "
                                             "supported by this build (Average only)");
    if (contraction != 0) return fail(OT_ERR_INVALID_ARGUMENT, "[SimplifyVertexClustering] unknown contraction");
    if (!(voxel_size > 0.0)) return fail(OT_ERR_INVALID_ARGUMENT, "[SimplifyVertexClustering] voxel_size <= 0.");
    ot_status st = check_sizes(who, nt, nv);
    if (st != OT_OK) return st;
    if (!n_out_vertices_host || !n_out_triangles_host ||
        (nv > 0 && (!vertices || !out_vertices || (normals && !out_normals) || (colors && !out_colors))) ||
        (nt > 0 && (!triangles || !out_triangles)))
        return fail(OT_ERR_INVALID_ARGUMENT, "[SimplifyVertexClustering] invalid buffers");
    *n_out_vertices_host = 0;
    *n_out_triangles_host = 0;
    st = check_indices(who, triangles, nt, nv, stream);  // (no vertices and a triangle: refused here)
    if (st != OT_OK) return st;
    if (nv == 0) return OT_OK;
    const size_t un = (size_t)nv, unt = (size_t)nt;
    auto [b, kin, kout, vin, vout, heads, seg, rank, row, newidx, flag, mapped, dup, drop] =
        carve(scratch_of(Slot::MF_WS), Arr<Bounds>{1}, Arr<unsigned long long>{un}, Arr<unsigned long long>{un},
              Arr<unsigned>{un}, Arr<unsigned>{un}, Arr<int>{un}, Arr<int>{un}, Arr<int>{un}, Arr<int>{un},
              Arr<int>{un}, Arr<unsigned char>{un}, Arr<int32_t>{3 * unt}, Arr<unsigned char>{unt},
              Arr<unsigned char>{unt});
    if (!b) return fail(OT_ERR_HIP, "scratch allocation failed");
    unsigned long long* part =
        (unsigned long long*)scratch(sizeof(unsigned long long) * BOUNDS_BLOCKS * 6, Slot::MF_BOUNDS_PARTIALS);
    if (!part) return fail(OT_ERR_HIP, "scratch allocation failed");
    launch_bounds(vertices, nv, b, part, stream);
    Bounds hb;
    OT_HIP_TRY(hipMemcpyAsync(&hb, b, sizeof(Bounds), hipMemcpyDeviceToHost, stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));
    const int end_bit = voxel_key_end_bit(hb, voxel_size);
    hipLaunchKernelGGL(k_voxel_keys, blocks_of(nv), dim3(256), 0, stream, vertices, nv, voxel_size, b, kin, vin);
    OT_LAUNCH_CHECK();
    st = sort_pairs_u64_u32(kin, kout, vin, vout, un, end_bit, stream, Slot::SORT_TMP);
    if (st != OT_OK) return st;
    int64_t K = 0;
    st = compact_segments(nv, kout, heads, seg, stream, &K, Slot::MF_COMPACT);  // synchronises
    if (st != OT_OK) return st;
    int err = 0;
    OT_HIP_TRY(hipMemcpyAsync(&err, &b->err, sizeof(int), hipMemcpyDeviceToHost, stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));
    if (err == 1) return fail(OT_ERR_INVALID_ARGUMENT, "[SimplifyVertexClustering] voxel_size is too small.");
    if (err == 2)
        return fail(OT_ERR_INVALID_ARGUMENT, "[SimplifyVertexClustering] voxel grid exceeds 64-bit key packing");
    // first-appearance numbering: the rank of each voxel's smallest old vertex index
    OT_HIP_TRY(hipMemsetAsync(flag, 0, un, stream));
    hipLaunchKernelGGL(k_mf_first, blocks_of(K), dim3(256), 0, stream, (const unsigned*)vout, (const int*)heads, K,
                       flag);
    OT_LAUNCH_CHECK();
    int64_t K2 = 0;
    st = compact(nv, FlagSetPred{flag}, RankEmit{rank}, stream, &K2, Slot::MF_COMPACT);
    if (st != OT_OK) return st;
    if (K2 != K) return fail(OT_ERR_HIP, "[SimplifyVertexClustering] internal error: voxel counts disagree");
    hipLaunchKernelGGL(k_mf_rows, blocks_of(nv), dim3(256), 0, stream, (const unsigned*)vout, (const int*)heads,
                       (const int*)seg, (const int*)rank, nv, row, newidx);
    hipLaunchKernelGGL(k_voxel_reduce, blocks_of(K), dim3(256), 0, stream, vertices, colors, normals,
                       (const unsigned*)vout, (const unsigned long long*)kout, (const int*)heads, K, nv,
                       (const Bounds*)b, voxel_size, out_vertices, out_colors, out_normals, (int32_t*)nullptr,
                       (const int*)row);
    OT_LAUNCH_CHECK();
    int64_t kept = 0;
    if (nt > 0) {
        hipLaunchKernelGGL(k_mf_map_tris, blocks_of(nt), dim3(256), 0, stream, triangles, nt, (const int*)newidx,
                           mapped, drop);
        OT_LAUNCH_CHECK();
        st = flag_duplicated_triangles(mapped, nt, K, dup, stream);
        if (st != OT_OK) return st;
        st = compact(nt, KeepTriPred{dup, drop}, TriRowEmit{mapped, out_triangles}, stream, &kept, Slot::MF_COMPACT);
        if (st != OT_OK) return st;
    }
    OT_HIP_TRY(hipStreamSynchronize(stream));
    *n_out_vertices_host = K;
    *n_out_triangles_host = kept;
    return OT_OK;
}

}  // extern "C"
