// grid.hip — builders of the neighbour grid (grid.h) that SOR, ROR, cloud distance (outlier.hip), DBSCAN
// (cluster.hip), normals (normals.hip), ICP (icp.hip) and the batch filter (filter_batch.hip) search.
//
//   build : (frame, cell) key per point -> stable radix sort -> cell heads -> open-addressing hash over columns
//           (column key -> its run of occupied cells) -> per cell the z-column ranges of its 3x3 / 5x5 block; points
//           are re-laid out in sorted order so a cell's points are contiguous in HBM.  A cloud that arrives in cell
//           order (build_grid_sorted) skips the sort and the copy.
#include <algorithm>
#include <cmath>
#include <vector>

#include "compact.h"
#include "grid.h"
#include "sort.h"

namespace ot {

template <typename KeyT>
__global__ __launch_bounds__(256) void k_cell_keys(const double* __restrict__ xyz, int64_t n, GridDev g, KeyT* keys,
                                                   unsigned* idx, int* err) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int f = g.nframes > 1 ? frame_of(g.foff, g.nframes, i) : 0;
    const double* o = g.origin + 3 * f;
    const int x = cell_coord(xyz[i * 3 + 0], o[0], g.h);
    const int y = cell_coord(xyz[i * 3 + 1], o[1], g.h);
    const int z = cell_coord(xyz[i * 3 + 2], o[2], g.h);
    const bool ok = cell_valid(g, x, y, z);
    if (!ok) *err = 1;
    keys[i] = ok ? (KeyT)cell_key(g, f, x, y, z) : (KeyT)0;
    idx[i] = (unsigned)i;
}

__global__ __launch_bounds__(256) void k_widen_keys(const unsigned* __restrict__ in, int64_t n,
                                                    unsigned long long* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = in[i];
}

// per occupied cell: its range and z; a column's first cell also inserts the column (its run of cells) into the hash
__global__ __launch_bounds__(256) void k_grid_insert(const unsigned long long* __restrict__ skeys,
                                                     const int* __restrict__ heads, int64_t ncells, int64_t n,
                                                     GridDev g) {
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncells) return;
    const int beg = heads[c];
    const int end = (c + 1 < ncells) ? heads[c + 1] : (int)n;
    const unsigned long long key = skeys[beg];
    g.crange[c] = make_int2(beg, end);
    g.cz[c] = (int)(key & ((1ull << g.sy) - 1));
    const unsigned long long col = key >> g.sy;
    if (c > 0 && (skeys[heads[c - 1]] >> g.sy) == col) return;
    // the column's cells are contiguous (cell-major keys): its end by galloping, then bisection -- a wall's column
    // holds dozens of cells, and a probe is two dependent loads
    int64_t lo = c, hi = ncells, step = 1;
    while (true) {
        const int64_t p = c + step;
        if (p >= ncells) break;
        if ((skeys[heads[p]] >> g.sy) != col) {
            hi = p;
            break;
        }
        lo = p;
        step <<= 1;
    }
    while (hi - lo > 1) {  // colkey(lo) == col; hi == ncells or colkey(hi) != col
        const int64_t mid = (lo + hi) >> 1;
        if ((skeys[heads[mid]] >> g.sy) == col) lo = mid;
        else hi = mid;
    }
    const int cnt = (int)(hi - c);
    unsigned slot = (unsigned)mix64(col) & (unsigned)g.hash_mask;
    while (true) {  // capacity >= 2 * ncells >= 2 * columns: always terminates
        const unsigned long long old = atomicCAS(&g.hkeys[slot], KEY_EMPTY, col);
        if (old == KEY_EMPTY) {
            g.hval[slot] = make_int2((int)c, cnt);
            return;
        }
        slot = (slot + 1) & (unsigned)g.hash_mask;
    }
}

// One lane per (cell, column of its (2R+1)^2 neighbourhood): one column probe, then the column's cells in
// z-R..z+R (and, R = 2, z-1..z+1 for the inner 3x3 columns) as contiguous point ranges.
template <int R>
__global__ __launch_bounds__(256) void k_cell_nbr(const unsigned long long* __restrict__ skeys,
                                                  const int* __restrict__ heads, int64_t ncells, GridDev g,
                                                  int2* __restrict__ nbr3, int2* __restrict__ nbr5) {
    constexpr int W = 2 * R + 1, COLS = W * W;
    const int64_t gid = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (gid >= ncells * COLS) return;
    const int64_t c = gid / COLS;
    const int t = (int)(gid - c * COLS);
    const int dx = t / W - R, dy = t % W - R;
    const unsigned long long key = skeys[heads[c]];
    const int f = (int)(key >> g.sf);
    const int z = (int)(key & ((1ull << g.sy) - 1));
    const int y = (int)((key >> g.sy) & ((1ull << (g.sx - g.sy)) - 1)) + dy;
    const int x = (int)((key >> g.sx) & ((1ull << (g.sf - g.sx)) - 1)) + dx;
    const int2 col = grid_column(g, f, x, y);
    if (R == 2) nbr5[c * NBR5 + t] = column_range(g, col, z - 2, z + 2);
    if (nbr3 && dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1)
        nbr3[c * NBR3 + (dx + 1) * 3 + (dy + 1)] = column_range(g, col, z - 1, z + 1);
}

__global__ __launch_bounds__(256) void k_gather_sorted(const double* __restrict__ xyz, const unsigned* __restrict__ sidx,
                                                       int64_t n, double* __restrict__ sxyz) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n * 3) return;
    const int64_t j = t / 3, a = t % 3;
    sxyz[t] = xyz[(int64_t)sidx[j] * 3 + a];
}

// ------------------------------------------------------------------------------------ builders (host)
// The tail both builders share: the column hash and the per-cell tables over the sorted cell list (skeys[heads[c]]
// = cell c's key, pcell: point -> cell).  No cells, no launches: a launch of zero blocks is an error, and only
// build_grid_sorted meets it (a batch whose frames are all empty) -- build_grid_frames' callers pass n >= 1, which
// has a cell.
static ot_status build_cells(const unsigned long long* skeys, const int* heads, const int* pcell, int64_t ncells,
                             int64_t n, int nbr, hipStream_t stream, GridBuild& out, Slot slot) {
    GridDev& g = out.g;
    int64_t cap = 1;
    while (cap < 2 * ncells + 2) cap <<= 1;
    const bool w3 = nbr & GRID_NBR3, w5 = nbr & GRID_NBR5;
    auto [hkeys, hval, n3, n5, crange, cz] = grid_cells_ws(scratch_of(slot), (size_t)cap, (size_t)ncells, w3, w5);
    if (!hkeys) return fail(OT_ERR_HIP, "scratch allocation failed");
    g.hkeys = hkeys;
    g.hval = (int2*)hval;
    int2 *nbr3 = w3 ? (int2*)n3 : nullptr, *nbr5 = w5 ? (int2*)n5 : nullptr;
    g.crange = (int2*)crange;
    g.cz = cz;
    g.hash_mask = (int)(cap - 1);
    OT_HIP_TRY(hipMemsetAsync(g.hkeys, 0xFF, sizeof(unsigned long long) * cap, stream));
    if (ncells > 0) {
        hipLaunchKernelGGL(k_grid_insert, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, stream, skeys, heads,
                           ncells, n, g);  // cell ranges / z and the column hash, read by k_cell_nbr
        if (w5)
            hipLaunchKernelGGL(k_cell_nbr<2>, dim3((unsigned)((ncells * NBR5 + 255) / 256)), dim3(256), 0, stream,
                               skeys, heads, ncells, g, nbr3, nbr5);
        else if (w3)
            hipLaunchKernelGGL(k_cell_nbr<1>, dim3((unsigned)((ncells * NBR3 + 255) / 256)), dim3(256), 0, stream,
                               skeys, heads, ncells, g, nbr3, nbr5);
        OT_LAUNCH_CHECK();
    }
    g.pkey = skeys;
    g.pcell = pcell;
    g.nbr3 = nbr3;  // (set after the launches: the kernels take the tables as arguments of their own)
    g.nbr5 = nbr5;
    out.ncells = ncells;
    return OT_OK;
}

ot_status build_grid_frames(const double* xyz, int64_t n, int nframes, const int* d_foff, const double* d_origin,
                            double h, const int dims[3], int nbr, hipStream_t stream, GridBuild& out,
                            const GridSlots& slots, const int* h_foff) {
    GridDev& g = out.g;
    g.h = h;
    g.origin = d_origin;
    g.foff = d_foff;
    g.nframes = nframes;
    int bits[3];
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < 1 || dims[a] > 1000000)
            return fail(OT_ERR_INVALID_ARGUMENT, "neighbour grid out of range (radius too small for the extent)");
        g.dim[a] = dims[a];
        bits[a] = bits_for(g.dim[a] - 1);
    }
    g.sy = bits[2];
    g.sx = bits[1] + bits[2];
    g.sf = bits[0] + bits[1] + bits[2];
    const int end_bit = g.sf + (nframes > 1 ? bits_for(nframes - 1) : 0);
    if (end_bit > 64) return fail(OT_ERR_INVALID_ARGUMENT, "neighbour grid keys exceed 64 bits");
    auto [err, kin, kout, vin, vout, heads, pcell, sxyz] = grid_points_ws(scratch_of(slots.points), (size_t)n);
    if (!err) return fail(OT_ERR_HIP, "scratch allocation failed");
    OT_HIP_TRY(hipMemsetAsync(err, 0, sizeof(int), stream));
    ot_status st;
    if (end_bit <= 32 && n > (int64_t)(1 << 21)) {  // large sorts on 32-bit keys: 8 B per pair per pass, not 12
        unsigned* k32 = (unsigned*)kin;  // aliased on purpose: both 32-bit key arrays live in kin's 8 n bytes
        unsigned* k32o = k32 + n;
        hipLaunchKernelGGL(k_cell_keys<unsigned>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, xyz, n, g,
                           k32, vin, err);
        OT_LAUNCH_CHECK();
        if (h_foff && nframes > 1 && nframes <= 64) {  // frames are contiguous: sort each on its cell bits alone
            std::vector<int64_t> seg((size_t)nframes + 1);
            for (int f = 0; f <= nframes; ++f) seg[f] = h_foff[f];
            st = sort_segments_u32_u32(k32, k32o, vin, vout, seg.data(), nframes, std::max(g.sf, 1), stream,
                                       Slot::SORT_TMP);
        } else {
            st = sort_pairs_u32_u32(k32, k32o, vin, vout, (size_t)n, std::max(end_bit, 1), stream, Slot::SORT_TMP);
        }
        if (st != OT_OK) return st;
        hipLaunchKernelGGL(k_widen_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, (const unsigned*)k32o,
                           n, kout);
    } else {
        hipLaunchKernelGGL(k_cell_keys<unsigned long long>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream,
                           xyz, n, g, kin, vin, err);
        OT_LAUNCH_CHECK();
        st = sort_pairs_u64_u32(kin, kout, vin, vout, (size_t)n, std::max(end_bit, 1), stream, Slot::SORT_TMP);
        if (st != OT_OK) return st;
    }
    int64_t ncells = 0;
    st = compact_segments(n, kout, heads, pcell, stream, &ncells, slots.compact);  // synchronises
    if (st != OT_OK) return st;
    int e = 0;
    OT_HIP_TRY(hipMemcpyAsync(&e, err, sizeof(int), hipMemcpyDeviceToHost, stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));
    if (e) return fail(OT_ERR_INVALID_ARGUMENT, "neighbour grid out of range (non-finite point coordinates)");
    st = build_cells(kout, heads, pcell, ncells, n, nbr, stream, out, slots.cells);
    if (st != OT_OK) return st;
    hipLaunchKernelGGL(k_gather_sorted, dim3((unsigned)((n * 3 + 255) / 256)), dim3(256), 0, stream, xyz, vout, n,
                       sxyz);
    OT_LAUNCH_CHECK();
    g.sxyz = sxyz;
    g.sidx = vout;
    return OT_OK;
}

ot_status build_grid_sorted(const double* xyz, const unsigned long long* ckeys, int64_t n, int nframes,
                            const int* d_foff, const double* d_origin, double h, const int bits[3], int nbr,
                            hipStream_t stream, GridBuild& out, const GridSlots& slots) {
    GridDev& g = out.g;
    g.h = h;
    g.origin = d_origin;
    g.foff = d_foff;
    g.nframes = nframes;
    for (int a = 0; a < 3; ++a) {
        if (bits[a] < 0 || bits[a] > 20)
            return fail(OT_ERR_INVALID_ARGUMENT, "neighbour grid out of range (radius too small for the extent)");
        g.dim[a] = 1 << bits[a];
    }
    g.sy = bits[2];
    g.sx = bits[1] + bits[2];
    g.sf = bits[0] + bits[1] + bits[2];
    auto [heads, pcell] = carve(scratch_of(slots.points), Arr<int>{(size_t)n}, Arr<int>{(size_t)n});
    if (!heads) return fail(OT_ERR_HIP, "scratch allocation failed");
    int64_t ncells = 0;
    ot_status st = compact_segments(n, ckeys, heads, pcell, stream, &ncells, slots.compact);  // synchronises
    if (st != OT_OK) return st;
    st = build_cells(ckeys, heads, pcell, ncells, n, nbr, stream, out, slots.cells);
    g.sxyz = xyz;  // the grid reads the cloud in place
    g.sidx = nullptr;
    return st;
}

ot_status bounds_host(const double* xyz, int64_t n, hipStream_t stream, double mn[3], double mx[3]) {
    Bounds* b = (Bounds*)scratch(sizeof(Bounds) + 64, Slot::BOUNDS);
    if (!b) return fail(OT_ERR_HIP, "scratch allocation failed");
    unsigned long long* part =
        (unsigned long long*)scratch(sizeof(unsigned long long) * BOUNDS_BLOCKS * 6, Slot::BOUNDS_PARTIALS);
    if (!part) return fail(OT_ERR_HIP, "scratch allocation failed");
    launch_bounds(xyz, n, b, part, stream);
    OT_LAUNCH_CHECK();
    Bounds hb;
    OT_HIP_TRY(hipMemcpyAsync(&hb, b, sizeof(Bounds), hipMemcpyDeviceToHost, stream));
    OT_HIP_TRY(hipStreamSynchronize(stream));
    for (int a = 0; a < 3; ++a) {
        mn[a] = ordered_to_dbl(hb.mn[a]);
        mx[a] = ordered_to_dbl(hb.mx[a]);
    }
    return OT_OK;
}

ot_status single_frame_grid(const double* xyz, int64_t n, double h, const double mn[3], const double mx[3], int nbr,
                            hipStream_t stream, GridBuild& gb) {
    int dims[3];
    for (int a = 0; a < 3; ++a) {
        const double span = std::floor((mx[a] - mn[a]) / h);
        if (!(span < 1.0e6))
            return fail(OT_ERR_INVALID_ARGUMENT, "neighbour grid out of range (radius too small for the extent)");
        dims[a] = (int)span + 1;
    }
    char* fr = (char*)scratch(64, Slot::CLOUD_FRAME);  // the device origin [3] and offsets {0, n}
    if (!fr) return fail(OT_ERR_HIP, "scratch allocation failed");
    const double org[4] = {mn[0], mn[1], mn[2], 0.0};
    const int off[2] = {0, (int)n};
    OT_HIP_TRY(hipMemcpyAsync(fr, org, sizeof(org), hipMemcpyHostToDevice, stream));
    OT_HIP_TRY(hipMemcpyAsync(fr + 32, off, sizeof(off), hipMemcpyHostToDevice, stream));
    // build_grid_frames synchronises the stream before returning, so org / off outlive their copies
    return build_grid_frames(xyz, n, 1, (const int*)(fr + 32), (const double*)fr, h, dims, nbr, stream, gb,
                             CLOUD_GRID_SLOTS);
}

ot_status occupancy_grid(const double* xyz, int64_t n, double target, int nbr, double mn[3], double mx[3],
                         hipStream_t stream, GridBuild& gb) {
    ot_status st = bounds_host(xyz, n, stream, mn, mx);
    if (st != OT_OK) return st;
    // First guess: the points cover half of the bounding box's largest face; refined once from the measured
    // occupancy (2-D scaling) when it is off by more than 2.5x.
    double ext[3];
    for (int a = 0; a < 3; ++a) ext[a] = std::max(mx[a] - mn[a], 1e-9);
    std::sort(ext, ext + 3);
    const double hmin = ext[2] / 5.0e5;
    double h = std::max(std::sqrt(0.5 * ext[2] * ext[1] * target / (double)n), hmin);
    st = single_frame_grid(xyz, n, h, mn, mx, nbr, stream, gb);
    if (st != OT_OK) return st;
    const double occ = (double)n / (double)std::max<int64_t>(gb.ncells, 1);
    if (occ > 2.5 * target || occ < 0.4 * target) {
        h = std::max(h * std::sqrt(target / occ), hmin);
        st = single_frame_grid(xyz, n, h, mn, mx, nbr, stream, gb);
    }
    return st;
}

}  // namespace ot
