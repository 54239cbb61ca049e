// grid.h — the multi-frame neighbour grid (built by grid.hip) under SOR, ROR, cloud distance, DBSCAN, normals, ICP and
// the batch filter.
//
// A cloud of n points grouped in F frames (frame f = point indices [foff[f], foff[f+1])) is binned into cubic cells
// of size h anchored at a per-frame origin.  Keys pack (frame, x, y, z) with z in the low bits, so a frame's points
// stay one contiguous range of the sorted order and cells (x', y', z-R .. z+R) of one frame are ONE contiguous range
// whichever of them are occupied.  The hash is over COLUMNS (frame, x, y) -> the column's run of occupied cells in
// the sorted cell list, so any z-range of a column costs one probe plus a short scan of the column's cells.  Per
// occupied cell the 3x3 (and optionally 5x5) column ranges of its block are precomputed.  The grid only decides
// which candidates a query scans, never a result.
#pragma once

#include "common.h"

namespace ot {

constexpr int NBR3 = 9;   // 3x3 columns, z-1 .. z+1
constexpr int NBR5 = 25;  // 5x5 columns, z-2 .. z+2

// ROR (outlier.hip): cells are this factor wider than the radius.  A point's cell is floor((v - origin) / h) with the
// subtraction and the division each rounded, so the computed cell quotients of two points d apart differ from d / h by
// up to 2^-31 (each quotient is below 2^20 cells and carries two roundings of 2^-53 relative).  With h = radius
// exactly, a pair a hair under the radius apart can land in cells that differ by 2 and the 3x3x3 block never meets
// it (tests/test_gpu_ror_edges.py builds such pairs); with d / h <= 1 - 2^-21 it cannot.  Only the candidate set
// grows: counts and kept indices are unchanged wherever no neighbour was missed.
constexpr double ROR_CELL_SCALE = 1.0 + 1.0 / (double)(1 << 20);

// neighbour structures a grid build can precompute (bit mask)
enum { GRID_NBR3 = 1, GRID_NBR5 = 2 };

struct GridDev {
    const double* sxyz;        // [n][3] points in sorted (frame, cell) order
    const unsigned* sidx;      // sorted position -> point index (nullptr: the identity, a presorted cloud)
    const unsigned long long* pkey;  // sorted position -> its cell key (the cell a query's guards are measured from)
    const int* pcell;          // sorted position -> cell (position in the sorted cell list)
    const int2* nbr3;          // per cell: NBR3 column ranges
    const int2* nbr5;          // per cell: NBR5 column ranges (nullptr unless built)
    unsigned long long* hkeys; // column hash: keys (cell key >> sy; KEY_EMPTY = free)
    int2* hval;                // column hash: {first cell, number of cells} (cells sorted by z inside a column)
    int hash_mask;
    int2* crange;              // per cell: [start, end) in the sorted order
    int* cz;                   // per cell: z
    int dim[3];                // cells per axis (every frame's cells lie in [0, dim))
    int sy, sx, sf;            // key = f << sf | x << sx | y << sy | z
    const double* origin;      // [F][3] per-frame grid origins (device)
    const int* foff;           // [F + 1] frame offsets (device; the same in input and sorted order)
    int nframes;
    double h;
};

struct GridBuild {
    GridDev g;
    int64_t ncells = 0;
};

// ---- device lookups ----------------------------------------------------------------------------------------------
__device__ inline int cell_coord(double v, double origin, double h) { return (int)floor((v - origin) / h); }

__device__ inline bool cell_valid(const GridDev& g, int x, int y, int z) {
    return x >= 0 && x < g.dim[0] && y >= 0 && y < g.dim[1] && z >= 0 && z < g.dim[2];
}
__device__ inline unsigned long long cell_key(const GridDev& g, int f, int x, int y, int z) {
    return ((unsigned long long)f << g.sf) | ((unsigned long long)x << g.sx) | ((unsigned long long)y << g.sy) |
           (unsigned long long)z;
}

__device__ inline int2 grid_probe(const GridDev& g, unsigned long long key, unsigned slot) {
    for (int probe = 0; probe <= g.hash_mask; ++probe) {
        const unsigned long long k = g.hkeys[slot];
        if (k == key) return g.hval[slot];
        if (k == KEY_EMPTY) return make_int2(0, 0);
        slot = (slot + 1) & (unsigned)g.hash_mask;
    }
    return make_int2(0, 0);
}

// the occupied cells of column (f, x, y): {first cell, count}
__device__ inline int2 grid_column(const GridDev& g, int f, int x, int y) {
    if (x < 0 || x >= g.dim[0] || y < 0 || y >= g.dim[1]) return make_int2(0, 0);
    const unsigned long long key = cell_key(g, f, x, y, 0) >> g.sy;
    return grid_probe(g, key, (unsigned)mix64(key) & (unsigned)g.hash_mask);
}

// points of the column's cells with zlo <= z <= zhi: one contiguous range of the sorted order (or empty)
__device__ inline int2 column_range(const GridDev& g, int2 col, int zlo, int zhi) {
    int b = 0, e = 0;
    bool any = false;
    int i0 = 0;
    if (col.y > 8) {  // tall column (a wall seen edge-on): bisect for the first cell with z >= zlo
        int lo = -1, hi = col.y;  // cz[lo] < zlo <= cz[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (g.cz[col.x + mid] < zlo) lo = mid;
            else hi = mid;
        }
        i0 = hi;
    }
    for (int i = i0; i < col.y; ++i) {
        const int z = g.cz[col.x + i];
        if (z > zhi) break;
        if (z >= zlo) {
            const int2 r = g.crange[col.x + i];
            if (!any) b = r.x;
            e = r.y;
            any = true;
        }
    }
    return any ? make_int2(b, e) : make_int2(0, 0);
}

__device__ inline int2 grid_find(const GridDev& g, int f, int x, int y, int z) {
    return column_range(g, grid_column(g, f, x, y), z, z);
}


__device__ inline double d2_l2(const double* q, const double* p) {
    const double d0 = q[0] - p[0], d1 = q[1] - p[1], d2 = q[2] - p[2];
    return ((d0 * d0) + d1 * d1) + d2 * d2;
}

// the cell the grid assigned to sorted point j (its key): SOR measures every guard from this cell's faces, so a
// point the rounding of its coordinates puts a hair outside its cell still gets correct (conservative) bounds
__device__ inline void query_cell(const GridDev& g, int64_t j, int& cx, int& cy, int& cz) {
    const unsigned long long key = g.pkey[j];
    cz = (int)(key & ((1ull << g.sy) - 1));
    cy = (int)((key >> g.sy) & ((1ull << (g.sx - g.sy)) - 1));
    cx = (int)((key >> g.sx) & ((1ull << (g.sf - g.sx)) - 1));
}

// distance from q to the faces of the (2R+1)^3 cell block around cell c, minus a rounding margin (f = q's position
// inside c: in [0, 1) up to rounding; outside it the formula is still q's distance to the block's faces)
__device__ inline double block_guard(const GridDev& g, const double q[3], const double* o, const int c[3], double R) {
    double guard = (R + 1.0) * g.h;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double u = (q[a] - o[a]) / g.h;
        const double f = u - (double)c[a];
        guard = fmin(guard, fmin(R + f, R + 1.0 - f) * g.h);
    }
    return guard - 1e-6 * g.h;
}

// Build the grid of n points (xyz device [n][3]) grouped in nframes frames.  d_foff / d_origin: device arrays
// ([F+1] ints, [F][3] doubles) that must outlive the grid; dims: cells per axis covering every frame; nbr: the
// GRID_* structures to precompute; h_foff (optional host copy of the frame offsets, <= 64 frames): the cell sort
// runs per frame (segmented, cell bits only) instead of over frame-prefixed keys.  Synchronises (cell count).
ot_status build_grid_frames(const double* xyz, int64_t n, int nframes, const int* d_foff, const double* d_origin,
                            double h, const int dims[3], int nbr, hipStream_t stream, GridBuild& out,
                            const GridSlots& slots, const int* h_foff = nullptr);

// The grid of a cloud already in cell order (filter_batch.hip: voxels sorted by cell-major keys): ckeys[i] = point i's
// cell key (frame << (bits[0] + bits[1] + bits[2]) | x << (bits[1] + bits[2]) | y << bits[2] | z, non-decreasing),
// cells of edge h at the per-frame origins; no sort, no copy (the grid reads xyz in place).  Synchronises (cell
// count).
ot_status build_grid_sorted(const double* xyz, const unsigned long long* ckeys, int64_t n, int nframes,
                            const int* d_foff, const double* d_origin, double h, const int bits[3], int nbr,
                            hipStream_t stream, GridBuild& out, const GridSlots& slots);

// per-axis bounds of a device cloud on the host.  Synchronises.
ot_status bounds_host(const double* xyz, int64_t n, hipStream_t stream, double mn[3], double mx[3]);

// one frame: origin = the cloud's minimum corner, cells per axis from the extent (the cloud grid's buffers)
ot_status single_frame_grid(const double* xyz, int64_t n, double h, const double mn[3], const double mx[3], int nbr,
                            hipStream_t stream, GridBuild& gb);

// The single-frame grid of a cloud (n > 0) with cells sized for ~target points per occupied cell of a surface-like
// cloud, rebuilt once from the measured occupancy when that is off by more than 2.5x; mn / mx receive the cloud's
// bounds.  The grid only changes speed, never a result.  Synchronises.
ot_status occupancy_grid(const double* xyz, int64_t n, double target, int nbr, double mn[3], double mx[3],
                         hipStream_t stream, GridBuild& gb);

// The grid a cross-cloud nearest-neighbour search runs over (ComputePointCloudDistance, registration): ~4 target
// points per occupied cell.
inline ot_status nn_target_grid(const double* tgt, int64_t m, int nbr, hipStream_t stream, double mn[3], double mx[3],
                                GridBuild& gb) {
    return occupancy_grid(tgt, m, 4.0, nbr, mn, mx, stream, gb);
}

}  // namespace ot
