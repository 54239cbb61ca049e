// nb_list.h — the canonical neighbour list of a query over the cloud grid: the first k points in ascending
// (d2, index) order, kept sorted and lane-private in LDS.  One text for normals.hip (covariances) and features.hip
// (SPFH / FPFH), so both read the same lists.
//
// Entry p of lane l lives at [p * 64 + l] (conflict-free, no scratch whatever k is).  The lane scans the 3x3x3 block
// of its cell (the precomputed column ranges), then Chebyshev rings of columns, until the k-th entry is provably
// inside the scanned block (block_guard) or, hybrid search, the block provably covers the radius; after NB_RMAX rings,
// or once every point was scanned, the search ends on its own: the lane scans the whole cloud (isolated points only).
// The grid only decides which candidates a query scans, never a result.
#pragma once

#include <cmath>

#include "grid.h"

namespace ot {

constexpr int NB_RMAX = 6;  // rings walked per lane before the whole-cloud scan (speed only, never a result)

// the 3x3 columns of a cell's block, nearest first (t = (dx + 1) * 3 + dy + 1): the k-th distance tightens early, so
// fewer later candidates enter the list only to be pushed out again (the order never changes the list)
static __constant__ unsigned char c_nb_cols3[NBR3] = {4, 1, 3, 5, 7, 0, 2, 6, 8};

// (d, id) sorts before (e, ie)
__device__ inline bool nb_less(double d, unsigned id, double e, unsigned ie) { return d < e || (d == e && id < ie); }

// The lane's list Ld / Li (already offset by the lane; stride 64) holds cnt <= kk entries ascending by (d2, index);
// insert (d, id), dropping the last entry of a full list.
__device__ inline void nb_insert(double* Ld, unsigned* Li, int& cnt, int kk, double d, unsigned id) {
    int p;
    if (cnt < kk) {
        p = cnt++;
    } else {
        p = kk - 1;
        if (!nb_less(d, id, Ld[p * 64], Li[p * 64])) return;
    }
    while (p > 0) {
        const double dp = Ld[(p - 1) * 64];
        const unsigned ip = Li[(p - 1) * 64];
        if (!nb_less(d, id, dp, ip)) break;
        Ld[p * 64] = dp;
        Li[p * 64] = ip;
        --p;
    }
    Ld[p * 64] = d;
    Li[p * 64] = id;
}

// candidates [beg, end) of the sorted points; kth: the last entry's d2 once the list is full, +inf before
__device__ inline void nb_scan(const GridDev& g, const double q[3], int beg, int end, double* Ld, unsigned* Li,
                               int& cnt, int kk, double& kth) {
    for (int m = beg; m < end; ++m) {
        const double d = d2_l2(q, g.sxyz + (int64_t)m * 3);
        if (d > kth) continue;
        nb_insert(Ld, Li, cnt, kk, d, g.sidx[m]);
        if (cnt == kk) kth = Ld[(kk - 1) * 64];
    }
}

// The list of sorted point j of a cloud of n points: its first kk = min(k, n) points by (d2, index) in Ld / Li (the
// lane's columns of two [>= kk][64] LDS arrays).  r2 <= 0: KNN; r2 > 0: hybrid (of the first kk, the ones with
// d2 < r2).  Returns the length of the list.
__device__ inline int nb_search(const GridDev& g, int64_t n, int64_t j, int kk, double r2, double* Ld, unsigned* Li) {
    const double q[3] = {g.sxyz[j * 3], g.sxyz[j * 3 + 1], g.sxyz[j * 3 + 2]};
    int cc[3];
    query_cell(g, j, cc[0], cc[1], cc[2]);
    int cnt = 0;
    double kth = INFINITY;
    long long have = 0;  // points scanned: every cell of the block exactly once
    const int2* r3 = g.nbr3 + (int64_t)g.pcell[j] * NBR3;
    for (int u = 0; u < NBR3; ++u) {
        const int2 se = r3[c_nb_cols3[u]];
        nb_scan(g, q, se.x, se.y, Ld, Li, cnt, kk, kth);
        have += se.y - se.x;
    }
    for (int r = 1; have < n; ++r) {
        // every point outside the (2r+1)^3 block is farther than guard (margins: block_guard), so it sorts after
        // the k-th entry, or lies outside the radius
        const double guard = block_guard(g, q, g.origin, cc, (double)r);
        if (guard > 0.0) {
            const double g2 = guard * guard;
            if (kth < g2 || (r2 > 0.0 && g2 >= r2)) break;
        }
        if (r >= NB_RMAX) {  // an isolated query: the whole cloud from scratch
            cnt = 0;
            kth = INFINITY;
            nb_scan(g, q, 0, (int)n, Ld, Li, cnt, kk, kth);
            break;
        }
        const int R = r + 1;  // ring R: border columns over z-R .. z+R, inner columns their two end cells
        for (int dx = -R; dx <= R; ++dx)
            for (int dy = -R; dy <= R; ++dy) {
                const int2 col = grid_column(g, 0, cc[0] + dx, cc[1] + dy);
                if (col.y == 0) continue;
                if (dx == -R || dx == R || dy == -R || dy == R) {
                    const int2 se = column_range(g, col, cc[2] - R, cc[2] + R);
                    nb_scan(g, q, se.x, se.y, Ld, Li, cnt, kk, kth);
                    have += se.y - se.x;
                } else {
                    const int2 a = column_range(g, col, cc[2] - R, cc[2] - R);
                    const int2 b = column_range(g, col, cc[2] + R, cc[2] + R);
                    nb_scan(g, q, a.x, a.y, Ld, Li, cnt, kk, kth);
                    nb_scan(g, q, b.x, b.y, Ld, Li, cnt, kk, kth);
                    have += (a.y - a.x) + (b.y - b.x);
                }
            }
    }
    int m = cnt;
    if (r2 > 0.0) {
        m = 0;
        while (m < cnt && Ld[m * 64] < r2) ++m;
    }
    return m;
}

}  // namespace ot
