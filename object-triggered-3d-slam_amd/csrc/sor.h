// sor.h — statistical outlier removal over a built neighbour grid (outlier.hip), for single clouds and for the batch
// filter's frame batches (filter_batch.hip).
#pragma once

#include "grid.h"

namespace ot {

// SOR (outlier.hip): radius (in cells) of the block a query scans first, and the matching cell occupancy target
// (points per occupied cell of a surface-like cloud); both only change speed, never a result.  Measured and settled
// (DESIGN.md §4): R = 2 with finer cells, occupancies 0.6-1.3 k, precomputed 5x5 ranges for stage 2 -- all slower.
constexpr int SOR_BLOCK_R = 1;
inline double sor_cell_target(int nb_neighbors) {
    const double t = 0.9 * (double)nb_neighbors;
    return t > 2.0 ? t : 2.0;
}

constexpr int SOR_GRID_NBR = GRID_NBR3;

// Statistical outlier removal over a built grid (Open3D RemoveStatisticalOutliers per frame):
// avg[i] = mean kNN distance of point i (-1 when none); per frame the cloud mean and squared-deviation sum are
// Open3D's sequential float64 accumulations (exact chains), stats[f] = {mean, std, valid, threshold}.
// h_foff: host copy of the frame offsets.  Synchronises once (job table).
ot_status sor_frames(const GridBuild& gb, int64_t n, const int* h_foff, int nb_neighbors, double std_ratio,
                     double* avg, double* stats, hipStream_t stream, const SorSlots& slots);

// The statistics half of sor_frames: from the mean kNN distances avg[0 .. n) (frame-major, d_foff / h_foff: device /
// host frame offsets) to stats[f] = {mean, std, valid, threshold}.  Synchronises once.
ot_status sor_stats_frames(const double* avg, const int* d_foff, const int* h_foff, int F, double std_ratio,
                           double* stats, hipStream_t stream, Slot slot);

// keep predicate of frame f's points: avg > 0 && avg < stats[f].threshold
struct SorKeep {
    const double* avg;
    const double* stats;  // [F][4]
    const int* foff;
    int nframes;
    __device__ inline bool operator()(int64_t i) const {
        int lo = 0, hi = nframes;
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (foff[mid] <= i) lo = mid;
            else hi = mid;
        }
        const double a = avg[i];
        return a > 0 && a < stats[lo * 4 + 3];
    }
};

}  // namespace ot
