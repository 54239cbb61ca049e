// tsdf_fused.hip — a deferred batch's integrate and the next batch's touch in one launch (k_integrate_touch,
// k_integrate_touch_fine): the one translation unit that holds both the touch's and the integrate's device text.
#include "tsdf_integrate.h"
#include "tsdf_touch.h"

namespace ot {

// The deferred integrate of a sharded volume's batch k and the touch of batch k + 1 in ONE launch (round 6): workgroups
// [0, nint) integrate batch k (its set's staging and work list), the rest are batch k + 1's touch tiles (frame groups
// along the grid).  A rank's integrate fills few of the CUs (a shard's batch is a few hundred units), so its latency-bound
// touch runs in the gaps, with no second stream and no event between them (two streams' fork + join cost ~25 us of idle
// GPU per batch: the double-buffered front end).  The touch writes only batch k + 1's state: its frame
// masks / slot list / pair counter, hash inserts of its units, and the staged pixels of its samples in its own set --
// nothing the integrate of batch k reads.  LDS: the touch's tables and the reciprocal table share one block.
// The IEEE-division float64 integrate needs 67 VGPRs: it takes the 5-wave bound k_batch_integrate gives it (under the
// 8-wave bound it spilled 20-32 B inside the frame loop; per launch the two measure the same).
template <bool C64, bool FAST>
__global__ __launch_bounds__(64 * INT_WG, (C64 && !FAST) ? 5 : INT_WAVES_PER_EU) void k_integrate_touch(
    const BatchFrame* __restrict__ frames, IntegrateParams p, TsdfDev d, const UnitWork* __restrict__ work,
    const int* __restrict__ wcount, int nint, const BatchFrame* __restrict__ tframes, BatchTouchParams tp, int tn) {
    union Lds {
        TouchLds t;
        RcpLds<C64, FAST> r;
    };
    __shared__ Lds lds;
    const int b = (int)blockIdx.x;
    if (b < nint) {
        integrate_body<C64, FAST, BZ, 1, true, INT_WG>(frames, p, d, work, wcount, lds.r.r32, lds.r.r64, b, nint);
    } else {
        const int t = b - nint;
        touch_body<false, false>(tframes, tp, d, tn, lds.t, t % tp.tiles, t / tp.tiles);
    }
}
// The same launch with the integrate in fine slices (2 voxels per lane along z, k_batch_integrate<.., 2, 1>'s per-voxel
// code and occupancy): the deferred batch's unit count is known on the host by then (its units kernel mailed it), so a
// batch of few units takes the fine slices without the guess the direct path makes from the previous batch
template <bool C64, bool FAST>
__global__ __launch_bounds__(64 * INT_WG, (C64 && !FAST) ? 5 : 4) void k_integrate_touch_fine(
    const BatchFrame* __restrict__ frames, IntegrateParams p, TsdfDev d, const UnitWork* __restrict__ work,
    const int* __restrict__ wcount, int nint, const BatchFrame* __restrict__ tframes, BatchTouchParams tp, int tn) {
    union Lds {
        TouchLds t;
        RcpLds<C64, FAST> r;
    };
    __shared__ Lds lds;
    const int b = (int)blockIdx.x;
    if (b < nint) {
        integrate_body<C64, FAST, 2, 1, true, INT_WG>(frames, p, d, work, wcount, lds.r.r32, lds.r.r64, b, nint);
    } else {
        const int t = b - nint;
        touch_body<false, false>(tframes, tp, d, tn, lds.t, t % tp.tiles, t / tp.tiles);
    }
}

hipError_t launch_integrate_touch(IntegrateForm form, const BatchFrame* frames, const IntegrateParams& p,
                                  const TsdfDev& dev, const UnitWork* work, const int* wcount, int nint,
                                  const BatchFrame* tframes, const BatchTouchParams& tp, int tn, hipStream_t stream) {
    static const void* const k[2][2][2] = {
        {{(const void*)k_integrate_touch<false, false>, (const void*)k_integrate_touch<false, true>},
         {(const void*)k_integrate_touch<true, false>, (const void*)k_integrate_touch<true, true>}},
        {{(const void*)k_integrate_touch_fine<false, false>, (const void*)k_integrate_touch_fine<false, true>},
         {(const void*)k_integrate_touch_fine<true, false>, (const void*)k_integrate_touch_fine<true, true>}}};
    void* args[] = {(void*)&frames, (void*)&p, (void*)&dev, (void*)&work, (void*)&wcount, (void*)&nint,
                    (void*)&tframes, (void*)&tp, (void*)&tn};
    const unsigned grid = (unsigned)nint + (unsigned)tp.tiles * (unsigned)((tn + tp.tf - 1) / tp.tf);
    return hipLaunchKernel(k[form.fine][form.c64][form.fast], dim3(grid), dim3(64 * INT_WG), args, 0, stream);
}

}  // namespace ot
