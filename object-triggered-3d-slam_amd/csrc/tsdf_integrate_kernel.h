// tsdf_integrate_kernel.h — k_batch_integrate and the table of its forms for one count of mask words.  Included by
// tsdf_integrate.hip (one word) and tsdf_integrate_wide.hip (FMASK_WORDS) alone: each instantiates its half of the forms.
#pragma once

#include "tsdf_integrate.h"

namespace ot {

// the integrate of a batch as a launch of its own (the product kernel: <C64, FAST, BZ, 1, 1>; ZB == 2: fine slices).
// The reciprocal table is the launch's dynamic LDS: rcp_hi + 1 entries of the kernel's precision (integrate_form), so a
// CU holds as many one-wave workgroups as it has wave slots until the table passes 5 KiB.
extern __shared__ double s_rcp_dyn[];
// WORDS: the batch's mask words (2 only for a batch of more than WORD_FRAMES frames: integrate_form)
template <bool C64, bool FAST, int ZB = BZ, int KT = 1, int WG = INT_WG, int WORDS = 1>
__global__ __launch_bounds__(64 * WG, (C64 && !FAST) ? 5 : (ZB == 2 ? 4 : INT_WAVES_PER_EU)) void k_batch_integrate(
    const BatchFrame* __restrict__ frames, IntegrateParams p, TsdfDev d, const UnitWork* __restrict__ work,
    const int* __restrict__ wcount) {
    integrate_body<C64, FAST, ZB, KT, false, WG, ZB == BZ, WORDS>(frames, p, d, work, wcount,
                                                                  reinterpret_cast<float*>(s_rcp_dyn), s_rcp_dyn,
                                                                  (int)blockIdx.x, (int)gridDim.x);
}

template <int ZB, int KT, int WG, int WORDS>
static const void* integrate_kernels(IntegrateForm form) {
    static const void* const k[2][2] = {{(const void*)k_batch_integrate<false, false, ZB, KT, WG, WORDS>,
                                         (const void*)k_batch_integrate<false, true, ZB, KT, WG, WORDS>},
                                        {(const void*)k_batch_integrate<true, false, ZB, KT, WG, WORDS>,
                                         (const void*)k_batch_integrate<true, true, ZB, KT, WG, WORDS>}};
    return k[form.c64][form.fast];
}
// wg: waves per workgroup of a coarse form (1, 2 or 4); the fine forms have INT_WG.  WORDS: the batch's mask words
template <int WORDS>
static const void* integrate_kernel_w(IntegrateForm form, int wg) {
    if (!form.fine)
        return wg == 1   ? integrate_kernels<BZ, 1, 1, WORDS>(form)
               : wg == 2 ? integrate_kernels<BZ, 1, 2, WORDS>(form)
                         : integrate_kernels<BZ, 1, 4, WORDS>(form);
    return form.kt == 3   ? integrate_kernels<2, 3, INT_WG, WORDS>(form)
           : form.kt == 2 ? integrate_kernels<2, 2, INT_WG, WORDS>(form)
                          : integrate_kernels<2, 1, INT_WG, WORDS>(form);
}

}  // namespace ot
