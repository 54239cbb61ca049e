// tsdf_integrate_wide.hip — the k_batch_integrate forms that read both frame-mask words (a whole volume's Direct batch
// of more than WORD_FRAMES frames).
#include "tsdf_integrate_kernel.h"

namespace ot {

const void* integrate_kernel_wide(IntegrateForm form, int wg) { return integrate_kernel_w<FMASK_WORDS>(form, wg); }

}  // namespace ot
