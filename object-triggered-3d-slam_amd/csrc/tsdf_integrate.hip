// tsdf_integrate.hip — the k_batch_integrate forms that read one frame-mask word (batches of at most WORD_FRAMES frames).
#include "tsdf_integrate_kernel.h"

namespace ot {

const void* integrate_kernel_word(IntegrateForm form, int wg) { return integrate_kernel_w<1>(form, wg); }

}  // namespace ot
