// Resident optimiser loop of the fused sparse evaluation: the Adadelta instantiations of the merged update + prep launch for batches
// whose cells hold rows out (sf_adam_prep.h, HOLD = 1; gprx_adadelta_batch_held).
#include "sf_adam_prep.h"

namespace gprx {

hipError_t sf_launch_adadelta_prep_held(hipStream_t st, int kid, int form, int iso, const SfParams& p, int cells, const SfAdam& adam,
                                        double* cpar_dst) {
  return sf_launch_step_prep<SF_OPT_ADADELTA, 1>(st, kid, form, iso, p, cells, adam, cpar_dst);
}

}  // namespace gprx
