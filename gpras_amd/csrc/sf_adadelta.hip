// Resident optimiser loop of the fused sparse evaluation: the Adadelta instantiations of the merged update + prep launch
// (sf_adam_prep.h; gprx_adadelta_batch, gpr.py:176-192).
#include "sf_adam_prep.h"

namespace gprx {

hipError_t sf_launch_adadelta_prep(hipStream_t st, int kid, int form, int iso, const SfParams& p, int cells, const SfAdam& adam,
                                   double* cpar_dst) {
  if (p.hold != nullptr) return sf_launch_adadelta_prep_held(st, kid, form, iso, p, cells, adam, cpar_dst);  // (sf_adadelta_held.hip)
  return sf_launch_step_prep<SF_OPT_ADADELTA, 0>(st, kid, form, iso, p, cells, adam, cpar_dst);
}

}  // namespace gprx
