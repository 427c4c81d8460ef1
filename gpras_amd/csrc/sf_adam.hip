// Resident optimiser loop of the fused sparse evaluation: the Adam instantiations of the merged update + prep launch (sf_adam_prep.h).
#include "sf_adam_prep.h"

namespace gprx {

hipError_t sf_launch_adam_prep(hipStream_t st, int kid, int form, int iso, const SfParams& p, int cells, const SfAdam& adam, double* cpar_dst) {
  if (p.hold != nullptr) return sf_launch_adam_prep_held(st, kid, form, iso, p, cells, adam, cpar_dst);  // (sf_adam_held.hip)
  return sf_launch_step_prep<SF_OPT_ADAM, 0>(st, kid, form, iso, p, cells, adam, cpar_dst);
}

}  // namespace gprx
