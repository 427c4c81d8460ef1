// Resident optimiser loop of the general sparse launch sequence: the step kernel (sgpr_step.h), one instantiation per optimiser.  Its
// body is sgpr_step_body (sgpr_step_dev.h); the twin for cells that hold rows out lives in sgpr_held.hip.
#include "sgpr_step_dev.h"

namespace gprx {

template <int OPT>
__global__ __launch_bounds__(256) void sgpr_step_kernel(SgprStep a, SfAdam ad) {
  sgpr_step_body<OPT, 0>(a, ad, nullptr);
}

hipError_t sgpr_launch_step(hipStream_t st, int opt, const SgprStep& a, const SfAdam& ad, int cells, const double* hold) {
  if (hold != nullptr) return sgpr_launch_step_held(st, opt, a, ad, cells, hold);  // (sgpr_held.hip)
  if (opt == SF_OPT_ADAM)
    hipLaunchKernelGGL((sgpr_step_kernel<SF_OPT_ADAM>), dim3(cells), dim3(256), 0, st, a, ad);
  else if (opt == SF_OPT_ADADELTA)
    hipLaunchKernelGGL((sgpr_step_kernel<SF_OPT_ADADELTA>), dim3(cells), dim3(256), 0, st, a, ad);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace gprx
