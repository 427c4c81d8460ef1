// Device helpers shared by the leave-one-event-out kernels (sf_loeo.hip, sf_loeo_blocked.hip).  After sgpr_fused_dev.h.
#pragma once

namespace gprx {

// the 64 columns [c0, c0 + 64) of the event's t2 (rows = inducing points) into sT; columns beyond the event are staged as zeros
// (an event's first column has no alignment beyond 8 bytes: one double per load)
__device__ __forceinline__ void loeo_stage(const double* __restrict__ T, int64_t ldk, int c0, int nc, double* __restrict__ sT, int tid) {
  double v[16];
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int q = tid + 256 * e, i = q >> 6, j = q & 63;
    v[e] = T[(int64_t)i * ldk + c0 + min(j, nc - 1)];  // (unconditional loads from clamped columns, masks afterwards)
  }
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int q = tid + 256 * e, i = q >> 6, j = q & 63;
    sT[i * SM_LD + j] = j < nc ? v[e] : 0.0;
  }
}

}  // namespace gprx
