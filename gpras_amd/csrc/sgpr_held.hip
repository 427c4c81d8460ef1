// Held-out rows in the general sparse launch sequence (gprx_*_held with "held_general" = 1): the three kernels of the sequence that look at
// a training row by its index, as twins that read the batch's hold table -- the Kuf / Kuu build (kmat.h, HOLD = 1), the stage-in and the
// step kernel of the resident loop (sgpr_step_dev.h, HOLD = 1).  With the held columns of P = Kuf and the held entries of the staged y
// exact zeros, every later launch of the sequence adds exact zeros for those columns and runs unchanged.  A unit of its own: the code
// objects that calls without holds run hold what they held before (sf_pass1.hip says why that matters).
#define GPRX_KMAT_NO_LAUNCHERS  // (the kernel bodies alone: kmat.h)
#include "kmat.h"
#include "sgpr_step_dev.h"

namespace gprx {

static_assert(KM_HOLD_W == SF_HOLD_W, "one table serves the build and the step kernel");

hipError_t launch_kmat_pair_held(hipStream_t st, int kid, KmatArgs p, KmatArgs q, int batch, const double* hold) {
  p.tiles_n = (p.n2p + KM_T - 1) / KM_T;
  q.tiles_n = (q.n2p + KM_T - 1) / KM_T;
  const int np_ = ((p.n1p + KM_T - 1) / KM_T) * p.tiles_n, nq = ((q.n1p + KM_T - 1) / KM_T) * q.tiles_n;
  if (np_ == 0 || nq == 0 || p.form != q.form || p.mode != 0 || p.tri != 0 || hold == nullptr) return hipErrorInvalidValue;
  dim3 grid(np_ + nq, batch), block(256);
#define GPRX_KMAT_CASE(K_)                                                                      \
  case K_:                                                                                      \
    if (p.form)                                                                                 \
      hipLaunchKernelGGL((kmat_pair_held_kernel<K_, 1>), grid, block, 0, st, p, q, np_, hold);  \
    else                                                                                        \
      hipLaunchKernelGGL((kmat_pair_held_kernel<K_, 0>), grid, block, 0, st, p, q, np_, hold);  \
    break;
  switch (kid) {
    GPRX_KMAT_CASE(0)
    GPRX_KMAT_CASE(1)
    GPRX_KMAT_CASE(2)
    GPRX_KMAT_CASE(3)
    GPRX_KMAT_CASE(4)
    default: return hipErrorInvalidValue;
  }
#undef GPRX_KMAT_CASE
  return hipGetLastError();
}

// sgpr_stage_in_kernel (sgpr.h) for cells that hold rows out: the staged y of a row inside the cell's [lo, hi) is 0.0.
// grid = (ceil(max(np, m d, par_doubles) / 256), cells)
__global__ void sgpr_stage_in_held_kernel(const double* __restrict__ Y, int np, const double* __restrict__ par_host, int par_doubles,
                                          double* __restrict__ cell_par, const double* __restrict__ z_host, int zn, double* __restrict__ z_dst,
                                          double* __restrict__ y_dst, int64_t cs, double* __restrict__ cell_res, int res_doubles,
                                          const double* __restrict__ hold) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t cell = blockIdx.y;
  if (i < res_doubles) cell_res[cell * res_doubles + i] = 0.0;
  if (i < par_doubles) cell_par[cell * par_doubles + i] = par_host[cell * par_doubles + i];
  if (i < zn) z_dst[cell * cs + i] = z_host[cell * zn + i];
  if (i < np) {
    const int unit = (int)par_host[cell * par_doubles + 2];
    const int hlo = (int)hold[cell * SF_HOLD_W], hhi = (int)hold[cell * SF_HOLD_W + 1];
    const double yv = Y[(int64_t)unit * np + i];
    y_dst[cell * cs + i] = (unsigned)(i - hlo) >= (unsigned)(hhi - hlo) ? yv : 0.0;
  }
}

hipError_t sgpr_launch_stage_in_held(hipStream_t st, int blocks_x, int cells, const double* Y, int np, const double* par_host, int par_doubles,
                                     double* cell_par, const double* z_host, int zn, double* z_dst, double* y_dst, int64_t cs, double* cell_res,
                                     int res_doubles, const double* hold) {
  if (hold == nullptr) return hipErrorInvalidValue;
  hipLaunchKernelGGL(sgpr_stage_in_held_kernel, dim3(blocks_x, cells), dim3(256), 0, st, Y, np, par_host, par_doubles, cell_par, z_host, zn, z_dst,
                     y_dst, cs, cell_res, res_doubles, hold);
  return hipGetLastError();
}

template <int OPT>
__global__ __launch_bounds__(256) void sgpr_step_held_kernel(SgprStep a, SfAdam ad, const double* __restrict__ hold) {
  sgpr_step_body<OPT, 1>(a, ad, hold);
}

hipError_t sgpr_launch_step_held(hipStream_t st, int opt, const SgprStep& a, const SfAdam& ad, int cells, const double* hold) {
  if (hold == nullptr) return hipErrorInvalidValue;
  if (opt == SF_OPT_ADAM)
    hipLaunchKernelGGL((sgpr_step_held_kernel<SF_OPT_ADAM>), dim3(cells), dim3(256), 0, st, a, ad, hold);
  else if (opt == SF_OPT_ADADELTA)
    hipLaunchKernelGGL((sgpr_step_held_kernel<SF_OPT_ADADELTA>), dim3(cells), dim3(256), 0, st, a, ad, hold);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

}  // namespace gprx
