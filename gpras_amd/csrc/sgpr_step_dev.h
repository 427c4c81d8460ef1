// Resident optimiser loop of the general sparse launch sequence: the body of the step kernel (sgpr_step.h), shared by the kernel that
// calls without holds launch (sgpr_step.hip) and its twin for cells that hold rows out (sgpr_held.hip).
// Sibling of sf_adam_body (sf_cell_dev.h), which serves the fused evaluation: same thread assignment (thread k owns hyperparameter k,
// thread 255 the loss and the stop rule, four Z elements per thread and pass), and the same code for both (opt_step_hyper,
// opt_step_close, opt_element of sf_cell_dev.h).  What differs is where the evaluation left its results: the trace sums come from the
// contraction partials (sgpr_trace_sums, shared with sgpr_stage_out_kernel), dZ is already scaled (dz_kernel), and sgpr_asm_dparam gets
// the padded M of the launch sequence (mp).
#pragma once
#include "sgpr_step.h"
#include "sf_cell_dev.h"
#include "sgpr_small_ops.h"

namespace gprx {

// HOLD = 1 (`hold`: the batch's table, SF_HOLD_W doubles per cell): the row count and y.y of the tail are the cell's own, from its row of
// the table; HOLD = 0 takes a.n and the y.y of the cell's unit.  Every thread of the workgroup must call it.
template <int OPT, int HOLD>
__device__ __forceinline__ void sgpr_step_body(const SgprStep& a, const SfAdam& ad, const double* __restrict__ hold) {
  __shared__ double shs[2 * (2 + CELL_PAR - CELL_PAR_LS)];  // trace sums
  __shared__ double sred[8];
  __shared__ double sPar[CELL_PAR];                          // the cell's parameter row of THIS step (the row in memory is overwritten below)
  __shared__ double sTh[2 + CELL_PAR - CELL_PAR_LS];         // the variables after the update
  __shared__ int keep;
  const int cell = blockIdx.x, tid = threadIdx.x;
  if (ad.active[cell] == 0) return;
  double* res = a.cellres + (int64_t)cell * a.res_doubles;
  int info = 0;
  __builtin_memcpy(&info, res + 2, sizeof(int));
  if (info != 0) {
    sf_adam_failed(ad, cell, tid);
    return;
  }
  double* A = a.arena + (int64_t)cell * a.ss;
  double* par = a.cellpar + (int64_t)cell * CELL_PAR;
  const int mask = a.ctl[SGPR_CTL_MASK], max_iter = a.ctl[SGPR_CTL_MAX_ITER];
  const int width = a.width, nt = ad.nt, nz = a.m * a.d, gw = nt + nz;
  // (the step and its alpha are read before the barrier: thread 255 stores tstep[cell] = t below -- sf_adam_body)
  const int t = ad.tstep[cell] + 1;
  double alpha = 0.0;
  if constexpr (OPT == SF_OPT_ADAM) alpha = ad.alpha[t - a.ctl[SGPR_CTL_ALPHA_T1]];
  if (tid < 8) sred[tid] = A[a.oRed + tid];
  if (tid < CELL_PAR) sPar[tid] = par[tid];
  sgpr_trace_sums(A + a.oPartP, a.nwg_p, A + a.oPartQ, a.nwg_q, width, tid, shs);
  __syncthreads();
  const double* ls = sPar + CELL_PAR_LS;
  const double variance = sPar[0], noise = sPar[1];
  const double nn = HOLD != 0 ? hold[(int64_t)cell * SF_HOLD_W + 2] : (double)a.n;
  const double* yy_cell = HOLD != 0 ? hold + (int64_t)cell * SF_HOLD_W + 3 : nullptr;
  double* th = ad.theta + (int64_t)cell * nt;
  double* mom = ad.mom + (int64_t)cell * gw;
  double* vel = ad.vel + (int64_t)cell * gw;
  if (tid < nt) {
    const int k = tid;
    const double w = opt_step_hyper<OPT>(ad, k, mask, alpha, a.d, width, nn, a.mp, variance, noise, ls, sred, shs, th, mom, vel);
    sTh[k] = w;
  }
  if ((mask & ASM_TRAIN_Z) != 0) {
    for (int e0 = 0; e0 < nz; e0 += 256 * 4) {  // four elements per thread at once: their loads in flight together
      double ge[4], mo[4], ve[4], x[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = min(e0 + 256 * u + tid, nz - 1);
        ge[u] = -A[a.odZ + e];
        mo[u] = mom[nt + e];
        ve[u] = vel[nt + e];
        x[u] = A[a.oZ + e];
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + 256 * u + tid;
        if (e < nz) {
          opt_element<OPT>(ge[u], alpha, mo[u], ve[u], x[u]);
          mom[nt + e] = mo[u];
          vel[nt + e] = ve[u];
          A[a.oZ + e] = x[u];
        }
      }
    }
  }
  if (tid == 255) keep = opt_step_close<OPT>(ad, cell, t, mask, max_iter, nn, variance, noise, ls, sred, yy_cell) ? 1 : 0;  // (a thread with no hyperparameter of its own)
  __syncthreads();  // (sTh and keep are complete; every read of this step's parameter row went through sPar)
  if (keep == 0) return;
  // ---- opens step t + 1: the parameter row of the updated variables (decode_theta's bits), the result words cleared; y stays in the
  // cell block from the opening stage-in ----
  if (tid < CELL_PAR) par[tid] = sf_par_from_theta(sTh, ad, cell, a.d, tid);
  if (tid < a.res_doubles) res[tid] = 0.0;
}

}  // namespace gprx
