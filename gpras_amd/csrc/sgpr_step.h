// Resident optimiser loop of the GENERAL sparse launch sequence (gp_sparse.h sgpr_batch_enqueue: M > 64, or M <= 64 with "sgpr_fused" = 0):
// the launch that closes step t and opens step t + 1 of every cell.  It does on the device what sgpr_stage_out_kernel, the host tail of
// sgpr_objective_batch / gprx_objective_batch, the host update of the optimiser loop and sgpr_stage_in_kernel do between two host-stepped
// evaluations -- with their arithmetic (sgpr_asm.h, px_math.h), so a cell ends with the same bits on either route.
// The kernel lives in sgpr_step.hip (one instantiation per optimiser); this header is its argument block and its launcher.
#pragma once
#include "sgpr_fused.h"

namespace gprx {

// ctl words (device memory: a replayed graph bakes its launch arguments in, so what changes between windows and calls is read from here)
constexpr int SGPR_CTL_MASK = 0, SGPR_CTL_MAX_ITER = 1, SGPR_CTL_ALPHA_T1 = 2, SGPR_CTL_WORDS = 4;

struct SgprStep {
  double* arena;    // cell blocks of the launch sequence, ss doubles apart
  int64_t ss;
  int64_t oZ, odZ, oRed, oPartP, oPartQ;  // offsets inside a cell block: Z (updated in place), dZ (scaled by dz_kernel), the 8 reductions, the contraction partials
  int nwg_p, nwg_q, width;                // rows of the two partial blocks, sums per row (2 + d)
  int n, m, d, mp;
  double* cellpar;  // device parameter table: the cell's row of step t is read, the row of step t + 1 written
  double* cellres;  // per cell res_doubles doubles; [2] carries the pivot status as an int; cleared for step t + 1
  int res_doubles;
  const int* ctl;   // SGPR_CTL_*: mask, max_iter, the first step of the current alpha window
};

// ad.mask, ad.max_iter and ad.alpha_t1 are NOT read (ctl carries them); ad.alpha is the window's table.  opt: SF_OPT_ADAM / SF_OPT_ADADELTA.
// grid = (cells), 256 threads
// hold (held-out rows, sgpr_fused.h: SF_HOLD_W doubles per cell on the device): given, the launch is the twin kernel of sgpr_held.hip, which
// takes every cell's row count and y.y from its row of the table; null: a.n and the y.y of the cell's unit, the kernel of sgpr_step.hip.
hipError_t sgpr_launch_step(hipStream_t st, int opt, const SgprStep& a, const SfAdam& ad, int cells, const double* hold = nullptr);
hipError_t sgpr_launch_step_held(hipStream_t st, int opt, const SgprStep& a, const SfAdam& ad, int cells, const double* hold);

// The stage-in of a batch whose cells hold rows out (sgpr_held.hip): sgpr_stage_in_kernel (sgpr.h) with the staged y of a held row 0.0.
// Same arguments and grid, and the batch's table.
hipError_t sgpr_launch_stage_in_held(hipStream_t st, int blocks_x, int cells, const double* Y, int np, const double* par_host, int par_doubles,
                                     double* cell_par, const double* z_host, int zn, double* z_dst, double* y_dst, int64_t cs, double* cell_res,
                                     int res_doubles, const double* hold);

}  // namespace gprx
