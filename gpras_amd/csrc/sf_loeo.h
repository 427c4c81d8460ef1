// Leave-one-event-out prediction of fitted sparse models (M <= 64): the downdate kernel's parameter block and launcher (sf_loeo.hip).
//
// A cell block holds LB = chol(I + A' A'^T / s) and c after an evaluation, and the predict path leaves t2 = LB^-1 L^-1 k(Z, X[rows]) in the
// cell's Kus tile.  Taking the rows [lo, hi) of one event out of the data turns B into B - t t^T / s (t = L^-1 k(Z, X[lo:hi])), i.e. in LB
// coordinates into H = I - t2 t2^T / s, and the right-hand side into c - t2 y[lo:hi] / s.  With Lh = chol(H):
//   c' = Lh^-1 (c - t2 y / s),  W = Lh^-1 t2,  mean_j = W[:, j]^T c',  var_j = v - colsum(t1^2)_j + colsum(W^2)_j  (+ s, added last)
// which is SGPR predict_y of the model on the remaining rows at the same hyperparameters and inducing points.  H >= B^-1 > 0: it factors
// whenever B did.  One workgroup per (event, cell); nothing is shared between workgroups and the 64-column chunks of an event are walked
// in ascending order, so a (cell, event) result has the same bits whatever else is in the launch.
#pragma once
#include "gprx_common.h"

namespace gprx {

constexpr int LOEO_EV = 4;  // ints per row of the event table: [0] first column of the event in the Kus tile, [1] rows, [2] output row, [3] -

struct LoeoParams {
  const double* arena;  // cell blocks, ss doubles apart
  int64_t ss;
  int64_t oKs, oC;      // offsets inside a cell block: the Kus tile (holds t2, 64 rows of ldk doubles) and c (64 doubles)
  int64_t ldk;
  const double* cpar;   // cell-parameter table: [1] s, [2] unit, [3] 1 / s
  const double* Y;      // (units, np) outputs, unit-major
  int np;
  const int* events;    // device event table of THIS launch: grid.x rows of LOEO_EV ints
  double* means;        // (cells, out_stride): written at the event's rows
  double* vars;         // (cells, out_stride): holds v - colsum(t1^2) at the event's rows on entry
  int64_t out_stride;
  int* status;          // (cells, status_stride) from this launch's first event on: 0, or the 1-based failing pivot of chol(H)
  int status_stride;
  int include_noise;    // 1: predict_y (the noise variance is added to the finished predict_f variance)
};

// grid (events, cells), 256 threads
hipError_t sf_launch_loeo(hipStream_t st, const LoeoParams& p, int events, int cells);

// ---- the same downdate for 64 < M <= 320 (sf_loeo_blocked.hip; mp = 64 works too): H is mp x mp and lives in a workspace slot per
// (cell, event) in device memory; the batched Cholesky and triangular inverse of the library run between the first and the other two of the kernels below.
// Slot of (cell, event e of the group) = ws + (cell * group_events + e) * slot_stride; inside it, in doubles:
//   oH   H, then Lh (mp x mp, ld mp; the gram kernel writes the tiles on and below the diagonal, diagonal tiles in full)
//   oP   P = Lh^-1 (mp x mp, ld mp; only the tiles on and below the diagonal are read, the diagonal tiles through a mask)
//   oU   u = t2 y[lo:hi] (mp), oCp: c' = P (c - u / s) (mp), oInfo: the info word of the slot's Cholesky (an int)
// Workgroups share nothing and every sum has one order: the result of a (cell, event) has the same bits whatever else the launch holds.
struct LoeoBlockedParams {
  LoeoParams base;      // arena, cell table, outputs and the event table of THIS GROUP (status from the group's first event on)
  int mp;               // 64 * ceil(M / 64), at most LOEO_BLOCKED_MAX_MP
  int group_events;
  double* ws;
  int64_t slot_stride;
  int64_t oH, oP, oU, oCp, oInfo;
};
constexpr int LOEO_BLOCKED_MAX_MP = 320;

// grid (lower tiles of H, events of the group, cells): H = I - t2 t2^T / s, u = t2 y, info word zeroed
hipError_t sf_launch_loeo_gram(hipStream_t st, const LoeoBlockedParams& p, int cells);
// grid (row bands, events of the group, cells): c' = P (c - u / s)
hipError_t sf_launch_loeo_cprime(hipStream_t st, const LoeoBlockedParams& p, int cells);
// grid (chunks, events of the group, cells), chunks = ceil(longest event of the group / 64): mean, var += colsum(W^2) (+ s); a slot whose
// info word is set writes it into status and NaN into its rows.
hipError_t sf_launch_loeo_apply(hipStream_t st, const LoeoBlockedParams& p, int chunks, int cells);

}  // namespace gprx
