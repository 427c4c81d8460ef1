// Mode-count sweep: the field metrics of export_metric_summary (gpras/metrics.py:11-82) at several truncations of ONE EOF projector, in
// one pass that never writes a field -- the outer loop of run_spatial_modes (production/analysis/cross_validation.py:96-102).
//
// pca_reverse_kernel (pca.h) adds the modes in the order kk = 0, 1, ... with one fma each, so its running sums after k terms ARE the
// field and the variance of the projector truncated to k modes (its trailing terms are fma(m, 0, s) = s).  This kernel walks the modes
// once per row, takes a snapshot of (s, v) after mode counts[j] - 1, and feeds each snapshot through the operations of the per-count
// chain in their order: s / w + base (pca_reverse_kernel), the two steps of field_to_depth_kernel, sqrt(v) (field_sqrt_kernel), then
// every accumulator of metrics_cells_kernel and metrics_rows_kernel (metrics.h).  Per cell the results are those of the chain bit for
// bit; the per-row sums over the cells are reduced in another (fixed) order than metrics_rows_kernel's.
//
// Mapping: a thread owns one cell and keeps its e[kk], a2[kk] in registers, blockIdx.y is the event, a workgroup walks the event's
// rows in blocks of PCA_RB with the rows' mode values in LDS as in pca_reverse_kernel.  The snapshots go through LDS (the count
// index is a run-time value inside the unrolled mode loop; every thread reads back only what it wrote); the accumulators of the
// counts of one launch (at most SWEEP_SMAX) stay in registers, so a longer list of counts takes several launches, each restarting the
// mode sum at zero and leaving the mode loop after its last count.  gfx950: <64> 256 VGPRs + 112 AGPRs, 61 568 bytes of LDS, one wave per
// SIMD; <16> 177 VGPRs, 36 992 bytes, two waves per SIMD; no scratch.
#pragma once
#include "gprx_common.h"
#include "pca.h"

namespace gprx {

constexpr int SWEEP_SMAX = 4;  // counts per launch; their values are packed into 8 bits each of one 32-bit word

struct SweepArgs {
  const double* mean;   // (rows, k)
  const double* var;    // (rows, k) or null
  const double* truth;  // (rows, cells), in metric space
  int64_t rows, cells;
  int k;
  const double* Eb;  // (k, lde)
  int64_t lde;
  const double *w, *base, *xm, *xs, *elev;
  int depth_mode;  // 0: none, 1: max(y - el, 0), 2: max((y + el) - el, 0)
  double v_tol;
  const int64_t *ev_lo, *ev_hi;  // (n_events) on the device: rows [lo, hi) of event blockIdx.y
  int64_t n_events;
  int ncnt;            // counts of this launch, 1..SWEEP_SMAX
  unsigned packed;     // counts[j] in bits 8j .. 8j+7, 0 beyond ncnt
  int klast;           // the largest of them
  double* cell_sums;   // (ncnt, n_events, 6, cells) of this launch's counts
  int* cell_arg;       // (ncnt, n_events, cells)
  double* truth_peak;  // (n_events, cells), or null: this launch does not write the truth's peak
  int* truth_arg;
  double* row_part;                   // (gridDim.x, ncnt, rows, 3): per-workgroup sums over its 256 cells
  unsigned long long* match_part;     // (ncnt, n_events, gridDim.x)
};

template <int KMAX>
__global__ __launch_bounds__(256) void pca_sweep_kernel(SweepArgs p) {
  __shared__ double sM[PCA_RB][KMAX];
  __shared__ double sV[PCA_RB][KMAX];
  __shared__ double snap[SWEEP_SMAX][2][256];
  __shared__ double sred[PCA_RB][SWEEP_SMAX][3][4];
  __shared__ unsigned long long smatch[SWEEP_SMAX][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t c = (int64_t)blockIdx.x * 256 + tid;
  const bool live = c < p.cells;
  const int64_t ev = blockIdx.y;
  const int64_t lo = p.ev_lo[ev], hi = p.ev_hi[ev];
  const int k = p.k;
  // a thread beyond the last cell stays in the loops (the wave reductions need every lane) as a cell of zeros
  double e[KMAX], a2[KMAX];
  const double wc = live ? p.w[c] : 1.0, b = live ? p.base[c] : 0.0, el = (live && p.depth_mode) ? p.elev[c] : 0.0;
#pragma unroll
  for (int kk = 0; kk < KMAX; ++kk) {
    e[kk] = (live && kk < k) ? p.Eb[(int64_t)kk * p.lde + c] : 0.0;
    const double a = (kk < k) ? p.xs[kk] * e[kk] / wc : 0.0;
    a2[kk] = a * a;
  }
  double se[SWEEP_SMAX], se2[SWEEP_SMAX], sc[SWEEP_SMAX], sa[SWEEP_SMAX], ypk[SWEEP_SMAX], xat[SWEEP_SMAX];
  int yarg[SWEEP_SMAX];
  unsigned nm[SWEEP_SMAX];
#pragma unroll
  for (int j = 0; j < SWEEP_SMAX; ++j) {
    se[j] = se2[j] = sc[j] = sa[j] = ypk[j] = xat[j] = 0.0;
    yarg[j] = 0;
    nm[j] = 0u;
  }
  double xpk = 0.0;
  int xarg = 0;
  double xnext = (live && lo < hi) ? p.truth[lo * p.cells + c] : 0.0;
  for (int64_t t0 = lo; t0 < hi; t0 += PCA_RB) {
    __syncthreads();
    for (int q = tid; q < PCA_RB * KMAX; q += 256) {
      const int r = q / KMAX, kk = q % KMAX;
      const bool ok = t0 + r < hi && kk < k;
      sM[r][kk] = ok ? p.mean[(t0 + r) * k + kk] * p.xs[kk] + p.xm[kk] : 0.0;
      sV[r][kk] = (ok && p.var) ? p.var[(t0 + r) * k + kk] : 0.0;
    }
    __syncthreads();
    const int nr = (int)((hi - t0 < PCA_RB) ? hi - t0 : PCA_RB);
    for (int r = 0; r < nr; ++r) {
      const int64_t t = t0 + r;
      const double xv = xnext;
      if (live && t + 1 < hi) xnext = p.truth[(t + 1) * p.cells + c];  // issued before this row's arithmetic
      double s = 0.0, v = 0.0;
      unsigned pk = p.packed;
      int j = 0;
#pragma unroll
      for (int kk = 0; kk < KMAX; ++kk) {
        if ((kk & 7) == 0 && kk >= p.klast) break;  // every snapshot of this launch is taken: the later modes belong to later launches
        s = __builtin_fma(sM[r][kk], e[kk], s);
        v = __builtin_fma(sV[r][kk], a2[kk], v);
        if ((unsigned)(kk + 1) == (pk & 0xffu)) {  // uniform: a scalar branch
          snap[j][0][tid] = s;
          snap[j][1][tid] = v;
          ++j;
          pk >>= 8;
        }
      }
      // the truth's first maximum; a NaN is taken as the maximum and sticks (metrics.h)
      // (written as selects: with the branch form of metrics.h the compiler kept only the argmax update of the per-count peaks below)
      const bool xtake = t == lo || (!(xpk != xpk) && (xv > xpk || xv != xv));
      xpk = xtake ? xv : xpk;
      xarg = xtake ? (int)(t - lo) : xarg;
#pragma unroll
      for (int jj = 0; jj < SWEEP_SMAX; ++jj) {
        if (jj >= p.ncnt) break;
        double y = snap[jj][0][tid] / wc + b;
        if (p.depth_mode) {
          {
#pragma clang fp contract(off)
            if (p.depth_mode == 2) y = y + el;
            y = y - el;
          }
          y = y < 0.0 ? 0.0 : y;
        }
        const double cf = sqrt(snap[jj][1][tid]);
        const double d = xv - y;
        se[jj] += d;
        se2[jj] = __builtin_fma(d, d, se2[jj]);
        sc[jj] += cf;
        sa[jj] += fabs(d);
        const bool ytake = t == lo || (!(ypk[jj] != ypk[jj]) && (y > ypk[jj] || y != y));
        ypk[jj] = ytake ? y : ypk[jj];
        yarg[jj] = ytake ? (int)(t - lo) : yarg[jj];
        xat[jj] = ytake ? xv : xat[jj];
        nm[jj] += (fabs(y - xv) <= p.v_tol) ? 1u : 0u;
        const double r0 = wave_sum_dpp(d), r1 = wave_sum_dpp(__builtin_fma(d, d, 0.0)), r2 = wave_sum_dpp(cf);
        if (lane == 0) {
          sred[r][jj][0][wave] = r0;
          sred[r][jj][1][wave] = r1;
          sred[r][jj][2][wave] = r2;
        }
      }
    }
    __syncthreads();
    // the four waves in a fixed order; consecutive threads write consecutive (row, quantity) of one count
    for (int q = tid; q < p.ncnt * nr * 3; q += 256) {
      const int jj = q / (nr * 3), rq = q - jj * nr * 3, r = rq / 3, qq = rq - r * 3;
      const double sum = ((sred[r][jj][qq][0] + sred[r][jj][qq][1]) + sred[r][jj][qq][2]) + sred[r][jj][qq][3];
      p.row_part[(((int64_t)blockIdx.x * p.ncnt + jj) * p.rows + (t0 + r)) * 3 + qq] = sum;
    }
  }
  if (live) {
    if (p.truth_peak) {
      p.truth_peak[ev * p.cells + c] = xpk;
      p.truth_arg[ev * p.cells + c] = xarg;
    }
#pragma unroll
    for (int jj = 0; jj < SWEEP_SMAX; ++jj) {
      if (jj >= p.ncnt) break;
      const int64_t blk = (int64_t)jj * p.n_events + ev;
      double* out = p.cell_sums + blk * 6 * p.cells + c;
      out[0] = se[jj];
      out[p.cells] = se2[jj];
      out[2 * p.cells] = sc[jj];
      out[3 * p.cells] = sa[jj];
      out[4 * p.cells] = ypk[jj];
      out[5 * p.cells] = xat[jj];
      p.cell_arg[blk * p.cells + c] = yarg[jj];
    }
  }
#pragma unroll
  for (int jj = 0; jj < SWEEP_SMAX; ++jj) {
    if (jj >= p.ncnt) break;
    unsigned long long mm = live ? nm[jj] : 0ull;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) mm += __shfl_xor(mm, off, 64);
    if (lane == 0) smatch[jj][wave] = mm;
  }
  __syncthreads();
  if (tid < p.ncnt) p.match_part[((int64_t)tid * p.n_events + ev) * gridDim.x + blockIdx.x] = smatch[tid][0] + smatch[tid][1] + smatch[tid][2] + smatch[tid][3];
}

// row_sums[j, t, q] = sum over the workgroups of row_part[b, j, t, q], b ascending
__global__ __launch_bounds__(256) void pca_sweep_rows_kernel(const double* __restrict__ row_part, int nblk, int64_t per_block, double* __restrict__ row_sums) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= per_block) return;
  double s = 0.0;
  for (int bq = 0; bq < nblk; ++bq) s += row_part[(int64_t)bq * per_block + i];
  row_sums[i] = s;
}

}  // namespace gprx
