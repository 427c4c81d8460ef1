// libgprx C ABI, EOF family: the projection either side of the GP path (gprx_pca_*), the fit of the preprocessor (gprx_pcafit_*)
// and HmsPreProcessor with the antecedent precipitation index (gprx_hms_*, gprx_api).  They share the split-K Gram plan.
#include "abi_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "gemm_f64.h"
#include "gprx_common.h"
#include "hms.h"
#include "pca.h"
#include "pca_fit.h"
#include "pca_fit_tall.h"
#include "sweep.h"
#include "ensemble.h"
#include "verify.h"
#include "timing.h"
#include "frequency.h"

using namespace gprx;

struct gprx_pca_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t cells = 0, cells_p = 0;  // cells_p: leading dimension of the device copies (multiple of 16, zero padded)
  int k = 0, depth = 0;
  bool has_elev = false;
  Buf mu, wfwd, wrev, elev, E, base, xm, xs;  // per-cell parameters expanded to all cells; E: (k, cells_p)
  Buf dX, dZ, ws, dMean, dVar, dFull, dVfull;
  Buf sweep_part, sweep_aux;  // gprx_pca_sweep_dev: per-workgroup row sums; event bounds, then the match counts per workgroup
  hipEvent_t ev[2] = {};
  double sweep_ms = 0.0;      // device time of the last gprx_pca_sweep_dev
  Buf ens_part;               // gprx_pca_member_stats_dev: per-workgroup wet areas
  double ens_ms = 0.0;        // device time of the last gprx_pca_ensemble_peaks_dev
  double ver_ms = 0.0;        // device time of the last gprx_pca_member_verify_dev
  double tim_ms = 0.0;        // device time of the last gprx_pca_ensemble_timing_dev
  Buf freq_lev;               // gprx_pca_freq_*_dev: the levels staged on the device, freq_lev_host what it holds
  std::vector<double> freq_lev_host;
  double freq_ms = 0.0;       // device time of the last gprx_pca_freq_accumulate_dev
  std::string err;
};

void gprx::launch_transpose_small(hipStream_t st, const double* src, int64_t rows, int64_t cols, double* dst) {
  hipLaunchKernelGGL(transpose_small_kernel, dim3((unsigned)std::min<int64_t>((rows * cols + 255) / 256, 4096)), dim3(256), 0, st, src, rows, cols, dst);
}

// ---- shared by the fit and HmsPreProcessor: the lower-triangle Gram stage and the components stage ----------------------------------
namespace {
// split-K plan of the lower-triangle product of n x n with K = kdim
SplitK gram_plan(int64_t n, int64_t kdim) {
  const int64_t tiles = (n + 63) / 64;
  return splitk_plan(tiles * (tiles + 1) / 2, kdim, n * n);
}

// *out (n, n) = X X^T of X (n, kdim), leading dimension ld: lower-triangle tiles, split-K slabs summed in a fixed order.  `ws` holds
// the slabs, then their sum, where *out points.
template <class Ctx>
int gram_lower(Ctx* c, hipStream_t st, const double* X, int64_t ld, int64_t n, int64_t kdim, Buf& ws, double** out) {
  const SplitK sk = gram_plan(n, kdim);
  int rc;
  if ((rc = ensure(c, ws, sizeof(double) * (size_t)(sk.nsplit + 1) * n * n))) return rc;
  *out = ws.p + (size_t)sk.nsplit * n * n;
  GemmArgs g{X, X, ws.p, ld, ld, n, (int)n, (int)n, (int)kdim, 1.0, 0.0, GEMM_C_LOWER, 0, 0, 0, 0, 0, 0, sk.kchunk, n * n};
  HIPCHK(c, (launch_gemm_t<0, 1, 64, 64>(st, g, 1, sk.nsplit)));
  hipLaunchKernelGGL(pcafit_gram_reduce_kernel, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, st, (const double*)ws.p, sk.nsplit, (int)n, *out);
  HIPCHK(c, hipGetLastError());
  return GPRX_OK;
}

// the argument checks of a components step, of the fit and of HmsPreProcessor (k == 0 passes them: the caller has nothing to do)
template <class Ctx>
int check_components(Ctx* c, int k, int64_t rows, const char* rows_name, bool null_argument, const double* lam) {
  if (k < 0 || k >= rows) return fail(c, GPRX_EINVAL, std::string("need 0 <= k < ") + rows_name + " (centring removes one direction)");
  if (k == 0) return GPRX_OK;
  if (null_argument) return fail(c, GPRX_EINVAL, "null argument");
  for (int i = 0; i < k; ++i)
    if (!(lam[i] > 0.0)) return fail(c, GPRX_EINVAL, "retained eigenvalues must be positive");
  return GPRX_OK;
}

// A (k, rows_p) on the device = diag(lambda^-1/2) U_k^T from u (rows, k) on the host, K padded to rows_p with zeros.  `a` stages
// it on the host: the caller keeps it until it has waited for `st`.
template <class Ctx>
int upload_scaled_ut(Ctx* c, hipStream_t st, const double* u, const double* lam, int k, int64_t rows, int64_t rows_p, std::vector<double>& a, double* A) {
  a.assign((size_t)k * rows_p, 0.0);
  for (int i = 0; i < k; ++i) {
    const double s = 1.0 / std::sqrt(lam[i]);
    for (int64_t t = 0; t < rows; ++t) a[(size_t)i * rows_p + t] = u[(size_t)t * k + i] * s;
  }
  HIPCHK(c, hipMemcpyAsync(A, a.data(), sizeof(double) * a.size(), hipMemcpyHostToDevice, st));
  return GPRX_OK;
}

// E (k, ld) = A X2 (NN, K = rows_p; X2 has rows_p rows, zero beyond the samples), then svd_flip on the first `cols` entries of its rows
template <class Ctx>
int components_gemm(Ctx* c, hipStream_t st, int k, const double* A, int64_t rows_p, const double* X2, int64_t ld, int64_t cols, double* E) {
  HIPCHK(c, launch_gemm(st, 0, 0, k, (int)ld, (int)rows_p, 1.0, A, rows_p, X2, ld, 0.0, E, ld, 0));
  hipLaunchKernelGGL(pcafit_sign_flip_kernel, dim3((unsigned)k), dim3(256), 0, st, E, ld, cols);
  HIPCHK(c, hipGetLastError());
  return GPRX_OK;
}
}  // namespace

extern "C" {

// ---- EOF projection either side of the GP path ------------------------------
namespace {
int pupload(gprx_pca_handle p, Buf& b, const std::vector<double>& v) {
  int rc = ensure(p, b, sizeof(double) * v.size());
  if (rc) return rc;
  HIPCHK(p, copy_sync(b.p, v.data(), sizeof(double) * v.size(), hipMemcpyHostToDevice));
  return GPRX_OK;
}
}  // namespace

int gprx_pca_create(int device, int64_t n_cells, int k, const unsigned char* dry, const double* elevations, const double* input_mean,
                    const double* weights, const double* eofs, const double* x_mean, const double* x_std, int depth_mode,
                    gprx_pca_handle* out) {
  if (!out) return fail(nullptr, GPRX_EINVAL, "out is null");
  *out = nullptr;
  if (n_cells <= 0 || k <= 0 || k > 64) return fail(nullptr, GPRX_EINVAL, "n_cells must be positive and 1 <= k <= 64");
  if (!input_mean || !eofs || !x_mean || !x_std) return fail(nullptr, GPRX_EINVAL, "input_mean, eofs, x_mean, x_std must be non-null");
  int64_t n_dry = 0;
  if (dry)
    for (int64_t c = 0; c < n_cells; ++c) n_dry += dry[c] != 0;
  if (depth_mode && !elevations) return fail(nullptr, GPRX_EINVAL, "depth mode needs the cell elevations");
  if (!depth_mode && n_dry > 0 && !elevations) return fail(nullptr, GPRX_EINVAL, "always-dry cells are filled with their elevations: elevations is null");
  gprx_pca_handle p = nullptr;
  const int rc = guarded(nullptr, [&]() -> int {
    p = new gprx_pca_ctx();
    int rc = open_handle(p, device, p->ev, 2);
    if (rc) return rc;
    p->has_elev = elevations != nullptr;
    p->cells = n_cells;
    p->cells_p = round_up(n_cells, 16);
    p->k = k;
    p->depth = depth_mode ? 1 : 0;
    const int64_t n_wet = n_cells - n_dry, cp = p->cells_p;
    // expand the wet-cell parameters to the full cell axis: dry cells get weight 0 (forward) / 1 (reverse), E = 0 and the fill value
    std::vector<double> mu(cp, 0.0), wf(cp, 0.0), wr(cp, 1.0), el(cp, 0.0), base(cp, 0.0), E((size_t)k * cp, 0.0);
    int64_t j = 0;
    for (int64_t c = 0; c < n_cells; ++c) {
      if (elevations) el[c] = elevations[c];
      if (dry && dry[c]) {
        base[c] = depth_mode ? 0.0 : elevations[c];
        continue;
      }
      mu[c] = input_mean[j];
      wf[c] = weights ? weights[j] : 1.0;
      wr[c] = wf[c];
      base[c] = input_mean[j];
      for (int kk = 0; kk < k; ++kk) E[(size_t)kk * cp + c] = eofs[(size_t)kk * n_wet + j];
      ++j;
    }
    std::vector<double> xm(x_mean, x_mean + k), xs(x_std, x_std + k);
    if ((rc = pupload(p, p->mu, mu)) || (rc = pupload(p, p->wfwd, wf)) || (rc = pupload(p, p->wrev, wr)) || (rc = pupload(p, p->elev, el)) ||
        (rc = pupload(p, p->base, base)) || (rc = pupload(p, p->E, E)) || (rc = pupload(p, p->xm, xm)) || (rc = pupload(p, p->xs, xs)))
      return rc;
    return GPRX_OK;
  });
  if (rc) gprx_pca_destroy(p);
  else *out = p;
  return rc;
}

int gprx_pca_destroy(gprx_pca_handle p) {
  if (!p) return GPRX_OK;
  release_handle(p->device, p->stream, {p->mu.p, p->wfwd.p, p->wrev.p, p->elev.p, p->E.p, p->base.p, p->xm.p, p->xs.p, p->dX.p, p->dZ.p, p->ws.p, p->dMean.p, p->dVar.p,
                                           p->dFull.p, p->dVfull.p, p->sweep_part.p, p->sweep_aux.p, p->ens_part.p, p->freq_lev.p}, p->ev, 2);
  delete p;
  return GPRX_OK;
}

// x_dev: (rows, ld) with ld = cells_p (padding columns may hold anything finite: their weight is 0); z_dev: (rows, k)
int gprx_pca_transform_dev(gprx_pca_handle p, const double* x_dev, int64_t rows, double* z_dev) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (rows < 0 || (rows > 0 && (!x_dev || !z_dev))) return fail(p, GPRX_EINVAL, "null argument");
    if (rows == 0) return GPRX_OK;
    if (rows > (1 << 30)) return fail(p, GPRX_EINVAL, "too many rows in one call");
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = p->stream;
    const int64_t cp = p->cells_p;
    // Z = ((g(X) - mu) w) E^T in ONE pass over X: the centring / weighting runs inside the GEMM's operand load
    // (gemm_f64_kernel AXF); M = rows, N = k, K = cells_p cut into slices so that a few thousand workgroups exist
    const SplitK sk = splitk_plan((rows + 63) / 64, cp, 1);
    int rc;
    if ((rc = ensure(p, p->ws, sizeof(double) * (size_t)sk.nsplit * rows * p->k))) return rc;
    HIPCHK(p, launch_gemm_splitk_axf(st, (int)rows, p->k, (int)cp, x_dev, cp, p->E.p, cp, z_dev, p->k, p->ws.p, sk.kchunk, p->mu.p, p->wfwd.p,
                                     p->depth ? p->elev.p : nullptr));
    hipLaunchKernelGGL(pca_standardize_kernel, dim3((unsigned)((rows * p->k + 255) / 256)), dim3(256), 0, st, z_dev, rows, p->k,
                       (const double*)p->xm.p, (const double*)p->xs.p);
    HIPCHK(p, hipGetLastError());
    return GPRX_OK;
  });
}

int gprx_pca_reverse_dev(gprx_pca_handle p, const double* mean_dev, const double* var_dev, int64_t rows, double* full_dev, double* vfull_dev) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (rows < 0 || (rows > 0 && (!mean_dev || !full_dev))) return fail(p, GPRX_EINVAL, "null argument");
    if ((var_dev == nullptr) != (vfull_dev == nullptr)) return fail(p, GPRX_EINVAL, "var and var_full must both be given or both be null");
    if (rows == 0) return GPRX_OK;
    HIPCHK(p, hipSetDevice(p->device));
    dim3 grid((unsigned)((p->cells + 255) / 256), (unsigned)std::min<int64_t>((rows + PCA_RB - 1) / PCA_RB, 64));
    if (p->k <= 16)
      hipLaunchKernelGGL(pca_reverse_kernel<16>, grid, dim3(256), 0, p->stream, mean_dev, var_dev, rows, p->k, p->cells, (const double*)p->E.p, p->cells_p,
                         (const double*)p->wrev.p, (const double*)p->base.p, (const double*)p->xm.p, (const double*)p->xs.p, full_dev, vfull_dev);
    else
      hipLaunchKernelGGL(pca_reverse_kernel<64>, grid, dim3(256), 0, p->stream, mean_dev, var_dev, rows, p->k, p->cells, (const double*)p->E.p, p->cells_p,
                         (const double*)p->wrev.p, (const double*)p->base.p, (const double*)p->xm.p, (const double*)p->xs.p, full_dev, vfull_dev);
    HIPCHK(p, hipGetLastError());
    return GPRX_OK;
  });
}

int gprx_pca_to_depth_dev(gprx_pca_handle p, double* field_dev, int64_t rows, int add_elevations_first) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (rows < 0 || (rows > 0 && !field_dev)) return fail(p, GPRX_EINVAL, "null argument");
    if (rows == 0) return GPRX_OK;
    HIPCHK(p, hipSetDevice(p->device));
    hipLaunchKernelGGL(field_to_depth_kernel, dim3(4096), dim3(256), 0, p->stream, field_dev, rows, p->cells, (const double*)p->elev.p,
                       add_elevations_first ? 1 : 0);
    HIPCHK(p, hipGetLastError());
    return GPRX_OK;
  });
}

int gprx_pca_sqrt_dev(gprx_pca_handle p, double* field_dev, int64_t count) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (count < 0 || (count > 0 && !field_dev)) return fail(p, GPRX_EINVAL, "null argument");
    if (count == 0) return GPRX_OK;
    HIPCHK(p, hipSetDevice(p->device));
    hipLaunchKernelGGL(field_sqrt_kernel, dim3(4096), dim3(256), 0, p->stream, field_dev, count);
    HIPCHK(p, hipGetLastError());
    return GPRX_OK;
  });
}

int gprx_pca_transpose_dev(gprx_pca_handle p, const double* src_dev, int64_t rows, int64_t cols, double* dst_dev) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (rows < 0 || cols < 0 || (rows * cols > 0 && (!src_dev || !dst_dev))) return fail(p, GPRX_EINVAL, "null argument");
    if (rows * cols == 0) return GPRX_OK;
    HIPCHK(p, hipSetDevice(p->device));
    launch_transpose_small(p->stream, src_dev, rows, cols, dst_dev);
    HIPCHK(p, hipGetLastError());
    return GPRX_OK;
  });
}

// The field metrics at every count of `counts` in one pass (sweep.h).  Counts go in groups of SWEEP_SMAX per launch.
int gprx_pca_sweep_dev(gprx_pca_handle p, const double* mean_dev, const double* var_dev, int64_t rows, const double* truth_dev, int64_t n_events,
                       const int64_t* event_lo, const int64_t* event_hi, int n_counts, const int* counts, int depth_mode, double v_tol,
                       double* cell_sums_dev, int* cell_arg_dev, double* truth_peak_dev, int* truth_arg_dev, double* row_sums_dev,
                       unsigned long long* matches) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (rows <= 0 || rows >= ((int64_t)1 << 31)) return fail(p, GPRX_EINVAL, "rows must be positive and below 2^31");
    if (!mean_dev) return fail(p, GPRX_EINVAL, "null argument: mean");
    if (!truth_dev) return fail(p, GPRX_EINVAL, "the sweep needs the truth field");
    if (!cell_sums_dev || !cell_arg_dev || !truth_peak_dev || !truth_arg_dev || !row_sums_dev || !matches)
      return fail(p, GPRX_EINVAL, "null argument: output block");
    if (n_counts < 1 || n_counts > 64 || !counts) return fail(p, GPRX_EINVAL, "need between 1 and 64 counts");
    for (int j = 0; j < n_counts; ++j)
      if (counts[j] < 1 || counts[j] > p->k || (j && counts[j] <= counts[j - 1]))
        return fail(p, GPRX_EINVAL, "counts must be strictly increasing in [1, " + std::to_string(p->k) + "]");
    if (depth_mode < 0 || depth_mode > 2) return fail(p, GPRX_EINVAL, "depth mode must be 0 (none), 1 (wse) or 2 (depth)");
    if (depth_mode && !p->has_elev) return fail(p, GPRX_EINVAL, "the depth conversion needs the cell elevations (the projector was created without them)");
    if (!(v_tol >= 0.0)) return fail(p, GPRX_EINVAL, "v_tol must be non-negative");
    if (n_events < 1 || n_events > 65535 || !event_lo || !event_hi) return fail(p, GPRX_EINVAL, "need between 1 and 65535 events");
    std::vector<std::pair<int64_t, int64_t>> evs((size_t)n_events);
    int64_t covered = 0;
    for (int64_t i = 0; i < n_events; ++i) {
      if (event_lo[i] < 0 || event_hi[i] > rows || event_lo[i] >= event_hi[i])
        return fail(p, GPRX_EINVAL, "event " + std::to_string((long long)i) + " is empty or outside [0, rows)");
      evs[(size_t)i] = {event_lo[i], event_hi[i]};
      covered += event_hi[i] - event_lo[i];
    }
    std::sort(evs.begin(), evs.end());
    for (size_t i = 1; i < evs.size(); ++i)
      if (evs[i].first < evs[i - 1].second) return fail(p, GPRX_EINVAL, "the events overlap");
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = p->stream;
    const int64_t cells = p->cells;
    const unsigned nbx = (unsigned)((cells + 255) / 256);
    const int smax = std::min(n_counts, SWEEP_SMAX);
    const size_t part_doubles = (size_t)nbx * smax * rows * 3;
    const size_t match_count = (size_t)n_counts * n_events * nbx;
    int rc;
    if ((rc = ensure(p, p->sweep_part, sizeof(double) * part_doubles, "the sweep's row sums")) ||
        (rc = ensure(p, p->sweep_aux, sizeof(int64_t) * 2 * (size_t)n_events + sizeof(unsigned long long) * match_count)))
      return rc;
    int64_t* ev_dev = (int64_t*)p->sweep_aux.p;
    unsigned long long* match_dev = (unsigned long long*)(ev_dev + 2 * n_events);
    std::vector<int64_t> ev_h((size_t)2 * n_events);
    std::copy(event_lo, event_lo + n_events, ev_h.begin());
    std::copy(event_hi, event_hi + n_events, ev_h.begin() + n_events);
    HIPCHK(p, hipMemcpyAsync(ev_dev, ev_h.data(), sizeof(int64_t) * ev_h.size(), hipMemcpyHostToDevice, st));
    HIPCHK(p, hipEventRecord(p->ev[0], st));
    for (int j0 = 0; j0 < n_counts; j0 += SWEEP_SMAX) {
      const int nc = std::min(SWEEP_SMAX, n_counts - j0);
      unsigned packed = 0;
      for (int j = 0; j < nc; ++j) packed |= (unsigned)counts[j0 + j] << (8 * j);
      // rows of no event are written by no workgroup: their sums are zero
      if (covered < rows) HIPCHK(p, hipMemsetAsync(p->sweep_part.p, 0, sizeof(double) * (size_t)nbx * nc * rows * 3, st));
      SweepArgs a{mean_dev, var_dev, truth_dev, rows, cells, p->k, p->E.p, p->cells_p, p->wrev.p, p->base.p, p->xm.p, p->xs.p, p->elev.p, depth_mode, v_tol,
                  ev_dev, ev_dev + n_events, n_events, nc, packed, counts[j0 + nc - 1], cell_sums_dev + (size_t)j0 * n_events * 6 * cells,
                  cell_arg_dev + (size_t)j0 * n_events * cells, j0 == 0 ? truth_peak_dev : nullptr, truth_arg_dev, p->sweep_part.p,
                  match_dev + (size_t)j0 * n_events * nbx};
      const dim3 grid(nbx, (unsigned)n_events);
      if (p->k <= 16) hipLaunchKernelGGL(pca_sweep_kernel<16>, grid, dim3(256), 0, st, a);
      else hipLaunchKernelGGL(pca_sweep_kernel<64>, grid, dim3(256), 0, st, a);
      HIPCHK(p, hipGetLastError());
      const int64_t per_block = (int64_t)nc * rows * 3;
      hipLaunchKernelGGL(pca_sweep_rows_kernel, dim3((unsigned)((per_block + 255) / 256)), dim3(256), 0, st, (const double*)p->sweep_part.p, (int)nbx,
                         per_block, row_sums_dev + (size_t)j0 * rows * 3);
      HIPCHK(p, hipGetLastError());
    }
    HIPCHK(p, hipEventRecord(p->ev[1], st));
    std::vector<unsigned long long> mh(match_count);
    HIPCHK(p, hipMemcpyAsync(mh.data(), match_dev, sizeof(unsigned long long) * match_count, hipMemcpyDeviceToHost, st));
    HIPCHK(p, hipStreamSynchronize(st));
    p->sweep_ms = elapsed_ms(p->ev[0], p->ev[1]);
    for (size_t i = 0; i < (size_t)n_counts * n_events; ++i) {
      unsigned long long total = 0;
      for (unsigned bq = 0; bq < nbx; ++bq) total += mh[i * nbx + bq];
      matches[i] = total;
    }
    return GPRX_OK;
  });
}

int gprx_pca_sweep_ms(gprx_pca_handle p, double* ms) {
  if (!p || !ms) return fail(p, GPRX_EINVAL, "null argument");
  *ms = p->sweep_ms;
  return GPRX_OK;
}

int gprx_pca_sweep_group(void) { return SWEEP_SMAX; }

// ---- peak ensembles (ensemble.h) ---------------------------------------------------------------------------------------------------
namespace {
// members per workgroup of the fused kernel: about four workgroups per compute unit before a workgroup takes a second member
int ensemble_group(int64_t cells, int64_t members) {
  const int64_t nbx = (cells + 255) / 256;
  const int64_t groups_wanted = (1024 + nbx - 1) / nbx;
  int64_t group = std::max<int64_t>(1, std::min<int64_t>(16, members / groups_wanted));
  while ((members + group - 1) / group > 65535) ++group;
  return (int)group;
}

int check_members(gprx_pca_handle p, int64_t members, int64_t rows_e) {
  if (members < 1 || rows_e < 1) return fail(p, GPRX_EINVAL, "members and the event's rows must be positive");
  if (rows_e >= ((int64_t)1 << 31) || members >= ((int64_t)1 << 31) / rows_e) return fail(p, GPRX_EINVAL, "members x rows must stay below 2^31");
  return GPRX_OK;
}

// the checks of a fused walk over the members' scores and its grid: *group members per workgroup, *ngroups of them
int ensemble_walk(gprx_pca_handle p, const double* scores_dev, int64_t members, int64_t rows_e, int depth_mode, int member_group, int* group, int64_t* ngroups) {
  if (!scores_dev) return fail(p, GPRX_EINVAL, "null argument");
  int rc;
  if ((rc = check_members(p, members, rows_e))) return rc;
  if (depth_mode < 0 || depth_mode > 2) return fail(p, GPRX_EINVAL, "depth mode must be 0 (none), 1 (wse) or 2 (depth)");
  if (depth_mode && !p->has_elev) return fail(p, GPRX_EINVAL, "the depth conversion needs the cell elevations (the projector was created without them)");
  if (member_group < 0 || member_group > 64) return fail(p, GPRX_EINVAL, "member_group must be 0 (the launcher's choice) or between 1 and 64");
  *group = member_group ? member_group : ensemble_group(p->cells, members);
  *ngroups = (members + *group - 1) / *group;
  if (*ngroups > 65535) return fail(p, GPRX_EINVAL, "too many member groups: raise member_group");
  return GPRX_OK;
}

// n_thr thresholds as the timing kernels take them, copied into dst[ENS_TMAX]
int check_thresholds(gprx_pca_handle p, int n_thr, const double* thr, double* dst) {
  if (n_thr < 0 || n_thr > ENS_TMAX || (n_thr && !thr)) return fail(p, GPRX_EINVAL, "at most " + std::to_string(ENS_TMAX) + " thresholds");
  for (int j = 0; j < n_thr; ++j) {
    if (thr[j] != thr[j]) return fail(p, GPRX_EINVAL, "a threshold is NaN");
    dst[j] = thr[j];
  }
  return GPRX_OK;
}
}  // namespace

int gprx_pca_ensemble_peaks_dev(gprx_pca_handle p, const double* scores_dev, int64_t members, int64_t rows_e, int depth_mode, int member_group,
                                double* peak_dev) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (!peak_dev) return fail(p, GPRX_EINVAL, "null argument");
    int rc, group;
    int64_t ngroups;
    if ((rc = ensemble_walk(p, scores_dev, members, rows_e, depth_mode, member_group, &group, &ngroups))) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = p->stream;
    EnsembleArgs a{scores_dev, members, rows_e, p->cells, p->k, p->E.p, p->cells_p, p->wrev.p, p->base.p, p->xm.p, p->xs.p, p->elev.p, depth_mode, group, peak_dev};
    const dim3 grid((unsigned)((p->cells + 255) / 256), (unsigned)ngroups);
    HIPCHK(p, hipEventRecord(p->ev[0], st));
    if (p->k <= 16) hipLaunchKernelGGL(pca_ensemble_peaks_kernel<16>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(pca_ensemble_peaks_kernel<64>, grid, dim3(256), 0, st, a);
    HIPCHK(p, hipGetLastError());
    HIPCHK(p, hipEventRecord(p->ev[1], st));
    HIPCHK(p, hipStreamSynchronize(st));
    p->ens_ms = elapsed_ms(p->ev[0], p->ev[1]);
    return GPRX_OK;
  });
}

int gprx_pca_ensemble_timing_dev(gprx_pca_handle p, const double* scores_dev, int64_t members, int64_t rows_e, int depth_mode, int member_group, int n_thr,
                                 const double* thresholds, double* peak_dev, int* timing_dev) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (!peak_dev || !timing_dev) return fail(p, GPRX_EINVAL, "null argument");
    int rc, group;
    int64_t ngroups;
    if ((rc = ensemble_walk(p, scores_dev, members, rows_e, depth_mode, member_group, &group, &ngroups))) return rc;
    if (rows_e > 2147483646) return fail(p, GPRX_EINVAL, "the event's rows must not exceed 2^31 - 2");
    TimingArgs a{};
    if ((rc = check_thresholds(p, n_thr, thresholds, a.thr))) return rc;
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = p->stream;
    a.e = EnsembleArgs{scores_dev, members, rows_e, p->cells, p->k, p->E.p, p->cells_p, p->wrev.p, p->base.p, p->xm.p, p->xs.p, p->elev.p, depth_mode, group, peak_dev};
    a.n_thr = n_thr, a.timing = timing_dev;
    const dim3 grid((unsigned)((p->cells + 255) / 256), (unsigned)ngroups);
    HIPCHK(p, hipEventRecord(p->ev[0], st));
    if (p->k <= 16) hipLaunchKernelGGL(pca_ensemble_timing_kernel<16>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(pca_ensemble_timing_kernel<64>, grid, dim3(256), 0, st, a);
    HIPCHK(p, hipGetLastError());
    HIPCHK(p, hipEventRecord(p->ev[1], st));
    HIPCHK(p, hipStreamSynchronize(st));
    p->tim_ms = elapsed_ms(p->ev[0], p->ev[1]);
    return GPRX_OK;
  });
}

int gprx_pca_ensemble_timing_ms(gprx_pca_handle p, double* ms) {
  if (!p || !ms) return fail(p, GPRX_EINVAL, "null argument");
  *ms = p->tim_ms;
  return GPRX_OK;
}

int gprx_pca_member_timing_dev(gprx_pca_handle p, const double* field_dev, int64_t members, int64_t rows_e, int n_thr, const double* thresholds,
                               double* peak_dev, int* timing_dev) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (!field_dev || !timing_dev) return fail(p, GPRX_EINVAL, "null argument");
    int rc;
    if ((rc = check_members(p, members, rows_e))) return rc;
    if (rows_e > 2147483646) return fail(p, GPRX_EINVAL, "the event's rows must not exceed 2^31 - 2");
    if (members > 65535) return fail(p, GPRX_EINVAL, "at most 65535 members per call");
    FieldTimingArgs a{};
    if ((rc = check_thresholds(p, n_thr, thresholds, a.thr))) return rc;
    a.f = field_dev, a.rows_e = rows_e, a.cells = p->cells, a.n_thr = n_thr, a.peak = peak_dev, a.timing = timing_dev;
    HIPCHK(p, hipSetDevice(p->device));
    hipLaunchKernelGGL(field_member_timing_kernel, dim3((unsigned)((p->cells + 255) / 256), (unsigned)members), dim3(256), 0, p->stream, a);
    HIPCHK(p, hipGetLastError());
    return GPRX_OK;
  });
}

int gprx_pca_timing_stats_dev(gprx_pca_handle p, const int* timing_dev, int64_t members, int n_maps, int map0, int n_sel, int64_t rows_e, int sentinel,
                              int n_lev, const int* levels, int n_rank, const int* ranks, const int* obs_dev, int* cdf_dev, int* n_valid_dev,
                              int64_t* sum_dev, int* order_dev, int* below_dev, int* equal_dev) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (!timing_dev || !n_valid_dev || !sum_dev) return fail(p, GPRX_EINVAL, "null argument");
    if (members < 1 || members > ENS_SMAX) return fail(p, GPRX_EINVAL, "members must be between 1 and " + std::to_string(ENS_SMAX));
    if (rows_e < 1 || rows_e > 2147483646) return fail(p, GPRX_EINVAL, "the event's rows must lie between 1 and 2^31 - 2");
    if (n_maps < 1 || n_maps > 1 + 2 * ENS_TMAX || map0 < 0 || n_sel < 1 || n_sel > n_maps - map0)
      return fail(p, GPRX_EINVAL, "the maps [map0, map0 + n_sel) must lie inside the block's n_maps <= " + std::to_string(1 + 2 * ENS_TMAX));
    if (sentinel != -1 && (sentinel < 0 || sentinel > rows_e)) return fail(p, GPRX_EINVAL, "the sentinel must be -1 (none) or a value in [0, rows]");
    if (n_lev < 0 || n_lev > TM_LMAX || (n_lev && (!levels || !cdf_dev)))
      return fail(p, GPRX_EINVAL, "at most " + std::to_string(TM_LMAX) + " levels, with their output block");
    if (n_rank < 0 || n_rank > ENS_RMAX || (n_rank && (!ranks || !order_dev)))
      return fail(p, GPRX_EINVAL, "at most " + std::to_string(ENS_RMAX) + " ranks, with their output block");
    for (int j = 0; j < n_rank; ++j)
      if (ranks[j] < 0 || ranks[j] >= members) return fail(p, GPRX_EINVAL, "ranks must lie in [0, members)");
    if (obs_dev && (!below_dev || !equal_dev)) return fail(p, GPRX_EINVAL, "the observed maps need the below and equal blocks");
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = p->stream;
    TimingStatsArgs a{};
    a.timing = timing_dev, a.members = members, a.cells = p->cells, a.n_maps = n_maps, a.map0 = map0, a.rows_e = (int)rows_e, a.sentinel = sentinel;
    a.n_lev = n_lev, a.n_rank = n_rank;
    for (int j = 0; j < n_lev; ++j) a.level[j] = levels[j];
    for (int j = 0; j < n_rank; ++j) a.rank[j] = ranks[j];
    a.obs = obs_dev, a.cdf = cdf_dev, a.n_valid = n_valid_dev, a.sum = reinterpret_cast<long long*>(sum_dev), a.order = order_dev, a.below = below_dev, a.equal = equal_dev;
    hipLaunchKernelGGL(member_timing_stats_kernel, dim3((unsigned)((p->cells + 255) / 256), (unsigned)n_sel), dim3(256), 0, st, a);
    HIPCHK(p, hipGetLastError());
    HIPCHK(p, hipStreamSynchronize(st));
    return GPRX_OK;
  });
}

int gprx_pca_pack_scores_dev(gprx_pca_handle p, const double* mean_dev, const double* w_dev, int64_t members, int64_t rows_e, int64_t tp,
                             double* scores_dev) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (!mean_dev || !w_dev || !scores_dev) return fail(p, GPRX_EINVAL, "null argument");
    int rc;
    if ((rc = check_members(p, members, rows_e))) return rc;
    if (tp < rows_e) return fail(p, GPRX_EINVAL, "the padded row count is smaller than the event's rows");
    HIPCHK(p, hipSetDevice(p->device));
    const int64_t total = members * rows_e * p->k;
    hipLaunchKernelGGL(ensemble_pack_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 8192)), dim3(256), 0, p->stream, mean_dev, w_dev, members,
                       rows_e, tp, p->k, scores_dev);
    HIPCHK(p, hipGetLastError());
    return GPRX_OK;
  });
}

int gprx_pca_normals_dev(gprx_pca_handle p, uint64_t seed, uint64_t stream, int64_t event, int64_t member0, int64_t members, int64_t pair_offset,
                         int64_t rows_e, int64_t tp, int raw, double* zn_dev) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (!zn_dev) return fail(p, GPRX_EINVAL, "null argument");
    if ((uintptr_t)zn_dev % 16) return fail(p, GPRX_EINVAL, "the block of normals must be 16-byte aligned");
    int rc;
    if ((rc = check_members(p, members, rows_e))) return rc;
    if (tp < rows_e) return fail(p, GPRX_EINVAL, "the padded row count is smaller than the event's rows");
    if (tp % 64) return fail(p, GPRX_EINVAL, "the padded row count must be a multiple of 64");
    if (member0 < 0 || member0 > ENS_SMAX - members) return fail(p, GPRX_EINVAL, "the members must lie in [0, " + std::to_string(ENS_SMAX) + ")");
    if (event < 0) return fail(p, GPRX_EINVAL, "the event index must not be negative");
    if (pair_offset < 0) return fail(p, GPRX_EINVAL, "pair_offset must be 0 (off) or positive");
    if (pair_offset && member0 + members > 2 * pair_offset) return fail(p, GPRX_EINVAL, "with pair_offset set the members must lie below 2 pair_offset");
    HIPCHK(p, hipSetDevice(p->device));
    NormalsArgs a{seed, stream, event, member0, members, pair_offset, rows_e, tp, p->k, raw ? 1 : 0, reinterpret_cast<unsigned long long*>(zn_dev)};
    const int64_t total = (int64_t)p->k * members * (tp / 4);
    hipLaunchKernelGGL(ensemble_normals_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 8192)), dim3(256), 0, p->stream, a);
    HIPCHK(p, hipGetLastError());
    return GPRX_OK;
  });
}

int gprx_pca_normal_transform_dev(gprx_pca_handle p, const uint64_t* words_dev, int64_t n, double* z_dev) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (!words_dev || !z_dev) return fail(p, GPRX_EINVAL, "null argument");
    if (n < 1 || n >= ((int64_t)1 << 31)) return fail(p, GPRX_EINVAL, "the word count must be positive and below 2^31");
    HIPCHK(p, hipSetDevice(p->device));
    hipLaunchKernelGGL(ensemble_normal_transform_kernel, dim3((unsigned)std::min<int64_t>((n + 255) / 256, 8192)), dim3(256), 0, p->stream,
                       reinterpret_cast<const unsigned long long*>(words_dev), n, z_dev);
    HIPCHK(p, hipGetLastError());
    return GPRX_OK;
  });
}

int gprx_pca_ensemble_ms(gprx_pca_handle p, double* ms) {
  if (!p || !ms) return fail(p, GPRX_EINVAL, "null argument");
  *ms = p->ens_ms;
  return GPRX_OK;
}

int gprx_pca_ensemble_group(gprx_pca_handle p, int64_t members, int* group) {
  if (!p || !group) return fail(p, GPRX_EINVAL, "null argument");
  if (members < 1) return fail(p, GPRX_EINVAL, "members must be positive");
  *group = ensemble_group(p->cells, members);
  return GPRX_OK;
}

int gprx_pca_member_peaks_dev(gprx_pca_handle p, const double* field_dev, int64_t members, int64_t rows_e, double* peak_dev) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (!field_dev || !peak_dev) return fail(p, GPRX_EINVAL, "null argument");
    int rc;
    if ((rc = check_members(p, members, rows_e))) return rc;
    if (members > 65535) return fail(p, GPRX_EINVAL, "at most 65535 members per call");
    HIPCHK(p, hipSetDevice(p->device));
    hipLaunchKernelGGL(field_member_peaks_kernel, dim3((unsigned)((p->cells + 255) / 256), (unsigned)members), dim3(256), 0, p->stream, field_dev, rows_e,
                       p->cells, peak_dev);
    HIPCHK(p, hipGetLastError());
    return GPRX_OK;
  });
}

int gprx_pca_member_stats_dev(gprx_pca_handle p, const double* peak_dev, int64_t members, int n_thr, const double* thresholds, int n_rank, const int* ranks,
                              const double* area_dev, int* exceed_dev, double* mean_dev, double* std_dev, double* order_dev, double* wet_area_dev) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (!peak_dev || !mean_dev || !std_dev) return fail(p, GPRX_EINVAL, "null argument");
    if (members < 1 || members > ENS_SMAX) return fail(p, GPRX_EINVAL, "members must be between 1 and " + std::to_string(ENS_SMAX));
    if (n_thr < 0 || n_thr > ENS_TMAX || (n_thr && (!thresholds || !exceed_dev || !wet_area_dev)))
      return fail(p, GPRX_EINVAL, "at most " + std::to_string(ENS_TMAX) + " thresholds, with their output blocks");
    if (n_rank < 0 || n_rank > ENS_RMAX || (n_rank && (!ranks || !order_dev)))
      return fail(p, GPRX_EINVAL, "at most " + std::to_string(ENS_RMAX) + " ranks, with their output block");
    for (int j = 0; j < n_thr; ++j)
      if (thresholds[j] != thresholds[j]) return fail(p, GPRX_EINVAL, "a threshold is NaN");
    for (int j = 0; j < n_rank; ++j)
      if (ranks[j] < 0 || ranks[j] >= members) return fail(p, GPRX_EINVAL, "ranks must lie in [0, members)");
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = p->stream;
    const int64_t cells = p->cells;
    const unsigned nbx = (unsigned)((cells + 255) / 256);
    MemberStatsArgs a{};
    a.peak = peak_dev, a.members = members, a.cells = cells, a.n_thr = n_thr, a.n_rank = n_rank;
    for (int j = 0; j < n_thr; ++j) a.thr[j] = thresholds[j];
    for (int j = 0; j < n_rank; ++j) a.rank[j] = ranks[j];
    a.exceed = exceed_dev, a.mean = mean_dev, a.std = std_dev, a.order = order_dev;
    hipLaunchKernelGGL(member_cell_stats_kernel, dim3(nbx), dim3(256), 0, st, a);
    HIPCHK(p, hipGetLastError());
    if (n_thr) {
      int rc;
      if ((rc = ensure(p, p->ens_part, sizeof(double) * (size_t)members * n_thr * nbx))) return rc;
      MemberAreaArgs b{};
      b.peak = peak_dev, b.area = area_dev, b.members = members, b.cells = cells, b.n_thr = n_thr, b.part = p->ens_part.p;
      for (int j = 0; j < n_thr; ++j) b.thr[j] = thresholds[j];
      hipLaunchKernelGGL(member_area_kernel, dim3(nbx, (unsigned)members), dim3(256), 0, st, b);
      HIPCHK(p, hipGetLastError());
      const int64_t total = members * n_thr;
      hipLaunchKernelGGL(member_area_sum_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double*)p->ens_part.p, (int)nbx, total,
                         wet_area_dev);
      HIPCHK(p, hipGetLastError());
    }
    HIPCHK(p, hipStreamSynchronize(st));
    return GPRX_OK;
  });
}

int gprx_pca_member_verify_dev(gprx_pca_handle p, const double* peak_dev, const double* obs_dev, int64_t members, int n_rank, const int* ranks,
                               double* crps_dev, int* below_dev, int* equal_dev, double* order_dev) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (!peak_dev || !obs_dev || !crps_dev || !below_dev || !equal_dev) return fail(p, GPRX_EINVAL, "null argument");
    if (members < 1 || members > ENS_SMAX) return fail(p, GPRX_EINVAL, "members must be between 1 and " + std::to_string(ENS_SMAX));
    if (n_rank < 0 || n_rank > ENS_RMAX || (n_rank && (!ranks || !order_dev)))
      return fail(p, GPRX_EINVAL, "at most " + std::to_string(ENS_RMAX) + " ranks, with their output block");
    for (int j = 0; j < n_rank; ++j)
      if (ranks[j] < 0 || ranks[j] >= members) return fail(p, GPRX_EINVAL, "ranks must lie in [0, members)");
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = p->stream;
    MemberVerifyArgs a{};
    a.peak = peak_dev, a.obs = obs_dev, a.members = members, a.cells = p->cells, a.n_rank = n_rank;
    a.log_sp = verify_log_sp(members);
    for (int j = 0; j < n_rank; ++j) a.rank[j] = ranks[j];
    a.crps = crps_dev, a.below = below_dev, a.equal = equal_dev, a.order = order_dev;
    const int64_t tile_cells = verify_tile_keys(a.log_sp) >> a.log_sp;
    const dim3 grid((unsigned)((p->cells + tile_cells - 1) / tile_cells));
    HIPCHK(p, hipEventRecord(p->ev[0], st));
    if (verify_tile_keys(a.log_sp) == 8192) hipLaunchKernelGGL(member_verify_kernel<8192>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(member_verify_kernel<4096>, grid, dim3(256), 0, st, a);
    HIPCHK(p, hipGetLastError());
    HIPCHK(p, hipEventRecord(p->ev[1], st));
    HIPCHK(p, hipStreamSynchronize(st));
    p->ver_ms = elapsed_ms(p->ev[0], p->ev[1]);
    return GPRX_OK;
  });
}

int gprx_pca_member_verify_ms(gprx_pca_handle p, double* ms) {
  if (!p || !ms) return fail(p, GPRX_EINVAL, "null argument");
  *ms = p->ver_ms;
  return GPRX_OK;
}

int gprx_pca_member_verify_tile(int64_t members, int* tile_cells) {
  if (!tile_cells || members < 1 || members > ENS_SMAX) return fail(nullptr, GPRX_EINVAL, "members must be between 1 and " + std::to_string(ENS_SMAX));
  *tile_cells = verify_tile_keys(verify_log_sp(members)) >> verify_log_sp(members);
  return GPRX_OK;
}

// ---- depth-frequency maps (frequency.h) -------------------------------------------------------------------------------------------
namespace {
int check_freq_levels(gprx_pca_handle p, int n_levels, const double* levels) {
  if (n_levels < 1 || n_levels > FREQ_LMAX) return fail(p, GPRX_EINVAL, "n_levels must be between 1 and " + std::to_string(FREQ_LMAX));
  if (!levels) return fail(p, GPRX_EINVAL, "null argument: levels");
  for (int l = 0; l < n_levels; ++l) {
    if (!std::isfinite(levels[l])) return fail(p, GPRX_EINVAL, "the levels must be finite");
    if (l && !(levels[l] > levels[l - 1])) return fail(p, GPRX_EINVAL, "the levels must be strictly increasing");
  }
  return GPRX_OK;
}

// the levels on the device; uploaded when they are not the ones staged last (freq_lev_host outlives the copy: the calls synchronise)
int stage_freq_levels(gprx_pca_handle p, int n_levels, const double* levels) {
  const size_t bytes = sizeof(double) * (size_t)n_levels;
  if (p->freq_lev.p && p->freq_lev_host.size() == (size_t)n_levels && !std::memcmp(p->freq_lev_host.data(), levels, bytes)) return GPRX_OK;
  int rc;
  if ((rc = ensure(p, p->freq_lev, sizeof(double) * FREQ_LMAX))) return rc;
  p->freq_lev_host.assign(levels, levels + n_levels);
  const hipError_t e = hipMemcpyAsync(p->freq_lev.p, p->freq_lev_host.data(), bytes, hipMemcpyHostToDevice, p->stream);
  if (e != hipSuccess) p->freq_lev_host.clear();
  HIPCHK(p, e);
  return GPRX_OK;
}
}  // namespace

int gprx_pca_freq_accumulate_dev(gprx_pca_handle p, const double* peak_dev, int64_t members, int n_levels, const double* levels, double weight,
                                 double* rate_dev, int* nan_dev) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (!peak_dev || !rate_dev || !nan_dev) return fail(p, GPRX_EINVAL, "null argument");
    if (members < 1 || members > FREQ_SMAX) return fail(p, GPRX_EINVAL, "members must be between 1 and " + std::to_string(FREQ_SMAX));
    int rc;
    if ((rc = check_freq_levels(p, n_levels, levels))) return rc;
    if (!std::isfinite(weight) || weight < 0.0) return fail(p, GPRX_EINVAL, "the weight must be finite and not negative");
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = p->stream;
    if ((rc = stage_freq_levels(p, n_levels, levels))) return rc;
    FreqAccumulateArgs a{peak_dev, p->freq_lev.p, members, p->cells, n_levels, weight, rate_dev, nan_dev};
    const dim3 grid((unsigned)((p->cells + FREQ_TILE - 1) / FREQ_TILE));
    HIPCHK(p, hipEventRecord(p->ev[0], st));
    if (n_levels <= 64) hipLaunchKernelGGL(freq_accumulate_kernel<64>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(freq_accumulate_kernel<FREQ_LMAX>, grid, dim3(256), 0, st, a);
    HIPCHK(p, hipGetLastError());
    HIPCHK(p, hipEventRecord(p->ev[1], st));
    HIPCHK(p, hipStreamSynchronize(st));
    p->freq_ms = elapsed_ms(p->ev[0], p->ev[1]);
    return GPRX_OK;
  });
}

int gprx_pca_freq_invert_dev(gprx_pca_handle p, const double* rate_dev, const int* nan_dev, int n_levels, const double* levels, int n_aep, const double* aep,
                             int interp, double* depth_dev, int* bracket_dev) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (!rate_dev || !nan_dev || !depth_dev || !bracket_dev) return fail(p, GPRX_EINVAL, "null argument");
    int rc;
    if ((rc = check_freq_levels(p, n_levels, levels))) return rc;
    if (n_aep < 1 || n_aep > FREQ_PMAX || !aep) return fail(p, GPRX_EINVAL, "need between 1 and " + std::to_string(FREQ_PMAX) + " targets");
    for (int j = 0; j < n_aep; ++j)
      if (!std::isfinite(aep[j]) || !(aep[j] > 0.0)) return fail(p, GPRX_EINVAL, "the targets must be finite and positive");
    if (interp != 0 && interp != 1) return fail(p, GPRX_EINVAL, "interp must be 0 (linear) or 1 (step)");
    HIPCHK(p, hipSetDevice(p->device));
    hipStream_t st = p->stream;
    if ((rc = stage_freq_levels(p, n_levels, levels))) return rc;
    FreqInvertArgs a{};
    a.rate = rate_dev, a.nan_members = nan_dev, a.levels = p->freq_lev.p, a.cells = p->cells, a.n_levels = n_levels, a.n_aep = n_aep, a.interp = interp;
    for (int j = 0; j < n_aep; ++j) a.aep[j] = aep[j];
    a.depth = depth_dev, a.bracket = bracket_dev;
    hipLaunchKernelGGL(freq_invert_kernel, dim3((unsigned)((p->cells + 255) / 256)), dim3(256), 0, st, a);
    HIPCHK(p, hipGetLastError());
    HIPCHK(p, hipStreamSynchronize(st));
    return GPRX_OK;
  });
}

int gprx_pca_freq_ms(gprx_pca_handle p, double* ms) {
  if (!p || !ms) return fail(p, GPRX_EINVAL, "null argument");
  *ms = p->freq_ms;
  return GPRX_OK;
}

int gprx_pca_synchronize(gprx_pca_handle p) {
  if (!p) return fail(p, GPRX_EINVAL, "null handle");
  return guarded(p, [&]() -> int { HIPCHK(p, hipStreamSynchronize(p->stream)); return GPRX_OK; });
}

int gprx_pca_transform(gprx_pca_handle p, const double* x, int64_t rows, double* z) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (rows < 0 || (rows > 0 && (!x || !z))) return fail(p, GPRX_EINVAL, "null argument");
    HIPCHK(p, hipSetDevice(p->device));
    const int64_t cp = p->cells_p, chunk = std::max<int64_t>(64, pca_chunk_doubles() / cp);
    int rc;
    for (int64_t t0 = 0; t0 < rows; t0 += chunk) {
      const int64_t nr = std::min(chunk, rows - t0);
      if ((rc = ensure(p, p->dX, sizeof(double) * (size_t)nr * cp)) || (rc = ensure(p, p->dZ, sizeof(double) * (size_t)nr * p->k))) return rc;
      if (cp > p->cells)  // padding columns must be finite (their weight is 0, and 0 * NaN is not)
        HIPCHK(p, hipMemset2DAsync(p->dX.p + p->cells, sizeof(double) * cp, 0, sizeof(double) * (cp - p->cells), nr, p->stream));
      HIPCHK(p, hipMemcpy2DAsync(p->dX.p, sizeof(double) * cp, x + t0 * p->cells, sizeof(double) * p->cells, sizeof(double) * p->cells, nr,
                                 hipMemcpyHostToDevice, p->stream));
      if ((rc = gprx_pca_transform_dev(p, p->dX.p, nr, p->dZ.p))) return rc;
      HIPCHK(p, hipMemcpyAsync(z + t0 * p->k, p->dZ.p, sizeof(double) * nr * p->k, hipMemcpyDeviceToHost, p->stream));
      HIPCHK(p, hipStreamSynchronize(p->stream));
    }
    return GPRX_OK;
  });
}

int gprx_pca_reverse(gprx_pca_handle p, const double* mean, const double* var, int64_t rows, double* full, double* var_full) {
  return guarded(p, [&]() -> int {
    if (!p) return fail(p, GPRX_EINVAL, "null handle");
    if (rows < 0 || (rows > 0 && (!mean || !full))) return fail(p, GPRX_EINVAL, "null argument");
    if ((var == nullptr) != (var_full == nullptr)) return fail(p, GPRX_EINVAL, "var and var_full must both be given or both be null");
    HIPCHK(p, hipSetDevice(p->device));
    const int64_t chunk = std::max<int64_t>(64, pca_chunk_doubles() / p->cells);
    int rc;
    for (int64_t t0 = 0; t0 < rows; t0 += chunk) {
      const int64_t nr = std::min(chunk, rows - t0);
      if ((rc = ensure(p, p->dMean, sizeof(double) * (size_t)nr * p->k)) || (rc = ensure(p, p->dFull, sizeof(double) * (size_t)nr * p->cells))) return rc;
      HIPCHK(p, hipMemcpyAsync(p->dMean.p, mean + t0 * p->k, sizeof(double) * nr * p->k, hipMemcpyHostToDevice, p->stream));
      if (var) {
        if ((rc = ensure(p, p->dVar, sizeof(double) * (size_t)nr * p->k)) || (rc = ensure(p, p->dVfull, sizeof(double) * (size_t)nr * p->cells))) return rc;
        HIPCHK(p, hipMemcpyAsync(p->dVar.p, var + t0 * p->k, sizeof(double) * nr * p->k, hipMemcpyHostToDevice, p->stream));
      }
      if ((rc = gprx_pca_reverse_dev(p, p->dMean.p, var ? p->dVar.p : nullptr, nr, p->dFull.p, var ? p->dVfull.p : nullptr))) return rc;
      HIPCHK(p, hipMemcpyAsync(full + t0 * p->cells, p->dFull.p, sizeof(double) * nr * p->cells, hipMemcpyDeviceToHost, p->stream));
      if (var) HIPCHK(p, hipMemcpyAsync(var_full + t0 * p->cells, p->dVfull.p, sizeof(double) * nr * p->cells, hipMemcpyDeviceToHost, p->stream));
      HIPCHK(p, hipStreamSynchronize(p->stream));
    }
    return GPRX_OK;
  });
}

int gprx_pca_slab_rows(gprx_pca_handle p, int64_t* rows) {
  if (!p || !rows) return fail(p, GPRX_EINVAL, "null argument");
  *rows = std::max<int64_t>(64, pca_chunk_doubles() / p->cells_p);
  return GPRX_OK;
}

const char* gprx_pca_last_error(gprx_pca_handle p) { return p ? p->err.c_str() : last_error().c_str(); }

// ---- fitting the EOF preprocessor (PreProcessor.fit, gpras/preprocess.py:947-1007) ---------------------------------------
struct gprx_pcafit_ctx {
  int device = 0, mode = 0;
  int route = GPRX_PCAFIT_GRAM;  // GPRX_PCAFIT_COV: the covariance route of gprx_pcafit_create_auto (pca_fit_tall.h)
  int rowsplit = 1;              // covariance route: the row-split kernels ("pcafit_rowsplit" at the time of the create)
  hipStream_t stream = nullptr;
  int64_t rows = 0, rows_p = 0, cells = 0, n_wet = 0, ldc = 0;  // ldc: leading dimension of the compacted matrices (multiple of 16)
  double *xc1 = nullptr, *xc2 = nullptr, *A = nullptr, *E = nullptr, *Z = nullptr;
  double *G = nullptr;                                    // the Gram matrix (covariance route: the covariance), inside ws
  double *U = nullptr, *lam = nullptr, *eig_ws = nullptr;  // device eigensolver: eigenvectors (gdim, gdim), ascending eigenvalues, workspace
  int64_t gdim() const { return route == GPRX_PCAFIT_COV ? n_wet : rows; }  // order of G
  std::vector<double> lam_h;                               // the eigenvalues, descending (empty before gprx_pcafit_eig)
  double eig_ms = 0.0;
  Buf ws;  // split-K slabs, then their sum
  std::vector<unsigned char> cls;    // wetness class per cell
  std::vector<double> mean, gram;    // input_mean over the wet cells, G (rows, rows)
  hipEvent_t ev[8] = {};
  double ms[6] = {0, 0, 0, 0, 0, 0};  // upload, stats, centring, Gram, components, projection
  std::string err;
};

namespace {
// Device temporaries of a create: x, the per-cell vectors and the operation list; on the covariance route also the leaves, the
// leaf scratch and ("pcafit_rowsplit" = 0) the row-major Xc2.  When the create ends the stream is waited for and they are freed; the
// host copies of what an asynchronous upload reads live as long.
struct PcafitTemps {
  double *X = nullptr, *elev = nullptr, *w = nullptr, *mu = nullptr, *m2 = nullptr, *lsum = nullptr, *lmax = nullptr, *lmin = nullptr, *xc2 = nullptr;
  unsigned char *cls = nullptr, *lnan = nullptr;
  int64_t* idx = nullptr;
  int2 *ops = nullptr, *leaves = nullptr;
  int nops = 0;
  std::vector<int2> ops_h, leaves_h;
  std::vector<int64_t> idx_h;
  DevTemps owner;
  explicit PcafitTemps(hipStream_t st)
      : owner(st, {(void**)&X, (void**)&elev, (void**)&w, (void**)&mu, (void**)&m2, (void**)&lsum, (void**)&lmax, (void**)&lmin, (void**)&xc2, (void**)&cls,
                   (void**)&lnan, (void**)&idx, (void**)&ops, (void**)&leaves}) {}
};

// the operation list T.ops_h goes to the device (a second list replaces the first once the stream has run what read it)
int pcafit_set_ops(gprx_pcafit_handle f, PcafitTemps& T) {
  hipStream_t st = f->stream;
  if (T.ops) {
    HIPCHK(f, hipStreamSynchronize(st));
    HIPCHK(f, hipFree(T.ops));
    T.ops = nullptr;
  }
  T.nops = (int)T.ops_h.size();
  HIPCHK(f, hipMalloc((void**)&T.ops, sizeof(int2) * T.ops_h.size()));
  HIPCHK(f, hipMemcpyAsync(T.ops, T.ops_h.data(), sizeof(int2) * T.ops_h.size(), hipMemcpyHostToDevice, st));
  return GPRX_OK;
}

// x goes up once, with the elevations and the weights
int pcafit_upload(gprx_pcafit_handle f, PcafitTemps& T, const double* x, const double* elevations, const double* weights) {
  const int64_t rows = f->rows, cells = f->cells;
  const size_t xb = sizeof(double) * (size_t)rows * cells;
  hipStream_t st = f->stream;
  HIPCHK(f, hipMalloc((void**)&T.X, xb));
  HIPCHK(f, hipMalloc((void**)&T.mu, sizeof(double) * cells));
  HIPCHK(f, hipMalloc((void**)&T.cls, (size_t)cells));
  if (f->mode != PCAFIT_VELOCITY) {
    HIPCHK(f, hipMalloc((void**)&T.elev, sizeof(double) * cells));
    HIPCHK(f, hipMemcpyAsync(T.elev, elevations, sizeof(double) * cells, hipMemcpyHostToDevice, st));
  }
  if (weights) {
    HIPCHK(f, hipMalloc((void**)&T.w, sizeof(double) * cells));
    HIPCHK(f, hipMemcpyAsync(T.w, weights, sizeof(double) * cells, hipMemcpyHostToDevice, st));
  }
  HIPCHK(f, hipEventRecord(f->ev[0], st));
  HIPCHK(f, hipMemcpyAsync(T.X, x, xb, hipMemcpyHostToDevice, st));
  HIPCHK(f, hipEventRecord(f->ev[1], st));
  return GPRX_OK;
}

// the classes and the column means come down; the wet cells (class != AD) in ascending order: x[:, ~dry_indices]
int pcafit_wet_cells(gprx_pcafit_handle f, PcafitTemps& T, std::vector<double>& mu_h) {
  const int64_t cells = f->cells;
  hipStream_t st = f->stream;
  mu_h.resize((size_t)cells);
  f->cls.resize((size_t)cells);
  HIPCHK(f, hipMemcpyAsync(f->cls.data(), T.cls, (size_t)cells, hipMemcpyDeviceToHost, st));
  HIPCHK(f, hipMemcpyAsync(mu_h.data(), T.mu, sizeof(double) * cells, hipMemcpyDeviceToHost, st));
  HIPCHK(f, hipStreamSynchronize(st));
  T.idx_h.clear();
  T.idx_h.reserve((size_t)cells);
  for (int64_t c = 0; c < cells; ++c)
    if (f->cls[c] != 1) T.idx_h.push_back(c);
  f->n_wet = (int64_t)T.idx_h.size();
  return GPRX_OK;
}

// input_mean over the wet cells and the leading dimension of the compacted matrices, once the route is known
void pcafit_keep_mean(gprx_pcafit_handle f, const PcafitTemps& T, const std::vector<double>& mu_h) {
  f->mean.resize((size_t)f->n_wet);
  for (int64_t j = 0; j < f->n_wet; ++j) f->mean[j] = mu_h[T.idx_h[j]];
  f->ldc = round_up(f->n_wet, 16);
}

// Gram route, steps 2 and 3: compaction + both centrings, Gram matrix
int pcafit_gram_stage(gprx_pcafit_handle f, PcafitTemps& T) {
  const int64_t rows = f->rows, cells = f->cells, ldc = f->ldc;
  hipStream_t st = f->stream;
  // 2. compaction, centring, weighting, then IncrementalPCA's centring; xc2 has rows_p rows (zero beyond `rows`: the K padding
  //    of the components GEMM)
  HIPCHK(f, hipMalloc((void**)&T.idx, sizeof(int64_t) * f->n_wet));
  HIPCHK(f, hipMalloc((void**)&T.m2, sizeof(double) * ldc));
  HIPCHK(f, hipMalloc((void**)&f->xc1, sizeof(double) * rows * ldc));
  HIPCHK(f, hipMalloc((void**)&f->xc2, sizeof(double) * f->rows_p * ldc));
  HIPCHK(f, hipMemcpyAsync(T.idx, T.idx_h.data(), sizeof(int64_t) * f->n_wet, hipMemcpyHostToDevice, st));
  if (f->rows_p > rows) HIPCHK(f, hipMemsetAsync(f->xc2 + rows * ldc, 0, sizeof(double) * (f->rows_p - rows) * ldc, st));
  HIPCHK(f, hipEventRecord(f->ev[3], st));
  hipLaunchKernelGGL(pcafit_compact_kernel, dim3((unsigned)((ldc + 255) / 256)), dim3(256), 0, st, (const double*)T.X, rows, cells,
                     (const int64_t*)T.idx, f->n_wet, ldc, (const double*)T.elev, f->mode, (const double*)T.mu, (const double*)T.w,
                     (const int2*)T.ops, T.nops, f->xc1, f->xc2, T.m2);
  HIPCHK(f, hipGetLastError());
  HIPCHK(f, hipEventRecord(f->ev[4], st));
  // 3. G = Xc2 Xc2^T: lower-triangle tiles, split-K slabs summed in a fixed order
  int rc;
  if ((rc = gram_lower(f, st, f->xc2, ldc, rows, ldc, f->ws, &f->G))) return rc;
  HIPCHK(f, hipEventRecord(f->ev[5], st));
  HIPCHK(f, hipStreamSynchronize(st));  // G stays on the device: gprx_pcafit_gram fetches it on its first call
  f->ms[0] = elapsed_ms(f->ev[0], f->ev[1]);
  f->ms[1] = elapsed_ms(f->ev[1], f->ev[2]);
  f->ms[2] = elapsed_ms(f->ev[3], f->ev[4]);
  f->ms[3] = elapsed_ms(f->ev[4], f->ev[5]);
  return GPRX_OK;
}

// leaf + combine pair over `cols` columns of src (rows, ld): the column sums in the order of T.ops (pca_fit_tall.h)
int pcafit_rowsplit_sums(gprx_pcafit_handle f, PcafitTemps& T, bool stats, const double* src, int64_t ld, int64_t cols, double thr, unsigned char* cls, double* mean) {
  const int64_t nleaves = (int64_t)T.leaves_h.size(), ncb = (cols + PCAFIT_LEAF_COLS - 1) / PCAFIT_LEAF_COLS;
  const int64_t nwg = ncb * ((nleaves + PCAFIT_LEAF_GROUP - 1) / PCAFIT_LEAF_GROUP);
  if (nwg >= ((int64_t)1 << 31)) return fail(f, GPRX_EINVAL, "x is too large for the grid of the leaf pass");
  hipLaunchKernelGGL(stats ? pcafit_leaf_kernel<true> : pcafit_leaf_kernel<false>, dim3((unsigned)nwg), dim3(256), 0, f->stream, src, ld, cols,
                     (const double*)T.elev, f->mode, (const int2*)T.leaves, nleaves, ncb, T.lsum, T.lmax, T.lmin, T.lnan);
  HIPCHK(f, hipGetLastError());
  hipLaunchKernelGGL(stats ? pcafit_combine_kernel<true> : pcafit_combine_kernel<false>, dim3((unsigned)((cols + 255) / 256)), dim3(256), 0, f->stream,
                     (const double*)T.lsum, (const double*)T.lmax, (const double*)T.lmin, (const unsigned char*)T.lnan, cols, f->rows, (const int2*)T.ops,
                     T.nops, f->mode, thr, cls, mean);
  HIPCHK(f, hipGetLastError());
  return GPRX_OK;
}

// Covariance route (pca_fit_tall.h), x on the device already: statistics in numpy's chunked order, compaction, second centring
// written cell-major, C = Xc2^T Xc2.
int pcafit_cov_stage(gprx_pcafit_handle f, PcafitTemps& T, double thr) {
  const int64_t rows = f->rows, rp = f->rows_p, cells = f->cells, cells_p = round_up(cells, 16);
  hipStream_t st = f->stream;
  int rc, depth = 0;
  T.ops_h.clear();
  pcafit_chunked_ops(rows, T.ops_h, depth);
  if (depth > PCAFIT_STACK) return fail(f, GPRX_EINVAL, "too many samples for the pairwise column sums");
  if (T.ops_h.size() >= ((size_t)1 << 31)) return fail(f, GPRX_EINVAL, "too many samples for the operation list");
  T.leaves_h.clear();
  for (const int2& op : T.ops_h)
    if (op.x >= 0) T.leaves_h.push_back(op);
  const int64_t nleaves = (int64_t)T.leaves_h.size();
  if (f->rowsplit) {
    // the leaf scratch serves the statistics (cells columns) and the second centring (ldc <= cells_p columns)
    if ((rc = need_device_bytes(f, 8.0 * (double)nleaves * (cells_p + 2.0 * cells + 1.0) + (double)nleaves * cells + 8.0 * T.ops_h.size(),
                                "the leaf sums of the fit")))
      return rc;
    HIPCHK(f, hipMalloc((void**)&T.leaves, sizeof(int2) * nleaves));
    HIPCHK(f, hipMalloc((void**)&T.lsum, sizeof(double) * nleaves * cells_p));
    HIPCHK(f, hipMalloc((void**)&T.lmax, sizeof(double) * nleaves * cells));
    HIPCHK(f, hipMalloc((void**)&T.lmin, sizeof(double) * nleaves * cells));
    HIPCHK(f, hipMalloc((void**)&T.lnan, (size_t)nleaves * cells));
    HIPCHK(f, hipMemcpyAsync(T.leaves, T.leaves_h.data(), sizeof(int2) * nleaves, hipMemcpyHostToDevice, st));
  }
  if ((rc = pcafit_set_ops(f, T))) return rc;
  // 1. classes and column means
  HIPCHK(f, hipEventRecord(f->ev[6], st));
  if (f->rowsplit) {
    if ((rc = pcafit_rowsplit_sums(f, T, true, T.X, cells, cells, thr, T.cls, T.mu))) return rc;
  } else {
    hipLaunchKernelGGL(pcafit_colstats_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, (const double*)T.X, rows, cells,
                       (const double*)T.elev, f->mode, thr, (const int2*)T.ops, T.nops, T.cls, T.mu);
    HIPCHK(f, hipGetLastError());
  }
  HIPCHK(f, hipEventRecord(f->ev[7], st));
  std::vector<double> mu_h;
  if ((rc = pcafit_wet_cells(f, T, mu_h))) return rc;
  const int64_t n = f->n_wet;
  if (n < 1) return fail(f, GPRX_EINVAL, "the fit needs at least one wet cell");
  if (n > 16384)
    return fail(f, GPRX_EINVAL, "the covariance route needs n_wet <= 16384 (eigendecomposition of n_wet x n_wet): " + std::to_string((long long)n) + " wet cells, " +
                                    std::to_string((long long)rows) + " samples");
  f->route = GPRX_PCAFIT_COV;
  pcafit_keep_mean(f, T, mu_h);
  const int64_t ldc = f->ldc, r2 = ldc;  // rows of Xc2^T: n_wet padded to 16
  const SplitK sk = gram_plan(n, rp);
  if (rp + sk.kchunk >= ((int64_t)1 << 31)) return fail(f, GPRX_EINVAL, "too many samples for the covariance product");
  if ((rc = need_device_bytes(f, 8.0 * ((double)rows * ldc * (f->rowsplit ? 1.0 : 2.0) + (double)r2 * rp + (double)(sk.nsplit + 1) * n * n + 3.0 * ldc),
                              "the covariance route of the fit")))
    return rc;
  // 2. compaction, centring, weighting; IncrementalPCA's centring written as Xc2^T (r2, rows_p), zero padded
  HIPCHK(f, hipMalloc((void**)&T.idx, sizeof(int64_t) * n));
  HIPCHK(f, hipMalloc((void**)&T.m2, sizeof(double) * ldc));
  HIPCHK(f, hipMalloc((void**)&f->xc1, sizeof(double) * rows * ldc));
  HIPCHK(f, hipMalloc((void**)&f->xc2, sizeof(double) * r2 * rp));
  HIPCHK(f, hipMemcpyAsync(T.idx, T.idx_h.data(), sizeof(int64_t) * n, hipMemcpyHostToDevice, st));
  const dim3 tgrid((unsigned)((rp + 31) / 32), (unsigned)((r2 + 31) / 32));
  HIPCHK(f, hipEventRecord(f->ev[3], st));
  if (f->rowsplit) {
    hipLaunchKernelGGL(pcafit_compact_rows_kernel, dim3((unsigned)((ldc + 255) / 256), (unsigned)std::min<int64_t>(rows, 8192)), dim3(256), 0, st,
                       (const double*)T.X, rows, cells, (const int64_t*)T.idx, n, ldc, (const double*)T.elev, f->mode, (const double*)T.mu,
                       (const double*)T.w, f->xc1);
    HIPCHK(f, hipGetLastError());
    if ((rc = pcafit_rowsplit_sums(f, T, false, f->xc1, ldc, ldc, thr, nullptr, T.m2))) return rc;
    hipLaunchKernelGGL(pcafit_centre_t_kernel, tgrid, dim3(256), 0, st, (const double*)f->xc1, rows, ldc, n, (const double*)T.m2, f->xc2, r2, rp);
  } else {
    HIPCHK(f, hipMalloc((void**)&T.xc2, sizeof(double) * rows * ldc));
    hipLaunchKernelGGL(pcafit_compact_kernel, dim3((unsigned)((ldc + 255) / 256)), dim3(256), 0, st, (const double*)T.X, rows, cells,
                       (const int64_t*)T.idx, n, ldc, (const double*)T.elev, f->mode, (const double*)T.mu, (const double*)T.w, (const int2*)T.ops,
                       T.nops, f->xc1, T.xc2, T.m2);
    HIPCHK(f, hipGetLastError());
    hipLaunchKernelGGL(pcafit_centre_t_kernel, tgrid, dim3(256), 0, st, (const double*)T.xc2, rows, ldc, n, (const double*)nullptr, f->xc2, r2, rp);
  }
  HIPCHK(f, hipGetLastError());
  HIPCHK(f, hipEventRecord(f->ev[4], st));
  // 3. C = Xc2^T Xc2 (n_wet, n_wet): the Gram stage on the cell-major matrix, K = rows_p
  if ((rc = gram_lower(f, st, f->xc2, rp, n, rp, f->ws, &f->G))) return rc;
  HIPCHK(f, hipEventRecord(f->ev[5], st));
  HIPCHK(f, hipStreamSynchronize(st));
  HIPCHK(f, hipFree(f->xc2));  // the components of this route are the eigenvectors themselves: Xc2^T is not read again
  f->xc2 = nullptr;
  f->ms[0] = elapsed_ms(f->ev[0], f->ev[1]);
  f->ms[1] = elapsed_ms(f->ev[6], f->ev[7]);
  f->ms[2] = elapsed_ms(f->ev[3], f->ev[4]);
  f->ms[3] = elapsed_ms(f->ev[4], f->ev[5]);
  return GPRX_OK;
}

// steps 1-3.  auto_route: fewer wet cells than samples, or a shape the Gram route does not take, goes to the covariance route
int pcafit_run(gprx_pcafit_handle f, const double* x, const double* elevations, const double* weights, double thr, bool auto_route) {
  const int64_t rows = f->rows, cells = f->cells;
  const double xb = 8.0 * (double)rows * cells;
  hipStream_t st = f->stream;
  PcafitTemps T(st);
  int rc;
  if (!auto_route || (rows <= cells && rows <= 16384)) {
    // device memory of the whole fit, before anything is allocated: x, per-cell vectors, both compacted matrices, Gram slabs
    const int64_t ldc_max = round_up(cells, 16);
    const int64_t nsplit = gram_plan(rows, ldc_max).nsplit;
    const double need = xb + 8.0 * (4.0 * cells + (double)(rows + f->rows_p) * ldc_max + (double)(nsplit + 1) * rows * rows) + cells;
    if ((rc = need_device_bytes(f, need, "the fit"))) return rc;
    int depth = 0;
    pcafit_pairwise_ops(0, (int)rows, 0, T.ops_h, depth);
    if (depth > PCAFIT_STACK) return fail(f, GPRX_EINVAL, "too many samples for the pairwise column sums");
    if ((rc = pcafit_set_ops(f, T)) || (rc = pcafit_upload(f, T, x, elevations, weights))) return rc;
    // 1. x goes up once; one pass gives the classes and the column means
    hipLaunchKernelGGL(pcafit_colstats_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st, (const double*)T.X, rows, cells,
                       (const double*)T.elev, f->mode, thr, (const int2*)T.ops, T.nops, T.cls, T.mu);
    HIPCHK(f, hipGetLastError());
    HIPCHK(f, hipEventRecord(f->ev[2], st));
    std::vector<double> mu_h;
    if ((rc = pcafit_wet_cells(f, T, mu_h))) return rc;
    if (f->n_wet >= rows) {
      pcafit_keep_mean(f, T, mu_h);
      return pcafit_gram_stage(f, T);
    }
    if (!auto_route)
      return fail(f, GPRX_EINVAL, "the fit needs at least as many wet cells as samples: " + std::to_string((long long)f->n_wet) + " wet cells, " +
                                       std::to_string((long long)rows) + " samples");
  } else {
    if ((rc = need_device_bytes(f, xb + 8.0 * 4.0 * cells + cells, "the fit")) || (rc = pcafit_upload(f, T, x, elevations, weights))) return rc;
  }
  return pcafit_cov_stage(f, T, thr);
}

// the blocks of the components step: A (k, rows_p), E (k, ldc), Z (rows, k)
int pcafit_components_alloc(gprx_pcafit_handle f, int k) {
  if (f->A) HIPCHK(f, hipFree(f->A));
  if (f->E) HIPCHK(f, hipFree(f->E));
  if (f->Z) HIPCHK(f, hipFree(f->Z));
  f->A = f->E = f->Z = nullptr;
  HIPCHK(f, hipMalloc((void**)&f->A, sizeof(double) * (size_t)k * f->rows_p));
  HIPCHK(f, hipMalloc((void**)&f->E, sizeof(double) * (size_t)k * f->ldc));
  HIPCHK(f, hipMalloc((void**)&f->Z, sizeof(double) * (size_t)f->rows * k));
  return GPRX_OK;
}

// steps 5 and 6 from A = diag(lambda^-1/2) U_k^T on the device (K padded to rows_p with zeros); covariance route: from the
// eigenvectors in the rows of E
int pcafit_project(gprx_pcafit_handle f, int k, double* eofs, double* z) {
  const int64_t rows = f->rows, rp = f->rows_p, ldc = f->ldc;
  hipStream_t st = f->stream;
  const SplitK sk = splitk_plan((rows + 63) / 64 * ((k + 63) / 64), ldc, rows * k);
  int rc;
  if ((rc = ensure(f, f->ws, sizeof(double) * (size_t)sk.nsplit * rows * k))) return rc;
  // 5. E = A Xc2, then svd_flip on its rows (covariance route: E holds the eigenvectors already, only the flip is left)
  HIPCHK(f, hipEventRecord(f->ev[5], st));
  if (f->route == GPRX_PCAFIT_COV) {
    hipLaunchKernelGGL(pcafit_sign_flip_kernel, dim3((unsigned)k), dim3(256), 0, st, f->E, ldc, f->n_wet);
    HIPCHK(f, hipGetLastError());
  } else if ((rc = components_gemm(f, st, k, f->A, rp, f->xc2, ldc, f->n_wet, f->E))) {
    return rc;
  }
  HIPCHK(f, hipEventRecord(f->ev[6], st));
  // 6. Z = Xc1 E^T (split-K NT; the padding columns of both operands are zero)
  HIPCHK(f, launch_gemm_splitk(st, 0, 1, (int)rows, k, (int)ldc, 1.0, f->xc1, ldc, f->E, ldc, 0.0, f->Z, k, f->ws.p, sk.kchunk));
  HIPCHK(f, hipEventRecord(f->ev[7], st));
  HIPCHK(f, hipMemcpy2DAsync(eofs, sizeof(double) * f->n_wet, f->E, sizeof(double) * ldc, sizeof(double) * f->n_wet, (size_t)k,
                             hipMemcpyDeviceToHost, st));
  HIPCHK(f, hipMemcpyAsync(z, f->Z, sizeof(double) * rows * k, hipMemcpyDeviceToHost, st));
  HIPCHK(f, hipStreamSynchronize(st));
  f->ms[4] = elapsed_ms(f->ev[5], f->ev[6]);
  f->ms[5] = elapsed_ms(f->ev[6], f->ev[7]);
  return GPRX_OK;
}

// step 4 on the device: G = U diag(lambda) U^T by the block Jacobi solver (eig_jacobi.h); G is overwritten
int pcafit_eig(gprx_pcafit_handle f, int* sweeps) {
  const int64_t rows = f->gdim();  // the order of G: n_samples, or n_wet on the covariance route
  hipStream_t st = f->stream;
  const size_t wsb = eig_jacobi_workspace_bytes((int)rows);
  int rc;
  if ((rc = need_device_bytes(f, 8.0 * ((double)rows * rows + rows) + (double)wsb, "the eigensolver"))) return rc;
  HIPCHK(f, hipMalloc((void**)&f->U, sizeof(double) * rows * rows));
  HIPCHK(f, hipMalloc((void**)&f->lam, sizeof(double) * rows));
  HIPCHK(f, hipMalloc((void**)&f->eig_ws, wsb));
  double off_rel = 0.0;
  std::string msg;
  HIPCHK(f, hipEventRecord(f->ev[6], st));
  if ((rc = eig_jacobi_run(st, (int)rows, f->G, rows, f->U, rows, f->lam, f->eig_ws, sweeps, &off_rel, &msg))) return fail(f, rc, msg);
  HIPCHK(f, hipEventRecord(f->ev[7], st));
  std::vector<double> asc((size_t)rows);
  HIPCHK(f, hipMemcpyAsync(asc.data(), f->lam, sizeof(double) * rows, hipMemcpyDeviceToHost, st));
  HIPCHK(f, hipStreamSynchronize(st));
  f->eig_ms = elapsed_ms(f->ev[6], f->ev[7]);
  f->lam_h.assign(asc.rbegin(), asc.rend());
  return GPRX_OK;
}
}  // namespace

int gprx_pcafit_destroy(gprx_pcafit_handle f) {
  if (!f) return GPRX_OK;
  release_handle(f->device, f->stream, {f->xc1, f->xc2, f->ws.p, f->A, f->E, f->Z, f->U, f->lam, f->eig_ws}, f->ev, 8);
  delete f;
  return GPRX_OK;
}

int gprx_pcafit_create(int device, const double* x, int64_t n_samples, int64_t n_cells, const double* elevations, const double* weights,
                       int mode, double wet_threshold, gprx_pcafit_handle* out) {
  if (!out) return fail(nullptr, GPRX_EINVAL, "out is null");
  *out = nullptr;
  if (!x) return fail(nullptr, GPRX_EINVAL, "x is null");
  if (mode < PCAFIT_WSE || mode > PCAFIT_VELOCITY) return fail(nullptr, GPRX_EINVAL, "mode must be 0 (wse), 1 (depth) or 2 (velocity)");
  if (mode != PCAFIT_VELOCITY && !elevations) return fail(nullptr, GPRX_EINVAL, "wse and depth need the cell elevations");
  if (n_samples < 2 || n_cells < n_samples || n_samples > 16384)
    return fail(nullptr, GPRX_EINVAL, "need 2 <= n_samples <= min(n_cells, 16384)");
  gprx_pcafit_handle f = nullptr;
  const int rc = guarded(nullptr, [&]() -> int {
    f = new gprx_pcafit_ctx();
    f->mode = mode;
    f->rows = n_samples;
    f->rows_p = round_up(n_samples, 16);
    f->cells = n_cells;
    const int rc = open_handle(f, device, f->ev, 8);
    return rc ? rc : pcafit_run(f, x, elevations, weights, wet_threshold, false);
  });
  if (rc) gprx_pcafit_destroy(f);
  else *out = f;
  return rc;
}

int gprx_pcafit_create_auto(int device, const double* x, int64_t n_samples, int64_t n_cells, const double* elevations, const double* weights,
                            int mode, double wet_threshold, int* route, gprx_pcafit_handle* out) {
  if (!out) return fail(nullptr, GPRX_EINVAL, "out is null");
  *out = nullptr;
  if (!x || !route) return fail(nullptr, GPRX_EINVAL, "x or route is null");
  if (mode < PCAFIT_WSE || mode > PCAFIT_VELOCITY) return fail(nullptr, GPRX_EINVAL, "mode must be 0 (wse), 1 (depth) or 2 (velocity)");
  if (mode != PCAFIT_VELOCITY && !elevations) return fail(nullptr, GPRX_EINVAL, "wse and depth need the cell elevations");
  if (n_samples < 2 || n_cells < 1 || n_samples >= ((int64_t)1 << 31) - 16) return fail(nullptr, GPRX_EINVAL, "need 2 <= n_samples < 2^31 - 16 and n_cells >= 1");
  gprx_pcafit_handle f = nullptr;
  const int rc = guarded(nullptr, [&]() -> int {
    f = new gprx_pcafit_ctx();
    f->mode = mode;
    f->rows = n_samples;
    f->rows_p = round_up(n_samples, 16);
    f->cells = n_cells;
    f->rowsplit = pcafit_rowsplit_tuning();
    const int rc = open_handle(f, device, f->ev, 8);
    return rc ? rc : pcafit_run(f, x, elevations, weights, wet_threshold, true);
  });
  if (rc) {
    gprx_pcafit_destroy(f);
  } else {
    *route = f->route;
    *out = f;
  }
  return rc;
}

namespace {
const char* pcafit_route_name(gprx_pcafit_handle f) { return f->route == GPRX_PCAFIT_COV ? "covariance" : "Gram"; }

int pcafit_wrong_route(gprx_pcafit_handle f, const char* call, const char* instead) {
  return fail(f, GPRX_ESTATE, std::string(call) + ": this handle took the " + pcafit_route_name(f) + " route; call " + instead);
}

// classes, input_mean, G (gdim, gdim) and n_wet to the host; G comes down from the device on the first call
int pcafit_fetch(gprx_pcafit_handle f, unsigned char* classes, double* input_mean, double* g, int64_t* n_wet, const char* what) {
  if (f->gram.empty()) {
    if (f->U) return fail(f, GPRX_ESTATE, std::string("the device eigensolver has overwritten the ") + what + " matrix of this handle");
    if (f->A) return fail(f, GPRX_ESTATE, std::string("the components step has reused the block that held the ") + what + " matrix");
    const int rc = guarded(f, [&]() -> int {
      HIPCHK(f, hipSetDevice(f->device));
      const size_t n = (size_t)f->gdim();
      f->gram.resize(n * n);
      const hipError_t e = hipMemcpyAsync(f->gram.data(), f->G, sizeof(double) * n * n, hipMemcpyDeviceToHost, f->stream);
      const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(f->stream) : e;
      if (e2 != hipSuccess) {
        f->gram.clear();
        return fail(f, GPRX_EHIP, std::string("download of the ") + what + " matrix: " + hipGetErrorString(e2));
      }
      return GPRX_OK;
    });
    if (rc) return rc;
  }
  std::memcpy(classes, f->cls.data(), f->cls.size());
  std::memcpy(input_mean, f->mean.data(), sizeof(double) * f->mean.size());
  std::memcpy(g, f->gram.data(), sizeof(double) * f->gram.size());
  *n_wet = f->n_wet;
  return GPRX_OK;
}
}  // namespace

int gprx_pcafit_gram(gprx_pcafit_handle f, unsigned char* classes, double* input_mean, double* gram, int64_t* n_wet) {
  if (!f) return fail(f, GPRX_EINVAL, "null handle");
  if (!classes || !input_mean || !gram || !n_wet) return fail(f, GPRX_EINVAL, "null argument");
  if (f->route != GPRX_PCAFIT_GRAM) return pcafit_wrong_route(f, "gprx_pcafit_gram", "gprx_pcafit_cov");
  return pcafit_fetch(f, classes, input_mean, gram, n_wet, "Gram");
}

int gprx_pcafit_cov(gprx_pcafit_handle f, unsigned char* classes, double* input_mean, double* cov, int64_t* n_wet) {
  if (!f) return fail(f, GPRX_EINVAL, "null handle");
  if (!classes || !input_mean || !cov || !n_wet) return fail(f, GPRX_EINVAL, "null argument");
  if (f->route != GPRX_PCAFIT_COV) return pcafit_wrong_route(f, "gprx_pcafit_cov", "gprx_pcafit_gram");
  return pcafit_fetch(f, classes, input_mean, cov, n_wet, "covariance");
}

int gprx_pcafit_components(gprx_pcafit_handle f, int k, const double* u, const double* lam, double* eofs, double* z) {
  if (!f) return fail(f, GPRX_EINVAL, "null handle");
  if (f->route != GPRX_PCAFIT_GRAM) return pcafit_wrong_route(f, "gprx_pcafit_components", "gprx_pcafit_components_cov");
  return guarded(f, [&]() -> int {
    int rc;
    if ((rc = check_components(f, k, f->rows, "n_samples", !u || !lam || !eofs || !z, lam)) || k == 0) return rc;
    HIPCHK(f, hipSetDevice(f->device));
    std::vector<double> a;  // read by the upload until pcafit_project has waited for the stream
    if ((rc = pcafit_components_alloc(f, k)) || (rc = upload_scaled_ut(f, f->stream, u, lam, k, f->rows, f->rows_p, a, f->A))) return rc;
    return pcafit_project(f, k, eofs, z);
  });
}

int gprx_pcafit_components_cov(gprx_pcafit_handle f, int k, const double* v, double* eofs, double* z) {
  if (!f) return fail(f, GPRX_EINVAL, "null handle");
  if (f->route != GPRX_PCAFIT_COV) return pcafit_wrong_route(f, "gprx_pcafit_components_cov", "gprx_pcafit_components");
  return guarded(f, [&]() -> int {
    if (k < 0 || k >= f->rows || k > f->n_wet) return fail(f, GPRX_EINVAL, "need 0 <= k <= min(n_samples - 1, n_wet) (centring removes one direction)");
    if (k == 0) return GPRX_OK;
    if (!v || !eofs || !z) return fail(f, GPRX_EINVAL, "null argument");
    HIPCHK(f, hipSetDevice(f->device));
    int rc;
    if ((rc = pcafit_components_alloc(f, k))) return rc;
    // the eigenvectors are the components: rows of E, padding columns zero (pcafit_project waits for the stream before v may go)
    HIPCHK(f, hipMemsetAsync(f->E, 0, sizeof(double) * (size_t)k * f->ldc, f->stream));
    HIPCHK(f, hipMemcpy2DAsync(f->E, sizeof(double) * f->ldc, v, sizeof(double) * f->n_wet, sizeof(double) * f->n_wet, (size_t)k, hipMemcpyHostToDevice,
                               f->stream));
    return pcafit_project(f, k, eofs, z);
  });
}

int gprx_pcafit_eig(gprx_pcafit_handle f, unsigned char* classes, double* input_mean, double* lam, int64_t* n_wet, int* sweeps) {
  if (!f) return fail(f, GPRX_EINVAL, "null handle");
  if (!classes || !input_mean || !lam || !n_wet || !sweeps) return fail(f, GPRX_EINVAL, "null argument");
  if (f->U) return fail(f, GPRX_ESTATE, "the eigensolver has run on this handle: it overwrites the Gram matrix");
  if (f->A) return fail(f, GPRX_ESTATE, "the components step has reused the block that held the Gram matrix: call gprx_pcafit_eig before it");
  const int rc = guarded(f, [&]() -> int { HIPCHK(f, hipSetDevice(f->device)); return pcafit_eig(f, sweeps); });
  if (rc) return rc;
  std::memcpy(classes, f->cls.data(), f->cls.size());
  std::memcpy(input_mean, f->mean.data(), sizeof(double) * f->mean.size());
  std::memcpy(lam, f->lam_h.data(), sizeof(double) * f->lam_h.size());
  *n_wet = f->n_wet;
  return GPRX_OK;
}

int gprx_pcafit_components_dev(gprx_pcafit_handle f, int k, double* eofs, double* z) {
  if (!f) return fail(f, GPRX_EINVAL, "null handle");
  if (f->lam_h.empty()) return fail(f, GPRX_ESTATE, "gprx_pcafit_eig has not run on this handle");
  return guarded(f, [&]() -> int {
    int rc;
    if (f->route == GPRX_PCAFIT_COV && k > f->n_wet) return fail(f, GPRX_EINVAL, "need 0 <= k <= min(n_samples - 1, n_wet) (the covariance has n_wet eigenpairs)");
    if ((rc = check_components(f, k, f->rows, "n_samples", !eofs || !z, f->lam_h.data())) || k == 0) return rc;
    HIPCHK(f, hipSetDevice(f->device));
    if ((rc = pcafit_components_alloc(f, k))) return rc;
    if (f->route == GPRX_PCAFIT_COV) {
      // the leading eigenvector columns of U, gathered as the rows of E
      const int64_t total = (int64_t)k * f->ldc;
      hipLaunchKernelGGL(pcafit_gather_v_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, f->stream, (const double*)f->U, f->n_wet, k, f->E,
                         f->ldc);
    } else {
      const int64_t total = (int64_t)k * f->rows_p;
      hipLaunchKernelGGL(pcafit_scale_u_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, f->stream, (const double*)f->U, (const double*)f->lam,
                         f->rows, f->rows_p, k, f->A);
    }
    HIPCHK(f, hipGetLastError());
    return pcafit_project(f, k, eofs, z);
  });
}

int gprx_pcafit_eig_ms(gprx_pcafit_handle f, double* ms) {
  if (!f || !ms) return fail(f, GPRX_EINVAL, "null argument");
  *ms = f->eig_ms;
  return GPRX_OK;
}

int gprx_pcafit_timings(gprx_pcafit_handle f, double* ms) {
  if (!f || !ms) return fail(f, GPRX_EINVAL, "null argument");
  for (int i = 0; i < 6; ++i) ms[i] = f->ms[i];
  return GPRX_OK;
}

const char* gprx_pcafit_last_error(gprx_pcafit_handle f) { return f ? f->err.c_str() : last_error().c_str(); }

// ---- HmsPreProcessor (gpras/preprocess.py:1165-1320): the precip EOF fit, the features and the API ---------------------------
struct gprx_hms_ctx {
  int device = 0, route = -1;
  hipStream_t stream = nullptr;
  int64_t rows = 0, nfeat = 0, n_bc = 0, p = 0, ld2 = 0;
  double *X = nullptr, *mu = nullptr, *X2 = nullptr;  // X: x column-major (rows, nfeat), ldx = rows
  Buf ws;  // split-K slabs, then their sum
  int64_t *bc = nullptr, *pc = nullptr;
  std::vector<int64_t> bc_h, pc_h;
  std::vector<double> mu_h;  // input_mean (nfeat)
  hipEvent_t ev[8] = {};
  double ms[7] = {0, 0, 0, 0, 0, 0, 0};  // upload, column pass, covariance / Gram, components, projection, API, statistics / standardise
  std::string err;
};

namespace {
// x goes up once and is kept column-major: an F-order x is copied as it is, a C-order x in row chunks through a staging buffer
int hms_upload(gprx_hms_handle h, const double* x, int64_t ld, int fortran) {
  const int64_t rows = h->rows, nf = h->nfeat;
  hipStream_t st = h->stream;
  HIPCHK(h, hipEventRecord(h->ev[0], st));
  if (fortran) {
    HIPCHK(h, hipMemcpy2DAsync(h->X, sizeof(double) * rows, x, sizeof(double) * ld, sizeof(double) * rows, (size_t)nf, hipMemcpyHostToDevice, st));
  } else {
    const int64_t chunk = std::min<int64_t>(rows, std::max<int64_t>(32, ((int64_t)1 << 22) / nf));  // <= 32 MiB staged
    double* S = nullptr;
    HIPCHK(h, hipMalloc((void**)&S, sizeof(double) * (size_t)chunk * nf));
    int rc = GPRX_OK;
    for (int64_t t0 = 0; t0 < rows && !rc; t0 += chunk) {
      const int64_t tc = std::min(chunk, rows - t0);
      hipError_t e = hipMemcpy2DAsync(S, sizeof(double) * nf, x + t0 * ld, sizeof(double) * ld, sizeof(double) * nf, (size_t)tc, hipMemcpyHostToDevice, st);
      if (e == hipSuccess) {
        hipLaunchKernelGGL(hms_transpose_kernel, dim3((unsigned)((tc + 31) / 32), (unsigned)((nf + 31) / 32)), dim3(256), 0, st, (const double*)S, tc, nf,
                           h->X + t0, rows);
        e = hipGetLastError();
      }
      if (e != hipSuccess) rc = fail(h, GPRX_EHIP, std::string("upload of x: ") + hipGetErrorString(e));
    }
    hipStreamSynchronize(st);  // the staging buffer is no longer read
    hipFree(S);
    if (rc) return rc;
  }
  HIPCHK(h, hipEventRecord(h->ev[1], st));
  return GPRX_OK;
}

// column pass and the covariance (route HMS_COV: C = X2^T X2, p x p) or Gram (HMS_GRAM: G = X2 X2^T, rows x rows) of the PCA input
int hms_cov(gprx_hms_handle h, double* cov) {
  const int64_t rows = h->rows, p = h->p;
  hipStream_t st = h->stream;
  const int route = rows >= p ? HMS_COV : HMS_GRAM;
  const int64_t n = route == HMS_COV ? p : rows;
  const int64_t ld2 = round_up(route == HMS_COV ? rows : p, 16), r2 = round_up(n, 16);
  int rc;
  if ((rc = need_device_bytes(h, 8.0 * ((double)r2 * ld2 + (double)(gram_plan(n, ld2).nsplit + 1) * n * n + p), "the covariance"))) return rc;
  double* m2 = nullptr;
  DevTemps tmp(st, {(void**)&m2});
  HIPCHK(h, hipMalloc((void**)&m2, sizeof(double) * p));
  HIPCHK(h, hipMalloc((void**)&h->X2, sizeof(double) * (size_t)r2 * ld2));
  h->ld2 = ld2;
  h->route = route;
  HIPCHK(h, hipEventRecord(h->ev[2], st));
  hipLaunchKernelGGL(hms_colmean_kernel, dim3((unsigned)h->nfeat), dim3(256), 0, st, (const double*)h->X, rows, rows, (const int64_t*)nullptr,
                     (const double*)nullptr, h->mu);
  hipLaunchKernelGGL(hms_colmean_kernel, dim3((unsigned)p), dim3(256), 0, st, (const double*)h->X, rows, rows, (const int64_t*)h->pc,
                     (const double*)h->mu, m2);
  if (r2 > n) HIPCHK(h, hipMemsetAsync(h->X2 + n * ld2, 0, sizeof(double) * (size_t)(r2 - n) * ld2, st));
  hipLaunchKernelGGL(hms_centre2_kernel, dim3((unsigned)((ld2 + 255) / 256), (unsigned)(route == HMS_COV ? p : rows)), dim3(256), 0, st,
                     (const double*)h->X, rows, rows, (const int64_t*)h->pc, p, (const double*)h->mu, (const double*)m2, route, h->X2, ld2);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[3], st));
  double* C = nullptr;
  if ((rc = gram_lower(h, st, h->X2, ld2, n, ld2, h->ws, &C))) return rc;
  HIPCHK(h, hipEventRecord(h->ev[4], st));
  h->mu_h.resize((size_t)h->nfeat);
  HIPCHK(h, hipMemcpyAsync(h->mu_h.data(), h->mu, sizeof(double) * h->nfeat, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(cov, C, sizeof(double) * n * n, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  h->ms[1] = elapsed_ms(h->ev[2], h->ev[3]);
  h->ms[2] = elapsed_ms(h->ev[3], h->ev[4]);
  return GPRX_OK;
}

// Gram route: E = diag(lambda^-1/2) U_k^T X2 (GEMM, K = rows padded to 16), svd_flip on its rows (pcafit_sign_flip_kernel)
int hms_components(gprx_hms_handle h, int k, const double* u, const double* lam, double* eofs) {
  const int64_t rows = h->rows, rp = round_up(rows, 16), ld2 = h->ld2;
  hipStream_t st = h->stream;
  int rc;
  if ((rc = need_device_bytes(h, 8.0 * ((double)k * rp + (double)k * ld2), "the components"))) return rc;
  std::vector<double> a;  // declared before tmp: it outlives the wait for the stream that reads it
  double *A = nullptr, *E = nullptr;
  DevTemps tmp(st, {(void**)&A, (void**)&E});
  HIPCHK(h, hipMalloc((void**)&A, sizeof(double) * (size_t)k * rp));
  HIPCHK(h, hipMalloc((void**)&E, sizeof(double) * (size_t)k * ld2));
  if ((rc = upload_scaled_ut(h, st, u, lam, k, rows, rp, a, A))) return rc;
  HIPCHK(h, hipEventRecord(h->ev[4], st));
  if ((rc = components_gemm(h, st, k, A, rp, h->X2, ld2, h->p, E))) return rc;
  HIPCHK(h, hipEventRecord(h->ev[5], st));
  HIPCHK(h, hipMemcpy2DAsync(eofs, sizeof(double) * h->p, E, sizeof(double) * ld2, sizeof(double) * h->p, (size_t)k, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  h->ms[3] = elapsed_ms(h->ev[4], h->ev[5]);
  return GPRX_OK;
}

// API on device vectors: lags = how many lags are summed (>= n_w: the weights beyond n_w are zeros)
hipError_t hms_api_launch(hipStream_t st, const double* a, int64_t n, const double* w, int64_t n_w, int64_t lags, double* out) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(hms_api_kernel, dim3((unsigned)((n + HMS_API_BT - 1) / HMS_API_BT)), dim3(HMS_API_NT), 0, st, a, n, w, n_w, lags, out);
  return hipGetLastError();
}

// features [x_bc, x_precip eofs^T, avg_precip, api_1, api_2] (:1251-1257, :1271-1277); fit: x_mean / x_std out; transform: out
int hms_features(gprx_hms_handle h, int ke, const double* eofs, const double* w1, int64_t n1, const double* w2, int64_t n2, double* x_mean,
                 double* x_std, int fit, double* out) {
  const int64_t rows = h->rows, p = h->p, n_bc = h->n_bc, nf = n_bc + ke + 3;
  hipStream_t st = h->stream;
  const int nmb = std::max(1, (ke + HMS_MB - 1) / HMS_MB);
  const int64_t ke_pad = (int64_t)nmb * HMS_MB;
  std::vector<double> et((size_t)p * ke_pad, 0.0), mup((size_t)p), mub((size_t)std::max<int64_t>(n_bc, 1), 0.0);
  for (int i = 0; i < ke; ++i)
    for (int64_t j = 0; j < p; ++j) et[(size_t)j * ke_pad + i] = eofs[(size_t)i * p + j];
  for (int64_t j = 0; j < p; ++j) mup[j] = h->mu_h[h->pc_h[j]];
  for (int64_t b = 0; b < n_bc; ++b) mub[b] = h->mu_h[h->bc_h[b]];
  int rc;
  if ((rc = need_device_bytes(h, 8.0 * ((double)et.size() + p + n_bc + n1 + n2 + 2.0 * nf + (double)nf * rows * (fit ? 1 : 2)) + 64, "the features")))
    return rc;
  double *Et = nullptr, *Mp = nullptr, *Mb = nullptr, *W1 = nullptr, *W2 = nullptr, *F = nullptr, *S = nullptr, *O = nullptr;
  int* flag = nullptr;
  DevTemps tmp(st, {(void**)&Et, (void**)&Mp, (void**)&Mb, (void**)&W1, (void**)&W2, (void**)&F, (void**)&S, (void**)&O, (void**)&flag});
  HIPCHK(h, hipMalloc((void**)&Et, sizeof(double) * et.size()));
  HIPCHK(h, hipMalloc((void**)&Mp, sizeof(double) * p));
  HIPCHK(h, hipMalloc((void**)&Mb, sizeof(double) * mub.size()));
  HIPCHK(h, hipMalloc((void**)&W1, sizeof(double) * std::max<int64_t>(n1, 1)));
  HIPCHK(h, hipMalloc((void**)&W2, sizeof(double) * std::max<int64_t>(n2, 1)));
  HIPCHK(h, hipMalloc((void**)&F, sizeof(double) * (size_t)nf * rows));
  HIPCHK(h, hipMalloc((void**)&S, sizeof(double) * 2 * nf));
  HIPCHK(h, hipMalloc((void**)&flag, sizeof(int)));
  HIPCHK(h, hipMemcpyAsync(Et, et.data(), sizeof(double) * et.size(), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(Mp, mup.data(), sizeof(double) * p, hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(Mb, mub.data(), sizeof(double) * mub.size(), hipMemcpyHostToDevice, st));
  if (n1) HIPCHK(h, hipMemcpyAsync(W1, w1, sizeof(double) * n1, hipMemcpyHostToDevice, st));
  if (n2) HIPCHK(h, hipMemcpyAsync(W2, w2, sizeof(double) * n2, hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemsetAsync(flag, 0, sizeof(int), st));
  HIPCHK(h, hipEventRecord(h->ev[5], st));
  hipLaunchKernelGGL(hms_project_kernel, dim3((unsigned)((rows + 255) / 256), (unsigned)nmb), dim3(256), 0, st, (const double*)h->X, rows, rows,
                     (const int64_t*)h->pc, (const double*)Mp, p, (const double*)Et, ke_pad, ke, (const int64_t*)h->bc, (const double*)Mb, n_bc, F,
                     rows, flag);
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[6], st));
  int nonfinite = 0;
  HIPCHK(h, hipMemcpyAsync(&nonfinite, flag, sizeof(int), hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipStreamSynchronize(st));
  // the exactly-zero tail of the weights is cut only when avg_precip is finite (0 * inf or 0 * NaN would be NaN)
  const double* a = F + (n_bc + ke) * rows;
  HIPCHK(h, hms_api_launch(st, a, rows, W1, n1, nonfinite ? rows : std::min(n1, rows), F + (n_bc + ke + 1) * rows));
  HIPCHK(h, hms_api_launch(st, a, rows, W2, n2, nonfinite ? rows : std::min(n2, rows), F + (n_bc + ke + 2) * rows));
  HIPCHK(h, hipEventRecord(h->ev[7], st));
  if (fit) {
    hipLaunchKernelGGL(hms_colstats_kernel, dim3((unsigned)nf), dim3(256), 0, st, (const double*)F, rows, rows, S, S + nf);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev[0], st));
    HIPCHK(h, hipMemcpyAsync(x_mean, S, sizeof(double) * nf, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(x_std, S + nf, sizeof(double) * nf, hipMemcpyDeviceToHost, st));
  } else {
    HIPCHK(h, hipMalloc((void**)&O, sizeof(double) * (size_t)nf * rows));
    HIPCHK(h, hipMemcpyAsync(S, x_mean, sizeof(double) * nf, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(S + nf, x_std, sizeof(double) * nf, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(hms_standardise_kernel, dim3((unsigned)((nf * rows + 255) / 256)), dim3(256), 0, st, (const double*)F, rows, rows, nf,
                       (const double*)S, (const double*)(S + nf), O);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev[0], st));
    HIPCHK(h, hipMemcpyAsync(out, O, sizeof(double) * nf * rows, hipMemcpyDeviceToHost, st));
  }
  HIPCHK(h, hipStreamSynchronize(st));
  h->ms[4] = elapsed_ms(h->ev[5], h->ev[6]);
  h->ms[5] = elapsed_ms(h->ev[6], h->ev[7]);
  h->ms[6] = elapsed_ms(h->ev[7], h->ev[0]);
  return GPRX_OK;
}
}  // namespace

int gprx_hms_destroy(gprx_hms_handle h) {
  if (!h) return GPRX_OK;
  release_handle(h->device, h->stream, {h->X, h->mu, h->X2, h->ws.p, h->bc, h->pc}, h->ev, 8);
  delete h;
  return GPRX_OK;
}

int gprx_hms_create(int device, const double* x, int64_t rows, int64_t ld, int64_t n_features, int fortran, const int64_t* bc_idx, int64_t n_bc,
                    const int64_t* precip_idx, int64_t n_precip, const double* input_mean, gprx_hms_handle* out) {
  if (!out) return fail(nullptr, GPRX_EINVAL, "out is null");
  *out = nullptr;
  if (!x || !precip_idx || (n_bc > 0 && !bc_idx)) return fail(nullptr, GPRX_EINVAL, "null argument");
  if (rows < 1 || n_features < 1 || n_bc < 0 || n_precip < 1) return fail(nullptr, GPRX_EINVAL, "need rows >= 1 and at least one precip column");
  if (ld < (fortran ? rows : n_features)) return fail(nullptr, GPRX_EINVAL, "ld is smaller than the contiguous dimension of x");
  if (rows > ((int64_t)1 << 31) - 1024 || n_features > 65535 * 32) return fail(nullptr, GPRX_EINVAL, "x is too large");
  for (int64_t j = 0; j < n_precip; ++j)
    if (precip_idx[j] < 0 || precip_idx[j] >= n_features) return fail(nullptr, GPRX_EINVAL, "precip column out of range");
  for (int64_t j = 0; j < n_bc; ++j)
    if (bc_idx[j] < 0 || bc_idx[j] >= n_features) return fail(nullptr, GPRX_EINVAL, "bc column out of range");
  if (std::min(rows, n_precip) > 16384) return fail(nullptr, GPRX_EINVAL, "min(rows, precip columns) must be <= 16384 (host eigh)");
  gprx_hms_handle h = nullptr;
  const int rc = guarded(nullptr, [&]() -> int {
    h = new gprx_hms_ctx();
    h->rows = rows;
    h->nfeat = n_features;
    h->n_bc = n_bc;
    h->p = n_precip;
    h->bc_h.assign(bc_idx, bc_idx + n_bc);
    h->pc_h.assign(precip_idx, precip_idx + n_precip);
    int rc = open_handle(h, device, h->ev, 8);
    const double staged = fortran ? 0.0 : (double)std::min<int64_t>(rows, std::max<int64_t>(32, ((int64_t)1 << 22) / n_features)) * n_features;
    if (rc || (rc = need_device_bytes(h, 8.0 * ((double)rows * n_features + staged + n_features + n_bc + n_precip), "x"))) return rc;
    HIPCHK(h, hipMalloc((void**)&h->X, sizeof(double) * (size_t)rows * n_features));
    HIPCHK(h, hipMalloc((void**)&h->mu, sizeof(double) * n_features));
    HIPCHK(h, hipMalloc((void**)&h->pc, sizeof(int64_t) * n_precip));
    HIPCHK(h, hipMalloc((void**)&h->bc, sizeof(int64_t) * std::max<int64_t>(n_bc, 1)));
    HIPCHK(h, hipMemcpyAsync(h->pc, precip_idx, sizeof(int64_t) * n_precip, hipMemcpyHostToDevice, h->stream));
    if (n_bc) HIPCHK(h, hipMemcpyAsync(h->bc, bc_idx, sizeof(int64_t) * n_bc, hipMemcpyHostToDevice, h->stream));
    if (input_mean) {
      h->mu_h.assign(input_mean, input_mean + n_features);
      HIPCHK(h, hipMemcpyAsync(h->mu, input_mean, sizeof(double) * n_features, hipMemcpyHostToDevice, h->stream));
    }
    if ((rc = hms_upload(h, x, ld, fortran))) return rc;
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->ms[0] = elapsed_ms(h->ev[0], h->ev[1]);
    return GPRX_OK;
  });
  if (rc) gprx_hms_destroy(h);
  else *out = h;
  return rc;
}

int gprx_hms_cov(gprx_hms_handle h, double* input_mean, double* cov, int* route) {
  if (!h) return fail(h, GPRX_EINVAL, "null handle");
  if (!input_mean || !cov || !route) return fail(h, GPRX_EINVAL, "null argument");
  if (h->route >= 0 || !h->mu_h.empty()) return fail(h, GPRX_ESTATE, "the covariance is computed once, by a handle created without input_mean");
  if (h->rows < 2) return fail(h, GPRX_EINVAL, "the fit needs rows >= 2");
  const int rc = guarded(h, [&]() -> int { HIPCHK(h, hipSetDevice(h->device)); return hms_cov(h, cov); });
  if (rc) return rc;
  std::memcpy(input_mean, h->mu_h.data(), sizeof(double) * h->nfeat);
  *route = h->route;
  return GPRX_OK;
}

int gprx_hms_components(gprx_hms_handle h, int k, const double* u, const double* lam, double* eofs) {
  if (!h) return fail(h, GPRX_EINVAL, "null handle");
  if (h->route != HMS_GRAM) return fail(h, GPRX_ESTATE, "components are formed on the device only on the Gram route (rows < precip columns)");
  return guarded(h, [&]() -> int {
    int rc;
    if ((rc = check_components(h, k, h->rows, "rows", !u || !lam || !eofs, lam)) || k == 0) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    return hms_components(h, k, u, lam, eofs);
  });
}

int gprx_hms_features(gprx_hms_handle h, int k, const double* eofs, const double* w1, int64_t n1, const double* w2, int64_t n2, double* x_mean,
                      double* x_std, int fit, double* out) {
  if (!h) return fail(h, GPRX_EINVAL, "null handle");
  if (k < 0 || n1 < 0 || n2 < 0 || (k > 0 && !eofs) || (n1 > 0 && !w1) || (n2 > 0 && !w2) || !x_mean || !x_std || (!fit && !out))
    return fail(h, GPRX_EINVAL, "null or negative argument");
  if (h->mu_h.empty()) return fail(h, GPRX_ESTATE, "input_mean is not known: run gprx_hms_cov first or pass it to gprx_hms_create");
  return guarded(h, [&]() -> int { HIPCHK(h, hipSetDevice(h->device)); return hms_features(h, k, eofs, w1, n1, w2, n2, x_mean, x_std, fit, out); });
}

int gprx_hms_timings(gprx_hms_handle h, double* ms) {
  if (!h || !ms) return fail(h, GPRX_EINVAL, "null argument");
  for (int i = 0; i < 7; ++i) ms[i] = h->ms[i];
  return GPRX_OK;
}

int gprx_api(int device, const double* a, int64_t n, const double* w, int64_t n_w, int64_t window, double* out) {
  return guarded(nullptr, [&]() -> int {
    if (n < 1 || window < 1) return fail(nullptr, GPRX_EINVAL, "the series and the window must not be empty");
    if (n_w < 0 || n_w > window || !a || !out || (n_w > 0 && !w)) return fail(nullptr, GPRX_EINVAL, "need 0 <= n_w <= window and non-null arrays");
    for (int64_t i = 0; i < n_w; ++i)
      if (!std::isfinite(w[i])) return fail(nullptr, GPRX_EINVAL, "the weights must be finite");
    bool finite = true;
    for (int64_t t = 0; t < n && finite; ++t) finite = std::isfinite(a[t]);
    const int64_t lags = std::min(finite ? n_w : window, n);
    HIPCHK(nullptr, hipSetDevice(device));
    const int rc0 = need_device_bytes(nullptr, 8.0 * (2.0 * n + std::max<int64_t>(n_w, 1)), "the API");
    if (rc0) return rc0;
    hipStream_t st = util_stream();
    double *A = nullptr, *W = nullptr, *O = nullptr;
    DevTemps tmp(st, {(void**)&A, (void**)&W, (void**)&O});
    HIPCHK(nullptr, hipMalloc((void**)&A, sizeof(double) * n));
    HIPCHK(nullptr, hipMalloc((void**)&O, sizeof(double) * n));
    HIPCHK(nullptr, hipMalloc((void**)&W, sizeof(double) * std::max<int64_t>(n_w, 1)));
    HIPCHK(nullptr, hipMemcpyAsync(A, a, sizeof(double) * n, hipMemcpyHostToDevice, st));
    if (n_w) HIPCHK(nullptr, hipMemcpyAsync(W, w, sizeof(double) * n_w, hipMemcpyHostToDevice, st));
    HIPCHK(nullptr, hms_api_launch(st, A, n, W, n_w, lags, O));
    HIPCHK(nullptr, hipMemcpyAsync(out, O, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(nullptr, hipStreamSynchronize(st));
    return GPRX_OK;
  });
}

const char* gprx_hms_last_error(gprx_hms_handle h) { return h ? h->err.c_str() : last_error().c_str(); }

}  // extern "C"
