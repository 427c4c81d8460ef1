// libgprx C ABI, storm-event selection (gprx_ev_*): production/pre_processing/event_selection.py:13-257 of the reference, the first
// stage of its workflow.  Kernels in events.h; the covariance and the scores go through the fp64 MFMA GEMM
// (gemm_f64.h), the sort of the block maxima through gprx_dg_sort_u64_dev, the optional device eigh through eig_jacobi_run.
#include "abi_common.h"

#include <algorithm>
#include <cmath>
#include <new>
#include <string>
#include <vector>

#include "events.h"
#include "gemm_f64.h"
#include "gprx_common.h"

using namespace gprx;

extern "C" {

struct gprx_ev_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[2] = {};
  int64_t rows = 0, E = 0, H = 0, ld = 0;  // ld: H rounded up to 16 doubles, the row stride of the pivots
  double* P[3] = {};                       // pivots (E, ld): precip-excess, precip-cum, inflow
  int32_t* len = nullptr;                  // (E)
  double* mx = nullptr;                    // (2, E) maxima of precip-cum and inflow
  double* rp = nullptr;                    // (2, E) their return periods
  gprx_dg_handle dg = nullptr;
  uint64_t *keys = nullptr, *sorted = nullptr;  // (nb_cap) each
  double *xk[2] = {}, *yk[2] = {};              // knots, (nb_cap) each
  int64_t* nk = nullptr;                        // (2) on the device
  int64_t nk_h[2] = {0, 0}, nb_cap = 0;
  double *Xc = nullptr, *mean = nullptr, *cov = nullptr;  // (E, ld) | (2, ld) | (H, H)
  double *V = nullptr, *lam = nullptr, *eig_ws = nullptr, *eig_v = nullptr;
  int centred = -1, cov_of = -1;
  bool have_mean[2] = {false, false};
  double* T = nullptr;  // (E, 2 kp) raw scores of both blocks
  int k = 0, kp = 0;
  bool have_scores[2] = {false, false};
  double *S = nullptr, *smean = nullptr;  // (E, 2k) | mean (64) and scale (64)
  int d = 0;
  Buf ws, part, fp;
  double ms[8] = {};
  std::string err;
};

int gprx_ev_destroy(gprx_ev_handle h) {
  if (!h) return GPRX_OK;
  if (h->dg) gprx_dg_destroy(h->dg);
  release_handle(h->device, h->stream, {h->P[0],  h->P[1],  h->P[2],  h->len, h->mx,  h->rp,  h->keys, h->sorted, h->xk[0], h->xk[1], h->yk[0],
                                        h->yk[1], h->nk,    h->Xc,    h->mean, h->cov, h->V,   h->lam,  h->eig_ws, h->eig_v, h->T,     h->S,
                                        h->smean, h->ws.p,  h->part.p, h->fp.p},
                 h->ev, 2);
  delete h;
  return GPRX_OK;
}

}  // extern "C"

namespace {
constexpr int64_t EV_MAX_H = 4096;                // hours per event
constexpr int64_t EV_MAX_CELLS = (int64_t)1 << 28;  // E x ld: 2 GiB per pivot
constexpr int64_t EV_MAX_E = ((int64_t)1 << 31) - 1;

template <class T>
int ev_alloc(gprx_ev_handle h, T*& p, double count, const char* what) {
  if (p) return GPRX_OK;
  const double bytes = std::max(count, 1.0) * sizeof(T);
  int rc;
  if ((rc = need_device_bytes(h, bytes, what))) return rc;
  HIPCHK(h, hipMalloc((void**)&p, (size_t)bytes));
  return GPRX_OK;
}

unsigned grid_for(int64_t n, int64_t cap = 4096) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>((n + EV_NT - 1) / EV_NT, cap)); }

int begin(gprx_ev_handle h) {
  HIPCHK(h, hipSetDevice(h->device));
  HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
  return GPRX_OK;
}
// waits for the stream; ms[slot] = (add ? ms[slot] : 0) + the device time since begin()
int finish(gprx_ev_handle h, int slot, bool add = false) {
  HIPCHK(h, hipGetLastError());
  HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->ms[slot] = (add ? h->ms[slot] : 0.0) + elapsed_ms(h->ev[0], h->ev[1]);
  return GPRX_OK;
}

int new_handle(int device, gprx_ev_handle* out) {
  gprx_ev_handle h = new gprx_ev_ctx();
  const int rc = open_handle(h, device, h->ev, 2);
  if (rc) gprx_ev_destroy(h);
  else *out = h;
  return rc;
}

// column means (as_scale 0, shift null) or scales of X (n, ncol) with row stride ld, in the fixed order of events.h
int column_pass(gprx_ev_handle h, const double* X, int64_t n, int64_t ncol, int64_t ld, const double* shift, int as_scale, double* out) {
  const int64_t chunks = (n + EV_SUM_CHUNK - 1) / EV_SUM_CHUNK;
  int rc;
  if ((rc = ensure(h, h->part, sizeof(double) * (size_t)(chunks * ncol), "the partial column sums"))) return rc;
  hipLaunchKernelGGL(ev_colsum_partial_kernel, dim3((unsigned)chunks, (unsigned)((ncol + 63) / 64)), dim3(64), 0, h->stream, X, n, ncol, ld, shift, h->part.p);
  hipLaunchKernelGGL(ev_colsum_final_kernel, dim3((unsigned)((ncol + EV_NT - 1) / EV_NT)), dim3(EV_NT), 0, h->stream, (const double*)h->part.p, chunks, ncol,
                     (double)n, as_scale, out);
  HIPCHK(h, hipGetLastError());
  return GPRX_OK;
}

int centre(gprx_ev_handle h, int which) {
  if (h->centred == which) return GPRX_OK;
  const double* X = h->P[which == 0 ? 0 : 2];
  int rc;
  const int64_t Ep = round_up(h->E, 16);  // zero rows up to a multiple of 16: the GEMM reads K in stages of 16
  if ((rc = ev_alloc(h, h->Xc, (double)Ep * h->ld, "the centred pivot"))) return rc;
  if ((rc = ev_alloc(h, h->mean, 2.0 * h->ld, "the column means"))) return rc;
  if (!h->have_mean[which]) {
    if ((rc = column_pass(h, X, h->E, h->H, h->ld, nullptr, 0, h->mean + which * h->ld))) return rc;
    h->have_mean[which] = true;
  }
  hipLaunchKernelGGL(ev_centre_kernel, dim3(grid_for(Ep * h->ld)), dim3(EV_NT), 0, h->stream, X, h->E, Ep, h->H, h->ld, (const double*)(h->mean + which * h->ld), h->Xc);
  HIPCHK(h, hipGetLastError());
  h->centred = which;
  return GPRX_OK;
}

int need_frame(gprx_ev_handle h) {
  if (!h) return fail(h, GPRX_EINVAL, "null handle");
  if (!h->E) return fail(h, GPRX_ESTATE, "the handle holds no frame (gprx_ev_create_empty): only gprx_ev_farthest on supplied scores");
  return GPRX_OK;
}
}  // namespace

extern "C" {

int gprx_ev_create_empty(int device, gprx_ev_handle* out) {
  if (!out) return fail(nullptr, GPRX_EINVAL, "out is null");
  *out = nullptr;
  return guarded(nullptr, [&]() -> int { return new_handle(device, out); });
}

int gprx_ev_create(int device, int64_t rows, int64_t n_events, int64_t n_hours, const int32_t* ev_rank, const int32_t* hour, const double* precip_excess,
                   const double* precip_cum, const double* inflow, gprx_ev_handle* out) {
  if (!out) return fail(nullptr, GPRX_EINVAL, "out is null");
  *out = nullptr;
  if (!ev_rank || !hour || !precip_excess || !precip_cum || !inflow) return fail(nullptr, GPRX_EINVAL, "null argument");
  if (n_events < 1 || n_events > EV_MAX_E) return fail(nullptr, GPRX_EINVAL, "need 1 <= n_events < 2^31");
  if (n_hours < 1 || n_hours > EV_MAX_H) return fail(nullptr, GPRX_EINVAL, "need 1 <= n_hours <= 4096");
  const int64_t E = n_events, H = n_hours, ld = round_up(H, 16);
  if (E * ld > EV_MAX_CELLS) return fail(nullptr, GPRX_EINVAL, "need n_events x (n_hours rounded up to 16) <= 2^28");
  if (rows < E || rows > E * H) return fail(nullptr, GPRX_EINVAL, "need n_events <= rows <= n_events x n_hours");
  return guarded(nullptr, [&]() -> int {
    gprx_ev_handle h = nullptr;
    int rc;
    if ((rc = new_handle(device, &h))) return rc;
    h->rows = rows;
    h->E = E;
    h->H = H;
    h->ld = ld;
    auto body = [&]() -> int {
      hipStream_t st = h->stream;
      int rc2;
      if ((rc2 = need_device_bytes(h, 8.0 * (3.0 * E * ld + 3.0 * rows + 5.0 * E) + 8.0 * rows + 64, "the event pivots"))) return rc2;
      for (double*& p : h->P)
        if ((rc2 = ev_alloc(h, p, (double)E * ld, "a pivot"))) return rc2;
      if ((rc2 = ev_alloc(h, h->len, (double)E, "the event lengths"))) return rc2;
      if ((rc2 = ev_alloc(h, h->mx, 2.0 * E, "the event maxima"))) return rc2;
      int32_t *rank_d = nullptr, *hour_d = nullptr;
      double* val_d = nullptr;
      int* bad_d = nullptr;
      DevTemps tmp(st, {(void**)&rank_d, (void**)&hour_d, (void**)&val_d, (void**)&bad_d});
      HIPCHK(h, hipMalloc((void**)&rank_d, sizeof(int32_t) * (size_t)rows));
      HIPCHK(h, hipMalloc((void**)&hour_d, sizeof(int32_t) * (size_t)rows));
      HIPCHK(h, hipMalloc((void**)&val_d, sizeof(double) * 3 * (size_t)rows));
      HIPCHK(h, hipMalloc((void**)&bad_d, sizeof(int)));
      if ((rc2 = begin(h))) return rc2;
      HIPCHK(h, hipMemsetAsync(bad_d, 0, sizeof(int), st));
      HIPCHK(h, hipMemcpyAsync(rank_d, ev_rank, sizeof(int32_t) * (size_t)rows, hipMemcpyHostToDevice, st));
      HIPCHK(h, hipMemcpyAsync(hour_d, hour, sizeof(int32_t) * (size_t)rows, hipMemcpyHostToDevice, st));
      const double* cols[3] = {precip_excess, precip_cum, inflow};
      for (int c = 0; c < 3; ++c) {
        HIPCHK(h, hipMemcpyAsync(val_d + (size_t)c * rows, cols[c], sizeof(double) * (size_t)rows, hipMemcpyHostToDevice, st));
        HIPCHK(h, hipMemsetAsync(h->P[c], 0xff, sizeof(double) * (size_t)(E * ld), st));  // one NaN pattern: "not written"
      }
      hipLaunchKernelGGL(ev_pivot_kernel, dim3(grid_for(rows)), dim3(EV_NT), 0, st, rows, (const int32_t*)rank_d, (const int32_t*)hour_d, (const double*)val_d,
                         (const double*)(val_d + rows), (const double*)(val_d + 2 * rows), E, H, ld, h->P[0], h->P[1], h->P[2], bad_d);
      hipLaunchKernelGGL(ev_lengths_kernel, dim3((unsigned)((E + EV_NT / 64 - 1) / (EV_NT / 64))), dim3(EV_NT), 0, st, E, H, ld, h->P[0], h->P[1], h->P[2], h->len,
                         h->mx);
      HIPCHK(h, hipGetLastError());
      int bad = 0;
      std::vector<int32_t> len((size_t)E);
      HIPCHK(h, hipMemcpyAsync(&bad, bad_d, sizeof(int), hipMemcpyDeviceToHost, st));
      HIPCHK(h, hipMemcpyAsync(len.data(), h->len, sizeof(int32_t) * (size_t)E, hipMemcpyDeviceToHost, st));
      if ((rc2 = finish(h, 0))) return rc2;
      if (bad) return fail(h, GPRX_EINVAL, "an event rank is outside [0, n_events) or an hour outside [0, n_hours)");
      int64_t total = 0;
      for (int64_t e = 0; e < E; ++e) {
        if (len[e] < 0)
          return fail(h, GPRX_EINVAL, "event " + std::to_string((long long)e) + ": its hours are not exactly 0 .. len - 1 (or one of its values is NaN)");
        total += len[e];
      }
      if (total != rows)
        return fail(h, GPRX_EINVAL, "(event, hour) pairs must be unique: " + std::to_string((long long)(rows - total)) + " rows repeat a pair");
      return GPRX_OK;
    };
    if ((rc = body())) {
      const std::string msg = h->err;
      gprx_ev_destroy(h);
      last_error() = msg;
      return rc;
    }
    *out = h;
    return GPRX_OK;
  });
}

// max_precip_cum, max_inflow (n_events doubles) and lengths (n_events int32), any of them NULL: host outputs
int gprx_ev_maxima(gprx_ev_handle h, double* max_precip_cum, double* max_inflow, int32_t* lengths) {
  return guarded(h, [&]() -> int {
    int rc;
    if ((rc = need_frame(h))) return rc;
    HIPCHK(h, hipSetDevice(h->device));
    hipStream_t st = h->stream;
    if (max_precip_cum) HIPCHK(h, hipMemcpyAsync(max_precip_cum, h->mx, sizeof(double) * (size_t)h->E, hipMemcpyDeviceToHost, st));
    if (max_inflow) HIPCHK(h, hipMemcpyAsync(max_inflow, h->mx + h->E, sizeof(double) * (size_t)h->E, hipMemcpyDeviceToHost, st));
    if (lengths) HIPCHK(h, hipMemcpyAsync(lengths, h->len, sizeof(int32_t) * (size_t)h->E, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return GPRX_OK;
  });
}

int gprx_ev_return_periods(gprx_ev_handle h, int64_t arrival_rate, double* rp_precip_cum, double* rp_inflow, int64_t* n_knots) {
  return guarded(h, [&]() -> int {
    int rc;
    if ((rc = need_frame(h))) return rc;
    if (arrival_rate < 1) return fail(h, GPRX_EINVAL, "need arrival_rate >= 1");
    const int64_t E = h->E, nb = (E + arrival_rate - 1) / arrival_rate;
    if (nb < 2) return fail(h, GPRX_EINVAL, "the return-period function needs at least two distinct block maxima, there is one block");
    HIPCHK(h, hipSetDevice(h->device));
    if (nb > h->nb_cap) {
      for (void* p : {(void*)h->keys, (void*)h->sorted, (void*)h->xk[0], (void*)h->xk[1], (void*)h->yk[0], (void*)h->yk[1]})
        if (p) HIPCHK(h, hipFree(p));
      h->keys = h->sorted = nullptr;
      h->xk[0] = h->xk[1] = h->yk[0] = h->yk[1] = nullptr;
      h->nb_cap = 0;
    }
    if ((rc = ev_alloc(h, h->keys, (double)nb, "the block keys"))) return rc;
    if ((rc = ev_alloc(h, h->sorted, (double)nb, "the sorted block keys"))) return rc;
    for (int w = 0; w < 2; ++w) {
      if ((rc = ev_alloc(h, h->xk[w], (double)nb, "the knots"))) return rc;
      if ((rc = ev_alloc(h, h->yk[w], (double)nb, "the knots"))) return rc;
    }
    h->nb_cap = std::max(h->nb_cap, nb);
    if ((rc = ev_alloc(h, h->nk, 2.0, "the knot counts"))) return rc;
    if ((rc = ev_alloc(h, h->rp, 2.0 * E, "the return periods"))) return rc;
    if (!h->dg && (rc = gprx_dg_create(h->device, &h->dg))) return fail(h, rc, last_error());
    hipStream_t st = h->stream;
    h->nk_h[0] = h->nk_h[1] = 0;
    h->ms[1] = 0.0;
    for (int w = 0; w < 2; ++w) {
      if ((rc = begin(h))) return rc;
      hipLaunchKernelGGL(ev_block_keys_kernel, dim3((unsigned)((nb + EV_NT - 1) / EV_NT)), dim3(EV_NT), 0, st, (const double*)(h->mx + w * E), E, arrival_rate, nb,
                         h->keys);
      if ((rc = finish(h, 1, true))) return rc;
      // (the sort runs on its own stream and waits for its work; ours is idle here)
      if ((rc = gprx_dg_sort_u64_dev(h->dg, h->keys, nb, h->sorted))) return fail(h, rc, last_error());
      if ((rc = begin(h))) return rc;
      hipLaunchKernelGGL(ev_knots_kernel, dim3(1), dim3(EV_KNOT_NT), 0, st, (const uint64_t*)h->sorted, nb, h->xk[w], h->yk[w], h->nk + w);
      HIPCHK(h, hipGetLastError());
      int64_t nk = 0;
      HIPCHK(h, hipMemcpyAsync(&nk, h->nk + w, sizeof(int64_t), hipMemcpyDeviceToHost, st));
      if ((rc = finish(h, 1, true))) return rc;
      if (nk < 2)
        return fail(h, GPRX_EINVAL, std::string("the return-period function of ") + (w ? "inflow" : "precip-cum") +
                                        " needs at least two distinct block maxima, there is one");
      h->nk_h[w] = nk;
      if ((rc = begin(h))) return rc;
      hipLaunchKernelGGL(ev_rp_eval_kernel, dim3((unsigned)((E + EV_NT - 1) / EV_NT)), dim3(EV_NT), 0, st, (const double*)h->xk[w], (const double*)h->yk[w],
                         (const int64_t*)(h->nk + w), (const double*)(h->mx + w * E), E, h->rp + w * E);
      HIPCHK(h, hipGetLastError());
      double* dst = w ? rp_inflow : rp_precip_cum;
      if (dst) HIPCHK(h, hipMemcpyAsync(dst, h->rp + w * E, sizeof(double) * (size_t)E, hipMemcpyDeviceToHost, st));
      if ((rc = finish(h, 1, true))) return rc;
    }
    if (n_knots) {
      n_knots[0] = h->nk_h[0];
      n_knots[1] = h->nk_h[1];
    }
    return GPRX_OK;
  });
}

// out[i] = the fitted return-period function of `which` (0 precip-cum, 1 inflow) at values[i]: n host doubles each
int gprx_ev_rp_eval(gprx_ev_handle h, int which, const double* values, int64_t n, double* out) {
  return guarded(h, [&]() -> int {
    int rc;
    if ((rc = need_frame(h))) return rc;
    if (which < 0 || which > 1) return fail(h, GPRX_EINVAL, "which must be 0 (precip-cum) or 1 (inflow)");
    if (!values || !out) return fail(h, GPRX_EINVAL, "null argument");
    if (n < 1 || n > ((int64_t)1 << 31)) return fail(h, GPRX_EINVAL, "need 1 <= n <= 2^31 values");
    if (h->nk_h[which] < 2) return fail(h, GPRX_ESTATE, "gprx_ev_return_periods has not fitted the function");
    HIPCHK(h, hipSetDevice(h->device));
    int rc2;
    if ((rc2 = ensure(h, h->ws, sizeof(double) * 2 * (size_t)n, "the values of the evaluation"))) return rc2;
    hipStream_t st = h->stream;
    HIPCHK(h, hipMemcpyAsync(h->ws.p, values, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ev_rp_eval_kernel, dim3((unsigned)((n + EV_NT - 1) / EV_NT)), dim3(EV_NT), 0, st, (const double*)h->xk[which], (const double*)h->yk[which],
                       (const int64_t*)(h->nk + which), (const double*)h->ws.p, n, h->ws.p + n);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, h->ws.p + n, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipStreamSynchronize(st));
    return GPRX_OK;
  });
}

// which: 0 the precip-excess pivot, 1 the inflow pivot.  mean (n_hours) and cov (n_hours, n_hours) = Xc^T Xc (NOT yet divided by
// n_events - 1) on the host; the covariance also stays on the device for gprx_ev_eigh.
int gprx_ev_cov(gprx_ev_handle h, int which, double* mean, double* cov) {
  return guarded(h, [&]() -> int {
    int rc;
    if ((rc = need_frame(h))) return rc;
    if (which < 0 || which > 1) return fail(h, GPRX_EINVAL, "which must be 0 (precip-excess) or 1 (inflow)");
    if (!mean || !cov) return fail(h, GPRX_EINVAL, "null argument");
    if (h->E < 2) return fail(h, GPRX_EINVAL, "the covariance needs at least two events");
    const int64_t E = h->E, H = h->H, ld = h->ld;
    // K = E in slices: at most 64 slabs, each a multiple of 16 rows and at least 256
    const int64_t Ep = round_up(E, 16);
    const int kchunk = (int)std::max<int64_t>(256, round_up((Ep + 63) / 64, 16));
    const int64_t nsplit = (Ep + kchunk - 1) / kchunk;
    if ((rc = begin(h))) return rc;
    if ((rc = centre(h, which))) return rc;
    if ((rc = ev_alloc(h, h->cov, (double)H * H, "the covariance"))) return rc;
    if ((rc = ensure(h, h->ws, sizeof(double) * (size_t)(nsplit * H * H), "the slabs of the covariance"))) return rc;
    hipStream_t st = h->stream;
    HIPCHK(h, launch_gemm_splitk(st, 1, 0, (int)H, (int)H, (int)Ep, 1.0, h->Xc, ld, h->Xc, ld, 0.0, h->cov, H, h->ws.p, kchunk));
    HIPCHK(h, hipMemcpyAsync(mean, h->mean + which * ld, sizeof(double) * (size_t)H, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(cov, h->cov, sizeof(double) * (size_t)(H * H), hipMemcpyDeviceToHost, st));
    if ((rc = finish(h, 2 + which))) return rc;
    h->cov_of = which;
    return GPRX_OK;
  });
}

// eigh of the covariance of the last gprx_ev_cov on the device (eig_jacobi.h); the device copy of the covariance is overwritten.
// lam (n_hours) ascending, v (n_hours, n_hours) eigenvectors in columns: host outputs.
int gprx_ev_eigh(gprx_ev_handle h, double* lam, double* v, int* sweeps) {
  return guarded(h, [&]() -> int {
    int rc;
    if ((rc = need_frame(h))) return rc;
    if (!lam || !v) return fail(h, GPRX_EINVAL, "null argument");
    if (h->cov_of < 0) return fail(h, GPRX_ESTATE, "no covariance: call gprx_ev_cov first (each covariance serves one gprx_ev_eigh)");
    const int64_t H = h->H;
    if ((rc = ev_alloc(h, h->eig_v, (double)H * H, "the eigenvectors"))) return rc;
    if ((rc = ev_alloc(h, h->lam, (double)H, "the eigenvalues"))) return rc;
    if (!h->eig_ws) {
      const double bytes = (double)eig_jacobi_workspace_bytes((int)H);
      if ((rc = need_device_bytes(h, bytes, "the eigensolver"))) return rc;
      HIPCHK(h, hipMalloc((void**)&h->eig_ws, (size_t)std::max(bytes, 8.0)));
    }
    if ((rc = begin(h))) return rc;
    int sw = 0;
    double off_rel = 0.0;
    std::string msg;
    h->cov_of = -1;
    if ((rc = eig_jacobi_run(h->stream, (int)H, h->cov, H, h->eig_v, H, h->lam, h->eig_ws, &sw, &off_rel, &msg))) return fail(h, rc, msg);
    if (sweeps) *sweeps = sw;
    HIPCHK(h, hipMemcpyAsync(lam, h->lam, sizeof(double) * (size_t)H, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(v, h->eig_v, sizeof(double) * (size_t)(H * H), hipMemcpyDeviceToHost, h->stream));
    return finish(h, 7);
  });
}

// scores of block `which` = Xc V: components (k, n_hours) host, rows = components in scikit-learn's layout (components_), signs applied
int gprx_ev_scores(gprx_ev_handle h, int which, int k, const double* components) {
  return guarded(h, [&]() -> int {
    int rc;
    if ((rc = need_frame(h))) return rc;
    if (which < 0 || which > 1) return fail(h, GPRX_EINVAL, "which must be 0 (precip-excess) or 1 (inflow)");
    if (!components) return fail(h, GPRX_EINVAL, "null argument");
    const int64_t E = h->E, H = h->H, ld = h->ld;
    if (k < 1 || 2 * k > EV_MAX_D || k > std::min(E, H)) return fail(h, GPRX_EINVAL, "need 1 <= k <= min(32, n_events, n_hours)");
    const int kp = (int)round_up(k, 8);
    if (h->k != k) {  // another number of components: both score blocks start over
      if (h->T) HIPCHK(h, hipFree(h->T));
      if (h->V) HIPCHK(h, hipFree(h->V));
      if (h->S) HIPCHK(h, hipFree(h->S));
      h->T = h->V = h->S = nullptr;
      h->have_scores[0] = h->have_scores[1] = false;
      h->k = k;
      h->kp = kp;
      h->d = 0;
    }
    if ((rc = ev_alloc(h, h->T, (double)E * 2 * kp, "the scores"))) return rc;
    if ((rc = ev_alloc(h, h->V, (double)ld * kp, "the components"))) return rc;
    std::vector<double> vt((size_t)(ld * kp), 0.0);  // (ld, kp): V[j][c] = components[c][j], zero padding
    for (int c = 0; c < k; ++c)
      for (int64_t j = 0; j < H; ++j) vt[(size_t)(j * kp + c)] = components[(size_t)c * H + j];
    if ((rc = begin(h))) return rc;
    if ((rc = centre(h, which))) return rc;
    hipStream_t st = h->stream;
    HIPCHK(h, hipMemcpyAsync(h->V, vt.data(), sizeof(double) * vt.size(), hipMemcpyHostToDevice, st));
    HIPCHK(h, launch_gemm(st, 0, 0, (int)E, k, (int)ld, 1.0, h->Xc, ld, h->V, kp, 0.0, h->T + which * kp, 2 * kp, 0));
    if ((rc = finish(h, 4, h->have_scores[1 - which]))) return rc;  // (vt is read until here)
    h->have_scores[which] = true;
    h->d = 0;
    return GPRX_OK;
  });
}

// The (n_events, 2k) matrix of both score blocks, its columns standardised with the population standard deviation (scale 1 for a constant
// column); it stays on the device for gprx_ev_farthest.  scores_out (n_events, 2k) host, may be NULL.
int gprx_ev_standardise(gprx_ev_handle h, double* scores_out) {
  return guarded(h, [&]() -> int {
    int rc;
    if ((rc = need_frame(h))) return rc;
    if (!h->have_scores[0] || !h->have_scores[1]) return fail(h, GPRX_ESTATE, "gprx_ev_scores has not run for both blocks");
    const int64_t E = h->E;
    const int d = 2 * h->k;
    if ((rc = ev_alloc(h, h->S, (double)E * d, "the standardised scores"))) return rc;
    if ((rc = ev_alloc(h, h->smean, 2.0 * EV_MAX_D, "the column statistics"))) return rc;
    if ((rc = begin(h))) return rc;
    hipStream_t st = h->stream;
    hipLaunchKernelGGL(ev_gather_scores_kernel, dim3(grid_for(E * d)), dim3(EV_NT), 0, st, (const double*)h->T, E, h->k, h->kp, h->S);
    if ((rc = column_pass(h, h->S, E, d, d, nullptr, 0, h->smean))) return rc;
    if ((rc = column_pass(h, h->S, E, d, d, h->smean, 1, h->smean + EV_MAX_D))) return rc;
    hipLaunchKernelGGL(ev_standardise_kernel, dim3(grid_for(E * d)), dim3(EV_NT), 0, st, h->S, E, d, (const double*)h->smean, (const double*)(h->smean + EV_MAX_D));
    HIPCHK(h, hipGetLastError());
    if (scores_out) HIPCHK(h, hipMemcpyAsync(scores_out, h->S, sizeof(double) * (size_t)(E * d), hipMemcpyDeviceToHost, st));
    if ((rc = finish(h, 5))) return rc;
    h->d = d;
    return GPRX_OK;
  });
}

// The loop of _select_diverse_storms (:173-180) on rows of a score matrix (n, d): scores_dev, or NULL for the handle's standardised
// scores (n = n_events, d = 2k).  selected (n_selected) distinct rows, host; picks (num) rows in pick order and pick_dist (num), the
// distance of each pick to its nearest selected row at the time: host outputs.
int gprx_ev_farthest(gprx_ev_handle h, const double* scores_dev, int64_t n, int d, const int32_t* selected, int64_t n_selected, int64_t num, int32_t* picks,
                     double* pick_dist) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (!selected || !picks || !pick_dist) return fail(h, GPRX_EINVAL, "null argument");
    if (!scores_dev) {
      if (!h->d) return fail(h, GPRX_ESTATE, "no standardised scores: call gprx_ev_standardise first, or pass scores_dev");
      if (n != h->E || d != h->d) return fail(h, GPRX_EINVAL, "with the handle's scores n must be n_events and d must be 2k");
      scores_dev = h->S;
    }
    if (n < 2 || n > EV_MAX_E) return fail(h, GPRX_EINVAL, "need 2 <= n < 2^31 rows");
    if (d < 1 || d > EV_MAX_D) return fail(h, GPRX_EINVAL, "need 1 <= d <= 64 columns");
    if (n_selected < 1) return fail(h, GPRX_EINVAL, "the initial selected set must be non-empty");
    if (n_selected >= n) return fail(h, GPRX_EINVAL, "the initial selected set leaves no candidate");
    if (num < 1 || num > n - n_selected)
      return fail(h, GPRX_EINVAL, "num_to_select must be between 1 and the number of candidates (" + std::to_string((long long)(n - n_selected)) + ")");
    {
      std::vector<char> seen((size_t)n, 0);
      for (int64_t s = 0; s < n_selected; ++s) {
        if (selected[s] < 0 || selected[s] >= n) return fail(h, GPRX_EINVAL, "selected row " + std::to_string((long long)s) + " is outside [0, n)");
        if (seen[(size_t)selected[s]]) return fail(h, GPRX_EINVAL, "selected row " + std::to_string((long long)selected[s]) + " is listed twice");
        seen[(size_t)selected[s]] = 1;
      }
    }
    HIPCHK(h, hipSetDevice(h->device));
    const int G = (int)std::min<int64_t>((n + EV_NT - 1) / EV_NT, EV_FP_MAX_BLOCKS);
    // one block of doubles: mind (n) | pv (2 G) | pick_dist (num) | pi (2 G ints) | picks (num ints) | sel (n_selected ints)
    const size_t n_dbl = (size_t)n + 2 * (size_t)G + (size_t)num;
    const size_t n_int = 2 * (size_t)G + (size_t)num + (size_t)n_selected;
    int rc;
    if ((rc = ensure(h, h->fp, sizeof(double) * n_dbl + sizeof(int32_t) * (n_int + 2), "the state of the selection"))) return rc;
    double *mind = h->fp.p, *pv = mind + n, *dist_d = pv + 2 * G;
    int32_t *pi = reinterpret_cast<int32_t*>(dist_d + num), *picks_d = pi + 2 * G, *sel_d = picks_d + num;
    if ((rc = begin(h))) return rc;
    hipStream_t st = h->stream;
    HIPCHK(h, hipMemcpyAsync(sel_d, selected, sizeof(int32_t) * (size_t)n_selected, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(ev_fp_fill_kernel, dim3(grid_for(n)), dim3(EV_NT), 0, st, mind, n);
    hipLaunchKernelGGL(ev_fp_mark_kernel, dim3((unsigned)((n_selected + EV_NT - 1) / EV_NT)), dim3(EV_NT), 0, st, mind, (const int32_t*)sel_d, n_selected);
    hipLaunchKernelGGL(ev_fp_init_kernel, dim3(G), dim3(EV_NT), 0, st, scores_dev, n, d, (const int32_t*)sel_d, n_selected, mind, pv, pi);
    for (int64_t it = 0; it < num; ++it) {
      const int in = (int)(it & 1), outb = 1 - in;
      hipLaunchKernelGGL(ev_fp_step_kernel, dim3(G), dim3(EV_NT), 0, st, scores_dev, n, d, mind, (const double*)(pv + in * G), (const int*)(pi + in * G), G, pv + outb * G,
                         pi + outb * G, picks_d, dist_d, (int)it);
    }
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(picks, picks_d, sizeof(int32_t) * (size_t)num, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(pick_dist, dist_d, sizeof(double) * (size_t)num, hipMemcpyDeviceToHost, st));
    if ((rc = finish(h, 6))) return rc;
    for (int64_t it = 0; it < num; ++it)
      if (picks[it] < 0) return fail(h, GPRX_EHIP, "pick " + std::to_string((long long)it) + " found no candidate");
    return GPRX_OK;
  });
}

int gprx_ev_synchronize(gprx_ev_handle h) {
  if (!h) return fail(h, GPRX_EINVAL, "null handle");
  return guarded(h, [&]() -> int { HIPCHK(h, hipStreamSynchronize(h->stream)); return GPRX_OK; });
}

int gprx_ev_timings(gprx_ev_handle h, double* ms) {
  if (!h || !ms) return fail(h, GPRX_EINVAL, "null argument");
  for (int i = 0; i < 8; ++i) ms[i] = h->ms[i];
  return GPRX_OK;
}

const char* gprx_ev_last_error(gprx_ev_handle h) { return h ? h->err.c_str() : last_error().c_str(); }

}  // extern "C"
