// libgprx C ABI, pseudo-surface low-fidelity model (gprx_ps_*) and the handle-less spline evaluation (gprx_spline_eval).
#include "abi_common.h"

#include <algorithm>
#include <string>
#include <vector>

#include "gprx_common.h"
#include "pseudo.h"

using namespace gprx;

extern "C" {

// ---- pseudo-surface low-fidelity model (gpras/preprocess.py:454-697) ------------------------------------
struct gprx_ps_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t cells = 0, C = 0, T = 0;
  double *elev = nullptr, *w = nullptr, *ds = nullptr;  // ds: second half of `us`
  Buf us, q, slab, cl;
  int* idx = nullptr;
  double* spl[2] = {nullptr, nullptr};  // per curve: knots [0, PS_MAX_KNOTS), coefficients [PS_MAX_KNOTS, 2 PS_MAX_KNOTS)
  int nt[2] = {0, 0};
  bool have_w = false;
  hipEvent_t ev[4] = {};  // around the last centerline fit kernel and the last surface launch
  bool fit_timed = false, surface_timed = false;
  std::string err;
};

namespace {
int ps_check_spline(gprx_ps_handle h, const double* t, int nt, const double* c) {
  if (!t || !c) return fail(h, GPRX_EINVAL, "null knots or coefficients");
  if (nt < 8 || nt > PS_MAX_KNOTS) return fail(h, GPRX_EINVAL, "a cubic spline needs 8 <= knots <= " + std::to_string(PS_MAX_KNOTS) + " (boundary knots included)");
  for (int i = 0; i + 1 < nt; ++i)
    if (!(t[i] <= t[i + 1])) return fail(h, GPRX_EINVAL, "the knots must be finite and non-decreasing");
  if (!(t[3] < t[nt - 4])) return fail(h, GPRX_EINVAL, "the knots span an empty interval");
  return GPRX_OK;
}

hipError_t ps_spline_launch(hipStream_t st, const double* x, int64_t n, const double* tc, int nt, double* out) {
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 2048);
  hipLaunchKernelGGL(ps_spline_kernel, dim3(grid), dim3(256), 0, st, x, n, tc, tc + PS_MAX_KNOTS, nt, out);
  return hipGetLastError();
}

hipError_t ps_surface_launch(hipStream_t st, const PsSurfaceArgs& a) {
  const int64_t pairs = (a.ldo + 1) / 2, tiles = ((pairs + PS_NT - 1) / PS_NT) * ((a.T + PS_RT - 1) / PS_RT);
  const unsigned grid = (unsigned)std::min<int64_t>(tiles, 2048);
  const size_t lds = a.w && a.C <= PS_W_LDS ? sizeof(double) * (size_t)a.C : 0;
  const bool vf = a.fluvial && a.ldf % 2 == 0 && (uintptr_t)a.fluvial % 16 == 0;
  const bool vo = a.ldo % 2 == 0 && (uintptr_t)a.out % 16 == 0;
  if (vf && vo)
    hipLaunchKernelGGL((ps_surface_kernel<true, true>), dim3(grid), dim3(PS_NT), lds, st, a);
  else if (vo)
    hipLaunchKernelGGL((ps_surface_kernel<false, true>), dim3(grid), dim3(PS_NT), lds, st, a);
  else if (vf)
    hipLaunchKernelGGL((ps_surface_kernel<true, false>), dim3(grid), dim3(PS_NT), lds, st, a);
  else
    hipLaunchKernelGGL((ps_surface_kernel<false, false>), dim3(grid), dim3(PS_NT), lds, st, a);
  return hipGetLastError();
}

int ps_boundary_buffers(gprx_ps_handle h, int64_t T) {
  if (T < 1 || T > ((int64_t)1 << 31) - 1024) return fail(h, GPRX_EINVAL, "need 1 <= T < 2^31 rows");
  const size_t bytes = sizeof(double) * 2 * (size_t)T;
  if (h->us.bytes < bytes) {
    int rc = ensure(h, h->us, bytes, "the boundary series");
    if (rc) return rc;
    h->ds = h->us.p + T;
  }
  h->ds = h->us.p + T;
  h->T = T;
  return GPRX_OK;
}
}  // namespace

int gprx_ps_destroy(gprx_ps_handle h) {
  if (!h) return GPRX_OK;
  release_handle(h->device, h->stream, {h->elev, h->w, h->us.p, h->q.p, h->slab.p, h->cl.p, h->idx, h->spl[0], h->spl[1]}, h->ev, 4);
  delete h;
  return GPRX_OK;
}

int gprx_ps_create(int device, int64_t n_cells, const double* elev, const int32_t* idx, int64_t n_centerline, const double* w, const double* us_knots,
                   int us_nt, const double* us_coef, const double* ds_knots, int ds_nt, const double* ds_coef, gprx_ps_handle* out) {
  if (!out) return fail(nullptr, GPRX_EINVAL, "out is null");
  *out = nullptr;
  if (!elev || !idx) return fail(nullptr, GPRX_EINVAL, "null argument");
  if (n_cells < 1 || n_centerline < 1 || n_cells > ((int64_t)1 << 31) - 1024 || n_centerline > ((int64_t)1 << 31) - 1024)
    return fail(nullptr, GPRX_EINVAL, "need 1 <= n_cells, n_centerline < 2^31");
  for (int64_t c = 0; c < n_cells; ++c)
    if (idx[c] < 0 || idx[c] >= n_centerline) return fail(nullptr, GPRX_EINVAL, "cell_interpolater holds an index outside [0, n_centerline)");
  const double* kn[2] = {us_knots, ds_knots};
  const double* co[2] = {us_coef, ds_coef};
  const int nts[2] = {us_nt, ds_nt};
  gprx_ps_handle h = nullptr;
  std::vector<double> el, tc[2];  // staged until the stream is idle, on the failure path too (gprx_ps_destroy waits for it)
  std::vector<int> ix;
  const int rc = guarded(nullptr, [&]() -> int {
    int rc;
    for (int s = 0; s < 2; ++s)
      if (nts[s] != 0 && (rc = ps_check_spline(nullptr, kn[s], nts[s], co[s]))) return rc;
    h = new gprx_ps_ctx();
    h->cells = n_cells;
    h->C = n_centerline;
    const int64_t ce = round_up(n_cells, 2);  // the surface kernel reads idx and elev in pairs
    el.assign(ce, 0.0);
    ix.assign(ce, 0);
    std::copy(elev, elev + n_cells, el.begin());
    std::copy(idx, idx + n_cells, ix.begin());
    if ((rc = open_handle(h, device, h->ev, 4)) || (rc = need_device_bytes(h, 12.0 * ce + 8.0 * n_centerline + 32.0 * PS_MAX_KNOTS, "the pseudo-surface state")))
      return rc;
    HIPCHK(h, hipMalloc((void**)&h->elev, sizeof(double) * ce));
    HIPCHK(h, hipMalloc((void**)&h->idx, sizeof(int) * ce));
    HIPCHK(h, hipMalloc((void**)&h->w, sizeof(double) * n_centerline));
    HIPCHK(h, hipMemcpyAsync(h->elev, el.data(), sizeof(double) * ce, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->idx, ix.data(), sizeof(int) * ce, hipMemcpyHostToDevice, h->stream));
    if (w) {
      HIPCHK(h, hipMemcpyAsync(h->w, w, sizeof(double) * n_centerline, hipMemcpyHostToDevice, h->stream));
      h->have_w = true;
    }
    for (int s = 0; s < 2; ++s) {
      if (!nts[s]) continue;
      tc[s].assign(2 * PS_MAX_KNOTS, 0.0);
      std::copy(kn[s], kn[s] + nts[s], tc[s].begin());
      std::copy(co[s], co[s] + nts[s] - 4, tc[s].begin() + PS_MAX_KNOTS);
      HIPCHK(h, hipMalloc((void**)&h->spl[s], sizeof(double) * 2 * PS_MAX_KNOTS));
      HIPCHK(h, hipMemcpyAsync(h->spl[s], tc[s].data(), sizeof(double) * 2 * PS_MAX_KNOTS, hipMemcpyHostToDevice, h->stream));
      h->nt[s] = nts[s];
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));  // the host vectors above are read until here
    return GPRX_OK;
  });
  if (rc) gprx_ps_destroy(h);
  else *out = h;
  return rc;
}

int gprx_spline_eval(int device, const double* knots, int nt, const double* coef, const double* x, int64_t n, double* out) {
  return guarded(nullptr, [&]() -> int {
    int rc = ps_check_spline(nullptr, knots, nt, coef);
    if (rc) return rc;
    if (n < 0 || (n > 0 && (!x || !out))) return fail(nullptr, GPRX_EINVAL, "null argument");
    if (n == 0) return GPRX_OK;
    HIPCHK(nullptr, hipSetDevice(device));
    if ((rc = need_device_bytes(nullptr, 16.0 * n + 16.0 * PS_MAX_KNOTS, "the spline evaluation"))) return rc;
    hipStream_t st = util_stream();
    double *X = nullptr, *O = nullptr, *TC = nullptr;
    std::vector<double> tc;  // read by the stream until `tmp` has synchronised it
    DevTemps tmp(st, {(void**)&X, (void**)&O, (void**)&TC});
    tc.assign(2 * PS_MAX_KNOTS, 0.0);
    std::copy(knots, knots + nt, tc.begin());
    std::copy(coef, coef + nt - 4, tc.begin() + PS_MAX_KNOTS);
    HIPCHK(nullptr, hipMalloc((void**)&X, sizeof(double) * n));
    HIPCHK(nullptr, hipMalloc((void**)&O, sizeof(double) * n));
    HIPCHK(nullptr, hipMalloc((void**)&TC, sizeof(double) * 2 * PS_MAX_KNOTS));
    HIPCHK(nullptr, hipMemcpyAsync(X, x, sizeof(double) * n, hipMemcpyHostToDevice, st));
    HIPCHK(nullptr, hipMemcpyAsync(TC, tc.data(), sizeof(double) * 2 * PS_MAX_KNOTS, hipMemcpyHostToDevice, st));
    HIPCHK(nullptr, ps_spline_launch(st, X, n, TC, nt, O));
    HIPCHK(nullptr, hipMemcpyAsync(out, O, sizeof(double) * n, hipMemcpyDeviceToHost, st));
    HIPCHK(nullptr, hipStreamSynchronize(st));
    return GPRX_OK;
  });
}

int gprx_ps_set_weights(gprx_ps_handle h, const double* w) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (!w) return fail(h, GPRX_EINVAL, "null argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpyAsync(h->w, w, sizeof(double) * h->C, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->have_w = true;
    return GPRX_OK;
  });
}

int gprx_ps_fit_centerline(gprx_ps_handle h, const double* us_wse, const double* ds_wse, const double* us_q, const double* ds_q,
                           const double* centerline_wse, int64_t rows, double* w) {
  if (!h) return fail(h, GPRX_EINVAL, "null handle");
  if (!us_wse || !ds_wse || !us_q || !ds_q || !centerline_wse || !w) return fail(h, GPRX_EINVAL, "null argument");
  if (rows < 1 || rows > ((int64_t)1 << 31) - 1024) return fail(h, GPRX_EINVAL, "need 1 <= rows < 2^31");
  return guarded(h, [&]() -> int {
    HIPCHK(h, hipSetDevice(h->device));
    double *W = nullptr, *B = nullptr;
    unsigned char* K = nullptr;
    const int64_t C = h->C;
    std::vector<unsigned char> keep;  // read by the stream until `tmp` has synchronised it
    DevTemps tmp(h->stream, {(void**)&W, (void**)&B, (void**)&K});
    keep.assign(rows, 0);
    int64_t n_keep = 0;
    for (int64_t r = 0; r < rows; ++r) n_keep += (keep[r] = (us_q[r] > 0 || ds_q[r] > 0) ? 1 : 0);
    if (n_keep == 0) return fail(h, GPRX_EINVAL, "no row has a positive upstream or downstream flow: the median is over nothing");
    int rc = need_device_bytes(h, 8.0 * ((double)rows * C + 2.0 * rows) + rows, "the centerline fit");
    if (rc) return rc;
    HIPCHK(h, hipMalloc((void**)&W, sizeof(double) * (size_t)rows * C));
    HIPCHK(h, hipMalloc((void**)&B, sizeof(double) * 2 * rows));
    HIPCHK(h, hipMalloc((void**)&K, rows));
    HIPCHK(h, hipMemcpyAsync(W, centerline_wse, sizeof(double) * (size_t)rows * C, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(B, us_wse, sizeof(double) * rows, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(B + rows, ds_wse, sizeof(double) * rows, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(K, keep.data(), rows, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    hipLaunchKernelGGL(ps_fit_kernel, dim3((unsigned)((C + PSF_COLS - 1) / PSF_COLS)), dim3(PSF_NT), 0, h->stream, (const double*)W, rows, C,
                       (const double*)B, (const double*)(B + rows), (const unsigned char*)K, (unsigned)n_keep, h->w);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    HIPCHK(h, hipMemcpyAsync(w, h->w, sizeof(double) * C, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->fit_timed = true;
    h->have_w = true;
    return GPRX_OK;
  });
}

int gprx_ps_timings(gprx_ps_handle h, double* ms) {
  return guarded(h, [&]() -> int {
    if (!h || !ms) return fail(h, GPRX_EINVAL, "null argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float v[2] = {0.f, 0.f};
    if (h->fit_timed) HIPCHK(h, hipEventElapsedTime(&v[0], h->ev[0], h->ev[1]));
    if (h->surface_timed) HIPCHK(h, hipEventElapsedTime(&v[1], h->ev[2], h->ev[3]));
    ms[0] = v[0];
    ms[1] = v[1];
    return GPRX_OK;
  });
}

int gprx_ps_rating(gprx_ps_handle h, const double* us_q, const double* ds_q, int64_t T, double* us_wse, double* ds_wse) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (!us_q || !ds_q) return fail(h, GPRX_EINVAL, "null argument");
    if (!h->nt[0] || !h->nt[1]) return fail(h, GPRX_ESTATE, "the handle was created without rating curves");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ps_boundary_buffers(h, T);
    if (rc) return rc;
    if ((rc = ensure(h, h->q, sizeof(double) * 2 * (size_t)T, "the flows"))) return rc;
    HIPCHK(h, hipMemcpyAsync(h->q.p, us_q, sizeof(double) * T, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->q.p + T, ds_q, sizeof(double) * T, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, ps_spline_launch(h->stream, h->q.p, T, h->spl[0], h->nt[0], h->us.p));
    HIPCHK(h, ps_spline_launch(h->stream, h->q.p + T, T, h->spl[1], h->nt[1], h->ds));
    if (us_wse) HIPCHK(h, hipMemcpyAsync(us_wse, h->us.p, sizeof(double) * T, hipMemcpyDeviceToHost, h->stream));
    if (ds_wse) HIPCHK(h, hipMemcpyAsync(ds_wse, h->ds, sizeof(double) * T, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return GPRX_OK;
  });
}

int gprx_ps_set_boundaries(gprx_ps_handle h, const double* us_wse, const double* ds_wse, int64_t T) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (!us_wse || !ds_wse) return fail(h, GPRX_EINVAL, "null argument");
    HIPCHK(h, hipSetDevice(h->device));
    int rc = ps_boundary_buffers(h, T);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(h->us.p, us_wse, sizeof(double) * T, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(h->ds, ds_wse, sizeof(double) * T, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return GPRX_OK;
  });
}

int gprx_ps_surface_dev(gprx_ps_handle h, int64_t t0, int64_t rows, const double* fluvial_dev, int64_t ldf, double* out_dev, int64_t ldo) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (rows == 0) return GPRX_OK;
    if (!out_dev) return fail(h, GPRX_EINVAL, "null argument");
    if (!h->have_w) return fail(h, GPRX_ESTATE, "the centerline interpolater is not set: fit it or pass it to gprx_ps_create");
    if (h->T == 0) return fail(h, GPRX_ESTATE, "no boundary series: call gprx_ps_rating or gprx_ps_set_boundaries first");
    if (t0 < 0 || rows < 0 || t0 + rows > h->T) return fail(h, GPRX_EINVAL, "rows [t0, t0 + rows) lie outside the boundary series");
    if (ldo < h->cells || (fluvial_dev && ldf < h->cells)) return fail(h, GPRX_EINVAL, "a leading dimension is smaller than n_cells");
    if (fluvial_dev == out_dev && ldf != ldo) return fail(h, GPRX_EINVAL, "in place needs equal leading dimensions");
    HIPCHK(h, hipSetDevice(h->device));
    PsSurfaceArgs a{h->us.p + t0, h->ds + t0, h->w, nullptr, h->idx, h->elev, fluvial_dev, out_dev, rows, h->cells, h->C, ldf, ldo};
    HIPCHK(h, hipEventRecord(h->ev[2], h->stream));
    HIPCHK(h, ps_surface_launch(h->stream, a));
    HIPCHK(h, hipEventRecord(h->ev[3], h->stream));
    h->surface_timed = true;
    return GPRX_OK;
  });
}

int gprx_ps_synchronize(gprx_ps_handle h) {
  if (!h) return fail(h, GPRX_EINVAL, "null handle");
  return guarded(h, [&]() -> int { HIPCHK(h, hipStreamSynchronize(h->stream)); return GPRX_OK; });
}

int gprx_ps_surface(gprx_ps_handle h, const double* fluvial, double* out) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (!out) return fail(h, GPRX_EINVAL, "null argument");
    if (h->T == 0) return fail(h, GPRX_ESTATE, "no boundary series: call gprx_ps_rating or gprx_ps_set_boundaries first");
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t cells = h->cells, chunk = std::max<int64_t>(64, pca_chunk_doubles() / cells);
    int rc;
    for (int64_t t0 = 0; t0 < h->T; t0 += chunk) {
      const int64_t nr = std::min(chunk, h->T - t0);
      if ((rc = ensure(h, h->slab, sizeof(double) * (size_t)nr * cells, "a slab of the surface"))) return rc;
      if (fluvial) HIPCHK(h, hipMemcpyAsync(h->slab.p, fluvial + t0 * cells, sizeof(double) * nr * cells, hipMemcpyHostToDevice, h->stream));
      if ((rc = gprx_ps_surface_dev(h, t0, nr, fluvial ? h->slab.p : nullptr, cells, h->slab.p, cells))) return rc;  // in place
      HIPCHK(h, hipMemcpyAsync(out + t0 * cells, h->slab.p, sizeof(double) * nr * cells, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return GPRX_OK;
  });
}

int gprx_ps_centerline(gprx_ps_handle h, double* out) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (!out) return fail(h, GPRX_EINVAL, "null argument");
    if (!h->have_w) return fail(h, GPRX_ESTATE, "the centerline interpolater is not set: fit it or pass it to gprx_ps_create");
    if (h->T == 0) return fail(h, GPRX_ESTATE, "no boundary series: call gprx_ps_rating or gprx_ps_set_boundaries first");
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t C = h->C, chunk = std::max<int64_t>(64, pca_chunk_doubles() / C);
    int rc;
    for (int64_t t0 = 0; t0 < h->T; t0 += chunk) {
      const int64_t nr = std::min(chunk, h->T - t0);
      if ((rc = ensure(h, h->slab, sizeof(double) * (size_t)nr * C, "a slab of the centerline"))) return rc;
      PsSurfaceArgs a{h->us.p + t0, h->ds + t0, h->w, nullptr, nullptr, nullptr, nullptr, h->slab.p, nr, C, C, C, C};
      HIPCHK(h, ps_surface_launch(h->stream, a));
      HIPCHK(h, hipMemcpyAsync(out + t0 * C, h->slab.p, sizeof(double) * nr * C, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return GPRX_OK;
  });
}

int gprx_ps_gather(gprx_ps_handle h, const double* centerline, int64_t rows, double* out) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (rows < 0 || (rows > 0 && (!centerline || !out))) return fail(h, GPRX_EINVAL, "null argument");
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t C = h->C, cells = h->cells, chunk = std::max<int64_t>(64, pca_chunk_doubles() / cells);
    int rc;
    for (int64_t t0 = 0; t0 < rows; t0 += chunk) {
      const int64_t nr = std::min(chunk, rows - t0);
      if ((rc = ensure(h, h->slab, sizeof(double) * (size_t)nr * cells, "a slab of the surface")) ||
          (rc = ensure(h, h->cl, sizeof(double) * (size_t)nr * C, "a slab of the centerline")))
        return rc;
      HIPCHK(h, hipMemcpyAsync(h->cl.p, centerline + t0 * C, sizeof(double) * nr * C, hipMemcpyHostToDevice, h->stream));
      PsSurfaceArgs a{nullptr, nullptr, nullptr, h->cl.p, h->idx, nullptr, nullptr, h->slab.p, nr, cells, C, cells, cells};
      HIPCHK(h, ps_surface_launch(h->stream, a));
      HIPCHK(h, hipMemcpyAsync(out + t0 * cells, h->slab.p, sizeof(double) * nr * cells, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return GPRX_OK;
  });
}

const char* gprx_ps_last_error(gprx_ps_handle h) { return h ? h->err.c_str() : last_error().c_str(); }

}  // extern "C"
