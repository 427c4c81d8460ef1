// libgprx C ABI, LF-to-HF mesh resampling (gprx_rs_*): the low-fidelity fields of the two "Upskill HEC-RAS" builders.
#include "abi_common.h"

#include <algorithm>
#include <limits>
#include <string>
#include <vector>

#include "gprx_common.h"
#include "resample.h"

using namespace gprx;

extern "C" {

// ---- mesh resampling (gpras/preprocess.py:163-174, :363-377, :433-451) ----------------------------------
struct gprx_rs_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int64_t n_src = 0, n_out = 0, ce = 0;  // ce: n_out rounded up to even, the length of one plane of idx / w
  int nv = 0;
  int* idx = nullptr;
  double *w = nullptr, *elev = nullptr;
  Buf src, src2, slab;
  hipEvent_t ev[2] = {};  // around the last kernel
  bool timed = false;
  std::string err;
};

namespace {
hipError_t rs_launch(hipStream_t st, int nv, const RsArgs& a) {
  const int64_t pairs = (a.ldo + 1) / 2, rows = RS_RT * rs_groups(nv), tiles = ((pairs + RS_NT - 1) / RS_NT) * ((a.T + rows - 1) / rows);
  const unsigned grid = (unsigned)std::min<int64_t>(tiles, 2048);
  const bool vo = a.ldo % 2 == 0 && (uintptr_t)a.out % 16 == 0;
  if (nv == 3) {
    if (vo)
      hipLaunchKernelGGL((rs_kernel<3, false, true>), dim3(grid), dim3(RS_NT), 0, st, a);
    else
      hipLaunchKernelGGL((rs_kernel<3, false, false>), dim3(grid), dim3(RS_NT), 0, st, a);
  } else if (a.src2) {
    if (vo)
      hipLaunchKernelGGL((rs_kernel<1, true, true>), dim3(grid), dim3(RS_NT), 0, st, a);
    else
      hipLaunchKernelGGL((rs_kernel<1, true, false>), dim3(grid), dim3(RS_NT), 0, st, a);
  } else {
    if (vo)
      hipLaunchKernelGGL((rs_kernel<1, false, true>), dim3(grid), dim3(RS_NT), 0, st, a);
    else
      hipLaunchKernelGGL((rs_kernel<1, false, false>), dim3(grid), dim3(RS_NT), 0, st, a);
  }
  return hipGetLastError();
}
}  // namespace

int gprx_rs_destroy(gprx_rs_handle h) {
  if (!h) return GPRX_OK;
  release_handle(h->device, h->stream, {h->idx, h->w, h->elev, h->src.p, h->src2.p, h->slab.p}, h->ev, 2);
  delete h;
  return GPRX_OK;
}

// The state of RasUpskillDataBuilder (n_vert = 1: idx = lf_resampler, :373, or hf_resampler, :173) and of RasInterpolaterBuilder
// (n_vert = 3: the located simplex's vertices and barycentric weights, :443-447); elev = cell_elevations (:375-376, :449-450).
int gprx_rs_create(int device, int64_t n_src, int64_t n_out, int n_vert, const int32_t* idx, const double* weights, const double* elev,
                   gprx_rs_handle* out) {
  if (!out) return fail(nullptr, GPRX_EINVAL, "out is null");
  *out = nullptr;
  if (n_vert != 1 && n_vert != 3) return fail(nullptr, GPRX_EINVAL, "n_vert must be 1 (nearest) or 3 (linear)");
  if (!idx) return fail(nullptr, GPRX_EINVAL, "idx is null");
  if ((n_vert == 3) != (weights != nullptr)) return fail(nullptr, GPRX_EINVAL, "weights go with n_vert = 3 and with nothing else");
  if (n_src < 1 || n_out < 1 || n_src > RS_MAX_SRC || n_out > ((int64_t)1 << 31) - 1024)
    return fail(nullptr, GPRX_EINVAL, "need 1 <= n_src <= 2^28 and 1 <= n_out < 2^31");
  gprx_rs_handle h = nullptr;
  std::vector<int> ix;  // staged until the stream is idle, on the failure path too (gprx_rs_destroy waits for it)
  std::vector<double> ww, el;
  const int rc = guarded(nullptr, [&]() -> int {
    for (int64_t j = 0; j < n_out; ++j) {
      const int32_t* t = idx + j * n_vert;
      if (n_vert == 3 && t[0] == -1 && t[1] == -1 && t[2] == -1) continue;  // outside the hull
      for (int v = 0; v < n_vert; ++v)
        if (t[v] < 0 || t[v] >= n_src)
          return fail(nullptr, GPRX_EINVAL, "idx holds an index outside [0, n_src)" + std::string(n_vert == 3 ? " that is not the outside marker (-1, -1, -1)" : ""));
    }
    h = new gprx_rs_ctx();
    h->n_src = n_src;
    h->n_out = n_out;
    h->nv = n_vert;
    const int64_t ce = h->ce = round_up(n_out, 2);  // the kernel reads the per-cell arrays in pairs
    // planes per vertex; an outside point becomes vertices (0, 0, 0) with NaN weights, so the kernel reads in range and yields NaN
    ix.assign((size_t)ce * n_vert, 0);
    ww.assign(weights ? (size_t)ce * 3 : 0, 0.0);
    el.assign(elev ? (size_t)ce : 0, 0.0);
    const double nan = std::numeric_limits<double>::quiet_NaN();
    for (int64_t j = 0; j < n_out; ++j) {
      const bool outside = idx[j * n_vert] < 0;
      for (int v = 0; v < n_vert; ++v) {
        ix[(size_t)v * ce + j] = outside ? 0 : idx[j * n_vert + v];
        if (weights) ww[(size_t)v * ce + j] = outside ? nan : weights[j * 3 + v];
      }
    }
    if (elev) std::copy(elev, elev + n_out, el.begin());
    int rc;
    if ((rc = open_handle(h, device, h->ev, 2)) ||
        (rc = need_device_bytes(h, (4.0 * n_vert + (weights ? 24.0 : 0.0) + (elev ? 8.0 : 0.0)) * ce, "the resampler state")))
      return rc;
    HIPCHK(h, hipMalloc((void**)&h->idx, sizeof(int) * ix.size()));
    HIPCHK(h, hipMemcpyAsync(h->idx, ix.data(), sizeof(int) * ix.size(), hipMemcpyHostToDevice, h->stream));
    if (weights) {
      HIPCHK(h, hipMalloc((void**)&h->w, sizeof(double) * ww.size()));
      HIPCHK(h, hipMemcpyAsync(h->w, ww.data(), sizeof(double) * ww.size(), hipMemcpyHostToDevice, h->stream));
    }
    if (elev) {
      HIPCHK(h, hipMalloc((void**)&h->elev, sizeof(double) * el.size()));
      HIPCHK(h, hipMemcpyAsync(h->elev, el.data(), sizeof(double) * el.size(), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipStreamSynchronize(h->stream));  // the host vectors above are read until here
    return GPRX_OK;
  });
  if (rc) gprx_rs_destroy(h);
  else *out = h;
  return rc;
}

// get_lf_plan_data of either builder (:363-377, :433-451) or get_hf_plan_data's gather (:163-174) on device buffers.
int gprx_rs_apply_dev(gprx_rs_handle h, int64_t rows, const double* src_dev, int64_t lds, const double* src2_dev, double* out_dev, int64_t ldo) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (rows < 0 || rows > ((int64_t)1 << 31) - 1024) return fail(h, GPRX_EINVAL, "need 0 <= rows < 2^31");
    if (src2_dev && (h->nv != 1 || h->elev)) return fail(h, GPRX_EINVAL, "a second operand (velocity) needs a nearest handle without elevations");
    if (lds < h->n_src) return fail(h, GPRX_EINVAL, "lds is smaller than n_src");
    if (ldo < h->n_out) return fail(h, GPRX_EINVAL, "ldo is smaller than n_out");
    if (rows == 0) return GPRX_OK;
    if (!src_dev || !out_dev) return fail(h, GPRX_EINVAL, "null argument");
    HIPCHK(h, hipSetDevice(h->device));
    RsArgs a{src_dev, src2_dev, h->idx, h->w, h->elev, out_dev, rows, h->n_out, h->ce, lds, ldo};
    HIPCHK(h, hipEventRecord(h->ev[0], h->stream));
    HIPCHK(h, rs_launch(h->stream, h->nv, a));
    HIPCHK(h, hipEventRecord(h->ev[1], h->stream));
    h->timed = true;
    return GPRX_OK;
  });
}

// The same on host arrays, src / src2 (T, n_src), out (T, n_out), in row slabs: device memory does not grow with T.
int gprx_rs_apply(gprx_rs_handle h, const double* src, const double* src2, int64_t T, double* out) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (T < 0 || (T > 0 && (!src || !out))) return fail(h, GPRX_EINVAL, "null argument");
    if (src2 && (h->nv != 1 || h->elev)) return fail(h, GPRX_EINVAL, "a second operand (velocity) needs a nearest handle without elevations");
    HIPCHK(h, hipSetDevice(h->device));
    const int64_t ns = h->n_src, no = h->n_out, chunk = std::max<int64_t>(64, pca_chunk_doubles() / std::max(ns, no));
    int rc;
    for (int64_t t0 = 0; t0 < T; t0 += chunk) {
      const int64_t nr = std::min(chunk, T - t0);
      if ((rc = ensure(h, h->src, sizeof(double) * (size_t)nr * ns, "a slab of the source rows")) ||
          (src2 && (rc = ensure(h, h->src2, sizeof(double) * (size_t)nr * ns, "a slab of the second operand"))) ||
          (rc = ensure(h, h->slab, sizeof(double) * (size_t)nr * no, "a slab of the resampled field")))
        return rc;
      HIPCHK(h, hipMemcpyAsync(h->src.p, src + t0 * ns, sizeof(double) * nr * ns, hipMemcpyHostToDevice, h->stream));
      if (src2) HIPCHK(h, hipMemcpyAsync(h->src2.p, src2 + t0 * ns, sizeof(double) * nr * ns, hipMemcpyHostToDevice, h->stream));
      if ((rc = gprx_rs_apply_dev(h, nr, h->src.p, ns, src2 ? h->src2.p : nullptr, h->slab.p, no))) return rc;
      HIPCHK(h, hipMemcpyAsync(out + t0 * no, h->slab.p, sizeof(double) * nr * no, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipStreamSynchronize(h->stream));
    }
    return GPRX_OK;
  });
}

int gprx_rs_timings(gprx_rs_handle h, double* ms) {
  return guarded(h, [&]() -> int {
    if (!h || !ms) return fail(h, GPRX_EINVAL, "null argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float v = 0.f;
    if (h->timed) HIPCHK(h, hipEventElapsedTime(&v, h->ev[0], h->ev[1]));
    ms[0] = v;
    return GPRX_OK;
  });
}

int gprx_rs_synchronize(gprx_rs_handle h) {
  if (!h) return fail(h, GPRX_EINVAL, "null handle");
  return guarded(h, [&]() -> int { HIPCHK(h, hipStreamSynchronize(h->stream)); return GPRX_OK; });
}

const char* gprx_rs_last_error(gprx_rs_handle h) { return h ? h->err.c_str() : last_error().c_str(); }

}  // extern "C"
