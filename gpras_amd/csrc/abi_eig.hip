// libgprx C ABI, symmetric eigensolver (gprx_eigh_*): parallel two-sided block Jacobi in fp64 (eig_jacobi.h, DESIGN.md section
// 3.16).  This unit holds the kernels; the fit of the EOF preprocessor (abi_eof.hip) reaches them through eig_jacobi_run.
#include "abi_common.h"

#include <string>

#include "eig_jacobi.h"

using namespace gprx;

struct gprx_eigh_ctx {
  int device = 0, n_max = 0;
  hipStream_t stream = nullptr;
  double *A = nullptr, *V = nullptr, *lam = nullptr, *ws = nullptr;  // A, V (n_max, n_max) and lam serve the host entry only
  int sweeps = 0;
  double off_rel = 0.0;
  std::string err;
};

size_t gprx::eig_jacobi_workspace_bytes(int n) { return eig_jacobi_workspace_bytes_impl(n); }

int gprx::eig_jacobi_run(hipStream_t st, int n, double* A, int64_t lda, double* V, int64_t ldv, double* lam, void* workspace, int* sweeps,
                         double* off_rel, std::string* err) {
  int status = 1;
  const hipError_t e = eig_jacobi_run_impl(st, n, A, lda, V, ldv, lam, static_cast<double*>(workspace), sweeps, off_rel, &status);
  if (e != hipSuccess) {
    *err = std::string("eigensolver: ") + hipGetErrorString(e);
    return e == hipErrorOutOfMemory ? GPRX_ENOMEM : GPRX_EHIP;
  }
  if (status) {
    *err = "eigensolver: no convergence after " + std::to_string(*sweeps) + " sweeps (off / norm = " + std::to_string(*off_rel) +
           "; the sweep cap is " + std::to_string(EIG_MAX_SWEEPS) + ", a non-finite matrix ends at once)";
    return GPRX_ENOCONV;
  }
  return GPRX_OK;
}

extern "C" {

int gprx_eigh_destroy(gprx_eigh_handle h) {
  if (!h) return GPRX_OK;
  release_handle(h->device, h->stream, {h->A, h->V, h->lam, h->ws});
  delete h;
  return GPRX_OK;
}

int gprx_eigh_create(int device, int n_max, gprx_eigh_handle* out) {
  if (!out) return fail(nullptr, GPRX_EINVAL, "out is null");
  *out = nullptr;
  if (n_max < 1 || n_max > 16384) return fail(nullptr, GPRX_EINVAL, "need 1 <= n_max <= 16384");
  gprx_eigh_handle h = nullptr;
  const int rc = guarded(nullptr, [&]() -> int {
    h = new gprx_eigh_ctx();
    h->n_max = n_max;
    const size_t nn = sizeof(double) * (size_t)n_max * n_max;
    int rc;
    if ((rc = open_handle(h, device)) ||
        (rc = need_device_bytes(nullptr, 2.0 * (double)nn + (double)eig_jacobi_workspace_bytes_impl(n_max) + 8.0 * n_max, "the eigensolver")))
      return rc;
    HIPCHK(nullptr, hipMalloc((void**)&h->A, nn));
    HIPCHK(nullptr, hipMalloc((void**)&h->V, nn));
    HIPCHK(nullptr, hipMalloc((void**)&h->lam, sizeof(double) * n_max));
    HIPCHK(nullptr, hipMalloc((void**)&h->ws, eig_jacobi_workspace_bytes_impl(n_max)));
    return GPRX_OK;
  });
  if (rc) gprx_eigh_destroy(h);
  else *out = h;
  return rc;
}

int gprx_eigh_dev(gprx_eigh_handle h, int n, double* a_dev, int64_t lda, double* lam_dev, double* v_dev, int64_t ldv) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (n < 1 || n > h->n_max) return fail(h, GPRX_EINVAL, "need 1 <= n <= n_max of the handle");
    if (!a_dev || !lam_dev || !v_dev) return fail(h, GPRX_EINVAL, "null argument");
    if (lda < n || ldv < n) return fail(h, GPRX_EINVAL, "lda and ldv must be at least n");
    HIPCHK(h, hipSetDevice(h->device));
    h->sweeps = 0;
    h->off_rel = 0.0;
    std::string msg;
    const int rc = eig_jacobi_run(h->stream, n, a_dev, lda, v_dev, ldv, lam_dev, h->ws, &h->sweeps, &h->off_rel, &msg);
    if (rc) return fail(h, rc, msg);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return GPRX_OK;
  });
}

int gprx_eigh(gprx_eigh_handle h, int n, const double* a_host, int64_t lda, double* lam_host, double* v_host) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    if (n < 1 || n > h->n_max) return fail(h, GPRX_EINVAL, "need 1 <= n <= n_max of the handle");
    if (!a_host || !lam_host) return fail(h, GPRX_EINVAL, "null argument");
    if (lda < n) return fail(h, GPRX_EINVAL, "lda must be at least n");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy2DAsync(h->A, sizeof(double) * n, a_host, sizeof(double) * lda, sizeof(double) * n, (size_t)n, hipMemcpyHostToDevice, h->stream));
    const int rc = gprx_eigh_dev(h, n, h->A, n, h->lam, h->V, n);
    if (rc) return rc;
    HIPCHK(h, hipMemcpyAsync(lam_host, h->lam, sizeof(double) * n, hipMemcpyDeviceToHost, h->stream));
    if (v_host) HIPCHK(h, hipMemcpyAsync(v_host, h->V, sizeof(double) * n * n, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return GPRX_OK;
  });
}

int gprx_eigh_info(gprx_eigh_handle h, int* sweeps, double* off_rel) {
  if (!h || !sweeps || !off_rel) return fail(h, GPRX_EINVAL, "null argument");
  *sweeps = h->sweeps;
  *off_rel = h->off_rel;
  return GPRX_OK;
}

const char* gprx_eigh_last_error(gprx_eigh_handle h) { return h ? h->err.c_str() : last_error().c_str(); }

}  // extern "C"
