// Host plumbing shared by the C ABI units (gprx.hip, abi_*.hip): the last-error string, the exception guard, the status check, device
// buffers, the free-memory check, event timing, the utility stream, the split-K plan, the opener of a stream-owning handle and the
// owners of a call's temporaries and a handle's blocks.
// Host code only: no kernel lives here, so any unit may include it.
#pragma once

#include "../../include/gprx.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <exception>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

namespace gprx {

// One message per host thread for the whole library: gprx_*_last_error(NULL) of every family reads it.  Defined in gprx.hip.
std::string& last_error();

// `c`: any context with an `err` member, or null
template <class Ctx>
int fail(Ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  last_error() = msg;
  return code;
}
inline int fail(std::nullptr_t, int code, const std::string& msg) {
  last_error() = msg;
  return code;
}

// No C++ exception crosses the C boundary: every extern "C" entry point whose body can allocate on the host (new, std::vector,
// std::string, a concatenated message) runs it as `return guarded(ctx, [&]() -> int { ... });`.  `c`: as for fail.
template <class Ctx, class F>
int guarded(Ctx c, F&& body) {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    return fail(c, GPRX_ENOMEM, "host allocation failed");
  } catch (const std::exception& e) {
    return fail(c, GPRX_EHIP, std::string("unexpected exception: ") + e.what());
  } catch (...) {
    return fail(c, GPRX_EHIP, "unexpected exception");
  }
}

#define HIPCHK(c, expr)                                                                            \
  do {                                                                                             \
    hipError_t e_ = (expr);                                                                        \
    if (e_ != hipSuccess) {                                                                        \
      return fail(c, e_ == hipErrorOutOfMemory ? GPRX_ENOMEM : GPRX_EHIP,                          \
                  std::string(#expr) + ": " + hipGetErrorString(e_));                              \
    }                                                                                              \
  } while (0)

// The legacy (NULL) stream is never used.  A legacy-stream call (hipMemcpy, hipMemset, a launch on stream 0, hipDeviceSynchronize)
// from one host thread is refused while ANOTHER thread captures a graph ("operation would make the legacy stream depend on a
// capturing blocking stream") and invalidates that capture -- in every capture mode of this runtime.  Synchronous copies and
// the handle-less entry points go through one non-blocking utility stream per device instead: one for the whole library (the
// handle-less entry points of every unit are ordered on it), defined in gprx.hip.
hipStream_t util_stream();

inline hipError_t copy_sync(void* dst, const void* src, size_t bytes, hipMemcpyKind kind) {
  hipStream_t st = util_stream();
  if (!st) return hipErrorInvalidValue;
  hipError_t e = hipMemcpyAsync(dst, src, bytes, kind, st);
  return e != hipSuccess ? e : hipStreamSynchronize(st);
}
inline hipError_t memset_sync(void* dst, int value, size_t bytes) {
  hipStream_t st = util_stream();
  if (!st) return hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(dst, value, bytes, st);
  return e != hipSuccess ? e : hipStreamSynchronize(st);
}

// the next allocations need `bytes` of device memory: GPRX_ENOMEM before any of them is made
template <class Ctx>
int need_device_bytes(Ctx c, double bytes, const char* what) {
  size_t fr = 0, tot = 0;
  HIPCHK(c, hipMemGetInfo(&fr, &tot));
  if (bytes > 0.95 * (double)fr)
    return fail(c, GPRX_ENOMEM, std::string(what) + " needs " + std::to_string((long long)(bytes / 1048576.0)) + " MiB of device memory, " +
                                    std::to_string((long long)(fr / 1048576)) + " MiB are free");
  return GPRX_OK;
}

struct Buf {
  double* p = nullptr;
  size_t bytes = 0;
  bool borrowed = false;  // view into the batch arena (gprx_select_slot): never freed through this Buf
};

// grow-only device buffer; `what` given: the free-memory check runs between the release of the old block and the allocation
template <class Ctx>
int ensure(Ctx c, Buf& b, size_t bytes, const char* what = nullptr) {
  if (b.bytes >= bytes) return GPRX_OK;
  if (b.p && !b.borrowed) HIPCHK(c, hipFree(b.p));
  b.p = nullptr;
  b.bytes = 0;
  b.borrowed = false;
  int rc;
  if (what && (rc = need_device_bytes(c, (double)bytes, what))) return rc;
  HIPCHK(c, hipMalloc((void**)&b.p, bytes));
  b.bytes = bytes;
  return GPRX_OK;
}

inline float elapsed_ms(hipEvent_t a, hipEvent_t b) {
  float ms = 0.f;
  hipEventElapsedTime(&ms, a, b);
  return ms;
}

// device staging per pass of the host-buffer entry points: 1 GiB of x / output (GPRX_PCA_CHUNK_DOUBLES overrides, for tests)
inline int64_t pca_chunk_doubles() {
  static const int64_t v = getenv("GPRX_PCA_CHUNK_DOUBLES") ? atoll(getenv("GPRX_PCA_CHUNK_DOUBLES")) : ((int64_t)1 << 27);
  return v;
}

// "pcafit_rowsplit" (gprx_set_tuning; process-wide, read by gprx_pcafit_create_auto): 1 = the covariance route of the EOF fit runs its
// row-split kernels, 0 = the one-thread-per-cell kernels on the same operation list.  Defined in gprx.hip, beside the other keys.
int& pcafit_rowsplit_tuning();

// dst (cols, rows) <- src (rows, cols)^T on `st` (pca.h transpose_small_kernel; defined in abi_eof.hip, the unit that holds pca.h)
void launch_transpose_small(hipStream_t st, const double* src, int64_t rows, int64_t cols, double* dst);

// The symmetric eigensolver (eig_jacobi.h; defined in abi_eig.hip, the unit that holds its kernels), all pointers on the device:
// A (n, lda) symmetric, lower triangle read, overwritten; V (n, ldv) eigenvectors in columns; lam (n) ascending; workspace of
// eig_jacobi_workspace_bytes(n).  Waits for `st` once per sweep.  GPRX_OK, GPRX_ENOCONV (30 sweeps, or a non-finite matrix) or a HIP
// status, the text in *err.
size_t eig_jacobi_workspace_bytes(int n);
int eig_jacobi_run(hipStream_t st, int n, double* A, int64_t lda, double* V, int64_t ldv, double* lam, void* workspace, int* sweeps, double* off_rel,
                   std::string* err);

// Device temporaries of one call, named where they are declared.  When the scope ends, on every path: the stream that may still
// read them is synchronised, then the non-null ones are freed.
struct DevTemps {
  hipStream_t st;
  std::vector<void**> ptrs;
  DevTemps(hipStream_t s, std::initializer_list<void**> p) : st(s), ptrs(p) {}
  DevTemps(const DevTemps&) = delete;
  ~DevTemps() {
    if (st) hipStreamSynchronize(st);
    for (void** q : ptrs)
      if (*q) hipFree(*q);
  }
};

// Split-K plan of a product with `tiles` output tiles of 64 x 64 and K = kdim: a few thousand workgroups, slices of at least 256 and
// a multiple of 16, the slabs (slab_doubles each; 1: no cap) held to 256 MiB in all.
struct SplitK {
  int kchunk, nsplit;
};
inline SplitK splitk_plan(int64_t tiles, int64_t kdim, int64_t slab_doubles) {
  int64_t nsplit = std::max<int64_t>(1, 2048 / std::max<int64_t>(tiles, 1));
  nsplit = std::min<int64_t>(nsplit, std::max<int64_t>(1, ((int64_t)1 << 25) / std::max<int64_t>(slab_doubles, 1)));
  const int64_t kchunk = std::max<int64_t>(((kdim + nsplit - 1) / nsplit + 15) / 16 * 16, 256);
  return {(int)kchunk, (int)((kdim + kchunk - 1) / kchunk)};
}

// What the *_create of a stream-owning handle does first, in this order: set the device and store it, create the non-blocking
// stream, create the events.  On failure the caller destroys the handle (release_handle skips what was not created).
template <class Ctx>
static int open_handle(Ctx* h, int device, hipEvent_t* ev = nullptr, int n_ev = 0) {
  h->device = device;
  HIPCHK(nullptr, hipSetDevice(device));
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  for (int i = 0; i < n_ev && e == hipSuccess; ++i) e = hipEventCreate(&ev[i]);
  if (e != hipSuccess) return fail(nullptr, GPRX_EHIP, std::string("hipStreamCreate / hipEventCreate: ") + hipGetErrorString(e));
  return GPRX_OK;
}

// What the *_destroy of a stream-owning handle does, in this order: wait for the stream, free the device blocks, destroy the
// events, destroy the stream.
inline void release_handle(int device, hipStream_t st, std::initializer_list<void*> blocks, hipEvent_t* ev = nullptr, int n_ev = 0) {
  hipSetDevice(device);
  if (st) hipStreamSynchronize(st);
  for (void* q : blocks)
    if (q) hipFree(q);
  for (int i = 0; i < n_ev; ++i)
    if (ev[i]) hipEventDestroy(ev[i]);
  if (st) hipStreamDestroy(st);
}

}  // namespace gprx
