// libgprx: the C boundary (include/gprx.h) of the GP path and of the raw kernel entry points -- handle life cycle, thin wrappers over
// gp_*.h, the building-block probes, the development stamps and the tuning keys.  The GP path itself is host orchestration in six
// headers (and gp_loeo.h, the leave-one-event-out sequence on top of the predict), included below in dependency order into THIS unit (one instantiation of the GEMM, Cholesky, solve and kernel-matrix
// kernels that the exact path, the sparse path and the probes all launch).  No CPU fallback exists for any device stage.
#include "abi_common.h"

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gemm_f64.h"
#include "gprx_common.h"
#include "grad.h"
#include "kmat.h"
#include "potrf.h"
#include "potrf_cell.h"
#include "potrf_dag.h"
#include "sgpr.h"
#include "sgpr_asm.h"
#include "sgpr_fused.h"
#include "sf_loeo.h"
#include "sgpr_step.h"
#include "solve.h"

using namespace gprx;

namespace gprx {

std::string& last_error() {
  thread_local std::string msg;
  return msg;
}

int& pcafit_rowsplit_tuning() {
  static int v = 1;  // gprx_set_tuning("pcafit_rowsplit", ...): see abi_common.h
  return v;
}

// (see abi_common.h: the one utility stream per device of the whole library)
hipStream_t util_stream() {
  static std::mutex m;
  static std::map<int, hipStream_t> streams;
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lock(m);
  auto it = streams.find(dev);
  if (it != streams.end()) return it->second;
  hipStream_t st = nullptr;
  if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return nullptr;
  streams.emplace(dev, st);
  return st;
}

}  // namespace gprx

#include "gp_ctx.h"
#include "gp_exact.h"
#include "gp_sparse.h"
#include "gp_resident.h"
#include "gp_objective.h"
#include "gp_predict.h"
#include "gp_loeo.h"
#include "gp_loeo_blocked.h"
#include "gp_joint.h"

namespace {

// back-to-back MFMA issue, 4 independent accumulators per wave, one wave per SIMD
__global__ __launch_bounds__(256) void mfma_f64_peak_kernel(double* out, int iters) {
  d4 c0 = {0, 0, 0, 0}, c1 = c0, c2 = c0, c3 = c0;
  const double a = 1.0 + threadIdx.x * 1e-9, b = 1.0 - threadIdx.x * 1e-9;
  for (int i = 0; i < iters; ++i) {
    c0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c0, 0, 0, 0);
    c1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c1, 0, 0, 0);
    c2 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c2, 0, 0, 0);
    c3 = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c3, 0, 0, 0);
  }
  const d4 s = c0 + c1 + c2 + c3;
  if (s.x == 123.456) out[0] = s.y;
}

}  // namespace

// ======================================================================================================
extern "C" {

int gprx_version(void) { return GPRX_VERSION; }

const char* gprx_last_error(gprx_handle h) { return h ? h->err.c_str() : last_error().c_str(); }

int gprx_device_count(int* count) {
  if (!count) return fail(nullptr, GPRX_EINVAL, "count is null");
  return guarded(nullptr, [&]() -> int { HIPCHK(nullptr, hipGetDeviceCount(count)); return GPRX_OK; });
}

int gprx_create(int device, int64_t n, int d, int64_t m, int kernel_id, int ard, gprx_handle* out) {
  if (!out) return fail(nullptr, GPRX_EINVAL, "out is null");
  *out = nullptr;
  if (n <= 0 || d <= 0 || m < 0) return fail(nullptr, GPRX_EINVAL, "n, d must be positive and m non-negative");
  if (kernel_id < 0 || kernel_id > 4) return fail(nullptr, GPRX_EINVAL, "unknown kernel id");
  if (n > (1 << 30) || m > (1 << 30)) return fail(nullptr, GPRX_EINVAL, "n or m too large");
  gprx_handle h = nullptr;
  const int rc = guarded(nullptr, [&]() -> int {
    h = new gprx_ctx();
    h->n = n;
    h->m = m;
    h->d = d;
    h->kid = kernel_id;
    h->ard = ard ? 1 : 0;
    h->nlen = ard ? d : 1;
    h->ntheta = 2 + h->nlen;
    h->np = round_up(n, NB);
    h->mp = round_up(m, NB);
    h->tune = potrf_tuning();  // a private copy: later gprx_set_tuning calls (process defaults) do not reach this handle
    h->predict_path = predict_path_tuning();
    h->sgpr_fused = sgpr_fused_tuning();
    h->sgpr_resident = sgpr_resident_tuning();
    h->own_stream = true;
    // normal priority on purpose: measured on MI355X, raised/lowered stream priorities do nothing for a single
    // cell and cut the throughput of several concurrent cells by up to 2x
    // the look-ahead stream is created on first use (ensure_lookahead): HIP binds streams to its 4 hardware
    // queues round-robin at creation, so an unused second stream per handle would leave the main streams of
    // many concurrent cells on half of the queues (measured: 584 instead of 797 fits/s with 12 cells)
    int rc;
    if ((rc = open_handle(h, device, h->ev, 5)) || (rc = ensure(h, h->invls, sizeof(double) * d)) || (rc = ensure(h, h->red, sizeof(double) * 16))) return rc;
    hipError_t e = hipMalloc((void**)&h->info, sizeof(int));
    if (e == hipSuccess) e = hipHostMalloc((void**)&h->pin, sizeof(double) * 80, hipHostMallocDefault);
    if (e == hipSuccess) e = hipMalloc((void**)&h->gparams, sizeof(double) * 2);
    return e == hipSuccess ? GPRX_OK : fail(nullptr, GPRX_ENOMEM, "hipMalloc(info) / hipHostMalloc(staging)");
  });
  if (rc) gprx_destroy(h);
  else *out = h;
  return rc;
}

int gprx_destroy(gprx_handle h) {
  if (!h) return GPRX_OK;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  for (Buf* b : {&h->X, &h->Y, &h->invls, &h->alpha, &h->red, &h->Kmat, &h->invD, &h->Xinv, &h->Tmp, &h->partial, &h->xs, &h->Ks, &h->pred,
                 &h->dstage, &h->arena, &h->cellpar, &h->cellres, &h->garena, &h->gpartial, &h->apart, &h->twork, &h->sarena, &h->hold, &h->loeo_ws, &h->joint_ws})
    if (b->p && !b->borrowed) hipFree(b->p);
  for (auto& ev : h->loeo_ev)
    if (ev) hipEventDestroy(ev);
  if (h->bpin) hipHostFree(h->bpin);
  if (h->spin) hipHostFree(h->spin);
  if (h->sf_stamps) hipFree(h->sf_stamps);
  for (auto& ev : h->sf_evs)
    if (ev) hipEventDestroy(ev);
  for (auto& sx : h->sf_streams)
    if (sx) hipStreamDestroy(sx);
  if (h->adam_dev.p) hipFree(h->adam_dev.p);
  if (h->adam_pin) hipHostFree(h->adam_pin);
  for (auto& ev : h->bev)
    if (ev) hipEventDestroy(ev);
  for (auto& ev : h->kev)
    if (ev) hipEventDestroy(ev);
  for (auto& ev : h->cev)
    if (ev) hipEventDestroy(ev);
  if (h->wev) hipEventDestroy(h->wev);
  if (h->info) hipFree(h->info);
  if (h->pin) hipHostFree(h->pin);
  if (h->gparams) hipFree(h->gparams);
  drop_graphs(h);
  for (auto& ev : h->ev)
    if (ev) hipEventDestroy(ev);
  h->pstreams.destroy();
  h->dag.destroy();
  if (h->own_stream && h->stream) hipStreamDestroy(h->stream);
  delete h;
  return GPRX_OK;
}

int gprx_set_stream(gprx_handle h, void* hip_stream) {
  return guarded(h, [&]() -> int {
    int rc;
    if ((rc = check_handle(h))) return rc;
    if (h->own_stream && h->stream) {
      hipStreamSynchronize(h->stream);
      hipStreamDestroy(h->stream);
    }
    h->stream = (hipStream_t)hip_stream;
    h->own_stream = false;
    return GPRX_OK;
  });
}

int gprx_set_distance_form(gprx_handle h, int form) {
  return guarded(h, [&]() -> int {
    int rc;
    if ((rc = check_handle(h))) return rc;
    if (form != GPRX_DIST_DIFFERENCE && form != GPRX_DIST_EXPANDED) return fail(h, GPRX_EINVAL, "unknown distance form");
    if (form != h->dist_form) {
      HIPCHK(h, hipStreamSynchronize(h->stream));
      h->dist_form = form;
      forget_factorizations(h, false);  // resident factorisations (and captured graphs) were built with the other form
    }
    return GPRX_OK;
  });
}

int gprx_synchronize(gprx_handle h) {
  return guarded(h, [&]() -> int {
    int rc;
    if ((rc = check_handle(h))) return rc;
    HIPCHK(h, wait_stream(h, h->stream));
    return GPRX_OK;
  });
}

int gprx_set_data(gprx_handle h, const double* x, const double* y, int n_units) {
  return guarded(h, [&]() -> int {
    int rc;
    if ((rc = check_handle(h))) return rc;
    if (!x || !y || n_units <= 0) return fail(h, GPRX_EINVAL, "x, y must be non-null and n_units positive");
    if ((rc = ensure(h, h->X, sizeof(double) * h->n * h->d))) return rc;
    if ((rc = ensure(h, h->Y, sizeof(double) * h->np * n_units))) return rc;
    // unit-major copy of y, zero padded to np
    std::vector<double> yt((size_t)h->np * n_units, 0.0);
    for (int64_t i = 0; i < h->n; ++i)
      for (int u = 0; u < n_units; ++u) yt[(size_t)u * h->np + i] = y[i * n_units + u];
    HIPCHK(h, copy_sync(h->X.p, x, sizeof(double) * h->n * h->d, hipMemcpyHostToDevice));
    HIPCHK(h, copy_sync(h->Y.p, yt.data(), sizeof(double) * yt.size(), hipMemcpyHostToDevice));
    h->n_units = n_units;
    forget_factorizations(h, true);  // resident batch slots were factorised from the old data
    h->yhost.swap(yt);
    h->yy.assign(n_units, 0.0);
    for (int u = 0; u < n_units; ++u) h->yy[u] = yy_rows(h, u, 0, h->n, 0.0);
    return GPRX_OK;
  });
}

int gprx_objective(gprx_handle h, int unit, const double* theta, const double* z, int mask, double* loss, double* grad) {
  return guarded(h, [&]() -> int { return objective_impl(h, unit, theta, z, mask, loss, grad); });
}

int gprx_factorize(gprx_handle h, int unit, const double* theta, const double* z, int mask, double* loss) {
  return guarded(h, [&]() -> int { return objective_impl(h, unit, theta, z, mask, loss, nullptr); });
}

int gprx_factorize_many(int count, gprx_handle* handles, const int* units, const double* thetas, int mask, double* losses) {
  return guarded(nullptr, [&]() -> int { return factorize_many(count, handles, units, thetas, mask, losses); });
}

int gprx_last_optimizer_route(gprx_handle h, int* route, int* host_waits) {
  if (!h || !route || !host_waits) return fail(h, GPRX_EINVAL, "null argument");
  *route = h->last_route;
  *host_waits = h->last_host_waits;
  return GPRX_OK;
}

int gprx_adam_batch(gprx_handle h, int count, const int* units, double* theta, double* z, int mask, int max_iter, int* n_evals, int* batches) {
  return guarded(h, [&]() -> int { return optimizer_routed(h, SF_OPT_ADAM, count, units, theta, z, mask, max_iter, nullptr, n_evals, batches); });
}

int gprx_adadelta_batch(gprx_handle h, int count, const int* units, double* theta, double* z, int mask, int max_iter, double* losses, int* n_evals,
                        int* batches) {
  return guarded(h, [&]() -> int { return optimizer_routed(h, SF_OPT_ADADELTA, count, units, theta, z, mask, max_iter, losses, n_evals, batches); });
}

int gprx_factorize_batch(gprx_handle h, int count, const int* units, const double* thetas, int mask, double* losses, int* status) {
  return guarded(h, [&]() -> int { return factorize_batch(h, count, units, thetas, mask, losses, status); });
}

int gprx_select_slot(gprx_handle h, int slot) {
  return guarded(h, [&]() -> int { const int rc = check_handle(h); return rc ? rc : select_slot(h, slot); });
}

int gprx_last_batch_ms(gprx_handle h, double* ms) {
  if (!h || !ms) return fail(h, GPRX_EINVAL, "null argument");
  *ms = h->batch_ms;
  return GPRX_OK;
}

int gprx_last_timings(gprx_handle h, double* ms4) {
  if (!h || !ms4) return fail(h, GPRX_EINVAL, "null argument");
  for (int s = 0; s < 4; ++s) ms4[s] = h->timings[s];
  return GPRX_OK;
}

int gprx_set_profiling(gprx_handle h, int enabled) {
  if (!h) return fail(h, GPRX_EINVAL, "null handle");
  h->profiling = enabled != 0;
  return GPRX_OK;
}

int gprx_last_profile(gprx_handle h, double* out8) {
  if (!h || !out8) return fail(h, GPRX_EINVAL, "null argument");
  for (int i = 0; i < 8; ++i) out8[i] = h->prof_out[i];
  return GPRX_OK;
}

int gprx_last_kernel_build(gprx_handle h, double* ms, double* bytes) {
  if (!h || !ms || !bytes) return fail(h, GPRX_EINVAL, "null argument");
  *ms = h->kmat_ms;
  *bytes = h->kmat_bytes;
  return GPRX_OK;
}

int gprx_last_cell_kernel(gprx_handle h, double* ms, double* flops, double* cells) {
  if (!h || !ms || !flops || !cells) return fail(h, GPRX_EINVAL, "null argument");
  *ms = h->cell_ms;
  *flops = h->cell_ms > 0.0 ? h->cell_flops : 0.0;
  *cells = h->cell_ms > 0.0 ? h->cell_cells : 0.0;
  return GPRX_OK;
}

int gprx_objective_batch(gprx_handle h, int count, const int* units, const double* theta, const double* z, int mask, double* losses,
                         double* grads) {
  return guarded(h, [&]() -> int { return objective_batch(h, count, units, theta, z, mask, losses, grads); });
}

int gprx_predict_dev(gprx_handle h, const double* xs_dev, int64_t ns, double* mean_dev, double* var_dev, int include_noise) {
  return guarded(h, [&]() -> int { return predict_dev(h, xs_dev, ns, mean_dev, var_dev, include_noise); });
}

int gprx_predict(gprx_handle h, const double* xs, int64_t ns, double* mean, double* var, int include_noise) {
  return guarded(h, [&]() -> int {
    int rc;
    if ((rc = check_handle(h))) return rc;
    if (ns < 0 || (ns > 0 && (!xs || !mean || !var))) return fail(h, GPRX_EINVAL, "null argument");
    if (ns == 0) return GPRX_OK;
    if ((rc = ensure(h, h->xs, sizeof(double) * (ns * h->d + 2 * ns)))) return rc;
    double* dxs = h->xs.p;
    double* dmean = dxs + ns * h->d;
    double* dvar = dmean + ns;
    HIPCHK(h, hipMemcpyAsync(dxs, xs, sizeof(double) * ns * h->d, hipMemcpyHostToDevice, h->stream));
    if ((rc = predict_dev(h, dxs, ns, dmean, dvar, include_noise))) return rc;
    HIPCHK(h, hipMemcpyAsync(mean, dmean, sizeof(double) * ns, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(var, dvar, sizeof(double) * ns, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, wait_stream(h, h->stream));
    return GPRX_OK;
  });
}

int gprx_predict_batch_dev(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs_dev, int64_t ns,
                           double* means_dev, double* vars_dev, int include_noise) {
  return guarded(h, [&]() -> int {
    int rc;
    if ((rc = check_handle(h))) return rc;
    if (count <= 0 || !units || !thetas || ns < 0 || (ns > 0 && (!xs_dev || !means_dev || !vars_dev))) return fail(h, GPRX_EINVAL, "null argument");
    return predict_batch_core(h, count, units, thetas, z, xs_dev, ns, means_dev, vars_dev, include_noise);
  });
}

int gprx_predict_joint_batch_dev(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs_dev, int64_t ns,
                                 double* means_dev, double* lc_dev, int include_noise) {
  return guarded(h, [&]() -> int { return predict_joint_batch(h, count, units, thetas, z, xs_dev, ns, means_dev, lc_dev, include_noise); });
}

int gprx_predict_batch(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs, int64_t ns,
                       double* means, double* vars, int include_noise) {
  return guarded(h, [&]() -> int {
    return predict_batch_slabs(h, count, units, thetas, z, xs, ns, means, vars, include_noise, false, (int64_t)1 << 27, NO_FORCED_SLAB);
  });
}

int gprx_predict_batch_t(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs, int64_t ns,
                         double* means_t, double* vars_t, int include_noise) {
  return guarded(h, [&]() -> int {
    return predict_batch_slabs(h, count, units, thetas, z, xs, ns, means_t, vars_t, include_noise, true, (int64_t)1 << 26,
                               env_int("GPRX_PREDICT_SLAB", NO_FORCED_SLAB));
  });
}

// ---- the held-out forms (include/gprx.h "Held-out rows"): their parents with one row range per cell that the cell's model does not see ----
int gprx_objective_batch_held(gprx_handle h, int count, const int* units, const double* theta, const double* z, int mask, double* losses,
                              double* grads, const int64_t* hold_lo, const int64_t* hold_hi) {
  return guarded(h, [&]() -> int { return objective_batch(h, count, units, theta, z, mask, losses, grads, true, hold_lo, hold_hi); });
}

int gprx_adam_batch_held(gprx_handle h, int count, const int* units, double* theta, double* z, int mask, int max_iter, int* n_evals, int* batches,
                         const int64_t* hold_lo, const int64_t* hold_hi) {
  return guarded(h, [&]() -> int {
    return optimizer_routed(h, SF_OPT_ADAM, count, units, theta, z, mask, max_iter, nullptr, n_evals, batches, true, hold_lo, hold_hi);
  });
}

int gprx_adadelta_batch_held(gprx_handle h, int count, const int* units, double* theta, double* z, int mask, int max_iter, double* losses,
                             int* n_evals, int* batches, const int64_t* hold_lo, const int64_t* hold_hi) {
  return guarded(h, [&]() -> int {
    return optimizer_routed(h, SF_OPT_ADADELTA, count, units, theta, z, mask, max_iter, losses, n_evals, batches, true, hold_lo, hold_hi);
  });
}

int gprx_predict_batch_held(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs, int64_t ns,
                            double* means, double* vars, int include_noise, const int64_t* hold_lo, const int64_t* hold_hi) {
  return guarded(h, [&]() -> int {
    return predict_batch_slabs(h, count, units, thetas, z, xs, ns, means, vars, include_noise, false, (int64_t)1 << 27, NO_FORCED_SLAB, true, hold_lo,
                               hold_hi);
  });
}

int gprx_loeo_batch(gprx_handle h, int count, const int* units, const double* thetas, const double* z, int n_events, const int64_t* ev_lo,
                    const int64_t* ev_hi, double* means, double* vars, int include_noise, int* status) {
  return guarded(h, [&]() -> int { return loeo_batch(h, count, units, thetas, z, n_events, ev_lo, ev_hi, means, vars, include_noise, status); });
}

int gprx_last_loeo(gprx_handle h, int* ran, double* stage_ms) {
  if (!h || !ran) return fail(h, GPRX_EINVAL, "null argument");
  *ran = h->last_loeo;
  if (stage_ms) std::copy(h->loeo_ms, h->loeo_ms + 4, stage_ms);
  return GPRX_OK;
}

int gprx_loeo_batch_blocked(gprx_handle h, int count, const int* units, const double* thetas, const double* z, int n_events, const int64_t* ev_lo,
                            const int64_t* ev_hi, double* means, double* vars, int include_noise, int max_slots, int* status) {
  return guarded(h, [&]() -> int {
    return loeo_blocked_batch(h, count, units, thetas, z, n_events, ev_lo, ev_hi, means, vars, include_noise, max_slots, status);
  });
}

int gprx_last_loeo_blocked(gprx_handle h, int* ran, int* groups, double* stage_ms) {
  return guarded(h, [&]() -> int {
    if (!h || !ran || !groups) return fail(h, GPRX_EINVAL, "null argument");
    *ran = h->last_loeo_blocked;
    *groups = h->loeo_blocked_groups;
    if (stage_ms) std::copy(h->loeo_blocked_ms, h->loeo_blocked_ms + 6, stage_ms);
    return GPRX_OK;
  });
}

int gprx_mem_info(int device, int64_t* free_bytes, int64_t* total_bytes) {
  return guarded(nullptr, [&]() -> int {
    if (!free_bytes || !total_bytes) return fail(nullptr, GPRX_EINVAL, "null argument");
    HIPCHK(nullptr, hipSetDevice(device));
    size_t f = 0, t = 0;
    HIPCHK(nullptr, hipMemGetInfo(&f, &t));
    *free_bytes = (int64_t)f;
    *total_bytes = (int64_t)t;
    return GPRX_OK;
  });
}

int gprx_cell_bytes(gprx_handle h, int with_gradient, int64_t* bytes) {
  if (!h || !bytes) return fail(h, GPRX_EINVAL, "null argument");
  if (h->m != 0) {
    *bytes = (int64_t)sizeof(double) * sgpr_batch_layout(h).ss;
    return GPRX_OK;
  }
  const int64_t np = h->np;
  int64_t doubles = round_up((np + NB) * np + np * NB + np * STAGE_LD + np, 64);  // arena cell (ensure_arena)
  if (with_gradient) doubles += 2 * np * np + (np / KM_T) * (np / KM_T) * (2 + h->d) + (2 + h->d);  // garena + trace partials
  *bytes = (int64_t)sizeof(double) * doubles;
  return GPRX_OK;
}

int gprx_dev_malloc(int device, int64_t bytes, void** out) {
  return guarded(nullptr, [&]() -> int {
    if (!out || bytes < 0) return fail(nullptr, GPRX_EINVAL, "bad argument");
    HIPCHK(nullptr, hipSetDevice(device));
    HIPCHK(nullptr, hipMalloc(out, (size_t)std::max<int64_t>(bytes, 16)));
    return GPRX_OK;
  });
}
int gprx_dev_free(int device, void* ptr) {
  return guarded(nullptr, [&]() -> int { HIPCHK(nullptr, hipSetDevice(device)); HIPCHK(nullptr, hipFree(ptr)); return GPRX_OK; });
}
int gprx_memcpy_h2d(int device, void* dst_dev, const void* src_host, int64_t bytes) {
  return guarded(nullptr, [&]() -> int {
    HIPCHK(nullptr, hipSetDevice(device));
    HIPCHK(nullptr, copy_sync(dst_dev, src_host, (size_t)bytes, hipMemcpyHostToDevice));
    return GPRX_OK;
  });
}
int gprx_memcpy_d2h(int device, void* dst_host, const void* src_dev, int64_t bytes) {
  return guarded(nullptr, [&]() -> int {
    HIPCHK(nullptr, hipSetDevice(device));
    HIPCHK(nullptr, copy_sync(dst_host, src_dev, (size_t)bytes, hipMemcpyDeviceToHost));
    return GPRX_OK;
  });
}

// ---- building blocks ----------------------------------------------------------------------------
int gprx_kmat(int device, int kernel_id, const double* a_dev, int64_t n1, const double* b_dev, int64_t n2, int d,
              const double* ls_host, double variance, double diag_add, double* out_dev, int64_t ld, int64_t n1p, int64_t n2p,
              int mode) {
  return guarded(nullptr, [&]() -> int {
    if (!a_dev || !b_dev || !ls_host || !out_dev) return fail(nullptr, GPRX_EINVAL, "null argument");
    if (n1p % NB || n2p % NB || ld % 2 || n1p < n1 || n2p < n2 || ld < n2p) return fail(nullptr, GPRX_EINVAL, "padded sizes must be multiples of 64");
    if (mode < 0 || mode > 6) return fail(nullptr, GPRX_EINVAL, "bad kernel id or mode");
    const int form = (mode & 4) ? GPRX_DIST_EXPANDED : GPRX_DIST_DIFFERENCE;  // mode + 4: gpflow's expanded distance form
    mode &= 3;
    if (kernel_id < 0 || kernel_id > 4 || mode < 0 || mode > 2) return fail(nullptr, GPRX_EINVAL, "bad kernel id or mode");
    HIPCHK(nullptr, hipSetDevice(device));
    double* dinv = nullptr;
    HIPCHK(nullptr, hipMalloc((void**)&dinv, sizeof(double) * d));
    HIPCHK(nullptr, copy_sync(dinv, ls_host, sizeof(double) * d, hipMemcpyHostToDevice));
    KmatArgs ka{a_dev, b_dev, dinv, out_dev, ld, (int)n1, (int)n2, d, (int)n1p, (int)n2p, variance, diag_add, mode, mode ? 1.0 : 0.0, nullptr, 0};
    ka.form = form;
    hipError_t e = launch_kmat(util_stream(), kernel_id, ka);
    hipError_t e2 = hipStreamSynchronize(util_stream());
    hipFree(dinv);
    HIPCHK(nullptr, e);
    HIPCHK(nullptr, e2);
    return GPRX_OK;
  });
}

// the kernel build's exponential (exp_nonpos_tab) / the gradient passes' (exp_nonpos) on an array: parity test of the function itself
namespace {
__global__ __launch_bounds__(256) void exp_probe_kernel(const double* __restrict__ x, double* __restrict__ out, int64_t n, int which) {
  __shared__ double sTab[64];
  exp_tab_fill(sTab);
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    out[i] = which == 0 ? exp_nonpos_tab(x[i], sTab) : exp_nonpos(x[i]);
}
}  // namespace

int gprx_exp_probe(int device, int which, const double* x, int64_t n, double* out) {
  return guarded(nullptr, [&]() -> int {
    if (!x || !out || n < 0 || which < 0 || which > 1) return fail(nullptr, GPRX_EINVAL, "bad argument");
    if (n == 0) return GPRX_OK;
    HIPCHK(nullptr, hipSetDevice(device));
    double *dx = nullptr, *dout = nullptr;
    HIPCHK(nullptr, hipMalloc((void**)&dx, sizeof(double) * n));
    hipError_t e = hipMalloc((void**)&dout, sizeof(double) * n);
    if (e == hipSuccess) e = copy_sync(dx, x, sizeof(double) * n, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(exp_probe_kernel, dim3(2048), dim3(256), 0, util_stream(), dx, dout, n, which);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = copy_sync(out, dout, sizeof(double) * n, hipMemcpyDeviceToHost);
    hipFree(dx);
    if (dout) hipFree(dout);
    HIPCHK(nullptr, e);
    return GPRX_OK;
  });
}

int gprx_gemm(int device, int ta, int tb, int64_t m, int64_t n, int64_t k, double alpha, const double* a_dev, int64_t lda,
              const double* b_dev, int64_t ldb, double beta, double* c_dev, int64_t ldc, int flags, int tile) {
  return guarded(nullptr, [&]() -> int {
    if (!a_dev || !b_dev || !c_dev) return fail(nullptr, GPRX_EINVAL, "null argument");
    if (k % 16 || lda % 2 || ldb % 2) return fail(nullptr, GPRX_EINVAL, "k must be a multiple of 16, leading dimensions even");
    if (!((ta == 0 && tb == 1) || (ta == 0 && tb == 0) || (ta == 1 && tb == 0))) return fail(nullptr, GPRX_EINVAL, "unsupported transpose pair");
    if (tile != 0 && tile != 64 && tile != 128) return fail(nullptr, GPRX_EINVAL, "tile must be 0, 64 or 128");
    HIPCHK(nullptr, hipSetDevice(device));
    HIPCHK(nullptr, launch_gemm(util_stream(), ta, tb, (int)m, (int)n, (int)k, alpha, a_dev, lda, b_dev, ldb, beta, c_dev, ldc, flags, tile));
    HIPCHK(nullptr, hipStreamSynchronize(util_stream()));
    return GPRX_OK;
  });
}

int gprx_potrf(int device, double* a_dev, int64_t lda, int64_t np, int64_t extra, double* inv_diag_dev, int* info_host) {
  return guarded(nullptr, [&]() -> int {
    if (!a_dev || !inv_diag_dev || !info_host) return fail(nullptr, GPRX_EINVAL, "null argument");
    if (np % NB || np <= 0 || extra < 0 || lda < np || lda % 2) return fail(nullptr, GPRX_EINVAL, "np must be a positive multiple of 64");
    HIPCHK(nullptr, hipSetDevice(device));
    int* dinfo = nullptr;
    HIPCHK(nullptr, hipMalloc((void**)&dinfo, sizeof(int)));
    HIPCHK(nullptr, memset_sync(dinfo, 0, sizeof(int)));
    PotrfStreams ps;
    hipStream_t st = nullptr;
    HIPCHK(nullptr, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    HIPCHK(nullptr, ps.init());
    double* dstage = nullptr;
    HIPCHK(nullptr, hipMalloc((void**)&dstage, sizeof(double) * np * STAGE_LD));
    DagPlan dag;
    const bool by_dag = use_dag(potrf_tuning(), (int)np) && extra % NB == 0;
    hipError_t e = by_dag ? potrf_dag(st, a_dev, lda, (int)np, (int)extra, inv_diag_dev, dinfo, dag)
                          : potrf_lower(st, a_dev, lda, (int)np, (int)extra, inv_diag_dev, dinfo, dstage, nullptr, &ps);
    hipError_t e2 = hipStreamSynchronize(st);
    if (ps.aux && e2 == hipSuccess) e2 = hipStreamSynchronize(ps.aux);
    int gave_up = 0;
    if (by_dag && e == hipSuccess && e2 == hipSuccess) copy_sync(&gave_up, dag.state + DAG_ABORT, sizeof(int), hipMemcpyDeviceToHost);
    dag.destroy();
    hipFree(dstage);
    ps.destroy();
    hipStreamDestroy(st);
    copy_sync(info_host, dinfo, sizeof(int), hipMemcpyDeviceToHost);
    hipFree(dinfo);
    HIPCHK(nullptr, e);
    HIPCHK(nullptr, e2);
    if (gave_up) return fail(nullptr, GPRX_EHIP, "tile-DAG factorisation: a dependency wait timed out");
    return *info_host ? fail(nullptr, GPRX_ENOTPD, "matrix not positive definite") : GPRX_OK;
  });
}

// ---- probes of the GEMM dispatcher and of solve.h (the block tests call every variant directly) -------------------------------------
// Each validates what its kernels cannot take and returns GPRX_EINVAL before any HIP call; then one launch sequence on util_stream().
// What is refused is what a kernel reads with 16-byte vector loads or in fixed granules: odd leading dimensions and batch / cell
// strides of the GEMM OPERANDS A and B, of L, inv_diag, the right-hand-side matrix, X and T, and of rowreduce's M; those pointers off
// a 16-byte boundary; K or kchunk off a multiple of 16; np off a multiple of 64.  What is read and written element by element is
// left free: ldc of a product (the vector form of the sparse path has ldc = 1), the vectors of trsv_lower, and everything of
// alpha_from_inverse, logdet_quad and colreduce.
namespace {
inline bool off16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }
inline bool odd(int64_t v) { return (v & 1) != 0; }
const char* gemm_probe_invalid(int ta, int tb, int64_t m, int64_t n, int64_t k, const double* a, int64_t lda, const double* b, int64_t ldb,
                               const double* c, int64_t ldc) {
  if (!a || !b || !c) return "null argument";
  if (!((ta == 0 && tb == 1) || (ta == 0 && tb == 0) || (ta == 1 && tb == 0))) return "unsupported transpose pair";
  if (m <= 0 || n <= 0 || k <= 0 || m > (1 << 30) || n > (1 << 30) || k > (1 << 30)) return "sizes must be positive";
  if (k % GEMM_BK) return "k must be a multiple of 16";
  // (an m/n-contiguous operand of ONE column is read element by element: the vector form of the sparse path has ldb = 1)
  if ((odd(lda) && !(ta == 1 && m == 1)) || (odd(ldb) && !(tb == 0 && n == 1))) return "leading dimensions must be even";
  if (lda < (ta ? m : k) || ldb < (tb ? k : n) || ldc < n) return "leading dimension shorter than a row";
  if (off16(a) || off16(b) || off16(c)) return "operands must be 16-byte aligned";
  return nullptr;
}
const char* solve_probe_invalid(const double* L, int64_t lda, const double* inv_diag, int64_t np, int64_t count, int64_t cs) {
  if (!L || !inv_diag) return "null argument";
  if (np <= 0 || np % NB || np > (1 << 30)) return "np must be a positive multiple of 64";
  if (lda < np || odd(lda)) return "leading dimension must be even and at least np";
  if (count < 1 || odd(cs) || cs < 0) return "count must be positive, strides even";
  if (off16(L) || off16(inv_diag)) return "operands must be 16-byte aligned";
  return nullptr;
}
}  // namespace

int gprx_gemm_batched(int device, int ta, int tb, int64_t m, int64_t n, int64_t k, double alpha, const double* a_dev, int64_t lda,
                      const double* b_dev, int64_t ldb, double beta, double* c_dev, int64_t ldc, int flags, int tile, int batch,
                      int64_t stride_a, int64_t stride_b, int64_t stride_c, int cells, int64_t cell_a, int64_t cell_b, int64_t cell_c,
                      const double* alpha_tab_dev, int alpha_stride, double* rowsq_dev, int64_t rowsq_ld) {
  return guarded(nullptr, [&]() -> int {
    if (const char* why = gemm_probe_invalid(ta, tb, m, n, k, a_dev, lda, b_dev, ldb, c_dev, ldc)) return fail(nullptr, GPRX_EINVAL, why);
    if (tile != 0 && tile != 64 && tile != 128) return fail(nullptr, GPRX_EINVAL, "tile must be 0, 64 or 128");
    if (flags < 0 || flags > 31) return fail(nullptr, GPRX_EINVAL, "unknown flag");
    if (batch < 1 || cells < 1 || alpha_stride < 0) return fail(nullptr, GPRX_EINVAL, "batch and cells must be positive");
    if (odd(stride_a) || odd(stride_b) || odd(stride_c) || odd(cell_a) || odd(cell_b) || odd(cell_c))
      return fail(nullptr, GPRX_EINVAL, "batch and cell strides must be even");
    if (stride_a < 0 || stride_b < 0 || stride_c < 0 || cell_a < 0 || cell_b < 0 || cell_c < 0) return fail(nullptr, GPRX_EINVAL, "negative stride");
    // (rowsq: one product whose 2 * ceil(n / tile) slabs the caller sized for the tile it names)
    if (rowsq_dev && (rowsq_ld < m || (tile != 64 && tile != 128) || batch != 1 || cells != 1))
      return fail(nullptr, GPRX_EINVAL, "rowsq needs tile 64 or 128, one entry, one cell, rowsq_ld at least m");
    HIPCHK(nullptr, hipSetDevice(device));
    HIPCHK(nullptr, launch_gemm(util_stream(), ta, tb, (int)m, (int)n, (int)k, alpha, a_dev, lda, b_dev, ldb, beta, c_dev, ldc, flags, tile, batch,
                                stride_a, stride_b, stride_c, cells, cell_a, cell_b, cell_c, alpha_tab_dev, alpha_stride, rowsq_dev, rowsq_ld));
    HIPCHK(nullptr, hipStreamSynchronize(util_stream()));
    return GPRX_OK;
  });
}

int gprx_gemm_splitk(int device, int ta, int tb, int64_t m, int64_t n, int64_t k, double alpha, const double* a_dev, int64_t lda,
                     const double* b_dev, int64_t ldb, double beta, double* c_dev, int64_t ldc, double* ws_dev, int kchunk, int cells,
                     int64_t cell_a, int64_t cell_b, int64_t cell_c, int64_t ws_cell, const double* alpha_tab_dev, int alpha_stride) {
  return guarded(nullptr, [&]() -> int {
    if (const char* why = gemm_probe_invalid(ta, tb, m, n, k, a_dev, lda, b_dev, ldb, c_dev, ldc)) return fail(nullptr, GPRX_EINVAL, why);
    if (!ws_dev || off16(ws_dev)) return fail(nullptr, GPRX_EINVAL, "workspace must be given, 16-byte aligned");
    if (kchunk <= 0 || kchunk % GEMM_BK) return fail(nullptr, GPRX_EINVAL, "kchunk must be a positive multiple of 16");
    if (cells < 1 || alpha_stride < 0) return fail(nullptr, GPRX_EINVAL, "cells must be positive");
    if (odd(cell_a) || odd(cell_b) || odd(cell_c) || odd(ws_cell) || cell_a < 0 || cell_b < 0 || cell_c < 0)
      return fail(nullptr, GPRX_EINVAL, "cell strides must be even");
    if (cells > 1 && ws_cell < (k + kchunk - 1) / kchunk * m * n) return fail(nullptr, GPRX_EINVAL, "ws_cell shorter than the slabs of one cell");
    HIPCHK(nullptr, hipSetDevice(device));
    HIPCHK(nullptr, launch_gemm_splitk(util_stream(), ta, tb, (int)m, (int)n, (int)k, alpha, a_dev, lda, b_dev, ldb, beta, c_dev, ldc, ws_dev, kchunk,
                                       cells, cell_a, cell_b, cell_c, ws_cell, alpha_tab_dev, alpha_stride));
    HIPCHK(nullptr, hipStreamSynchronize(util_stream()));
    return GPRX_OK;
  });
}

int gprx_trsv_lower(int device, const double* l_dev, int64_t lda, const double* inv_diag_dev, double* b_dev, int64_t np, int transpose,
                    int batch, int64_t cs, double* work_dev) {
  return guarded(nullptr, [&]() -> int {
    if (const char* why = solve_probe_invalid(l_dev, lda, inv_diag_dev, np, batch, cs)) return fail(nullptr, GPRX_EINVAL, why);
    if (!b_dev || (work_dev && (!transpose || batch != 1))) return fail(nullptr, GPRX_EINVAL, "work is for the transposed solve of one system");
    HIPCHK(nullptr, hipSetDevice(device));
    HIPCHK(nullptr, trsv_lower(util_stream(), l_dev, lda, inv_diag_dev, b_dev, (int)np, transpose != 0, batch, cs, work_dev));
    HIPCHK(nullptr, hipStreamSynchronize(util_stream()));
    return GPRX_OK;
  });
}

int gprx_trsm_lower_left(int device, const double* l_dev, int64_t lda, const double* inv_diag_dev, double* b_dev, int64_t ldb, int64_t n,
                         int64_t ncols, int cells, int64_t cs, const double* src_dev) {
  return guarded(nullptr, [&]() -> int {
    if (const char* why = solve_probe_invalid(l_dev, lda, inv_diag_dev, n, cells, cs)) return fail(nullptr, GPRX_EINVAL, why);
    if (!b_dev || off16(b_dev) || (src_dev && off16(src_dev))) return fail(nullptr, GPRX_EINVAL, "right-hand side must be given, 16-byte aligned");
    if (ncols <= 0 || ncols > (1 << 30) || ldb < ncols || odd(ldb)) return fail(nullptr, GPRX_EINVAL, "ldb must be even and at least ncols");
    if (src_dev && n != NB) return fail(nullptr, GPRX_EINVAL, "src is for n == 64 only");
    HIPCHK(nullptr, hipSetDevice(device));
    HIPCHK(nullptr, trsm_lower_left(util_stream(), l_dev, lda, inv_diag_dev, b_dev, ldb, (int)n, (int)ncols, cells, cs, src_dev));
    HIPCHK(nullptr, hipStreamSynchronize(util_stream()));
    return GPRX_OK;
  });
}

int gprx_trtri_lower(int device, const double* l_dev, int64_t lda, const double* inv_diag_dev, double* x_dev, int64_t ldx, double* t_dev,
                     int64_t ldt, int64_t np, int cells, int64_t cs_l, int64_t cs_x, int tile) {
  return guarded(nullptr, [&]() -> int {
    if (const char* why = solve_probe_invalid(l_dev, lda, inv_diag_dev, np, cells, cs_l)) return fail(nullptr, GPRX_EINVAL, why);
    if (!x_dev || !t_dev || off16(x_dev) || off16(t_dev)) return fail(nullptr, GPRX_EINVAL, "X and T must be given, 16-byte aligned");
    if (ldx < np || ldt < np || odd(ldx) || odd(ldt) || odd(cs_x) || cs_x < 0) return fail(nullptr, GPRX_EINVAL, "ldx, ldt, cs_x must be even, rows at least np");
    if (tile != 0 && tile != 64 && tile != 128) return fail(nullptr, GPRX_EINVAL, "tile must be 0, 64 or 128");
    HIPCHK(nullptr, hipSetDevice(device));
    HIPCHK(nullptr, trtri_lower(util_stream(), l_dev, lda, inv_diag_dev, x_dev, ldx, t_dev, ldt, (int)np, cells, cs_l, cs_x, tile));
    HIPCHK(nullptr, hipStreamSynchronize(util_stream()));
    return GPRX_OK;
  });
}

// The batched factorisation, every route of it: potrf_lower with the fused panel (route 0) or the split panel (1), potrf_cells (2).
// A, inv_diag, the staging area (np * STAGE_LD doubles) and the vector right-hand side of cell c live at the given pointers + c * cs.
// The schedule comes from a PotrfTuning of the call's own (outer_block: any multiple of 64 -- 64 itself is the only way to the
// separate K = 64 update; update_tile 64 | 128; 0 = the defaults): the process-wide knobs are neither read nor written.
// info_host[batch]: 0, or col_base + the 1-based failing pivot of that cell; every cell's word is delivered with GPRX_ENOTPD.
int gprx_potrf_batched(int device, double* a_dev, int64_t lda, int64_t np, int64_t extra, double* inv_diag_dev, double* stage_dev,
                       double* yvec_dev, int batch, int64_t cs, int route, int outer_block, int update_tile, int lookahead, int col_base,
                       int* info_host) {
  return guarded(nullptr, [&]() -> int {
    if (!a_dev || !inv_diag_dev || !stage_dev || !info_host) return fail(nullptr, GPRX_EINVAL, "null argument");
    if (np <= 0 || np % NB) return fail(nullptr, GPRX_EINVAL, "np must be a positive multiple of 64");
    if (extra < 0 || np > (1 << 30) || extra > (1 << 30)) return fail(nullptr, GPRX_EINVAL, "extra must not be negative, np and extra at most 2^30");
    if (lda < np || odd(lda) || odd(cs) || cs < 0) return fail(nullptr, GPRX_EINVAL, "lda and cs must be even, lda at least np");
    if (batch > 1 && cs < lda * (np + extra)) return fail(nullptr, GPRX_EINVAL, "cs shorter than one cell's matrix: the cells would overlap");
    if (off16(a_dev) || off16(inv_diag_dev) || off16(stage_dev) || (yvec_dev && off16(yvec_dev)))
      return fail(nullptr, GPRX_EINVAL, "operands must be 16-byte aligned");
    if (batch < 1 || route < 0 || route > 2 || col_base < 0) return fail(nullptr, GPRX_EINVAL, "batch must be positive, route 0, 1 or 2");
    if (yvec_dev && (route != 1 || batch == 1 || extra != 0))
      return fail(nullptr, GPRX_EINVAL, "the vector right-hand side is the split panel's, for batched cells without right-hand-side rows");
    if (route == 2 && extra % NB) return fail(nullptr, GPRX_EINVAL, "the cell kernel takes right-hand-side rows in tiles of 64");
    if (lookahead != 0 && (lookahead != 1 || batch > 1 || route == 2)) return fail(nullptr, GPRX_EINVAL, "look-ahead is for one matrix on routes 0 and 1");
    if (outer_block < 0 || outer_block % NB || (update_tile != 0 && update_tile != 64 && update_tile != 128))
      return fail(nullptr, GPRX_EINVAL, "outer_block must be a multiple of 64, update_tile 0, 64 or 128");
    PotrfTuning tune;  // (defaults, not the process-wide knobs)
    tune.outer_block = outer_block;
    tune.update_tile = update_tile;
    tune.split_panel = route == 1 ? 1 : -1;
    tune.rows_pair = potrf_tuning().rows_pair;  // (the one process default the probe reads: both forms of the split panel's rows launches)
    HIPCHK(nullptr, hipSetDevice(device));
    hipStream_t st = util_stream();
    int* dinfo = nullptr;
    HIPCHK(nullptr, hipMalloc((void**)&dinfo, sizeof(int) * batch));
    hipError_t e = memset_sync(dinfo, 0, sizeof(int) * batch);
    PotrfStreams ps;
    if (e == hipSuccess && lookahead) e = ps.init();
    if (e == hipSuccess)
      e = route == 2 ? potrf_cells(st, a_dev, lda, (int)np, (int)extra, inv_diag_dev, dinfo, batch, cs, 1, col_base)
                     : potrf_lower(st, a_dev, lda, (int)np, (int)extra, inv_diag_dev, dinfo, stage_dev, nullptr, lookahead ? &ps : nullptr, batch, cs, 1,
                                   &tune, col_base, yvec_dev);
    hipError_t e2 = hipStreamSynchronize(st);
    if (ps.aux && e2 == hipSuccess) e2 = hipStreamSynchronize(ps.aux);
    ps.destroy();
    if (e == hipSuccess && e2 == hipSuccess) e2 = copy_sync(info_host, dinfo, sizeof(int) * batch, hipMemcpyDeviceToHost);
    hipFree(dinfo);
    HIPCHK(nullptr, e);
    HIPCHK(nullptr, e2);
    for (int c = 0; c < batch; ++c)
      if (info_host[c]) return fail(nullptr, GPRX_ENOTPD, "matrix not positive definite");
    return GPRX_OK;
  });
}

int gprx_transpose_inplace(int device, double* x_dev, int64_t ld, int64_t n, int cells, int64_t cs) {
  return guarded(nullptr, [&]() -> int {
    if (!x_dev || off16(x_dev)) return fail(nullptr, GPRX_EINVAL, "X must be given, 16-byte aligned");
    if (n <= 0 || n % 64 || n > (1 << 30) || ld < n || odd(ld) || cells < 1 || odd(cs) || cs < 0)
      return fail(nullptr, GPRX_EINVAL, "n must be a positive multiple of 64, ld and cs even");
    HIPCHK(nullptr, hipSetDevice(device));
    HIPCHK(nullptr, transpose_inplace(util_stream(), x_dev, ld, (int)n, cells, cs));
    HIPCHK(nullptr, hipStreamSynchronize(util_stream()));
    return GPRX_OK;
  });
}

int gprx_alpha_from_inverse(int device, const double* x_dev, int64_t ldx, const double* beta_dev, double* part_dev, double* alpha_dev, int64_t np,
                            int cells, int64_t cs_x, int64_t cs_b, int64_t cs_a) {
  return guarded(nullptr, [&]() -> int {
    if (!x_dev || !beta_dev || !part_dev || !alpha_dev) return fail(nullptr, GPRX_EINVAL, "null argument");
    if (np <= 0 || np % NB || np > (1 << 30) || ldx < np || cells < 1 || cs_x < 0 || cs_b < 0 || cs_a < 0)
      return fail(nullptr, GPRX_EINVAL, "np must be a positive multiple of 64");
    HIPCHK(nullptr, hipSetDevice(device));
    HIPCHK(nullptr, alpha_from_inverse(util_stream(), x_dev, ldx, beta_dev, part_dev, alpha_dev, (int)np, cells, cs_x, cs_b, cs_a));
    HIPCHK(nullptr, hipStreamSynchronize(util_stream()));
    return GPRX_OK;
  });
}

int gprx_reduce_probe(int device, int op, const double* m_dev, int64_t ldm, const double* w_dev, int64_t nrows, int64_t ncols, double base,
                      double scale, int accumulate, double* partial_dev, int rows_per_chunk, double* out_dev, int cells, int64_t m_cell,
                      int64_t w_cell, int64_t p_cell, int64_t out_cell, const double* base_tab_dev, const double* base_tab2_dev, int base_stride) {
  return guarded(nullptr, [&]() -> int {
    if (!m_dev || !out_dev) return fail(nullptr, GPRX_EINVAL, "null argument");
    if (nrows <= 0 || ncols <= 0 || nrows > (1 << 30) || ncols > (1 << 30) || cells < 1) return fail(nullptr, GPRX_EINVAL, "sizes must be positive");
    if (m_cell < 0 || w_cell < 0 || p_cell < 0 || out_cell < 0 || base_stride < 0) return fail(nullptr, GPRX_EINVAL, "negative stride");
    hipStream_t st = nullptr;
    switch (op) {
      case GPRX_REDUCE_LOGDET_QUAD:  // M = L (nrows x nrows), w = v or null; out[cell * out_cell + {0, 1}]
        if (ldm < nrows || ncols != nrows || out_cell > (1 << 30)) return fail(nullptr, GPRX_EINVAL, "logdet_quad: square matrix, ldm at least its order");
        HIPCHK(nullptr, hipSetDevice(device));
        st = util_stream();
        hipLaunchKernelGGL(logdet_quad_kernel, dim3(cells), dim3(256), 0, st, m_dev, ldm, w_dev, (int)nrows, out_dev, m_cell, (int)out_cell);
        break;
      case GPRX_REDUCE_COL: {
        if (ldm < ncols || !partial_dev || rows_per_chunk < 1) return fail(nullptr, GPRX_EINVAL, "colreduce: partial and rows_per_chunk needed");
        const int nchunks = (int)((nrows + rows_per_chunk - 1) / rows_per_chunk);
        if (cells > 1 && p_cell < (int64_t)nchunks * ncols) return fail(nullptr, GPRX_EINVAL, "colreduce: p_cell shorter than the partial sums of one cell");
        HIPCHK(nullptr, hipSetDevice(device));
        st = util_stream();
        hipLaunchKernelGGL(colreduce_partial, dim3((unsigned)((ncols + 255) / 256), nchunks, cells), dim3(256), 0, st, m_dev, ldm, w_dev, (int)nrows,
                           (int)ncols, rows_per_chunk, partial_dev, m_cell, w_cell, p_cell);
        hipLaunchKernelGGL(colreduce_final, dim3((unsigned)((ncols + 255) / 256), cells), dim3(256), 0, st, (const double*)partial_dev, nchunks,
                           (int)ncols, base, scale, accumulate, out_dev, p_cell, out_cell, base_tab_dev, base_tab2_dev, base_stride);
        break;
      }
      case GPRX_REDUCE_ROWSQ_FINAL:  // M = the ncols slabs a rowsq GEMM left, ldm apart
        if (ldm < nrows || cells != 1) return fail(nullptr, GPRX_EINVAL, "rowsq_final: one cell, ldm at least nrows");
        HIPCHK(nullptr, hipSetDevice(device));
        st = util_stream();
        hipLaunchKernelGGL(rowsq_final_kernel, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, st, m_dev, (int)ncols, ldm, (int)nrows, base, out_dev);
        break;
      case GPRX_REDUCE_ROW:
        if (ldm < ncols || odd(ldm) || odd(ncols) || off16(m_dev) || (w_dev && off16(w_dev)) || cells != 1)
          return fail(nullptr, GPRX_EINVAL, "rowreduce: one cell, ncols and ldm even, M and w 16-byte aligned");
        HIPCHK(nullptr, hipSetDevice(device));
        st = util_stream();
        hipLaunchKernelGGL(rowreduce_kernel, dim3((unsigned)((nrows + 3) / 4)), dim3(256), 0, st, m_dev, ldm, w_dev, (int)nrows, (int)ncols, base, scale,
                           out_dev);
        break;
      default:
        return fail(nullptr, GPRX_EINVAL, "unknown reduction");
    }
    HIPCHK(nullptr, hipGetLastError());
    HIPCHK(nullptr, hipStreamSynchronize(st));
    return GPRX_OK;
  });
}

// development aid (GPRX_DAG_STAMPS=1): the stamps of the handle's last tile-DAG factorisation; returns the number of words
extern "C" int gprx_dag_stamps(gprx_handle h, unsigned long long* out, int max_words, int* T, int* grid) {
  if (!h || !h->dag.stamps) return 0;
  const int n = (int)std::min<size_t>(h->dag.stamp_words, (size_t)max_words);
  hipStreamSynchronize(h->stream);
  copy_sync(out, h->dag.stamps, sizeof(unsigned long long) * n, hipMemcpyDeviceToHost);
  if (T) *T = h->dag.T;
  if (grid) *grid = h->dag.grid;
  return n;
}

#ifdef GPRX_CHAIN_STAMPS
extern "C" int gprx_chain_stamps(unsigned long long* out16) {
  hipMemcpyFromSymbol(out16, HIP_SYMBOL(gprx::g_chain_stamps), sizeof(unsigned long long) * 16);
  return 0;
}
#endif

#ifdef GPRX_PANEL_ACC
int gprx_panel_acc(unsigned long long* out8, int reset) {
  if (reset) {
    unsigned long long z[8] = {0};
    hipMemcpyToSymbol(HIP_SYMBOL(gprx::g_panel_acc), z, sizeof(z));
  }
  hipMemcpyFromSymbol(out8, HIP_SYMBOL(gprx::g_panel_acc), sizeof(unsigned long long) * 8);
  return 0;
}
#endif
#ifdef GPRX_CELL_ACC
int gprx_cell_acc(unsigned long long* out16, int reset) {
  if (reset) {
    unsigned long long z[16] = {0};
    hipMemcpyToSymbol(HIP_SYMBOL(gprx::g_cell_acc), z, sizeof(z));
  }
  hipMemcpyFromSymbol(out16, HIP_SYMBOL(gprx::g_cell_acc), sizeof(unsigned long long) * 16);
  return 0;
}
#endif
// Development aid: phase stamps (s_memtime, shader clocks) of workgroup (0, 0) of each of the five fused sparse kernels (sgpr_fused.h
// SF_STAMP) for the evaluations that follow enable = 1; out (may be null): SF_STAMP_WORDS words of the last evaluation.
int gprx_sf_stamps(gprx_handle h, int enable, unsigned long long* out) {
  return guarded(h, [&]() -> int {
    if (!h) return fail(h, GPRX_EINVAL, "null handle");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (out && h->sf_stamps) HIPCHK(h, copy_sync(out, h->sf_stamps, sizeof(unsigned long long) * SF_STAMP_WORDS, hipMemcpyDeviceToHost));
    if (enable && !h->sf_stamps) {
      HIPCHK(h, hipMalloc((void**)&h->sf_stamps, sizeof(unsigned long long) * SF_STAMP_WORDS));
      HIPCHK(h, memset_sync(h->sf_stamps, 0, sizeof(unsigned long long) * SF_STAMP_WORDS));
      drop_graphs(h);
    } else if (!enable && h->sf_stamps) {
      HIPCHK(h, hipFree(h->sf_stamps));
      h->sf_stamps = nullptr;
      drop_graphs(h);
    }
    return GPRX_OK;
  });
}
#ifdef GPRX_PANEL_STAMPS
int gprx_panel_stamps(unsigned long long* out64) {
  hipMemcpyFromSymbol(out64, HIP_SYMBOL(gprx::g_panel_stamps), sizeof(unsigned long long) * 64);
  return 0;
}
#endif

namespace {
bool apply_tuning(PotrfTuning& t, int& predict_path, int& fused, int& resident, const std::string& k, int value) {
  if (k == "outer_block" && value >= 0 && value % 128 == 0) t.outer_block = value;
  else if (k == "update_tile" && (value == 0 || value == 64 || value == 128)) t.update_tile = value;
  else if (k == "no_lookahead") t.no_lookahead = value != 0;
  else if (k == "split_panel" && value >= -1 && value <= 1) t.split_panel = value;
  else if (k == "dag" && value >= -1 && value <= 1) t.dag = value;
  else if (k == "rhs_vector" && value >= -1 && value <= 1) t.rhs_vector = value;
  else if (k == "cell_kernel" && value >= -1 && value <= 1) t.cell_kernel = value;
  else if (k == "rows_pair" && value >= 0 && value <= 1) t.rows_pair = value;
  else if (k == "poison_workspace" && value >= 0 && value <= 1) t.poison_workspace = value;
  else if (k == "predict_path" && value >= 0 && value <= 2) predict_path = value;
  else if (k == "sgpr_fused" && value >= 0 && value <= 1) fused = value;
  else if (k == "sgpr_resident" && value >= 0 && value <= 1) resident = value;  // 0: sparse optimiser loops are stepped by the host
  else if (k == "wait_handover_us" && value >= 0) wait_handover_us() = value;  // (process-wide whichever entry point sets it)
  else if (k == "sgpr_groups_from" && value >= 0) sf_groups_from() = value;    // (process-wide; 0: the resident Adam loop never splits a batch into groups)
  // measurement aid of the blocked leave-one-event-out route (process-wide; -1: the schedule gp_loeo_blocked.h fixes per mp)
  else if (k == "loeo_blocked_potrf" && value >= -1 && value <= 2) loeo_blocked_potrf_force() = value;
  // yardstick of the covariance route of the EOF fit (process-wide; read when gprx_pcafit_create_auto runs): 0 = one thread per cell
  else if (k == "pcafit_rowsplit" && value >= 0 && value <= 1) pcafit_rowsplit_tuning() = value;
  else return false;
  return true;
}
}  // namespace

int gprx_set_tuning(const char* key, int value) {
  return guarded(nullptr, [&]() -> int {
    if (!key) return fail(nullptr, GPRX_EINVAL, "null key");
    if (!apply_tuning(potrf_tuning(), predict_path_tuning(), sgpr_fused_tuning(), sgpr_resident_tuning(), key, value)) return fail(nullptr, GPRX_EINVAL, "unknown tuning key or bad value");
    return GPRX_OK;
  });
}

int gprx_set_handle_tuning(gprx_handle h, const char* key, int value) {
  return guarded(h, [&]() -> int {
    if (!h || !key) return fail(h, GPRX_EINVAL, "null argument");
    const int fused_before = h->sgpr_fused;
    if (std::string(key) == "held_general") {  // (a handle key only: gprx.h)
      if (value < 0 || value > 1) return fail(h, GPRX_EINVAL, "unknown tuning key or bad value");
      h->held_general = value;
    } else if (!apply_tuning(h->tune, h->predict_path, h->sgpr_fused, h->sgpr_resident, key, value)) {
      return fail(h, GPRX_EINVAL, "unknown tuning key or bad value");
    }
    if (hipSetDevice(h->device) == hipSuccess && hipStreamSynchronize(h->stream) == hipSuccess) drop_graphs(h);  // captured with the old schedule
    if (h->sgpr_fused != fused_before) {  // the cell blocks of the two sparse schedules differ (sgpr_batch_layout): the arena is rebuilt on the next call
      h->sarena_slots = 0;
      if (h->m != 0) h->factorized = false;
    }
    return GPRX_OK;
  });
}

int gprx_mfma_f64_peak(int device, double* tflops) {
  return guarded(nullptr, [&]() -> int {
    if (!tflops) return fail(nullptr, GPRX_EINVAL, "null argument");
    HIPCHK(nullptr, hipSetDevice(device));
    double* out = nullptr;
    HIPCHK(nullptr, hipMalloc((void**)&out, 64));
    hipEvent_t e0, e1;
    hipEventCreate(&e0);
    hipEventCreate(&e1);
    const int iters = 20000, blocks = 256 * 4;
    hipStream_t us = util_stream();
    hipLaunchKernelGGL(mfma_f64_peak_kernel, dim3(blocks), dim3(256), 0, us, out, 100);
    hipEventRecord(e0, us);
    hipLaunchKernelGGL(mfma_f64_peak_kernel, dim3(blocks), dim3(256), 0, us, out, iters);
    hipEventRecord(e1, us);
    hipError_t e = hipStreamSynchronize(us);
    float ms = 0.f;
    hipEventElapsedTime(&ms, e0, e1);
    hipEventDestroy(e0);
    hipEventDestroy(e1);
    hipFree(out);
    HIPCHK(nullptr, e);
    const double flops = (double)blocks * 4 /*waves*/ * iters * 4 /*mfma*/ * 2048.0;
    *tflops = flops / (ms * 1e-3) / 1e12;
    return GPRX_OK;
  });
}

}  // extern "C"
