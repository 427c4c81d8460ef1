// libgprx: C ABI (include/gprx.h) over the gfx950 kernels in this directory.
// Host orchestration only: parameter transforms and priors (scalar math), buffer ownership,
// launch sequences.  No CPU fallback exists for any device stage.
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
#include "sgpr_step.h"
#include "solve.h"

using namespace gprx;

namespace gprx {

std::string& last_error() {
  thread_local std::string msg;
  return msg;
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

struct Theta {
  double variance, noise;
  std::vector<double> ls;
  double w_var, w_noise;
  std::vector<double> w_len;
};

struct gprx_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  bool own_stream = false;
  int64_t n = 0, m = 0, np = 0, mp = 0;
  int d = 0, kid = 0, ard = 0, nlen = 1, ntheta = 3, n_units = 0;
  int dist_form = 0;  // GPRX_DIST_DIFFERENCE / GPRX_DIST_EXPANDED
  DagPlan dag;        // task list and state words of the tile-DAG factorisation of a lone matrix (potrf_dag.h), created on first use
  bool dag_used = false;  // the current single factorisation ran through it: its abort word travels with the results
  PotrfTuning tune;   // schedule knobs of this handle: the process defaults at creation, then gprx_set_handle_tuning
  int predict_path = 0;
  std::string err;
  // data
  Buf X, Y, invls, alpha, red, Kmat, invD, Xinv, Tmp, partial, xs, Ks, pred;
  Buf dstage;
  std::vector<double> yy;  // y.y per unit
  int* info = nullptr;
  double* pin = nullptr;  // pinned host staging: [0..63] lengthscales up, [64..71] reductions down, [72] info (as int),
                          // [74] variance, [75] noise (graph replay reads them through the device block `gparams`)
  double* gparams = nullptr;            // device {variance, noise} for captured kernel-matrix builds
  std::map<int, hipGraphExec_t> graphs;  // unit -> captured single-stream exact factorisation
  std::map<std::pair<int, int>, hipGraphExec_t> sgraphs;  // (cells, with gradient) -> captured sparse batch evaluation
  bool sgraph_off = false;                                // a capture failed once: this handle stays on eager launches
  std::map<std::pair<int, int>, hipGraphExec_t> rgraphs;  // (cells, optimiser) -> captured step of the resident loop of the launch sequence
  int sgpr_resident = 1;                                  // sparse models: the optimiser loops stay on the device ("sgpr_resident" tuning key)
  int last_route = 0, last_host_waits = 0;                // gprx_last_optimizer_route
  int host_waits = 0;                                     // stream waits of the running optimiser call (wait_stream and the loops' own)
  int sgpr_fused = 1;                                     // M <= 64: the five-launch evaluation of sgpr_fused.h ("sgpr_fused" tuning key)
  Buf adam_dev;                                           // device state of the resident optimiser loops (resident_state)
  double* adam_pin = nullptr;                             // pinned: stop flags of the cells + the error word, read every few steps
  size_t adam_pin_bytes = 0;
  unsigned long long* sf_stamps = nullptr;                // development aid (gprx_sf_stamps): phase stamps of the fused sparse kernels
  static constexpr int SF_MAX_GROUPS = 2;
  hipStream_t sf_streams[SF_MAX_GROUPS - 1] = {};          // extra streams of the resident Adam loop: large batches run as groups of cells (sf_group_plan)
  hipEvent_t sf_evs[SF_MAX_GROUPS] = {};
  // current factorisation (a sparse model's lives in cell block 0 of `sarena`)
  bool factorized = false;
  bool have_linv = false;  // Xinv holds L^-1 of the current factorisation (exact path)
  int cur_unit = -1;
  double variance = 1.0, noise = 1.0;
  std::vector<double> ls;
  double timings[4] = {0, 0, 0, 0};
  bool profiling = false;
  PotrfProfile prof;
  PotrfStreams pstreams;
  double prof_out[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  // batched exact factorisations (gprx_factorize_batch): `arena_slots` cell blocks, `cell_stride` doubles apart, each
  // [K (np + 64) x np | invD np x 64 | staged diagonal blocks np x 128 | alpha np]; parameter / result tables, one row per cell
  Buf arena, cellpar, cellres, garena, gpartial;  // garena: per cell [L^-1 | K^-1] for batched gradients
  Buf apart;                                      // row-chunk partial sums of alpha_from_inverse
  Buf twork;                                      // work vector of the lone backward solve (np doubles)
  hipEvent_t kev[2] = {nullptr, nullptr};         // profiling: events around the kernel-build launch
  double kmat_ms = 0.0, kmat_bytes = 0.0;
  std::vector<Theta> batch_thetas;                // gprx_factorize_batch: decoded parameter sets of the last call (buffers reused)
  std::vector<double> batch_lml;
  hipEvent_t wev = nullptr;                       // completion event of wait_stream
  hipEvent_t cev[2] = {nullptr, nullptr};         // profiling: events around the one-workgroup-per-cell kernel's launch
  bool cev_recorded = false;
  double cell_ms = 0.0, cell_flops = 0.0, cell_cells = 0.0;
  Buf sarena;                                   // batched sparse models: one cell block per slot (sgpr_batch_layout)
  int sarena_slots = 0;
  double* spin = nullptr;  // pinned staging of the sparse batch: parameters up, reductions / gradients down
  size_t spin_doubles = 0;
  double* bpin = nullptr;  // pinned: [slots][CELL_PAR] parameters up, then [slots][CELL_RES] results down
  int arena_slots = 0;
  int64_t cell_stride = 0, off_invd = 0, off_stage = 0, off_alpha = 0;
  std::vector<Theta> slot_theta;
  std::vector<int> slot_unit;
  std::vector<char> slot_ok;
  double batch_ms = 0.0;  // device time of the last batch (events around the whole batch)
  hipEvent_t bev[2] = {nullptr, nullptr};
};

namespace {

// kernel-matrix and trace launches evaluate r2 in the handle's distance form (gprx_set_distance_form)
template <class Args>
Args with_form(Args a, gprx_handle h) {
  a.form = h->dist_form;
  return a;
}

int& predict_path_tuning() {
  static int v = 0;  // 0: choose, 1: always through L^-1, 2: always forward substitution
  return v;
}

// ---- scalar transforms (gpflow positive() / LogNormal(0,1) priors; see oracle/transforms.py) ------
// (round 5: the portable forms of px_math.h -- the device-resident Adam loop evaluates the same functions inside a kernel and must get the
// same bits as this host code)
double softplus(double w) { return px_softplus(w); }
double sigmoid(double w) { return px_sigmoid(w); }
double ln_logpdf(double u) { return px_ln_logpdf(u); }
double ln_dlogpdf(double u) { return px_ln_dlogpdf(u); }

__global__ void set_rhs_rows_kernel(double* dst, int64_t ld, const double* y, int n, int np, int rows) {
  const int64_t total = (int64_t)rows * np;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(e / np), c = (int)(e % np);
    dst[(int64_t)r * ld + c] = (r == 0 && c < n) ? y[c] : 0.0;
  }
}

__global__ void copy_row_kernel(const double* src, double* dst, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

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

void decode_theta_into(gprx_handle h, const double* theta, Theta& t) {
  t.w_var = theta[0];
  t.w_noise = theta[1 + h->nlen];
  t.variance = softplus(t.w_var);
  t.noise = NOISE_LOWER + softplus(t.w_noise);
  t.w_len.assign(theta + 1, theta + 1 + h->nlen);
  t.ls.resize(h->d);
  if (h->ard) {
    for (int k = 0; k < h->d; ++k) t.ls[k] = softplus(t.w_len[k]);
  } else {
    const double l = softplus(t.w_len[0]);  // (one shared lengthscale: one softplus, not d)
    for (int k = 0; k < h->d; ++k) t.ls[k] = l;
  }
}
Theta decode_theta(gprx_handle h, const double* theta) {
  Theta t;
  decode_theta_into(h, theta, t);
  return t;
}

// Wait for everything enqueued on `st`.  hipStreamSynchronize blocks in the driver and returns 60-100 us after the GPU has finished
// (tools/batch_overhead.py: 150 us of host time around a 1.1 ms batch of 512 cells of N = 512 -- 12 % of the call, 3 % at N = 1024, 4 % of a
// lone N = 4096 fit); a completion event polled from the calling thread returns within a few us.  Pure spinning for the first 2 ms, then the
// poll yields the core between queries, and after 200 ms (the long batched steps, where the wake-up latency is noise) it hands over to
// hipStreamSynchronize.  GPRX_WAIT_BLOCKING=1 restores the blocking wait.
int& wait_handover_us() {
  static int v = 200000;  // gprx_set_tuning("wait_handover_us", ...): tests lower it to 0 to force the hand-over path
  return v;
}
hipError_t wait_stream(gprx_handle h, hipStream_t st) {
  static const bool blocking = getenv("GPRX_WAIT_BLOCKING") && atoi(getenv("GPRX_WAIT_BLOCKING")) != 0;
  if (blocking) {
    ++h->host_waits;
    return hipStreamSynchronize(st);
  }
  if (!h->wev) {
    hipError_t e = hipEventCreateWithFlags(&h->wev, hipEventDisableTiming);
    if (e != hipSuccess) return e;
  }
  hipError_t e = hipEventRecord(h->wev, st);
  if (e != hipSuccess) return e;
  ++h->host_waits;
  const auto t0 = std::chrono::steady_clock::now();
  for (int spins = 0;; ++spins) {
    e = hipEventQuery(h->wev);
    if (e != hipErrorNotReady) {
      // (a poll that found the event pending may have left hipErrorNotReady behind as the thread's "last error": the launch helpers end
      // with hipGetLastError() and must not trip over it)
      if (spins > 0) (void)hipGetLastError();
      return e;
    }
    if ((spins & 63) == 63) {
      const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
      if (us > (double)wait_handover_us()) {
        // (the polls above left hipErrorNotReady as the thread's last error -- it is sticky across later successful calls on
        // this runtime -- and the next launch helper ending in hipGetLastError() would report it for a good call)
        (void)hipGetLastError();
        return hipStreamSynchronize(st);
      }
      if (us > 2000.0) std::this_thread::yield();
    }
  }
}

double log_prior(gprx_handle h, const Theta& t, int mask) {
  double lp = 0.0;
  if (mask & GPRX_TRAIN_VARIANCE) lp += ln_logpdf(t.variance);
  if (mask & GPRX_TRAIN_LENGTHSCALE)
    for (int k = 0; k < h->nlen; ++k) lp += ln_logpdf(t.ls[k]);
  if (mask & GPRX_TRAIN_NOISE) lp += ln_logpdf(t.noise);
  return lp;
}

int upload_inv_ls(gprx_handle h, const Theta& t) {  // uploads the lengthscales (kernels divide by them)
  if (h->d <= 64) {
    // pinned staging: truly asynchronous (the previous use of the staging area was synchronised by the
    // previous call's final stream synchronisation)
    std::memcpy(h->pin, t.ls.data(), sizeof(double) * h->d);
    HIPCHK(h, hipMemcpyAsync(h->invls.p, h->pin, sizeof(double) * h->d, hipMemcpyHostToDevice, h->stream));
    return GPRX_OK;
  }
  HIPCHK(h, hipMemcpyAsync(h->invls.p, t.ls.data(), sizeof(double) * h->d, hipMemcpyHostToDevice, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return GPRX_OK;
}

// ---- exact GP ------------------------------------------------------------------------------------
// K = k(X,X) + s I (lower tiles) with y appended as row np; potrf gives L and beta = L^-1 y in that
// row; alpha by the backward solve; red[0] = sum log diag L, red[1] = |beta|^2.
int ensure_lookahead(gprx_handle h) {
  if (h->pstreams.aux) return GPRX_OK;
  HIPCHK(h, h->pstreams.init());
  return GPRX_OK;
}

// "dag" (gprx_set_tuning) = 1: a lone matrix takes the tile-DAG factorisation (potrf_dag.h: one persistent launch, the dependent
// chain in one workgroup, tile tasks ordered by version counters).  Opt-in: measured on MI355X at N = 4096 it reaches 2.33 ms
// against 2.16 ms for the launch-per-panel schedule (every row block has a dependent TRSM -> update pair
// per column, each costing two or more ~2 us memory hops, as much as the 1.7 us of MFMA work in a 64^3 tile).
bool use_dag(const PotrfTuning& tune, int np) { return tune.dag > 0 && np >= NB; }

// Batched cells: the one-workgroup-per-cell factorisation (potrf_cell.h) for matrices of at most 1024 rows once the batch has
// enough cells ("cell_kernel": 1 always, -1 never).  Equal to the batched launch sequence to rounding, not bit for bit (a tile's
// whole update is one sum there); larger matrices or fewer cells keep the launch sequence (bit-identical to single calls).
bool use_cell_kernel(const PotrfTuning& tune, int np, int cells) {
  if (tune.cell_kernel < 0) return false;
  if (tune.cell_kernel > 0) return true;
  // measured crossovers (tools/batch_n1024.py, fits/s cell kernel vs launch sequence): N = 256: 137 k vs 118 k at 32 cells (76 k vs 92 k
  // at 16); N = 512: tie at 128 cells, 262 k vs 223 k at 256; N = 1024: 64.3 k vs 62.5 k at 256 cells, 71 k vs 67.8 k at 512, 38 k vs
  // 53 k at 128 -- one workgroup per cell needs a cell for every CU before it beats launches that spread one cell over many
  if (np <= 256) return cells >= 32;
  if (np <= 512) return cells >= 160;
  return np <= 1024 && cells >= 256;
}

// with_alpha = false: the backward substitution is left out -- the caller goes on to the gradient, which forms alpha from the
// explicit inverse it builds anyway (alpha_from_inverse)
int exact_factorize_enqueue(gprx_handle h, int unit, const Theta& t, bool lookahead = true, bool capture = false, bool with_alpha = true) {
  const int np = (int)h->np;
  const int64_t ld = h->np;
  int rc;
  if ((rc = ensure(h, h->Kmat, sizeof(double) * (h->np + NB) * ld))) return rc;
  if ((rc = ensure(h, h->invD, sizeof(double) * h->np * NB))) return rc;
  if ((rc = ensure(h, h->alpha, sizeof(double) * h->np))) return rc;
  if ((rc = ensure(h, h->twork, sizeof(double) * h->np))) return rc;
  if ((rc = ensure(h, h->dstage, sizeof(double) * h->np * STAGE_LD))) return rc;
  if (lookahead && (rc = ensure_lookahead(h))) return rc;
  if (h->Kmat.borrowed && h->arena.p && h->cell_stride > 0) {
    // Kmat / invD / alpha are views into a slot of the last batch (gprx_select_slot): this call overwrites that slot's
    // factorisation, so the slot no longer holds what slot_theta / slot_unit say
    const int64_t slot = (h->Kmat.p - h->arena.p) / h->cell_stride;
    if (slot >= 0 && slot < (int64_t)h->slot_ok.size()) {
      h->slot_ok[slot] = 0;
      h->slot_unit[slot] = -1;
    }
  }
  hipStream_t st = h->stream;
  if (capture) {
    // replayable form: every theta-dependent value travels pinned host -> device inside the graph
    HIPCHK(h, hipMemcpyAsync(h->invls.p, h->pin, sizeof(double) * h->d, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(h->gparams, h->pin + 74, sizeof(double) * 2, hipMemcpyHostToDevice, st));
  } else {
    if ((rc = upload_inv_ls(h, t))) return rc;
    HIPCHK(h, hipEventRecord(h->ev[0], st));
  }
  KmatArgs ka{h->X.p, h->X.p, h->invls.p, h->Kmat.p, ld, (int)h->n, (int)h->n, h->d, np, np, t.variance, t.noise, 1, 1.0,
              capture ? h->gparams : nullptr, 0};
  if (h->profiling && !capture) {
    if (!h->kev[0]) {
      HIPCHK(h, hipEventCreate(&h->kev[0]));
      HIPCHK(h, hipEventCreate(&h->kev[1]));
    }
    HIPCHK(h, hipEventRecord(h->kev[0], st));
  }
  HIPCHK(h, launch_kmat(st, h->kid, with_form(ka, h)));
  if (h->profiling && !capture) {
    HIPCHK(h, hipEventRecord(h->kev[1], st));
    h->kmat_bytes = 8.0 * KM_T * KM_T * (double)(np / KM_T) * (np / KM_T + 1) / 2;  // the lower 64 x 64 tiles
  }
  hipLaunchKernelGGL(set_rhs_rows_kernel, dim3(64), dim3(256), 0, st, h->Kmat.p + (int64_t)np * ld, ld, h->Y.p + (int64_t)unit * h->np,
                     (int)h->n, np, NB);
  if (!capture) HIPCHK(h, hipEventRecord(h->ev[1], st));
  HIPCHK(h, hipMemsetAsync(h->info, 0, sizeof(int), st));
  if (h->profiling) h->prof.reset();
  h->dag_used = false;
  if (use_dag(h->tune, np) && !capture && !h->profiling) {
    HIPCHK(h, potrf_dag(st, h->Kmat.p, ld, np, NB, h->invD.p, h->info, h->dag));
    h->dag_used = true;
  } else {
    HIPCHK(h, potrf_lower(st, h->Kmat.p, ld, np, NB, h->invD.p, h->info, h->dstage.p, h->profiling ? &h->prof : nullptr,
                          lookahead ? &h->pstreams : nullptr, 1, 0, 0, &h->tune));
  }
  if (!capture) HIPCHK(h, hipEventRecord(h->ev[2], st));
  const double* beta = h->Kmat.p + (int64_t)np * ld;
  // (alpha = L^-T beta: beta is copied into a work vector that the solve uses up, alpha receives the solution -- two block steps per launch)
  if (with_alpha) hipLaunchKernelGGL(copy_row_kernel, dim3((np + 255) / 256), dim3(256), 0, st, beta, h->twork.p, np);
  hipLaunchKernelGGL(logdet_quad_kernel, dim3(1), dim3(256), 0, st, (const double*)h->Kmat.p, ld, beta, np, h->red.p, (int64_t)0, 0);
  if (with_alpha) HIPCHK(h, trsv_lower(st, h->Kmat.p, ld, h->invD.p, h->alpha.p, np, true, 1, 0, h->twork.p));
  if (!capture) HIPCHK(h, hipEventRecord(h->ev[3], st));
  HIPCHK(h, hipMemcpyAsync(h->pin + 64, h->red.p, sizeof(double) * 2, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(h->pin + 72, h->info, sizeof(int), hipMemcpyDeviceToHost, st));
  if (h->dag_used) HIPCHK(h, hipMemcpyAsync(h->pin + 73, h->dag.state + DAG_ABORT, sizeof(int), hipMemcpyDeviceToHost, st));
  h->factorized = false;
  h->cur_unit = unit;
  h->variance = t.variance;
  h->noise = t.noise;
  h->ls = t.ls;
  return GPRX_OK;
}

// one stream capture at a time in the process (two concurrent thread-local captures on different handles disturbed each other)
std::mutex& capture_mutex() {
  static std::mutex m;
  return m;
}

// Throughput mode (gprx_factorize_many with several cells): the ~250 launches of one single-stream fit are
// captured once per (handle, unit) into a hipGraph and replayed; only the pinned parameter block changes.
// Measured on MI355X with 16 cells of N = 4096 in flight: 784 fits/s eager, 800 fits/s replayed -- the limit is
// the device (4 hardware queues, each cell ~1.8x slower under 4-way sharing), the replay mainly frees the host.
int exact_factorize_replay(gprx_handle h, int unit, const Theta& t) {
  static const bool no_graph = getenv("GPRX_NO_GRAPH") != nullptr;  // escape hatch: eager launches
  if (h->d > 64 || h->profiling || no_graph) return exact_factorize_enqueue(h, unit, t, false);
  auto it = h->graphs.find(unit);
  if (it == h->graphs.end()) {
    // buffers must exist before capture: a first eager pass allocates them (and is a valid fit by itself)
    if (!h->Kmat.p || !h->invD.p || !h->alpha.p || !h->dstage.p) return exact_factorize_enqueue(h, unit, t, false);
    std::memcpy(h->pin, t.ls.data(), sizeof(double) * h->d);
    h->pin[74] = t.variance;
    h->pin[75] = t.noise;
    std::lock_guard<std::mutex> lock(capture_mutex());  // (captures are serialised over the process, see sgpr_objective_batch)
    hipGraph_t graph = nullptr;
    HIPCHK(h, hipStreamBeginCapture(h->stream, hipStreamCaptureModeRelaxed));
    const int rc = exact_factorize_enqueue(h, unit, t, false, true);
    hipError_t e = hipStreamEndCapture(h->stream, &graph);
    if (rc) {
      if (graph) hipGraphDestroy(graph);
      return rc;
    }
    HIPCHK(h, e);
    hipGraphExec_t exec = nullptr;
    e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
    hipGraphDestroy(graph);
    HIPCHK(h, e);
    it = h->graphs.emplace(unit, exec).first;
  }
  std::memcpy(h->pin, t.ls.data(), sizeof(double) * h->d);
  h->pin[74] = t.variance;
  h->pin[75] = t.noise;
  HIPCHK(h, hipGraphLaunch(it->second, h->stream));
  h->dag_used = false;  // a replayed fit is always the launch-per-panel schedule ("dag" applies to eager single factorisations only)
  h->factorized = false;
  h->cur_unit = unit;
  h->variance = t.variance;
  h->noise = t.noise;
  h->ls = t.ls;
  return GPRX_OK;
}

void summarize_profile(gprx_handle h) {
  double gemm_ms = 0.0, gemm_flops = 0.0, panel_ms = 0.0;
  for (auto& mk : h->prof.gemm_marks) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, h->prof.pool[mk.first], h->prof.pool[mk.first + 1]);
    gemm_ms += ms;
    gemm_flops += mk.second;
  }
  for (auto idx : h->prof.panel_marks) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, h->prof.pool[idx], h->prof.pool[idx + 1]);
    panel_ms += ms;
  }
  h->prof_out[0] = gemm_ms;
  h->prof_out[1] = (double)h->prof.gemm_marks.size();
  h->prof_out[2] = gemm_flops;
  h->prof_out[3] = panel_ms;
  h->prof_out[4] = (double)h->prof.panel_marks.size();
  double strip_ms = 0.0, strip_flops = 0.0;
  for (auto& mk : h->prof.strip_marks) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, h->prof.pool[mk.first], h->prof.pool[mk.first + 1]);
    strip_ms += ms;
    strip_flops += mk.second;
  }
  if (h->kev[0]) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->kev[0], h->kev[1]) == hipSuccess) h->kmat_ms = ms;
  }
  h->cell_ms = 0.0;
  if (h->cev_recorded) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, h->cev[0], h->cev[1]) == hipSuccess) h->cell_ms = ms;
    h->cev_recorded = false;
  }
  h->prof_out[5] = strip_ms;
  h->prof_out[6] = (double)h->prof.strip_marks.size();
  h->prof_out[7] = strip_flops;
}

int exact_factorize_finish(gprx_handle h, double* lml_out) {
  HIPCHK(h, wait_stream(h, h->stream));
  const double* red = h->pin + 64;
  int info = 0;
  std::memcpy(&info, h->pin + 72, sizeof(int));
  if (h->profiling) summarize_profile(h);
  if (h->dag_used) {
    int gave_up = 0;
    std::memcpy(&gave_up, h->pin + 73, sizeof(int));
    if (gave_up != 0) {
      h->factorized = false;
      return fail(h, GPRX_EHIP, "tile-DAG factorisation: a dependency wait timed out (scheduler gave up, code " + std::to_string(gave_up) + ")");
    }
  }
  if (info != 0) {
    h->factorized = false;
    char msg[128];
    snprintf(msg, sizeof msg, "matrix not positive definite: pivot %d", info);
    return fail(h, GPRX_ENOTPD, msg);
  }
  h->factorized = true;
  h->have_linv = false;
  if (lml_out) *lml_out = -0.5 * red[1] - red[0] - 0.5 * (double)h->n * PX_LOG_2PI;
  return GPRX_OK;
}

int exact_factorize(gprx_handle h, int unit, const Theta& t, double* lml_out) {
  int rc = exact_factorize_enqueue(h, unit, t);
  if (rc) return rc;
  return exact_factorize_finish(h, lml_out);
}

// ---- batched exact factorisations -------------------------------------------------------------------------
// Independent cells (one unit and one hyperparameter vector each, all on this handle's x) factorised by the
// SAME launches: every kernel of the single-cell schedule carries the cell index in a grid dimension, so one
// panel launch is cells x (rows / 128) workgroups and one trailing update is cells x tiles -- the chip is full
// although a single N = 4096 panel occupies 33 of 256 CUs.  Same kernels, same per-element operation order:
// the results are bit-identical to gprx_factorize on each cell.
constexpr int CELL_RES = 4;  // per cell: [0] sum log diag L, [1] |L^-1 y|^2, [2] info (int), [3] unused

__global__ void set_rhs_rows_batch_kernel(double* dst, int64_t ld, const double* ybase, const double* cell_par, int n, int np, int rows,
                                          int64_t cs) {
  const int cell = blockIdx.y;
  const double* y = ybase + (int64_t)cell_par[(int64_t)cell * CELL_PAR + 2] * np;
  dst += (int64_t)cell * cs;
  const int64_t total = (int64_t)rows * np;
  for (int64_t e = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; e < total; e += (int64_t)gridDim.x * blockDim.x) {
    const int r = (int)(e / np), c = (int)(e % np);
    dst[(int64_t)r * ld + c] = (r == 0 && c < n) ? y[c] : 0.0;
  }
}

__global__ void copy_row_batch_kernel(const double* src, double* dst, int n, int64_t cs) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[(int64_t)blockIdx.y * cs + i] = src[(int64_t)blockIdx.y * cs + i];
}

void drop_graphs(gprx_handle h) {
  for (auto& kv : h->graphs) hipGraphExecDestroy(kv.second);
  h->graphs.clear();
  for (auto& kv : h->sgraphs)
    if (kv.second) hipGraphExecDestroy(kv.second);
  h->sgraphs.clear();
  for (auto& kv : h->rgraphs)
    if (kv.second) hipGraphExecDestroy(kv.second);
  h->rgraphs.clear();
}

// views of the single-cell buffers into the arena are invalid once it moves
void drop_arena_views(gprx_handle h) {
  for (Buf* b : {&h->Kmat, &h->invD, &h->alpha})
    if (b->borrowed) {
      b->p = nullptr;
      b->bytes = 0;
      b->borrowed = false;
      h->factorized = false;
      h->have_linv = false;
    }
  drop_graphs(h);
}

int ensure_arena(gprx_handle h, int slots) {
  if (h->arena_slots >= slots) return GPRX_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  drop_arena_views(h);
  const int64_t np = h->np;
  h->off_invd = (np + NB) * np;
  h->off_stage = h->off_invd + np * NB;
  h->off_alpha = h->off_stage + np * STAGE_LD;
  h->cell_stride = round_up(h->off_alpha + np, 64);
  for (Buf* b : {&h->arena, &h->cellpar, &h->cellres}) {
    if (b->p) HIPCHK(h, hipFree(b->p));
    b->p = nullptr;
    b->bytes = 0;
  }
  if (h->bpin) HIPCHK(h, hipHostFree(h->bpin));
  h->bpin = nullptr;
  h->arena_slots = 0;
  int rc;
  if ((rc = ensure(h, h->arena, sizeof(double) * (size_t)h->cell_stride * slots))) return rc;
  if ((rc = ensure(h, h->cellpar, sizeof(double) * CELL_PAR * slots))) return rc;
  if ((rc = ensure(h, h->cellres, sizeof(double) * CELL_RES * slots))) return rc;
  HIPCHK(h, hipHostMalloc((void**)&h->bpin, sizeof(double) * (CELL_PAR + CELL_RES) * slots, hipHostMallocDefault));
  if (!h->bev[0]) {
    HIPCHK(h, hipEventCreate(&h->bev[0]));
    HIPCHK(h, hipEventCreate(&h->bev[1]));
  }
  h->arena_slots = slots;
  h->slot_theta.assign(slots, Theta());
  h->slot_unit.assign(slots, -1);
  h->slot_ok.assign(slots, 0);
  return GPRX_OK;
}

int exact_factorize_batch(gprx_handle h, int count, const int* units, const Theta* ts, double* lml_out, int* status_out, bool with_alpha = true) {
  int rc;
  if ((rc = ensure_arena(h, count))) return rc;
  const int np = (int)h->np;
  const int64_t ld = h->np, cs = h->cell_stride;
  hipStream_t st = h->stream;
  double* par = h->bpin;
  double* res = h->bpin + (size_t)CELL_PAR * h->arena_slots;
  for (int c = 0; c < count; ++c) {
    double* row = par + (size_t)c * CELL_PAR;
    std::memset(row, 0, sizeof(double) * CELL_PAR);
    row[0] = ts[c].variance;
    row[1] = ts[c].noise;
    row[2] = (double)units[c];
    for (int k = 0; k < h->d; ++k) row[CELL_PAR_LS + k] = ts[c].ls[k];
    h->slot_ok[c] = 0;
  }
  // Optional (GPRX_BATCH_GROUPS=2): two groups of cells on two streams run the same launch sequence out of phase, so
  // the panel launches of one overlap the MFMA-bound updates of the other.  Measured at N = 4096: +2.5 % at 32 cells,
  // +3 % at 64, nothing at 16, -5 % at 8 -- not worth a default whose per-launch timings depend on what the other
  // stream happens to run.  Per-cell arithmetic is the same either way.
  static const int env_groups = getenv("GPRX_BATCH_GROUPS") ? atoi(getenv("GPRX_BATCH_GROUPS")) : 0;
  const int groups = (h->profiling || count < 2) ? 1 : (env_groups > 1 ? 2 : 1);
  if (groups > 1 && (rc = ensure_lookahead(h))) return rc;
  HIPCHK(h, hipEventRecord(h->bev[0], st));
  HIPCHK(h, hipMemcpyAsync(h->cellpar.p, par, sizeof(double) * CELL_PAR * count, hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemsetAsync(h->cellres.p, 0, sizeof(double) * CELL_RES * count, st));
  if (h->profiling) h->prof.reset();
  auto enqueue_group = [&](hipStream_t gs, int c0, int cnt) -> int {
    double* K0 = h->arena.p + (int64_t)c0 * cs;
    const double* cpar = h->cellpar.p + (int64_t)c0 * CELL_PAR;
    double* cres = h->cellres.p + (int64_t)c0 * CELL_RES;
    KmatArgs ka{h->X.p, h->X.p, nullptr, K0, ld, (int)h->n, (int)h->n, h->d, np, np, 0.0, 0.0, 1, 1.0, nullptr, 0};
    ka.cell_par = cpar;
    ka.out_stride = cs;
    // (under profiling the launch sequence is instrumented launch by launch; the cell kernel -- ONE launch -- is timed when the handle
    // forces it, "cell_kernel" = 1: gprx_last_cell_kernel)
    const bool cell_kernel = use_cell_kernel(h->tune, np, cnt) && (!h->profiling || h->tune.cell_kernel > 0);
    // (the column-pair cell kernel evaluates K where it consumes it: no build launch, nothing written but the right-hand-side rows)
    const bool cell_builds_k = cell_kernel && potrf_cells_builds_k(h->kid, h->dist_form, np, h->d);
    if (h->profiling) {
      if (!h->kev[0]) {
        HIPCHK(h, hipEventCreate(&h->kev[0]));
        HIPCHK(h, hipEventCreate(&h->kev[1]));
      }
      HIPCHK(h, hipEventRecord(h->kev[0], gs));
    }
    if (!cell_builds_k) HIPCHK(h, launch_kmat(gs, h->kid, with_form(ka, h), cnt));
    if (h->profiling) {
      HIPCHK(h, hipEventRecord(h->kev[1], gs));
      h->kmat_bytes = 8.0 * KM_T * KM_T * (double)(np / KM_T) * (np / KM_T + 1) / 2 * cnt;
    }
    // (the column-pair cell kernel carries the right-hand side as a vector: one row, of which it reads and writes the first np entries)
    // (so does the launch sequence's split panel: potrf_rows_kernel<..., YVEC>)
    const bool rhs_vector = !cell_kernel && potrf_rhs_vector_ok(h->tune, cnt);
    const bool beta_vector = rhs_vector || (cell_kernel && !cell_builds_k && potrf_cells_beta_vector(np, NB, false));
    hipLaunchKernelGGL(set_rhs_rows_batch_kernel, dim3(beta_vector ? 4 : 64, cnt), dim3(256), 0, gs, K0 + (int64_t)np * ld, ld, (const double*)h->Y.p, cpar,
                       (int)h->n, np, beta_vector ? 1 : NB, cs);
    int* info0 = reinterpret_cast<int*>(cres + 2);
    if (cell_kernel) {
      // small matrices in many cells: one workgroup owns one cell from the first column to the last (potrf_cell.h)
      if (h->profiling) {
        if (!h->cev[0]) {
          HIPCHK(h, hipEventCreate(&h->cev[0]));
          HIPCHK(h, hipEventCreate(&h->cev[1]));
        }
        HIPCHK(h, hipEventRecord(h->cev[0], gs));
      }
      if (cell_builds_k)
        HIPCHK(h, potrf_cells(gs, K0, ld, np, NB, K0 + h->off_invd, info0, cnt, cs, 2 * CELL_RES, 0, h->X.p, cpar, (int)h->n, h->d));
      else
        HIPCHK(h, potrf_cells(gs, K0, ld, np, NB, K0 + h->off_invd, info0, cnt, cs, 2 * CELL_RES));
      if (h->profiling) {
        HIPCHK(h, hipEventRecord(h->cev[1], gs));
        h->cev_recorded = true;
        h->cell_cells = cnt;
        h->cell_flops = (double)np * np * np / 3.0 * cnt;  // algorithmic: N^3 / 3 per cell (the right-hand-side rows' N^2 not counted)
      }
    } else {
      HIPCHK(h, potrf_lower(gs, K0, ld, np, rhs_vector ? 0 : NB, K0 + h->off_invd, info0, K0 + h->off_stage, h->profiling ? &h->prof : nullptr, nullptr, cnt, cs,
                            2 * CELL_RES, &h->tune, 0, rhs_vector ? K0 + (int64_t)np * ld : nullptr));
    }
    const double* beta = K0 + (int64_t)np * ld;
    if (with_alpha) hipLaunchKernelGGL(copy_row_batch_kernel, dim3((np + 255) / 256, cnt), dim3(256), 0, gs, beta, K0 + h->off_alpha, np, cs);
    hipLaunchKernelGGL(logdet_quad_kernel, dim3(cnt), dim3(256), 0, gs, (const double*)K0, ld, beta, np, cres, cs, CELL_RES);
    if (with_alpha) HIPCHK(h, trsv_lower(gs, K0, ld, K0 + h->off_invd, K0 + h->off_alpha, np, true, cnt, cs));  // (else: exact_gradient_batch)
    return GPRX_OK;
  };
  if (groups == 1) {
    if ((rc = enqueue_group(st, 0, count))) return rc;
  } else {
    const int first = (count + 1) / 2;
    hipStream_t aux = h->pstreams.aux;
    HIPCHK(h, hipEventRecord(h->pstreams.block_done, st));  // parameter table and cleared results are on the main stream
    HIPCHK(h, hipStreamWaitEvent(aux, h->pstreams.block_done, 0));
    // (the two groups start in phase; staggering the second behind the first group's first in-block phase measured -1.7 %: DESIGN.md 7b.2)
    if ((rc = enqueue_group(st, 0, first))) return rc;
    if ((rc = enqueue_group(aux, first, count - first))) return rc;
    HIPCHK(h, hipEventRecord(h->pstreams.tail_done, aux));
    HIPCHK(h, hipStreamWaitEvent(st, h->pstreams.tail_done, 0));
  }
  HIPCHK(h, hipMemcpyAsync(res, h->cellres.p, sizeof(double) * CELL_RES * count, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipEventRecord(h->bev[1], st));
  HIPCHK(h, wait_stream(h, st));
  float ms = 0.f;
  hipEventElapsedTime(&ms, h->bev[0], h->bev[1]);
  h->batch_ms = ms;
  if (h->profiling) summarize_profile(h);
  int first_error = GPRX_OK;
  for (int c = 0; c < count; ++c) {
    int info = 0;
    std::memcpy(&info, res + (size_t)c * CELL_RES + 2, sizeof(int));
    h->slot_theta[c] = ts[c];
    h->slot_unit[c] = units[c];
    h->slot_ok[c] = info == 0;
    if (status_out) status_out[c] = info == 0 ? GPRX_OK : GPRX_ENOTPD;
    if (info != 0) {
      if (!first_error) {
        char msg[160];
        snprintf(msg, sizeof msg, "cell %d: matrix not positive definite: pivot %d", c, info);
        first_error = fail(h, GPRX_ENOTPD, msg);
      }
      if (lml_out) lml_out[c] = std::numeric_limits<double>::quiet_NaN();
      continue;
    }
    const double* r = res + (size_t)c * CELL_RES;
    if (lml_out) lml_out[c] = -0.5 * r[1] - r[0] - 0.5 * (double)h->n * PX_LOG_2PI;
  }
  // a single-cell view into a slot of this batch is stale now
  for (Buf* b : {&h->Kmat, &h->invD, &h->alpha})
    if (b->borrowed) {
      h->factorized = false;
      h->have_linv = false;
    }
  return first_error;
}

// make slot `slot` of the last batch the handle's current factorisation (predict / gradient work on it)
int select_slot(gprx_handle h, int slot) {
  if (slot < 0 || slot >= h->arena_slots || h->slot_unit[slot] < 0) return fail(h, GPRX_EINVAL, "slot holds no factorisation");
  if (!h->slot_ok[slot]) return fail(h, GPRX_ESTATE, "the factorisation of this slot failed");
  double* base = h->arena.p + (int64_t)slot * h->cell_stride;
  auto view = [&](Buf& b, double* p, size_t bytes) {
    if (b.p && !b.borrowed) hipFree(b.p);
    b.p = p;
    b.bytes = bytes;
    b.borrowed = true;
  };
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (h->Kmat.p != base) drop_graphs(h);
  view(h->Kmat, base, sizeof(double) * (h->np + NB) * h->np);
  view(h->invD, base + h->off_invd, sizeof(double) * h->np * NB);
  view(h->alpha, base + h->off_alpha, sizeof(double) * h->np);
  const Theta& t = h->slot_theta[slot];
  int rc;
  if ((rc = upload_inv_ls(h, t))) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->cur_unit = h->slot_unit[slot];
  h->variance = t.variance;
  h->noise = t.noise;
  h->ls = t.ls;
  h->factorized = true;
  h->have_linv = false;
  return GPRX_OK;
}

// K^-1 = X^T X (X = L^-1) as the TN product on the LDS-DMA kernel (default), or GPRX_KINV_TN=0: X transposed in place and the NT
// product of L^-T with itself (one more pass over X: 5.9 ms per 128 cells of N = 4096); the same sums in the same k order.
bool kinv_tn() {
  static const bool v = !(getenv("GPRX_KINV_TN") && atoi(getenv("GPRX_KINV_TN")) == 0);
  return v;
}

// Gradients of the LML for every cell of the batch just factorised (slots 0 .. count-1): the single-cell stages
// (L^-1 by bottom-up doubling, K^-1 = L^-T L^-1 on the lower tiles, one trace pass for all 2 + d derivatives) with
// the cell index in the grid.  g: count x ntheta, constrained parameters (variance, lengthscales, noise); rows of
// failed cells are left untouched.
int exact_gradient_batch(gprx_handle h, int count, double* g, bool form_alpha = false) {
  const int np = (int)h->np;
  const int64_t ld = h->np, cs = h->cell_stride, gs = 2 * (int64_t)h->np * h->np;
  int rc;
  if ((rc = ensure(h, h->garena, sizeof(double) * (size_t)gs * count))) return rc;
  const int tiles = np / KM_T;
  const int width = 2 + h->d;
  const int64_t ps = (int64_t)tiles * tiles * width;  // partials per cell; the count x width sums follow all partials
  if ((rc = ensure(h, h->gpartial, sizeof(double) * (size_t)(ps + width) * count))) return rc;
  hipStream_t st = h->stream;
  double* X0 = h->garena.p;
  double* T0 = h->garena.p + (int64_t)np * ld;
  double* K0 = h->arena.p;
  // (X needs no zeroing: scatter_inv_diag writes the diagonal blocks whole -- zeros above the diagonal included --, every tile
  // below them is written with beta = 0 before it is read.  The triangular K ranges of the products stay on or below the diagonal
  // blocks at 64 x 64 tiles; a 128 x 128 tile also reads the block to the right of an even diagonal block, and scatter_inv_diag
  // writes that one as zeros.  The 128 memsets of 134 MB were 1.5 % of a batched evaluation.  "poison_workspace" = 1 fills X
  // with NaN patterns instead, for the test that proves it.)
  if (h->tune.poison_workspace)
    for (int c = 0; c < count; ++c) HIPCHK(h, hipMemsetAsync(X0 + (int64_t)c * gs, 0xff, sizeof(double) * h->np * ld, st));
  // 64 x 64 tiles throughout: with many cells per launch they beat the 128 x 128 tiles on these triangular products
  // (measured at 32 cells of N = 4096: 52.8 ms against 60.7 ms per batched objective + gradient)
  const int tile = h->tune.update_tile ? h->tune.update_tile : 64;
  HIPCHK(h, trtri_lower(st, K0, ld, K0 + h->off_invd, X0, ld, T0, ld, np, count, cs, gs, tile));
  if (form_alpha) {  // the factorisation left the backward substitution out: alpha = X^T beta (T is free until the next product)
    if ((rc = ensure(h, h->apart, sizeof(double) * (size_t)count * ((np + ALPHA_CHUNK - 1) / ALPHA_CHUNK) * np))) return rc;
    HIPCHK(h, alpha_from_inverse(st, X0, ld, K0 + (int64_t)np * ld, h->apart.p, K0 + h->off_alpha, np, count, gs, cs, cs));
  }
  // K^-1 = L^-T L^-1 on the lower tiles, as an NT product of Xt = L^-T with itself (transposed in place; same sums in the same
  // k order as the TN form it replaces, so the values are unchanged)
  if (kinv_tn()) {
    HIPCHK(h, launch_gemm(st, 1, 0, np, np, np, 1.0, X0, ld, X0, ld, 0.0, T0, ld, GEMM_C_LOWER | GEMM_A_UPPER | GEMM_B_LOWER, 64, count, gs, gs, gs));
  } else {
    HIPCHK(h, transpose_inplace(st, X0, ld, np, count, gs));
    HIPCHK(h, launch_gemm(st, 0, 1, np, np, np, 1.0, X0, ld, X0, ld, 0.0, T0, ld, GEMM_C_LOWER | GEMM_A_UPPER | GEMM_B_LOWER, tile, count, gs, gs,
                          gs));
  }
  TraceArgs ta{h->X.p, h->X.p, nullptr, T0, ld, K0 + h->off_alpha, K0 + h->off_alpha, -1.0, 1.0, (int)h->n, (int)h->n, h->d, 0.0, 1, h->gpartial.p,
               nullptr, 0, tiles};
  ta.cell_par = h->cellpar.p;
  ta.iso = h->ard ? 0 : 1;
  ta.w_stride = gs;
  ta.uv_stride = cs;
  ta.partial_stride = ps;
  HIPCHK(h, launch_trace(st, h->kid, with_form(ta, h), tiles * tiles, count));
  double* sums0 = h->gpartial.p + ps * count;
  hipLaunchKernelGGL(trace_final, dim3(width, count), dim3(64), 0, st, (const double*)h->gpartial.p, tiles * tiles, width, sums0, ps);
  std::vector<double> host((size_t)width * count);
  HIPCHK(h, hipMemcpyAsync(host.data(), sums0, sizeof(double) * width * count, hipMemcpyDeviceToHost, st));
  HIPCHK(h, wait_stream(h, st));
  for (int c = 0; c < count; ++c) {
    if (!h->slot_ok[c]) continue;
    const double* hs = host.data() + (size_t)c * width;
    double* gc = g + (size_t)c * h->ntheta;
    gc[0] = 0.5 * hs[0];
    if (h->ard) {
      for (int k = 0; k < h->d; ++k) gc[1 + k] = 0.5 * hs[2 + k];
    } else {
      double sum = 0.0;
      for (int k = 0; k < h->d; ++k) sum += hs[2 + k];
      gc[1] = 0.5 * sum;
    }
    gc[1 + h->nlen] = 0.5 * hs[1];
  }
  return GPRX_OK;
}

// gradient of the LML w.r.t. constrained (variance, lengthscales[nlen], noise) -> g[0 .. nlen+1]
// Enqueue the gradient's launches behind the factorisation on the handle's stream; `host` (2 + d doubles, alive until the
// stream has been synchronised) receives the trace sums.  form_alpha: the factorisation left the backward substitution out.
int exact_gradient_enqueue(gprx_handle h, const Theta& t, double* host, bool form_alpha) {
  const int np = (int)h->np;
  const int64_t ld = h->np;
  int rc;
  if ((rc = ensure(h, h->Xinv, sizeof(double) * h->np * ld))) return rc;
  if ((rc = ensure(h, h->Tmp, sizeof(double) * h->np * ld))) return rc;
  hipStream_t st = h->stream;
  if (h->tune.poison_workspace) HIPCHK(h, hipMemsetAsync(h->Xinv.p, 0xff, sizeof(double) * h->np * ld, st));  // (see exact_gradient_batch)
  HIPCHK(h, trtri_lower(st, h->Kmat.p, ld, h->invD.p, h->Xinv.p, ld, h->Tmp.p, ld, np));
  if (form_alpha) {
    if ((rc = ensure(h, h->apart, sizeof(double) * (size_t)((np + ALPHA_CHUNK - 1) / ALPHA_CHUNK) * np))) return rc;
    HIPCHK(h, alpha_from_inverse(st, h->Xinv.p, ld, h->Kmat.p + (int64_t)np * ld, h->apart.p, h->alpha.p, np));
  }
  // K^-1 = X^T X on the lower tiles, into Tmp
  h->have_linv = false;  // (Xinv is not zeroed above its diagonal, or holds L^-T: a later predict forms L^-1 again)
  if (kinv_tn()) {
    HIPCHK(h, launch_gemm(st, 1, 0, np, np, np, 1.0, h->Xinv.p, ld, h->Xinv.p, ld, 0.0, h->Tmp.p, ld, GEMM_C_LOWER | GEMM_A_UPPER | GEMM_B_LOWER, 64));
  } else {
    HIPCHK(h, transpose_inplace(st, h->Xinv.p, ld, np));
    HIPCHK(h, launch_gemm(st, 0, 1, np, np, np, 1.0, h->Xinv.p, ld, h->Xinv.p, ld, 0.0, h->Tmp.p, ld,
                          GEMM_C_LOWER | GEMM_A_UPPER | GEMM_B_LOWER, h->tune.update_tile));
  }
  const int tiles = np / KM_T;
  const int width = 2 + h->d;
  if ((rc = ensure(h, h->partial, sizeof(double) * ((size_t)tiles * tiles * width + width)))) return rc;
  TraceArgs ta{h->X.p, h->X.p, h->invls.p, h->Tmp.p, ld, h->alpha.p, h->alpha.p, -1.0, 1.0, (int)h->n, (int)h->n, h->d, t.variance, 1, h->partial.p, nullptr, 0, tiles};
  ta.iso = h->ard ? 0 : 1;
  HIPCHK(h, launch_trace(st, h->kid, with_form(ta, h), tiles * tiles));
  double* sums = h->partial.p + (size_t)tiles * tiles * width;
  hipLaunchKernelGGL(trace_final, dim3(width), dim3(64), 0, st, h->partial.p, tiles * tiles, width, sums);
  HIPCHK(h, hipMemcpyAsync(host, sums, sizeof(double) * width, hipMemcpyDeviceToHost, st));
  return GPRX_OK;
}
// gradient of the LML w.r.t. constrained (variance, lengthscales[nlen], noise) -> g[0 .. nlen+1], from the synchronised trace sums
void exact_gradient_collect(gprx_handle h, const double* host, double* g) {
  g[0] = 0.5 * host[0];
  if (h->ard) {
    for (int k = 0; k < h->d; ++k) g[1 + k] = 0.5 * host[2 + k];
  } else {
    double s = 0.0;
    for (int k = 0; k < h->d; ++k) s += host[2 + k];
    g[1] = 0.5 * s;
  }
  g[1 + h->nlen] = 0.5 * host[1];
}
int exact_gradient(gprx_handle h, const Theta& t, double* g) {
  std::vector<double> host(2 + h->d);
  int rc;
  if ((rc = exact_gradient_enqueue(h, t, host.data(), false))) return rc;
  HIPCHK(h, wait_stream(h, h->stream));
  exact_gradient_collect(h, host.data(), g);
  return GPRX_OK;
}

// ---- sparse GP (SGPR) -----------------------------------------------------------------------------
// Device restatement of gpflow SGPR._common_calculation / elbo / predict_f (oracle/sgpr.py) with
//   P = Kuf (mp x np), Q = Kuu + jitter I -> L, A' = L^-1 P (unscaled: A = A' / sqrt(s)),
//   B = I + A' A'^T / s -> LB, c = LB^-1 A' y / s (carried through the Cholesky as an appended row).
// The SM block of a cell holds ten mp x mp scratch matrices.
constexpr int SPLITK_CHUNK = 256;
constexpr int SGPR_PRED_TILE = 4096;  // test points per pass of the sparse predict
enum { SM_BFULL = 0, SM_LINV, SM_LBINV, SM_QINV, SM_SINV, SM_R, SM_T1, SM_T2, SM_W, SM_GQ, SM_COUNT };

// ---- batched sparse models ------------------------------------------------------------------------------------
// The reference fits its per-mode SGPR models one after the other (gpr.py:272-274); every evaluation is ~45 tiny
// dependent launches (M = 50 inducing points: every M x M matrix is one 64 x 64 tile), i.e. pure launch latency.
// Here `count` cells (unit, theta, Z) on the handle's x go through ONE launch sequence, the cell index in a grid
// dimension of every kernel: each cell owns one block of `ss` doubles holding all its matrices at fixed offsets, so
// a kernel adds blockIdx * ss to its per-cell pointers; hyperparameters (and 1 / s for the GEMM scalings) come from the
// cell-parameter table.  A lone model (gprx_objective / gprx_factorize / gprx_predict) is a batch of one cell: a cell's
// values do not depend on its position in a batch or on the batch's size, bit for bit.
// M <= 64 takes the five launches of sgpr_fused.h unless "sgpr_fused" = 0; its kernels read the lengthscales from the parameter table only
bool sgpr_five_launches(gprx_handle h) { return h->mp == NB && h->sgpr_fused != 0 && h->d <= CELL_PAR - CELL_PAR_LS; }

// Where the kernels of the launch sequence and of the predict read a cell's hyperparameters.  Table: row `cell` of the cell-parameter
// table -- the values travel through device memory, so the sequence can be captured and replayed.  Direct (d > 64: a row has 64
// lengthscale slots): the handle's lengthscale vector and the scalars themselves in the launch arguments; the kernels then apply no
// per-cell stride, so it serves ONE cell and is never captured.
struct SgprParSrc {
  const double* table = nullptr;  // nullptr: direct
  const double* ls = nullptr;
  double variance = 0.0, noise = 0.0, inv_noise = 0.0;
  void stamp(KmatArgs& a) const {
    a.cell_par = table;
    a.ls = ls;
    a.variance = variance;
  }
  void stamp(TraceArgs& a, bool noise_scaled) const {
    a.cell_par = table;
    a.ls = ls;
    a.variance = variance;
    a.scale_inv_noise = noise_scaled ? 1 : 0;
    if (noise_scaled) a.w_scale = a.uv_scale = inv_noise;
  }
};
SgprParSrc sgpr_par_src(gprx_handle h, double variance, double noise) {  // (direct: the one cell's values; upload_inv_ls has filled invls)
  SgprParSrc ps;
  if (h->d <= CELL_PAR - CELL_PAR_LS) {
    ps.table = h->cellpar.p;
  } else {
    ps.ls = h->invls.p;
    ps.variance = variance;
    ps.noise = noise;
    ps.inv_noise = 1.0 / noise;
  }
  return ps;
}

struct SgprLayout {
  int64_t oZ, oY, oP, oAm, oQm, oBm, oInvDL, oInvDB, oSM, oWP, oWHP, oWHQ, oVecs, odZ, oStage, oPart, oWs, oRed, oKs, oPred, ss;
  int64_t oFU, oFP2;  // fused evaluation (sgpr_fused.h): u partials of the chunks, pass-2 partial blocks
  int64_t part_p, part_q;
  int width, nsplit, p2w;
};

SgprLayout sgpr_batch_layout(gprx_handle h) {
  const int64_t mp = h->mp, np = h->np, m = h->m, d = h->d;
  SgprLayout L{};
  L.width = 2 + (int)d;
  L.nsplit = (int)((np + SPLITK_CHUNK - 1) / SPLITK_CHUNK);
  L.part_p = (mp / KM_T) * (np / KM_T) * L.width;
  L.part_q = (mp / KM_T) * (mp / KM_T) * L.width;
  int64_t o = 0;
  auto take = [&](int64_t doubles) {
    const int64_t at = o;
    o += round_up(doubles, 64);
    return at;
  };
  // (the five-launch evaluation of sgpr_fused.h never stores Kuf, A', W Kuf or the weighted derivative: the four M x N matrices and the
  // trace partials of the launch sequence shrink to nothing -- 8.4 of 9.9 MB per cell at M = 50, N = 4096, which a fit allocated and cleared)
  const bool fused = sgpr_five_launches(h);
  const int64_t big = fused ? 0 : mp * np;
  L.oZ = take(m * d);
  L.oY = take(np);
  L.oP = take(big);
  L.oAm = take(big);
  L.oQm = take(mp * mp);
  L.oBm = take((mp + NB) * mp);
  L.oInvDL = take(mp * NB);
  L.oInvDB = take(mp * NB);
  L.oSM = take((int64_t)SM_COUNT * mp * mp);
  L.oWP = take(big);
  L.oWHP = take(big);
  L.oWHQ = take(mp * mp);
  L.oVecs = take(4 * mp + np);
  L.odZ = take(m * d);
  L.oStage = take(mp * STAGE_LD);
  L.oPart = take(fused ? 0 : L.part_p + L.part_q + 2 * L.width);
  L.oWs = take((int64_t)L.nsplit * mp * mp);
  L.oRed = take(8);
  L.oKs = take(mp * SGPR_PRED_TILE);                                           // batched predict: Kus tile of this cell
  L.oPred = take(((mp + 255) / 256) * (int64_t)SGPR_PRED_TILE);                // its column-reduction partials
  L.p2w = (int)round_up(SF_P2_HEAD + NB * d, 2);
  L.oFU = take((int64_t)L.nsplit * NB);
  L.oFP2 = take((int64_t)(L.nsplit + 1) * L.p2w);
  L.ss = o;
  return L;
}

int ensure_sarena(gprx_handle h, int slots, const SgprLayout& L) {
  if (h->sarena_slots >= slots) return GPRX_OK;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  drop_graphs(h);  // captured evaluations hold the addresses of the buffers released below
  h->factorized = false;  // a lone model's factorisation lived in cell block 0 of the arena released below
  if (h->sarena.p) HIPCHK(h, hipFree(h->sarena.p));
  h->sarena.p = nullptr;
  h->sarena.bytes = 0;
  h->sarena_slots = 0;
  int rc;
  if ((rc = ensure(h, h->sarena, sizeof(double) * (size_t)L.ss * slots))) return rc;
  HIPCHK(h, hipMemsetAsync(h->sarena.p, 0, sizeof(double) * (size_t)L.ss * slots, h->stream));  // padding of every matrix stays zero
  if ((rc = ensure(h, h->cellpar, sizeof(double) * CELL_PAR * slots))) return rc;
  if ((rc = ensure(h, h->cellres, sizeof(double) * CELL_RES * slots))) return rc;
  const size_t need = (size_t)slots * (CELL_PAR + CELL_RES + 8 + 2 * L.width + 2 * h->m * h->d);
  if (h->spin_doubles < need) {
    if (h->spin) HIPCHK(h, hipHostFree(h->spin));
    h->spin = nullptr;
    HIPCHK(h, hipHostMalloc((void**)&h->spin, sizeof(double) * need, hipHostMallocDefault));
    h->spin_doubles = need;
  }
  h->sarena_slots = slots;
  return GPRX_OK;
}

// Pinned staging block of the sparse batch (h->spin), offsets in doubles for `count` cells.
struct SgprStage {
  size_t par, res, red, sum, dz, z;
};
SgprStage sgpr_stage(gprx_handle h, int count, const SgprLayout& L) {
  SgprStage s{};
  s.par = 0;
  s.res = s.par + (size_t)count * CELL_PAR;
  s.red = s.res + (size_t)count * CELL_RES;
  s.sum = s.red + (size_t)count * 8;
  s.dz = s.sum + (size_t)count * 2 * L.width;
  s.z = s.dz + (size_t)count * h->m * h->d;
  return s;
}

// M <= 64: the five launches of sgpr_fused.h (prep, pass 1, mid, pass 2, final) instead of the 21 below; same staging block, same host
// tail.  "sgpr_fused" = 0 (gprx_set_tuning) keeps the launch sequence -- which larger M and d > 64 always take.
int& sgpr_fused_tuning() {
  static int v = 1;
  return v;
}
// 1: the optimiser loops of sparse models (d <= 64) stay on the device; 0: the host-stepped loop for all of them (one process can compare)
int& sgpr_resident_tuning() {
  static int v = 1;
  return v;
}
static_assert(SF_CHUNK == SPLITK_CHUNK, "the fused evaluation stores its slabs in the split-K workspace of the cell block");

SfParams sgpr_fused_params(gprx_handle h, const SgprLayout& L, bool want_grad) {
  const int64_t mm = (int64_t)h->mp * h->mp;
  SfParams p{};
  p.X = h->X.p;
  p.Y = h->Y.p;
  p.arena = h->sarena.p;
  p.ss = L.ss;
  p.cpar = h->cellpar.p;
  p.n = (int)h->n;
  p.np = (int)h->np;
  p.m = (int)h->m;
  p.d = h->d;
  p.nchunks = L.nsplit;
  p.oZ = L.oZ;
  p.oL = L.oQm;
  p.oLinv = L.oInvDL;
  p.oLB = L.oBm;
  p.oLBinv = L.oInvDB;
  p.oW = L.oSM + SM_W * mm;
  p.oGQ = L.oSM + SM_GQ * mm;
  p.oM = L.oVecs;
  p.oSlab = L.oWs;
  p.oU = L.oFU;
  p.oP2 = L.oFP2;
  p.oRed = L.oRed;
  p.p2w = L.p2w;
  p.cellres = h->cellres.p;
  p.cellres_stride = CELL_RES;
  p.want_grad = want_grad ? 1 : 0;
  p.store_factors = 1;
  p.stamps = h->sf_stamps;
  return p;
}

// The resident Adam loop on large batches: TWO groups of cells on two streams.  Two of the four launches of a step (mid, Adam + prep) are
// one workgroup per cell around a 64 x 64 chain: with all cells in lock step the chip idles through them (16 of 256 CUs busy for half of a
// 16-cell step), and a pass over more than 16 cells takes a second round of 256 workgroups.  Two groups that start one launch apart keep
// that distance: one group's single-workgroup launches run beside the other's streamed passes.  Measured per lock-step step (N = 4096,
// d = 10, M = 50): 17 cells 183 -> 128 us, 28 cells 187 -> 131, 36 cells 244 -> 205, 50 cells 303 -> 223; 32 cells 188 -> 187 (a pass workgroup fills its CU --
// 512 threads x 256 registers -- and a group of 16 cells occupies all 256: the other group's single workgroups find no CU until the
// round ends); three and more groups LOSE (24 cells as three groups 252 us, 32 as three 258, 50 as five 307: streams beyond the second
// do not run beside the first two on this runtime).  Every cell's arithmetic is untouched: same bits (tools/sgpr_groups_probe.py).
// From `sf_groups_from()` cells on at 16 chunks per cell ("sgpr_groups_from", 0: never; sf_group_count).  Host-driven evaluations stay one group: the cross-stream edges cost a
// single call more than the overlap returns (16 cells 154 -> 210 us per call, 50 cells 360 -> 343).
int& sf_groups_from() {
  static int v = [] {
    const char* e = getenv("GPRX_SF_GROUPS_FROM");
    return e ? atoi(e) : 17;
  }();
  return v;
}
// (the threshold is stated in cells at N = 4096, i.e. 16 chunks of 256 columns per cell; what counts is whether a pass -- cells x chunks
// workgroups -- needs more than one round of the 256 CUs: N = 8192 splits from 9 cells on, N = 2048 from 33)
int sf_group_count(int count, int nchunks) {
  if (sf_groups_from() <= 0 || count < 2) return 1;
  return (int64_t)count * nchunks > (int64_t)(sf_groups_from() - 1) * 16 ? 2 : 1;
}
int sf_group_streams(gprx_handle h, int ngroups) {
  for (int g = 0; g + 1 < ngroups; ++g)
    if (!h->sf_streams[g]) HIPCHK(h, hipStreamCreateWithFlags(&h->sf_streams[g], hipStreamNonBlocking));
  for (int g = 0; g < ngroups; ++g)
    if (!h->sf_evs[g]) HIPCHK(h, hipEventCreateWithFlags(&h->sf_evs[g], hipEventDisableTiming));
  return GPRX_OK;
}
// the parameter block of the cells [cell0, ...) of a batch: every per-cell base pointer moved (the kernels index cells from 0)
SfParams sf_params_from(SfParams p, int cell0) {
  p.arena += (int64_t)cell0 * p.ss;
  p.cpar += (int64_t)cell0 * CELL_PAR;
  p.cellres += (int64_t)cell0 * p.cellres_stride;
  if (p.active) p.active += cell0;
  if (cell0 != 0) p.stamps = nullptr;
  return p;
}

int sgpr_fused_enqueue(gprx_handle h, int count, const SgprLayout& L, bool want_grad) {
  hipStream_t st = h->stream;
  const SgprStage sg = sgpr_stage(h, count, L);
  const SfParams p = sgpr_fused_params(h, L, want_grad);
  const int iso = (h->ard || h->dist_form) ? 0 : 1;
  HIPCHK(h, sf_launch_prep(st, h->kid, h->dist_form, p, count, h->spin + sg.par, h->spin + sg.z, h->cellpar.p));
  HIPCHK(h, sf_launch_pass1(st, h->kid, h->dist_form, p, count));
  HIPCHK(h, sf_launch_mid(st, p, count));
  if (want_grad) HIPCHK(h, sf_launch_pass2(st, h->kid, h->dist_form, iso, p, count));
  HIPCHK(h, sf_launch_final(st, iso, p, count, h->spin + sg.res, h->spin + sg.red, h->spin + sg.sum, h->spin + sg.dz));
  return GPRX_OK;
}

// Device part of one batched evaluation: everything between the staged inputs (parameter table and Z in pinned memory) and
// the staged outputs (pivot status, reductions, trace sums, dZ in pinned memory).  Nothing here depends on the VALUES of the
// parameters -- they travel through the cell-parameter table -- so the sequence is captured once per (cells, gradient) into a
// hipGraph and replayed (sgpr_objective_batch): ~45 launches whose enqueue cost, not their device time, bounded a step.
// The sequence in three parts -- stage-in, body, stage-out -- so that the resident optimiser loop (sgpr_resident_general) can run the body
// alone between two launches of its step kernel; a host-driven evaluation (sgpr_batch_enqueue) is the three in a row.
int sgpr_stage_in_enqueue(gprx_handle h, int count, const SgprLayout& L) {
  const int np = (int)h->np, m = (int)h->m, d = h->d;
  const SgprStage sg = sgpr_stage(h, count, L);
  double* A0 = h->sarena.p;
  static_assert(CELL_RES <= 256 && CELL_PAR <= 256, "sgpr_stage_in_kernel moves them with its first workgroup");
  hipLaunchKernelGGL(sgpr_stage_in_kernel, dim3((std::max(np, m * d) + 255) / 256, count), dim3(256), 0, h->stream, (const double*)h->Y.p, np,
                     (const double*)(h->spin + sg.par), CELL_PAR, h->cellpar.p, (const double*)(h->spin + sg.z), m * d, A0 + L.oZ, A0 + L.oY, L.ss,
                     h->cellres.p, CELL_RES);
  return GPRX_OK;
}

int sgpr_body_enqueue(gprx_handle h, int count, const SgprLayout& L, bool want_grad, const SgprParSrc& ps) {
  const int mp = (int)h->mp, np = (int)h->np, m = (int)h->m, n = (int)h->n, d = h->d;
  const int64_t ss = L.ss, mm = (int64_t)mp * mp;
  const size_t pitch = sizeof(double) * (size_t)ss;
  hipStream_t st = h->stream;
  double* A0 = h->sarena.p;
  // (Tried: the independent branches of the evaluation -- Kuf beside Kuu's factorisation; R, Sinv / T2, T1 / Qinv, m; the
  // two contractions and the noise terms -- on side streams, i.e. parallel branches of the captured graph.  The dependent chain
  // drops from 34 to 20 launches, but every cross-branch edge costs more than an in-order kernel boundary on this runtime:
  // 16 cells 0.427 ms against 0.400 ms serial.  One stream it is.)
  const double* inv_s = h->cellpar.p + 3;  // alpha table: 1 / s, CELL_PAR apart
  // ---- factorisation ----
  KmatArgs kp{A0 + L.oZ, h->X.p, nullptr, A0 + L.oP, np, m, n, d, mp, np, 0.0, 0.0, 0, 0.0, nullptr, 0};
  ps.stamp(kp);
  kp.out_stride = ss;
  kp.a_stride = ss;
  kp.diag_const = 1;
  KmatArgs kq{A0 + L.oZ, A0 + L.oZ, nullptr, A0 + L.oQm, mp, m, m, d, mp, mp, 0.0, JITTER, 2, 1.0, nullptr, 0};
  ps.stamp(kq);
  kq.out_stride = ss;
  kq.a_stride = ss;
  kq.b_stride = ss;
  kq.diag_const = 1;
  HIPCHK(h, launch_kmat_pair(st, h->kid, with_form(kp, h), with_form(kq, h), count));  // Kuf and Kuu in one launch
  int* info0 = reinterpret_cast<int*>(h->cellres.p + 2);
  HIPCHK(h, potrf_lower(st, A0 + L.oQm, mp, mp, 0, A0 + L.oInvDL, info0, A0 + L.oStage, nullptr, nullptr, count, ss, 2 * CELL_RES, &h->tune));
  const bool one_block = mp == NB;  // M <= 64 (the reference's default is 50): every M x M matrix is one 64 x 64 tile
  if (one_block) {
    HIPCHK(h, trsm_lower_left(st, A0 + L.oQm, mp, A0 + L.oInvDL, A0 + L.oAm, np, mp, np, count, ss, A0 + L.oP));  // A = L^-1 P straight from P
  } else {
    HIPCHK(h, hipMemcpy2DAsync(A0 + L.oAm, pitch, A0 + L.oP, pitch, sizeof(double) * (size_t)mp * np, count, hipMemcpyDeviceToDevice, st));
    HIPCHK(h, trsm_lower_left(st, A0 + L.oQm, mp, A0 + L.oInvDL, A0 + L.oAm, np, mp, np, count, ss));
  }
  if (mp <= 512 && np >= 4 * SPLITK_CHUNK) {
    HIPCHK(h, launch_gemm_splitk(st, 0, 1, mp, mp, np, 0.0, A0 + L.oAm, np, A0 + L.oAm, np, 0.0, A0 + L.oBm, mp, A0 + L.oWs, SPLITK_CHUNK, count, ss, ss,
                                 ss, ss, inv_s, CELL_PAR));
  } else {
    HIPCHK(h, launch_gemm(st, 0, 1, mp, mp, np, 0.0, A0 + L.oAm, np, A0 + L.oAm, np, 0.0, A0 + L.oBm, mp, 0, 0, 1, 0, 0, 0, count, ss, ss, ss, inv_s,
                          CELL_PAR));
  }
  double* SM0 = A0 + L.oSM;
  auto smb = [&](int slot) { return SM0 + (size_t)slot * mm; };
  double* crow = A0 + L.oBm + mm;
  if (mp <= 128) {
    hipLaunchKernelGGL(sgpr_b_finish_kernel, dim3(count), dim3(256), 0, st, A0 + L.oBm, mp, A0 + L.oRed + 2, smb(SM_BFULL), ss);
  } else {
    hipLaunchKernelGGL(add_diag_kernel, dim3((mp + 255) / 256, count), dim3(256), 0, st, A0 + L.oBm, (int64_t)mp, mp, 1.0, ss);
    hipLaunchKernelGGL(diag_sum_kernel, dim3(1, count), dim3(256), 0, st, (const double*)(A0 + L.oBm), (int64_t)mp, mp, 1.0, A0 + L.oRed + 2, ss);
    HIPCHK(h, hipMemcpy2DAsync(smb(SM_BFULL), pitch, A0 + L.oBm, pitch, sizeof(double) * (size_t)mm, count, hipMemcpyDeviceToDevice, st));
    HIPCHK(h, hipMemset2DAsync(crow, pitch, 0, sizeof(double) * (size_t)NB * mp, count, st));
  }
  if (np >= 4 * SPLITK_CHUNK) {
    HIPCHK(h, launch_gemm_splitk(st, 0, 0, mp, 1, np, 0.0, A0 + L.oAm, np, A0 + L.oY, 1, 0.0, crow, 1, A0 + L.oWs, SPLITK_CHUNK, count, ss, ss, ss, ss,
                                 inv_s, CELL_PAR));
  } else {
    HIPCHK(h, launch_gemm(st, 0, 0, mp, 1, np, 0.0, A0 + L.oAm, np, A0 + L.oY, 1, 0.0, crow, 1, 0, 64, 1, 0, 0, 0, count, ss, ss, ss, inv_s, CELL_PAR));
  }
  HIPCHK(h, potrf_lower(st, A0 + L.oBm, mp, mp, NB, A0 + L.oInvDB, info0, A0 + L.oStage, nullptr, nullptr, count, ss, 2 * CELL_RES, &h->tune));
  const bool fused_small = one_block && want_grad;  // sgpr_small_kernel: the M x M algebra of the gradient, and these two reductions with it
  if (!fused_small)
    hipLaunchKernelGGL(logdet_quad_kernel, dim3(count), dim3(256), 0, st, (const double*)(A0 + L.oBm), (int64_t)mp, (const double*)crow, mp,
                       A0 + L.oRed, ss, (int)ss);
  // ---- gradient ----
  // one block: L^-1 and LB^-1 ARE the inverses of the diagonal blocks that the factorisations left behind (trtri_lower would
  // clear a matrix and copy them into it)
  double *Linv = one_block ? A0 + L.oInvDL : smb(SM_LINV), *LBinv = one_block ? A0 + L.oInvDB : smb(SM_LBINV), *Qinv = smb(SM_QINV), *Sinv = smb(SM_SINV), *R = smb(SM_R), *T1 = smb(SM_T1),
         *T2 = smb(SM_T2), *W = smb(SM_W), *GQ = smb(SM_GQ), *Bfull = smb(SM_BFULL);
  double* mvec = A0 + L.oVecs;
  double* qvec = A0 + L.oVecs + 4 * mp;
  double* partP = A0 + L.oPart;
  double* partQ = partP + L.part_p;
  double* sums = partQ + L.part_q;
  const int tiles_m = mp / KM_T, tiles_n = np / KM_T;
  if (want_grad) {
    auto gemm_mm = [&](hipStream_t sx, int ta, int tb, const double* A, const double* B, double* C, int flags) {
      return launch_gemm(sx, ta, tb, mp, mp, mp, 1.0, A, mp, B, mp, 0.0, C, mp, flags, 0, 1, 0, 0, 0, count, ss, ss, ss);
    };
    if (fused_small) {
      hipLaunchKernelGGL(sgpr_small_kernel, dim3(count), dim3(256), 0, st, (const double*)(A0 + L.oBm), (const double*)crow,
                         (const double*)(A0 + L.oInvDL), (const double*)(A0 + L.oInvDB), (const double*)Bfull, A0 + L.oRed, mvec, W, GQ, ss);
    } else {
      if (!one_block) {
        HIPCHK(h, hipMemset2DAsync(Linv, pitch, 0, sizeof(double) * (size_t)mm, count, st));
        HIPCHK(h, trtri_lower(st, A0 + L.oQm, mp, A0 + L.oInvDL, Linv, mp, T1, mp, mp, count, ss, ss));
        HIPCHK(h, hipMemset2DAsync(LBinv, pitch, 0, sizeof(double) * (size_t)mm, count, st));
        HIPCHK(h, trtri_lower(st, A0 + L.oBm, mp, A0 + L.oInvDB, LBinv, mp, T1, mp, mp, count, ss, ss));
      }
      HIPCHK(h, gemm_mm(st, 0, 0, LBinv, Linv, R, GEMM_A_LOWER | GEMM_B_LOWER));
      HIPCHK(h, gemm_mm(st, 1, 0, R, R, Sinv, GEMM_A_UPPER | GEMM_B_LOWER));
      HIPCHK(h, gemm_mm(st, 0, 0, Bfull, Linv, T2, GEMM_B_LOWER));
      HIPCHK(h, gemm_mm(st, 1, 0, Linv, T2, T1, GEMM_A_UPPER));
      // m = L^-T LB^-T c
      HIPCHK(h, gemm_mm(st, 1, 0, Linv, Linv, Qinv, GEMM_A_UPPER | GEMM_B_LOWER));
      hipLaunchKernelGGL(copy_row_batch_kernel, dim3((mp + 255) / 256, count), dim3(256), 0, st, (const double*)crow, mvec, mp, ss);
      HIPCHK(h, trsv_lower(st, A0 + L.oBm, mp, A0 + L.oInvDB, mvec, mp, true, count, ss));
      HIPCHK(h, trsv_lower(st, A0 + L.oQm, mp, A0 + L.oInvDL, mvec, mp, true, count, ss));
      hipLaunchKernelGGL(sgpr_combine_kernel, dim3((mp * mp + 255) / 256, count), dim3(256), 0, st, (const double*)Qinv, (const double*)Sinv,
                         (const double*)T1, (const double*)mvec, mp, W, GQ, ss);
    }
    HIPCHK(h, launch_gemm(st, 0, 0, mp, np, mp, 1.0, W, mp, A0 + L.oP, np, 0.0, A0 + L.oWP, np, 0, 0, 1, 0, 0, 0, count, ss, ss, ss));
    TraceArgs tp{A0 + L.oZ, h->X.p, nullptr, A0 + L.oWP, np, mvec, A0 + L.oY, 0.0, 0.0, m, n, d, 0.0, 0, partP, A0 + L.oWHP, np, tiles_n};
    ps.stamp(tp, true);
    tp.w_stride = ss;
    tp.uv_stride = ss;
    tp.partial_stride = ss;
    tp.a_stride = ss;
    tp.wh_stride = ss;
    tp.iso = h->ard ? 0 : 1;
    TraceArgs tq{A0 + L.oZ, A0 + L.oZ, nullptr, GQ, mp, nullptr, nullptr, 1.0, 0.0, m, m, d, 0.0, 0, partQ, A0 + L.oWHQ, mp, tiles_m};
    ps.stamp(tq, false);
    tq.w_stride = ss;
    tq.partial_stride = ss;
    tq.a_stride = ss;
    tq.b_stride = ss;
    tq.wh_stride = ss;
    tq.iso = h->ard ? 0 : 1;
    HIPCHK(h, launch_trace_pair(st, h->kid, with_form(tp, h), tiles_m * tiles_n, with_form(tq, h), tiles_m * tiles_m, count));
    HIPCHK(h, launch_gemm(st, 1, 0, np, 1, mp, 1.0, A0 + L.oP, np, mvec, 1, 0.0, qvec, 1, 0, 64, 1, 0, 0, 0, count, ss, ss, ss));
    hipLaunchKernelGGL(resid_sumsq_kernel, dim3(1, count), dim3(256), 0, st, (const double*)(A0 + L.oY), (const double*)qvec, n, A0 + L.oRed + 4, ss,
                       ss);
    if (fused_small) {
      // (|LB^-1|_F^2 came out of sgpr_small_kernel)
    } else {
      const int nb = mp < 64 ? mp : 64;
      double* part = A0 + L.oVecs + 2 * mp;
      hipLaunchKernelGGL(sumsq_partial_kernel, dim3(nb, count), dim3(256), 0, st, (const double*)LBinv, (int64_t)mp, mp, mp, part, ss);
      hipLaunchKernelGGL(sum_partials_kernel, dim3(1, count), dim3(64), 0, st, (const double*)part, nb, A0 + L.oRed + 3, ss);
    }
    hipLaunchKernelGGL(dz_kernel, dim3(dz_grid(m, d), count), dim3(256), 0, st, (const double*)(A0 + L.oZ), (const double*)h->X.p,
                       (const double*)(A0 + L.oWHP), (int64_t)np, (const double*)(A0 + L.oWHQ), (int64_t)mp, ps.ls, m, n, d,
                       A0 + L.odZ, ss, ps.table);
  }
  return GPRX_OK;
}

// ---- results: reductions, pivot status, trace sums, dZ -> pinned memory ----
int sgpr_stage_out_enqueue(gprx_handle h, int count, const SgprLayout& L, bool want_grad) {
  const int mp = (int)h->mp, np = (int)h->np, m = (int)h->m, d = h->d;
  const SgprStage sg = sgpr_stage(h, count, L);
  double* A0 = h->sarena.p;
  const double* partP = A0 + L.oPart;
  const double* partQ = partP + L.part_p;
  const int tiles_m = mp / KM_T, tiles_n = np / KM_T;
  hipLaunchKernelGGL(sgpr_stage_out_kernel, dim3(count), dim3(256), 0, h->stream, (const double*)h->cellres.p, CELL_RES, h->spin + sg.res,
                     (const double*)(A0 + L.oRed), h->spin + sg.red, want_grad ? partP : nullptr, tiles_m * tiles_n, partQ, tiles_m * tiles_m,
                     L.width, h->spin + sg.sum, want_grad ? (const double*)(A0 + L.odZ) : nullptr, m * d, h->spin + sg.dz, L.ss);
  return GPRX_OK;
}

int sgpr_batch_enqueue(gprx_handle h, int count, const SgprLayout& L, bool want_grad, const SgprParSrc& ps) {
  if (sgpr_five_launches(h)) return sgpr_fused_enqueue(h, count, L, want_grad);
  int rc;
  if ((rc = sgpr_stage_in_enqueue(h, count, L))) return rc;
  if ((rc = sgpr_body_enqueue(h, count, L, want_grad, ps))) return rc;
  if ((rc = sgpr_stage_out_enqueue(h, count, L, want_grad))) return rc;
  HIPCHK(h, hipGetLastError());
  return GPRX_OK;
}

// a cell's row of the parameter table (kfun.h CELL_PAR layout) as the stage-in reads it from pinned memory
void sgpr_par_row(gprx_handle h, double* row, int unit, const Theta& t) {
  std::memset(row, 0, sizeof(double) * CELL_PAR);
  row[0] = t.variance;
  row[1] = t.noise;
  row[2] = (double)unit;
  row[3] = 1.0 / t.noise;
  for (int k = 0; k < std::min(h->d, CELL_PAR - CELL_PAR_LS); ++k) row[CELL_PAR_LS + k] = t.ls[k];
}

// Eager, capture, replay: the first launch sequence of a shape (`key` in `graphs`) goes out eagerly -- every kernel's code object gets
// loaded outside a capture -- the second is captured into a hipGraph, and from then on the graph is replayed.  *replayed = false: the
// caller enqueues the sequence itself (the first time, GPRX_NO_GRAPH, profiling, or after a capture that failed).
template <class Enqueue>
int sgpr_replay(gprx_handle h, std::map<std::pair<int, int>, hipGraphExec_t>& graphs, const std::pair<int, int> key, Enqueue enqueue, bool* replayed) {
  static const bool no_graph = getenv("GPRX_NO_GRAPH") != nullptr;  // escape hatch: eager launches
  hipStream_t st = h->stream;
  *replayed = false;
  if (no_graph || h->sgraph_off || h->profiling) return GPRX_OK;
  auto it = graphs.find(key);
  if (it == graphs.end()) {
    graphs.emplace(key, nullptr);
    return GPRX_OK;
  }
  if (it->second == nullptr) {
    // Relaxed capture mode: another host thread may call a legacy-stream API (hipMemset / hipMemcpy of another handle's set-up)
    // while this capture runs; in the global and thread-local modes the runtime refuses that call ("operation would make the
    // legacy stream depend on a capturing blocking stream") AND invalidates this capture.  The handle's streams are
    // non-blocking, so no implicit dependency on the legacy stream exists that the capture could miss.  Captures are
    // serialised over the process as well; one that fails anyway is abandoned and the handle stays on eager launches.
    std::lock_guard<std::mutex> lock(capture_mutex());
    hipGraph_t graph = nullptr;
    hipGraphExec_t exec = nullptr;
    hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed);
    if (e == hipSuccess) {
      const int crc = enqueue();
      e = hipStreamEndCapture(st, &graph);
      if (!crc && e == hipSuccess && graph) e = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
      if (crc) e = hipErrorUnknown;
    }
    if (graph) hipGraphDestroy(graph);
    if (e != hipSuccess || !exec) {
      (void)hipGetLastError();
      h->err.clear();
      h->sgraph_off = true;
      graphs.erase(it);
      return GPRX_OK;
    }
    it->second = exec;
  }
  HIPCHK(h, hipGraphLaunch(it->second, st));
  *replayed = true;
  return GPRX_OK;
}

// elbo_out[c] (NaN if a Cholesky failed), g: count x ntheta constrained-parameter derivatives, gz: count x m x d (host);
// g / gz may be null (loss only).  status[c]: GPRX_OK / GPRX_ENOTPD.
int sgpr_objective_batch(gprx_handle h, int count, const int* units, const Theta* ts, const double* zs, double* elbo_out, double* g, double* gz,
                         int* status) {
  const SgprLayout L = sgpr_batch_layout(h);
  int rc;
  const bool direct = h->d > CELL_PAR - CELL_PAR_LS;  // (SgprParSrc)
  if (direct && count != 1) return fail(h, GPRX_EINVAL, "d > 64: sparse models are evaluated one cell at a time");
  if ((rc = ensure_sarena(h, count, L))) return rc;
  if (direct && (rc = upload_inv_ls(h, ts[0]))) return rc;
  const SgprParSrc ps = sgpr_par_src(h, ts[0].variance, ts[0].noise);
  const int mp = (int)h->mp, m = (int)h->m, d = h->d;
  const int width = L.width;
  hipStream_t st = h->stream;
  const SgprStage sg = sgpr_stage(h, count, L);
  double* par = h->spin + sg.par;
  for (int c = 0; c < count; ++c)
    sgpr_par_row(h, par + (size_t)c * CELL_PAR, units[c], ts[c]);
  std::memcpy(h->spin + sg.z, zs, sizeof(double) * (size_t)count * m * d);
  const bool want_grad = g != nullptr;
  bool replayed = false;
  // (the five launches of the fused evaluation go out eagerly: replaying them from a graph starts the first kernel later than a direct
  // launch does -- 178.8 against 172.5 us per 16-cell evaluation, MI355X_MICROARCH.md "graph-replay-floor")
  if (!sgpr_five_launches(h) && !direct &&
      (rc = sgpr_replay(h, h->sgraphs, {count, want_grad ? 1 : 0}, [&] { return sgpr_batch_enqueue(h, count, L, want_grad, ps); }, &replayed)))
    return rc;
  if (!replayed && (rc = sgpr_batch_enqueue(h, count, L, want_grad, ps))) return rc;
  const double* hres = h->spin + sg.res;
  const double* hred = h->spin + sg.red;
  const double* hsum = h->spin + sg.sum;
  const double* hdz = h->spin + sg.dz;
  HIPCHK(h, wait_stream(h, st));
  h->factorized = false;  // (objective_impl sets it for a lone model: cell block 0 is then what gprx_predict reads)
  int first_error = GPRX_OK;
  const double nn = (double)h->n;
  for (int c = 0; c < count; ++c) {
    int info = 0;
    std::memcpy(&info, hres + (size_t)c * CELL_RES + 2, sizeof(int));
    if (status) status[c] = info == 0 ? GPRX_OK : GPRX_ENOTPD;
    if (info != 0) {
      if (!first_error) {
        char msg[160];
        snprintf(msg, sizeof msg, "cell %d: Kuu or B not positive definite: pivot %d", c, info);
        first_error = fail(h, GPRX_ENOTPD, msg);
      }
      elbo_out[c] = std::numeric_limits<double>::quiet_NaN();
      continue;
    }
    const double* red = hred + (size_t)c * 8;
    const double s = ts[c].noise, v = ts[c].variance;
    elbo_out[c] = sgpr_asm_elbo(nn, h->yy[units[c]], v, s, red);  // (sgpr_asm.h: the resident Adam loop forms the same sums on the device)
    if (!g) continue;
    const double* hs = hsum + (size_t)c * 2 * width;
    double* gc = g + (size_t)c * h->ntheta;
    for (int k = 0; k < h->ntheta; ++k) gc[k] = sgpr_asm_dparam(k, h->nlen, h->ard, d, width, nn, mp, v, s, red, hs);
    if (gz) std::memcpy(gz + (size_t)c * m * d, hdz + (size_t)c * m * d, sizeof(double) * m * d);
  }
  return first_error;
}

// SGPR.predict_y for every cell of the batch that sgpr_objective_batch has just factorised (its cell blocks hold L, invDL, LB,
// invDB and c): the nine small launches of one model's predict serve all cells -- Kus per cell (own Z and hyperparameters),
// tmp1 = L^-1 Kus, tmp2 = LB^-1 tmp1, mean = tmp2^T c, var = v + colsum(tmp2^2) - colsum(tmp1^2) (+ s).  Same kernels and
// operation order whatever the count (gprx_predict_dev is count = 1): bit-identical values.  means / vars: (count, ns) device, row-major.
int sgpr_predict_batch(gprx_handle h, int count, const double* xs_dev, int64_t ns, double* means_dev, double* vars_dev, int include_noise) {
  const SgprLayout L = sgpr_batch_layout(h);
  const int mp = (int)h->mp, m = (int)h->m;
  const int64_t ss = L.ss;
  hipStream_t st = h->stream;
  double* A0 = h->sarena.p;
  const SgprParSrc ps = sgpr_par_src(h, h->variance, h->noise);
  const double* cpar = ps.table;
  const double base = ps.variance + (include_noise ? ps.noise : 0.0);  // (direct only: 0 beside a table)
  const int rows_per_chunk = 256;
  const int nchunks = (mp + rows_per_chunk - 1) / rows_per_chunk;
  const int tile = SGPR_PRED_TILE;
  const double* cvec = A0 + L.oBm + (int64_t)mp * mp;
  for (int64_t t0 = 0; t0 < ns; t0 += tile) {
    const int ts = (int)std::min<int64_t>(tile, ns - t0);
    const int tsp = (int)round_up(ts, NB);
    KmatArgs ka{A0 + L.oZ, xs_dev + t0 * h->d, nullptr, A0 + L.oKs, tile, m, ts, h->d, mp, tsp, 0.0, 0.0, 0, 0.0, nullptr, 0};
    ps.stamp(ka);
    ka.out_stride = ss;
    ka.a_stride = ss;
    ka.diag_const = 1;
    HIPCHK(h, launch_kmat(st, h->kid, with_form(ka, h), count));
    const dim3 pgrid((ts + 255) / 256, nchunks, count), fgrid((ts + 255) / 256, count);
    HIPCHK(h, trsm_lower_left(st, A0 + L.oQm, mp, A0 + L.oInvDL, A0 + L.oKs, tile, mp, tsp, count, ss));
    hipLaunchKernelGGL(colreduce_partial, pgrid, dim3(256), 0, st, (const double*)(A0 + L.oKs), (int64_t)tile, (const double*)nullptr, mp, ts,
                       rows_per_chunk, A0 + L.oPred, ss, (int64_t)0, ss);
    // var = (v [+ s]) - colsum(tmp1^2): per-cell base from the parameter table ([0] variance, [1] noise)
    hipLaunchKernelGGL(colreduce_final, fgrid, dim3(256), 0, st, (const double*)(A0 + L.oPred), nchunks, ts, base, -1.0, 0, vars_dev + t0, ss, ns, cpar,
                       include_noise && cpar ? cpar + 1 : (const double*)nullptr, CELL_PAR);
    HIPCHK(h, trsm_lower_left(st, A0 + L.oBm, mp, A0 + L.oInvDB, A0 + L.oKs, tile, mp, tsp, count, ss));
    hipLaunchKernelGGL(colreduce_partial, pgrid, dim3(256), 0, st, (const double*)(A0 + L.oKs), (int64_t)tile, cvec, mp, ts, rows_per_chunk,
                       A0 + L.oPred, ss, ss, ss);
    hipLaunchKernelGGL(colreduce_final, fgrid, dim3(256), 0, st, (const double*)(A0 + L.oPred), nchunks, ts, 0.0, 1.0, 0, means_dev + t0, ss, ns);
    hipLaunchKernelGGL(colreduce_partial, pgrid, dim3(256), 0, st, (const double*)(A0 + L.oKs), (int64_t)tile, (const double*)nullptr, mp, ts,
                       rows_per_chunk, A0 + L.oPred, ss, (int64_t)0, ss);
    hipLaunchKernelGGL(colreduce_final, fgrid, dim3(256), 0, st, (const double*)(A0 + L.oPred), nchunks, ts, 0.0, 1.0, 1, vars_dev + t0, ss, ns);
  }
  HIPCHK(h, hipGetLastError());
  return GPRX_OK;
}

// ---- what the two resident optimiser loops below share ------------------------------------------------------------------------------
// steps between two reads of the stop flags
int resident_check_every() {
  static const int every = [] {
    const char* e = getenv("GPRX_ADAM_CHECK_EVERY");
    const int v = e ? atoi(e) : 0;
    return v > 0 ? v : 25;
  }();
  return every;
}

// Grows the device state block of the resident loops.  The captured steps of sgpr_resident_general (h->rgraphs) hold addresses inside
// it: whoever reallocates it drops them (the stream is idle: every optimiser call ends with a synchronisation).
int ensure_adam_dev(gprx_handle h, size_t bytes) {
  if (h->adam_dev.bytes >= bytes) return GPRX_OK;
  for (auto& kv : h->rgraphs)
    if (kv.second) hipGraphExecDestroy(kv.second);
  h->rgraphs.clear();
  return ensure(h, h->adam_dev, bytes);
}

// Grows the pinned block of the resident loops; a failed allocation leaves neither a block nor a size behind.
int ensure_adam_pin(gprx_handle h, size_t bytes) {
  if (h->adam_pin_bytes >= bytes) return GPRX_OK;
  if (h->adam_pin) HIPCHK(h, hipHostFree(h->adam_pin));
  h->adam_pin = nullptr;
  h->adam_pin_bytes = 0;
  HIPCHK(h, hipHostMalloc((void**)&h->adam_pin, bytes, hipHostMallocDefault));
  h->adam_pin_bytes = bytes;
  return GPRX_OK;
}

// The state of a residency of `cells` cells: one layout for both loops.  Device block (h->adam_dev), doubles first: theta, mom, vel, best,
// loss (SfAdam), the window block, y.y of every unit; then ints: stale, active, n_evals, tstep, units, SF_MAX_GROUPS error words (one
// per group of cells).  A window block is check_every alpha values (one window, not max_iter: a call "until the early stop" passes
// max_iter = 2^31 - 1) and two doubles that carry the general route's control words (the fused route reads neither).  Pinned block
// (h->adam_pin): a window block, then the stop flags of the cells and the error words as last read.
struct ResidentState {
  SfAdam ad;                                              // the pointers, nt, nlen, ard; mask, max_iter and the alpha window are the route's to set
  double* win;                                            // the window block on the device
  size_t n_dbl, n_int;                                    // doubles and ints of the device block (the ints start at ad.stale)
  size_t o_mom, o_vel, o_best, o_loss, o_yy;              // where a host copy of the doubles holds each array (theta: 0)
  size_t o_stale, o_active, o_n_evals, o_tstep, o_units;  // the same for the ints
  double* hwin;                                           // pinned
  int* hflags;                                            // pinned: [cells] stop flags, then the error words
};
static_assert(SGPR_CTL_WORDS * sizeof(int) == 2 * sizeof(double), "the control words travel as two doubles behind the alpha table");

// lays the state of `cells` cells out and grows the two blocks to hold it
int resident_state(gprx_handle h, int cells, int check_every, ResidentState* out) {
  const size_t c = (size_t)cells, nt = (size_t)h->ntheta, gw = nt + (size_t)(h->m * h->d), win_dbl = (size_t)check_every + 2;
  ResidentState rs{};
  rs.o_mom = c * nt;
  rs.o_vel = rs.o_mom + c * gw;
  rs.o_best = rs.o_vel + c * gw;
  rs.o_loss = rs.o_best + c;
  const size_t o_win = rs.o_loss + c;
  rs.o_yy = o_win + win_dbl;
  rs.n_dbl = rs.o_yy + (size_t)h->n_units;
  rs.o_stale = 0;
  rs.o_active = c;
  rs.o_n_evals = 2 * c;
  rs.o_tstep = 3 * c;
  rs.o_units = 4 * c;
  rs.n_int = 5 * c + gprx_ctx::SF_MAX_GROUPS;
  int rc;
  if ((rc = ensure_adam_dev(h, sizeof(double) * rs.n_dbl + sizeof(int) * rs.n_int))) return rc;
  if ((rc = ensure_adam_pin(h, sizeof(double) * win_dbl + sizeof(int) * (c + gprx_ctx::SF_MAX_GROUPS)))) return rc;
  double* dp = h->adam_dev.p;
  int* ip = reinterpret_cast<int*>(dp + rs.n_dbl);
  rs.ad.theta = dp;
  rs.ad.mom = dp + rs.o_mom;
  rs.ad.vel = dp + rs.o_vel;
  rs.ad.best = dp + rs.o_best;
  rs.ad.loss = dp + rs.o_loss;
  rs.win = dp + o_win;
  rs.ad.yy = dp + rs.o_yy;
  rs.ad.stale = ip + rs.o_stale;
  rs.ad.active = ip + rs.o_active;
  rs.ad.n_evals = ip + rs.o_n_evals;
  rs.ad.tstep = ip + rs.o_tstep;
  rs.ad.units = ip + rs.o_units;
  rs.ad.error = ip + 5 * c;
  rs.ad.nt = h->ntheta;
  rs.ad.nlen = h->nlen;
  rs.ad.ard = h->ard;
  rs.hwin = h->adam_pin;
  rs.hflags = reinterpret_cast<int*>(h->adam_pin + win_dbl);
  *out = rs;
  return GPRX_OK;
}

// the alpha values of the window of steps done + 1 .. done + k (every running cell is at the same step)
void resident_fill_window(double* win, int done, int k) {
  for (int i = 0; i < k; ++i) win[i] = adam_alpha((double)done + 1.0 + i);
}

// the stop flags of the `cells` cells and n_err error words -> rs.hflags, one wait for the stream; *running: how many cells still run
int resident_read_flags(gprx_handle h, const ResidentState& rs, int cells, int n_err, int* running) {
  HIPCHK(h, hipMemcpyAsync(rs.hflags, rs.ad.active, sizeof(int) * cells, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(rs.hflags + cells, rs.ad.error, sizeof(int) * n_err, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, wait_stream(h, h->stream));
  *running = 0;
  for (int c = 0; c < cells; ++c) *running += rs.hflags[c] != 0 ? 1 : 0;
  return GPRX_OK;
}

// the end of a resident call: *batches = the most evaluations any cell took part in; bad_cell >= 0: that cell's Kuu or B was not
// positive definite, the call fails
int resident_finish(gprx_handle h, int count, const int* n_evals, int* batches, int bad_cell) {
  if (batches) {
    int mx = 0;
    for (int c = 0; c < count; ++c) mx = std::max(mx, n_evals[c]);
    *batches = mx;
  }
  if (bad_cell >= 0) {
    char msg[160];
    snprintf(msg, sizeof msg, "cell %d: Kuu or B not positive definite", bad_cell);
    return fail(h, GPRX_ENOTPD, msg);
  }
  return GPRX_OK;
}

// the arguments of sgpr_step_kernel for the launch sequence's layout; ctl: the control words on the device
SgprStep sgpr_step_params(gprx_handle h, const SgprLayout& L, const int* ctl) {
  const int mp = (int)h->mp, np = (int)h->np;
  SgprStep a{};
  a.arena = h->sarena.p;
  a.ss = L.ss;
  a.oZ = L.oZ;
  a.odZ = L.odZ;
  a.oRed = L.oRed;
  a.oPartP = L.oPart;
  a.oPartQ = L.oPart + L.part_p;
  a.nwg_p = (mp / KM_T) * (np / KM_T);
  a.nwg_q = (mp / KM_T) * (mp / KM_T);
  a.width = L.width;
  a.n = (int)h->n;
  a.m = (int)h->m;
  a.d = h->d;
  a.mp = mp;
  a.cellpar = h->cellpar.p;
  a.cellres = h->cellres.p;
  a.res_doubles = CELL_RES;
  a.ctl = ctl;
  return a;
}

// joins the other groups' streams of the fused loop into the handle's stream: on request and when it goes out of scope
struct SfJoin {
  gprx_handle h;
  hipStream_t st;
  int n = 0;
  hipStream_t other[gprx_ctx::SF_MAX_GROUPS] = {};
  void join() {
    for (int g = 1; g < n; ++g)
      if (hipEventRecord(h->sf_evs[g], other[g]) == hipSuccess) (void)hipStreamWaitEvent(st, h->sf_evs[g], 0);
    n = 0;
  }
  ~SfJoin() { join(); }
};

// gprx_adam_batch for sparse models with M <= 64: the loop RESIDENT on the device.  A step is FOUR launches (sgpr_fused.h: pass 1, mid,
// pass 2, and sf_adam_prep_kernel = partial sums + loss + gradient + Keras's update + the stop rule of gpr.py:160-171, then Kuu, L, L^-1
// of the updated variables with the positive transforms evaluated on the device); cells that have stopped return at once from every
// launch.  The host enqueues `check_every` steps, then reads the stop flags (count + 1 ints through pinned memory) -- no gradient, loss
// or parameter crosses the host link during the run (round 4: every step synchronised, downloaded the gradients, updated on the host
// and uploaded).  Same variables as the host-stepped loop, bit for bit (sgpr_asm.h, px_math.h; tests/test_gpu_gpras.py).  A cell whose
// Kuu or B stops being positive definite ends the call with GPRX_ENOTPD at the next check; the other cells may then be up to
// check_every - 1 steps past that evaluation.
// kind = SF_OPT_ADADELTA (gprx_adadelta_batch): the same loop with Keras's Adadelta update (gpr.py:176-192) in the fourth launch -- no alpha
// table, every cell runs max_iter steps; `losses` (optional) receives the loss of each cell's last evaluation.
// The other groups' streams are joined into the handle's stream before EVERY return (SfJoin): after a failed HIP call inside the step
// loop nothing may stay in flight on buffers the handle reuses.
int sgpr_resident_fused(gprx_handle h, int kind, int count, const int* units, double* theta, double* z, int mask, int max_iter, double* losses,
                        int* n_evals, int* batches) {
  const SgprLayout L = sgpr_batch_layout(h);
  int rc;
  if ((rc = ensure_sarena(h, count, L))) return rc;
  hipStream_t st = h->stream;
  const int nt = h->ntheta;
  const int64_t nz = h->m * h->d, gw = nt + nz;
  const int check_every = resident_check_every();
  ResidentState rs;
  if ((rc = resident_state(h, count, check_every, &rs))) return rc;
  SfAdam& ad = rs.ad;
  ad.alpha = nullptr;  // (set per window)
  ad.mask = mask;
  ad.max_iter = max_iter;
  // ---- initial state (host vectors live until the synchronisation below) ----
  std::vector<double> hd(rs.n_dbl, 0.0);
  std::vector<int> hi(rs.n_int, 0);
  std::memcpy(hd.data(), theta, sizeof(double) * (size_t)count * nt);
  std::memcpy(&hd[rs.o_yy], h->yy.data(), sizeof(double) * h->n_units);
  for (int c = 0; c < count; ++c) {
    hd[rs.o_best + c] = std::numeric_limits<double>::infinity();
    hd[rs.o_loss + c] = std::numeric_limits<double>::quiet_NaN();  // (no evaluation yet)
    hi[rs.o_active + c] = 1;
    hi[rs.o_units + c] = units[c];
  }
  HIPCHK(h, hipMemcpyAsync(h->adam_dev.p, hd.data(), sizeof(double) * rs.n_dbl, hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpyAsync(ad.stale, hi.data(), sizeof(int) * rs.n_int, hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemcpy2DAsync(h->sarena.p + L.oZ, sizeof(double) * (size_t)L.ss, z, sizeof(double) * (size_t)nz, sizeof(double) * (size_t)nz, count,
                             hipMemcpyHostToDevice, st));
  ++h->host_waits;
  HIPCHK(h, hipStreamSynchronize(st));
  SfParams p = sgpr_fused_params(h, L, true);
  p.active = ad.active;
  p.store_factors = 0;  // (nobody predicts from the cell blocks of a running optimisation)
  const int iso = (h->ard || h->dist_form) ? 0 : 1;
  const int* flags = rs.hflags;
  int error_cell = 0;
  h->factorized = false;  // the cell blocks are overwritten
  // (large batches: two groups of cells on two streams, one launch apart -- sf_group_count)
  constexpr int MAXG = gprx_ctx::SF_MAX_GROUPS;
  const int ngroups = sf_group_count(count, L.nsplit);
  if (ngroups > 1 && (rc = sf_group_streams(h, ngroups))) return rc;
  SfParams pg[MAXG];
  SfAdam adg[MAXG];
  int cells_g[MAXG], cell0_g[MAXG];
  hipStream_t sg_[MAXG];
  SfJoin joiner{h, st};
  for (int g = 0, cell0 = 0; g < ngroups; ++g) {
    const int cells = count / ngroups + (g < count % ngroups ? 1 : 0);
    sg_[g] = g == 0 ? st : h->sf_streams[g - 1];
    cell0_g[g] = cell0;
    cells_g[g] = cells;
    pg[g] = sf_params_from(p, cell0);
    adg[g] = ad;
    adg[g].theta += (int64_t)cell0 * nt;
    adg[g].mom += (int64_t)cell0 * gw;
    adg[g].vel += (int64_t)cell0 * gw;
    adg[g].best += cell0;
    adg[g].loss += cell0;
    adg[g].stale += cell0;
    adg[g].active += cell0;
    adg[g].n_evals += cell0;
    adg[g].tstep += cell0;
    adg[g].units += cell0;
    adg[g].error += g;
    joiner.other[g] = sg_[g];
    cell0 += cells;
  }
  joiner.n = ngroups;
  const bool adam = kind == SF_OPT_ADAM;
  for (int g = 0; g < ngroups; ++g)
    HIPCHK(h, sf_launch_prep(sg_[g], h->kid, h->dist_form, pg[g], cells_g[g], nullptr, nullptr, h->cellpar.p + (size_t)cell0_g[g] * CELL_PAR, &adg[g]));  // opens step 1
  for (int done = 0; done < max_iter;) {
    const int k = std::min(check_every, max_iter - done);
    // this window's alpha values: the pinned block is free, the previous window's upload has completed before its stop flags were read
    if (adam) {
      resident_fill_window(rs.hwin, done, k);
      HIPCHK(h, hipMemcpyAsync(rs.win, rs.hwin, sizeof(double) * (size_t)k, hipMemcpyHostToDevice, st));
    }
    if (adam && ngroups > 1) {
      HIPCHK(h, hipEventRecord(h->sf_evs[0], st));
      for (int g = 1; g < ngroups; ++g) HIPCHK(h, hipStreamWaitEvent(sg_[g], h->sf_evs[0], 0));
    }
    for (int g = 0; g < ngroups; ++g) {
      adg[g].alpha = rs.win;
      adg[g].alpha_t1 = done + 1;
    }
    for (int i = 0; i < k; ++i) {
      for (int g = 0; g < ngroups; ++g) {
        // (a group starts one launch behind the group before it; groups that start together stay in lock step and gain nothing)
        const bool first = done == 0 && i == 0;
        if (first && g > 0) HIPCHK(h, hipStreamWaitEvent(sg_[g], h->sf_evs[g - 1], 0));
        HIPCHK(h, sf_launch_pass1(sg_[g], h->kid, h->dist_form, pg[g], cells_g[g]));
        if (first && g + 1 < ngroups) HIPCHK(h, hipEventRecord(h->sf_evs[g], sg_[g]));
        HIPCHK(h, sf_launch_mid(sg_[g], pg[g], cells_g[g]));
        HIPCHK(h, sf_launch_pass2(sg_[g], h->kid, h->dist_form, iso, pg[g], cells_g[g]));
        // closes this step, opens the next
        HIPCHK(h, (adam ? sf_launch_adam_prep : sf_launch_adadelta_prep)(sg_[g], h->kid, h->dist_form, iso, pg[g], cells_g[g], adg[g],
                                                                         h->cellpar.p + (size_t)cell0_g[g] * CELL_PAR));
      }
    }
    done += k;
    for (int g = 1; g < ngroups; ++g) {
      HIPCHK(h, hipEventRecord(h->sf_evs[g], sg_[g]));
      HIPCHK(h, hipStreamWaitEvent(st, h->sf_evs[g], 0));
    }
    int running = 0;
    if ((rc = resident_read_flags(h, rs, count, ngroups, &running))) return rc;
    error_cell = 0;  // (1 + the cell: a group's error word counts the group's own cells from 1)
    for (int g = ngroups - 1; g >= 0; --g)
      if (flags[count + g] != 0) error_cell = cell0_g[g] + flags[count + g];
    if (error_cell != 0 || running == 0) break;
  }
  // ---- results ----
  joiner.join();  // (nothing of the other group's stream may outlive the call: max_iter = 0 enqueued its prep launch only)
  HIPCHK(h, hipMemcpyAsync(theta, ad.theta, sizeof(double) * (size_t)count * nt, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpy2DAsync(z, sizeof(double) * (size_t)nz, h->sarena.p + L.oZ, sizeof(double) * (size_t)L.ss, sizeof(double) * (size_t)nz, count,
                             hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(n_evals, ad.n_evals, sizeof(int) * count, hipMemcpyDeviceToHost, st));
  if (losses) HIPCHK(h, hipMemcpyAsync(losses, ad.loss, sizeof(double) * count, hipMemcpyDeviceToHost, st));
  ++h->host_waits;
  HIPCHK(h, hipStreamSynchronize(st));
  return resident_finish(h, count, n_evals, batches, error_cell - 1);
}

// gprx_adam_batch / gprx_adadelta_batch for the sparse models that the fused route above does not take (M > 64, or M <= 64 with
// "sgpr_fused" = 0; d <= 64): the loop resident on the device around the GENERAL launch sequence.  A step is the body of
// sgpr_batch_enqueue (no stage-in, no stage-out) followed by sgpr_step_kernel (sgpr_step.h), which forms the loss and the gradient, runs
// the update and the stop rule and writes the next step's parameter row -- what the host did between two evaluations of the host-stepped
// loop, with the same arithmetic: the same bits.  One stream, a linear graph per (cells, optimiser): the first step of a shape goes out
// eagerly, the second is captured, later ones are replayed (sgpr_replay); everything that changes between steps, windows or calls
// (step count, mask, max_iter, the window's alpha values and their first step) is read from device memory.  Every `check_every` steps
// the host reads the stop flags and the error word.  Between two reads a stopped cell is still evaluated but the step kernel leaves it
// alone; at a read where cells have stopped the residency is closed (state down) and reopened for the cells that still run (state up,
// stage-in): a cell's bits depend neither on its slot nor on the batch size.  Failure: as sgpr_resident_fused.
int sgpr_resident_general(gprx_handle h, int kind, int count, const int* units, double* theta, double* z, int mask, int max_iter, double* losses,
                          int* n_evals, int* batches) {
  const SgprLayout L = sgpr_batch_layout(h);
  int rc;
  if ((rc = ensure_sarena(h, count, L))) return rc;
  hipStream_t st = h->stream;
  const int nt = h->ntheta;
  const int64_t nz = h->m * h->d, gw = nt + nz;
  const int check_every = resident_check_every();
  const bool adam = kind == SF_OPT_ADAM;
  // ---- the optimiser's state of every cell on the host: what a residency is opened from and closed into ----
  std::vector<double> mom((size_t)count * gw, 0.0), vel((size_t)count * gw, 0.0), best(count, std::numeric_limits<double>::infinity()),
      loss(count, std::numeric_limits<double>::quiet_NaN());
  std::vector<int> stale(count, 0), active(count);
  for (int c = 0; c < count; ++c) active[c] = c;
  const SgprParSrc ps = sgpr_par_src(h, 0.0, 0.0);  // (d <= 64: the parameter table)
  h->factorized = false;                            // the cell blocks are overwritten
  int done = 0, error_cell = -1;
  while (!active.empty() && done < max_iter && error_cell < 0) {
    // ---- open: state and staged inputs of the `na` running cells up, stage-in (the first residency is the largest: it sizes the
    // blocks) ----
    const int na = (int)active.size();
    ResidentState rs;
    if ((rc = resident_state(h, na, check_every, &rs))) return rc;
    SfAdam& ad = rs.ad;
    ad.alpha = rs.win;
    int* hctl = reinterpret_cast<int*>(rs.hwin + check_every);
    const int* flags = rs.hflags;
    std::fill(rs.hwin, rs.hwin + check_every, 0.0);  // (Adadelta reads no alpha)
    std::vector<double> hd(rs.n_dbl, 0.0), zc((size_t)na * nz);
    std::vector<int> hi(rs.n_int, 0);
    const SgprStage sg = sgpr_stage(h, na, L);
    for (int j = 0; j < na; ++j) {
      const int i = active[j];
      std::memcpy(&hd[(size_t)j * nt], theta + (size_t)i * nt, sizeof(double) * nt);
      std::memcpy(&hd[rs.o_mom + (size_t)j * gw], &mom[(size_t)i * gw], sizeof(double) * gw);
      std::memcpy(&hd[rs.o_vel + (size_t)j * gw], &vel[(size_t)i * gw], sizeof(double) * gw);
      hd[rs.o_best + j] = best[i];
      hd[rs.o_loss + j] = loss[i];
      hi[rs.o_stale + j] = stale[i];
      hi[rs.o_active + j] = 1;
      hi[rs.o_n_evals + j] = n_evals[i];
      hi[rs.o_tstep + j] = done;
      hi[rs.o_units + j] = units[i];
      sgpr_par_row(h, h->spin + sg.par + (size_t)j * CELL_PAR, units[i], decode_theta(h, theta + (size_t)i * nt));
      std::memcpy(h->spin + sg.z + (size_t)j * nz, z + (size_t)i * nz, sizeof(double) * nz);
    }
    std::memcpy(&hd[rs.o_yy], h->yy.data(), sizeof(double) * h->n_units);
    HIPCHK(h, hipMemcpyAsync(h->adam_dev.p, hd.data(), sizeof(double) * rs.n_dbl, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(ad.stale, hi.data(), sizeof(int) * rs.n_int, hipMemcpyHostToDevice, st));
    if ((rc = sgpr_stage_in_enqueue(h, na, L))) return rc;
    HIPCHK(h, hipGetLastError());
    ++h->host_waits;
    HIPCHK(h, hipStreamSynchronize(st));  // (the host vectors and the pinned rows are free again)
    const SgprStep sa = sgpr_step_params(h, L, reinterpret_cast<const int*>(rs.win + check_every));
    auto step_enqueue = [&]() -> int {
      int erc;
      if ((erc = sgpr_body_enqueue(h, na, L, true, ps))) return erc;
      HIPCHK(h, sgpr_launch_step(st, kind, sa, ad, na));
      return GPRX_OK;
    };
    // ---- windows of check_every steps until a cell stops ----
    int running = na;
    while (done < max_iter && running == na && error_cell < 0) {
      const int k = std::min(check_every, max_iter - done);
      // this window's alpha values and the control words: the pinned block is free, the previous window's upload had completed before
      // its stop flags were read
      if (adam) resident_fill_window(rs.hwin, done, k);
      hctl[SGPR_CTL_MASK] = mask;
      hctl[SGPR_CTL_MAX_ITER] = max_iter;
      hctl[SGPR_CTL_ALPHA_T1] = done + 1;
      hctl[3] = 0;
      HIPCHK(h, hipMemcpyAsync(rs.win, rs.hwin, sizeof(double) * ((size_t)check_every + 2), hipMemcpyHostToDevice, st));
      for (int i = 0; i < k; ++i) {
        bool replayed = false;
        if ((rc = sgpr_replay(h, h->rgraphs, {na, kind}, step_enqueue, &replayed))) return rc;
        if (!replayed && (rc = step_enqueue())) return rc;
      }
      done += k;
      if ((rc = resident_read_flags(h, rs, na, 1, &running))) return rc;
      if (flags[na] != 0) error_cell = active[flags[na] - 1];
    }
    // ---- close: the state of the na cells down ----
    HIPCHK(h, hipMemcpyAsync(hd.data(), h->adam_dev.p, sizeof(double) * rs.n_dbl, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpyAsync(hi.data(), ad.stale, sizeof(int) * rs.n_int, hipMemcpyDeviceToHost, st));
    HIPCHK(h, hipMemcpy2DAsync(zc.data(), sizeof(double) * (size_t)nz, h->sarena.p + L.oZ, sizeof(double) * (size_t)L.ss, sizeof(double) * (size_t)nz, na,
                               hipMemcpyDeviceToHost, st));
    ++h->host_waits;
    HIPCHK(h, hipStreamSynchronize(st));
    std::vector<int> next;
    for (int j = 0; j < na; ++j) {
      const int i = active[j];
      std::memcpy(theta + (size_t)i * nt, &hd[(size_t)j * nt], sizeof(double) * nt);
      std::memcpy(&mom[(size_t)i * gw], &hd[rs.o_mom + (size_t)j * gw], sizeof(double) * gw);
      std::memcpy(&vel[(size_t)i * gw], &hd[rs.o_vel + (size_t)j * gw], sizeof(double) * gw);
      best[i] = hd[rs.o_best + j];
      loss[i] = hd[rs.o_loss + j];
      stale[i] = hi[rs.o_stale + j];
      n_evals[i] = hi[rs.o_n_evals + j];
      std::memcpy(z + (size_t)i * nz, &zc[(size_t)j * nz], sizeof(double) * nz);
      if (hi[rs.o_active + j] != 0) next.push_back(i);
    }
    active.swap(next);
  }
  if (losses)
    for (int c = 0; c < count; ++c) losses[c] = loss[c];
  return resident_finish(h, count, n_evals, batches, error_cell);
}

int check_handle(gprx_handle h) {
  if (!h) return fail(nullptr, GPRX_EINVAL, "null handle");
  hipError_t e = hipSetDevice(h->device);
  if (e != hipSuccess) return fail(h, GPRX_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
  return GPRX_OK;
}

}  // namespace

// ======================================================================================================
extern "C" {

int gprx_version(void) { return GPRX_VERSION; }

const char* gprx_last_error(gprx_handle h) { return h ? h->err.c_str() : last_error().c_str(); }

int gprx_device_count(int* count) {
  if (!count) return fail(nullptr, GPRX_EINVAL, "count is null");
  HIPCHK(nullptr, hipGetDeviceCount(count));
  return GPRX_OK;
}

int gprx_create(int device, int64_t n, int d, int64_t m, int kernel_id, int ard, gprx_handle* out) {
  if (!out) return fail(nullptr, GPRX_EINVAL, "out is null");
  *out = nullptr;
  if (n <= 0 || d <= 0 || m < 0) return fail(nullptr, GPRX_EINVAL, "n, d must be positive and m non-negative");
  if (kernel_id < 0 || kernel_id > 4) return fail(nullptr, GPRX_EINVAL, "unknown kernel id");
  if (n > (1 << 30) || m > (1 << 30)) return fail(nullptr, GPRX_EINVAL, "n or m too large");
  HIPCHK(nullptr, hipSetDevice(device));
  gprx_handle h = new gprx_ctx();
  h->device = device;
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
  // normal priority on purpose: measured on MI355X, raised/lowered stream priorities do nothing for a single
  // cell and cut the throughput of several concurrent cells by up to 2x
  hipError_t e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete h;
    return fail(nullptr, GPRX_EHIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
  }
  h->own_stream = true;
  for (auto& ev : h->ev) hipEventCreate(&ev);
  // the look-ahead stream is created on first use (ensure_lookahead): HIP binds streams to its 4 hardware
  // queues round-robin at creation, so an unused second stream per handle would leave the main streams of
  // many concurrent cells on half of the queues (measured: 584 instead of 797 fits/s with 12 cells)
  int rc;
  if ((rc = ensure(h, h->invls, sizeof(double) * d)) || (rc = ensure(h, h->red, sizeof(double) * 16))) {
    gprx_destroy(h);
    return rc;
  }
  e = hipMalloc((void**)&h->info, sizeof(int));
  if (e == hipSuccess) e = hipHostMalloc((void**)&h->pin, sizeof(double) * 80, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&h->gparams, sizeof(double) * 2);
  if (e != hipSuccess) {
    gprx_destroy(h);
    return fail(nullptr, GPRX_ENOMEM, "hipMalloc(info) / hipHostMalloc(staging)");
  }
  *out = h;
  return GPRX_OK;
}

int gprx_destroy(gprx_handle h) {
  if (!h) return GPRX_OK;
  hipSetDevice(h->device);
  if (h->stream) hipStreamSynchronize(h->stream);
  for (Buf* b : {&h->X, &h->Y, &h->invls, &h->alpha, &h->red, &h->Kmat, &h->invD, &h->Xinv, &h->Tmp, &h->partial, &h->xs, &h->Ks, &h->pred,
                 &h->dstage, &h->arena, &h->cellpar, &h->cellres, &h->garena, &h->gpartial, &h->apart, &h->twork, &h->sarena})
    if (b->p && !b->borrowed) hipFree(b->p);
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
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (h->own_stream && h->stream) {
    hipStreamSynchronize(h->stream);
    hipStreamDestroy(h->stream);
  }
  h->stream = (hipStream_t)hip_stream;
  h->own_stream = false;
  return GPRX_OK;
}

int gprx_set_distance_form(gprx_handle h, int form) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (form != GPRX_DIST_DIFFERENCE && form != GPRX_DIST_EXPANDED) return fail(h, GPRX_EINVAL, "unknown distance form");
  if (form != h->dist_form) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->dist_form = form;
    h->factorized = false;  // resident factorisations (and captured graphs) were built with the other form
    h->have_linv = false;
    drop_graphs(h);
    std::fill(h->slot_ok.begin(), h->slot_ok.end(), 0);
  }
  return GPRX_OK;
}

int gprx_synchronize(gprx_handle h) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  HIPCHK(h, wait_stream(h, h->stream));
  return GPRX_OK;
}

int gprx_set_data(gprx_handle h, const double* x, const double* y, int n_units) {
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
  h->factorized = false;
  h->have_linv = false;
  std::fill(h->slot_ok.begin(), h->slot_ok.end(), 0);  // resident batch slots were factorised from the old data
  std::fill(h->slot_unit.begin(), h->slot_unit.end(), -1);
  drop_graphs(h);
  h->yy.assign(n_units, 0.0);
  for (int u = 0; u < n_units; ++u) {
    double acc = 0.0;
    for (int64_t i = 0; i < h->n; ++i) acc += y[i * n_units + u] * y[i * n_units + u];
    h->yy[u] = acc;
  }
  return GPRX_OK;
}

// priors and softplus chain rule on the hyperparameter part of a gradient; loss = -(value + log prior)
void chain_rule(gprx_handle h, const Theta& t, int mask, const double* g, double* grad) {
  grad[0] = sgpr_asm_chain(g[0], t.variance, t.w_var, (mask & GPRX_TRAIN_VARIANCE) != 0);
  for (int k = 0; k < h->nlen; ++k)
    grad[1 + k] = sgpr_asm_chain(g[1 + k], t.ls[k], t.w_len[k], (mask & GPRX_TRAIN_LENGTHSCALE) != 0);
  grad[1 + h->nlen] = sgpr_asm_chain(g[1 + h->nlen], t.noise, t.w_noise, (mask & GPRX_TRAIN_NOISE) != 0);
}

static int objective_impl(gprx_handle h, int unit, const double* theta, const double* z, int mask, double* loss, double* grad) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (!theta) return fail(h, GPRX_EINVAL, "theta is null");
  if (unit < 0 || unit >= h->n_units) return fail(h, GPRX_EINVAL, "unit out of range (call gprx_set_data first)");
  for (int k = 0; k < h->ntheta; ++k)
    if (!std::isfinite(theta[k])) return fail(h, GPRX_EINVAL, "theta is not finite");
  const Theta t = decode_theta(h, theta);
  double value = 0.0;  // LML (exact) or ELBO (sparse)
  if (h->m != 0) {
    // one model is a batch of one cell -- the same kernels, the same summation order as any batch (a model evaluated alone and
    // inside a batch agree bit for bit); the factorisation stays in cell block 0, where gprx_predict reads it
    if (!z) return fail(h, GPRX_EINVAL, "z (inducing inputs) is null for a sparse model");
    const int64_t nz = h->m * h->d;
    for (int64_t e = 0; e < nz; ++e)
      if (!std::isfinite(z[e])) return fail(h, GPRX_EINVAL, "z is not finite");
    std::vector<double> g(grad ? h->ntheta : 0), gzv(grad ? nz : 0);
    int st = GPRX_OK;
    if ((rc = sgpr_objective_batch(h, 1, &unit, &t, z, &value, grad ? g.data() : nullptr, grad ? gzv.data() : nullptr, &st))) return rc;
    if (loss) *loss = -(value + log_prior(h, t, mask));
    if (grad) {
      chain_rule(h, t, mask, g.data(), grad);
      double* gz = grad + h->ntheta;
      for (int64_t e = 0; e < nz; ++e) gz[e] = (mask & GPRX_TRAIN_Z) ? -gzv[e] : 0.0;
    }
    for (double& tm : h->timings) tm = 0.0;  // (no phase events inside a sequence that is replayed from a graph)
    h->factorized = true;
    h->cur_unit = unit;
    h->variance = t.variance;
    h->noise = t.noise;
    h->ls = t.ls;
    return GPRX_OK;
  }
  // exact model with gradient: ONE stream synchronisation for both halves, and alpha from the inverse the gradient builds (the
  // 64 dependent launches of the backward substitution drop out of the evaluation); a non-PD matrix is reported by the
  // factorisation's status as before (the gradient launches behind it are then wasted, not wrong: nothing is read back)
  static const bool fused_eval = !(getenv("GPRX_FUSED_EVAL") && atoi(getenv("GPRX_FUSED_EVAL")) == 0);
  const bool fused = grad && fused_eval && !h->profiling;
  std::vector<double> ghost(fused ? 2 + h->d : 0);
  if (fused) {
    if ((rc = exact_factorize_enqueue(h, unit, t, true, false, false))) return rc;
    if ((rc = exact_gradient_enqueue(h, t, ghost.data(), true))) {
      hipStreamSynchronize(h->stream);
      return rc;
    }
    if ((rc = exact_factorize_finish(h, &value))) return rc;
  } else {
    if ((rc = exact_factorize(h, unit, t, &value))) return rc;
  }
  const double lp = log_prior(h, t, mask);
  if (loss) *loss = -(value + lp);
  if (grad) {
    std::vector<double> g(h->ntheta, 0.0);
    if (fused) {
      exact_gradient_collect(h, ghost.data(), g.data());
    } else {
      if ((rc = exact_gradient(h, t, g.data()))) return rc;
    }
    HIPCHK(h, hipEventRecord(h->ev[4], h->stream));
    chain_rule(h, t, mask, g.data(), grad);
  } else {
    HIPCHK(h, hipEventRecord(h->ev[4], h->stream));
  }
  HIPCHK(h, wait_stream(h, h->stream));
  for (int s = 0; s < 4; ++s) {
    float ms = 0.f;
    hipEventElapsedTime(&ms, h->ev[s], h->ev[s + 1]);
    h->timings[s] = ms;
  }
  return GPRX_OK;
}

int gprx_objective(gprx_handle h, int unit, const double* theta, const double* z, int mask, double* loss, double* grad) {
  return objective_impl(h, unit, theta, z, mask, loss, grad);
}

int gprx_factorize(gprx_handle h, int unit, const double* theta, const double* z, int mask, double* loss) {
  return objective_impl(h, unit, theta, z, mask, loss, nullptr);
}

int gprx_factorize_many(int count, gprx_handle* handles, const int* units, const double* thetas, int mask, double* losses) {
  if (count < 0 || !handles || !units || !thetas) return fail(nullptr, GPRX_EINVAL, "null argument");
  std::vector<Theta> ts(count);
  // enqueue every cell's work first (nothing blocks), then wait for each: the cells overlap on the device.
  // With several cells in flight each one runs on its single stream (no look-ahead stream): measured, 12
  // cells reach 2.2x the single-cell rate that way and only 1.5x with two streams per cell.
  for (int i = 0; i < count; ++i) {
    gprx_handle h = handles[i];
    int rc;
    if ((rc = check_handle(h))) return rc;
    if (h->m != 0) return fail(h, GPRX_EINVAL, "gprx_factorize_many: exact models only");
    if (units[i] < 0 || units[i] >= h->n_units) return fail(h, GPRX_EINVAL, "unit out of range");
    for (int k = 0; k < h->ntheta; ++k)
      if (!std::isfinite(thetas[(int64_t)i * h->ntheta + k])) return fail(h, GPRX_EINVAL, "theta is not finite");
    ts[i] = decode_theta(h, thetas + (int64_t)i * h->ntheta);
    if ((rc = (count == 1) ? exact_factorize_enqueue(h, units[i], ts[i], true) : exact_factorize_replay(h, units[i], ts[i]))) return rc;
  }
  int first_error = GPRX_OK;
  for (int i = 0; i < count; ++i) {
    gprx_handle h = handles[i];
    hipSetDevice(h->device);
    double lml = 0.0;
    const int rc = exact_factorize_finish(h, &lml);
    if (rc && !first_error) first_error = rc;
    if (losses) losses[i] = rc ? std::numeric_limits<double>::quiet_NaN() : -(lml + log_prior(h, ts[i], mask));
  }
  return first_error;
}

// gprx_adam_batch and gprx_adadelta_batch: one loop, two updates (kind: SF_OPT_ADAM, SF_OPT_ADADELTA of sgpr_asm.h).  Adadelta has no stop
// rule, so its batch never shrinks.  last_losses (optional): the loss of each cell's last evaluation.
static int optimizer_batch(gprx_handle h, int kind, int count, const int* units, double* theta, double* z, int mask, int max_iter,
                           double* last_losses, int* n_evals, int* batches) {
#pragma clang fp contract(off)
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (count <= 0 || !units || !theta || !n_evals || max_iter < 0) return fail(h, GPRX_EINVAL, "null argument");
  if (h->m != 0 && !z) return fail(h, GPRX_EINVAL, "z (inducing inputs) is null for a sparse model");
  const int nt = h->ntheta;
  const int64_t nz = h->m * h->d, gw = nt + nz;
  if (batches) *batches = 0;
  for (int i = 0; i < count; ++i) n_evals[i] = 0;
  if (last_losses)
    for (int i = 0; i < count; ++i) last_losses[i] = std::numeric_limits<double>::quiet_NaN();  // (no evaluation yet)
  const bool adam = kind == SF_OPT_ADAM;
  // trainable elements of a cell's gradient row [d theta | d Z] (theta: [variance, lengthscales..., noise])
  std::vector<char> train((size_t)gw, 0);
  train[0] = (mask & GPRX_TRAIN_VARIANCE) != 0;
  for (int k = 1; k < nt - 1; ++k) train[k] = (mask & GPRX_TRAIN_LENGTHSCALE) != 0;
  train[nt - 1] = (mask & GPRX_TRAIN_NOISE) != 0;
  for (int64_t e = 0; e < nz; ++e) train[nt + e] = (mask & GPRX_TRAIN_Z) != 0;
  bool any = false;
  for (char t : train) any = any || t;
  if (!any) return GPRX_OK;  // nothing trainable: no step can change anything (optimizers._optimize_adam returns at once)
  static const bool adam_on_host = getenv("GPRX_ADAM_HOST") && atoi(getenv("GPRX_ADAM_HOST")) != 0;  // escape hatch: the host-stepped loop
  // sparse models with d <= 64 keep the loop on the device ("sgpr_resident" = 0: never): around the five fused launches where the
  // evaluation takes them (M <= 64), around the general launch sequence otherwise
  if (h->m != 0 && h->sgpr_resident && h->d <= CELL_PAR - CELL_PAR_LS && !adam_on_host && max_iter > 0) {
    for (int i = 0; i < count; ++i) {
      if (units[i] < 0 || units[i] >= h->n_units) return fail(h, GPRX_EINVAL, "unit out of range (call gprx_set_data first)");
      for (int k = 0; k < nt; ++k)
        if (!std::isfinite(theta[(size_t)i * nt + k])) return fail(h, GPRX_EINVAL, "theta is not finite");
    }
    for (int64_t e = 0; e < (int64_t)count * nz; ++e)
      if (!std::isfinite(z[e])) return fail(h, GPRX_EINVAL, "z is not finite");
    h->last_route = sgpr_five_launches(h) ? 1 : 2;
    return (sgpr_five_launches(h) ? sgpr_resident_fused : sgpr_resident_general)(h, kind, count, units, theta, z, mask, max_iter, last_losses, n_evals,
                                                                                   batches);
  }
  std::vector<double> mom((size_t)count * gw, 0.0), vel((size_t)count * gw, 0.0), best(count, std::numeric_limits<double>::infinity());
  std::vector<int> stale(count, 0), active(count);
  for (int i = 0; i < count; ++i) active[i] = i;
  std::vector<int> a_units(count);
  std::vector<double> a_theta((size_t)count * nt), a_z((size_t)count * nz), losses(count), grads((size_t)count * gw);
  for (int t = 1; t <= max_iter && !active.empty(); ++t) {
    const int na = (int)active.size();
    for (int j = 0; j < na; ++j) {
      const int i = active[j];
      a_units[j] = units[i];
      std::memcpy(&a_theta[(size_t)j * nt], theta + (size_t)i * nt, sizeof(double) * nt);
      if (nz) std::memcpy(&a_z[(size_t)j * nz], z + (size_t)i * nz, sizeof(double) * nz);
    }
    rc = gprx_objective_batch(h, na, a_units.data(), a_theta.data(), nz ? a_z.data() : nullptr, mask, losses.data(), grads.data());
    if (batches) ++*batches;
    for (int j = 0; j < na; ++j) ++n_evals[active[j]];
    if (last_losses)  // (a failed cell holds NaN; after any other error the evaluation wrote no loss)
      for (int j = 0; j < na; ++j) last_losses[active[j]] = (rc == GPRX_OK || rc == GPRX_ENOTPD) ? losses[j] : std::numeric_limits<double>::quiet_NaN();
    if (rc) return rc;  // (GPRX_ENOTPD included: the reference's optimiser dies with the exception of that evaluation)
    const double alpha = adam ? adam_alpha((double)t) : 0.0;
    std::vector<int> next;
    next.reserve(na);
    for (int j = 0; j < na; ++j) {
      const int i = active[j];
      double* mo = &mom[(size_t)i * gw];
      double* ve = &vel[(size_t)i * gw];
      const double* g = &grads[(size_t)j * gw];
      for (int64_t e = 0; e < gw; ++e) {
        if (!train[e]) continue;
        double* x = e < nt ? theta + (size_t)i * nt + e : z + (size_t)i * nz + (e - nt);
        if (adam)
          adam_element(g[e], alpha, mo[e], ve[e], *x);  // (sgpr_asm.h: the resident loop's kernel runs the same function)
        else
          adadelta_element(g[e], mo[e], ve[e], *x);  // (the accumulated squared gradients and updates in the moments' arrays)
      }
      if (!adam || adam_keep_running(losses[j], best[i], stale[i])) next.push_back(i);
    }
    active.swap(next);
  }
  return GPRX_OK;
}

// (gprx_last_optimizer_route: the route and the stream waits of this call)
static int optimizer_routed(gprx_handle h, int kind, int count, const int* units, double* theta, double* z, int mask, int max_iter,
                            double* last_losses, int* n_evals, int* batches) {
  if (h) {
    h->last_route = 0;
    h->host_waits = 0;
  }
  const int rc = optimizer_batch(h, kind, count, units, theta, z, mask, max_iter, last_losses, n_evals, batches);
  if (h) h->last_host_waits = h->host_waits;
  return rc;
}

int gprx_last_optimizer_route(gprx_handle h, int* route, int* host_waits) {
  if (!h || !route || !host_waits) return fail(h, GPRX_EINVAL, "null argument");
  *route = h->last_route;
  *host_waits = h->last_host_waits;
  return GPRX_OK;
}

int gprx_adam_batch(gprx_handle h, int count, const int* units, double* theta, double* z, int mask, int max_iter, int* n_evals, int* batches) {
  try {
    return optimizer_routed(h, SF_OPT_ADAM, count, units, theta, z, mask, max_iter, nullptr, n_evals, batches);
  } catch (const std::bad_alloc&) {  // (no C++ exception may cross the C ABI)
    return fail(h, GPRX_ENOMEM, "host allocation failed");
  }
}

int gprx_adadelta_batch(gprx_handle h, int count, const int* units, double* theta, double* z, int mask, int max_iter, double* losses, int* n_evals,
                        int* batches) {
  try {
    return optimizer_routed(h, SF_OPT_ADADELTA, count, units, theta, z, mask, max_iter, losses, n_evals, batches);
  } catch (const std::bad_alloc&) {
    return fail(h, GPRX_ENOMEM, "host allocation failed");
  }
}

int gprx_factorize_batch(gprx_handle h, int count, const int* units, const double* thetas, int mask, double* losses, int* status) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (count <= 0 || !units || !thetas) return fail(h, GPRX_EINVAL, "count must be positive, units and thetas non-null");
  if (h->m != 0) return fail(h, GPRX_EINVAL, "gprx_factorize_batch: exact models only");
  if (h->d > CELL_PAR - CELL_PAR_LS) return fail(h, GPRX_EINVAL, "gprx_factorize_batch: d <= 64 only");
  // (the handle keeps the decoded parameter sets of the last batch: their lengthscale vectors are reused, no allocation per cell and call --
  // 512 cells of N = 512 spent 68 us here, 5 % of the call)
  std::vector<Theta>& ts = h->batch_thetas;
  if ((int)ts.size() < count) ts.resize(count);
  for (int i = 0; i < count; ++i) {
    if (units[i] < 0 || units[i] >= h->n_units) return fail(h, GPRX_EINVAL, "unit out of range (call gprx_set_data first)");
    for (int k = 0; k < h->ntheta; ++k)
      if (!std::isfinite(thetas[(int64_t)i * h->ntheta + k])) return fail(h, GPRX_EINVAL, "theta is not finite");
    decode_theta_into(h, thetas + (int64_t)i * h->ntheta, ts[i]);
  }
  std::vector<double>& lml = h->batch_lml;
  if ((int)lml.size() < count) lml.resize(count);
  rc = exact_factorize_batch(h, count, units, ts.data(), lml.data(), status);
  if (rc != GPRX_OK && rc != GPRX_ENOTPD) return rc;
  if (losses)
    for (int i = 0; i < count; ++i) losses[i] = -(lml[i] + log_prior(h, ts[i], mask));  // NaN for a failed cell
  return rc;
}

int gprx_select_slot(gprx_handle h, int slot) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  return select_slot(h, slot);
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
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (count < 0 || !units || !theta || !losses) return fail(h, GPRX_EINVAL, "null argument");
  const int64_t gw = h->ntheta + h->m * h->d;
  if (h->m == 0 && count > 1 && h->d <= CELL_PAR - CELL_PAR_LS) {
    // exact models: every stage once for all cells (batched launches), results identical to the loop below
    std::vector<Theta> ts(count);
    for (int i = 0; i < count; ++i) {
      if (units[i] < 0 || units[i] >= h->n_units) return fail(h, GPRX_EINVAL, "unit out of range (call gprx_set_data first)");
      for (int k = 0; k < h->ntheta; ++k)
        if (!std::isfinite(theta[(int64_t)i * h->ntheta + k])) return fail(h, GPRX_EINVAL, "theta is not finite");
      ts[i] = decode_theta(h, theta + (int64_t)i * h->ntheta);
    }
    std::vector<double> lml(count);
    static const bool fused_eval = !(getenv("GPRX_FUSED_EVAL") && atoi(getenv("GPRX_FUSED_EVAL")) == 0);
    const bool form_alpha = grads && fused_eval;  // (as gprx_objective: alpha from the gradient's inverse, same kernels -> same bits)
    const int frc = exact_factorize_batch(h, count, units, ts.data(), lml.data(), nullptr, !form_alpha);
    if (frc != GPRX_OK && frc != GPRX_ENOTPD) return frc;
    for (int i = 0; i < count; ++i) losses[i] = -(lml[i] + log_prior(h, ts[i], mask));
    if (grads) {
      std::vector<double> g((size_t)count * h->ntheta, 0.0);
      if ((rc = exact_gradient_batch(h, count, g.data(), form_alpha))) {
        if (form_alpha)  // (the slots hold factors without their alpha: nothing may predict from them)
          for (int i = 0; i < count; ++i) {
            h->slot_ok[i] = 0;
            h->slot_unit[i] = -1;
          }
        return rc;
      }
      for (int i = 0; i < count; ++i) {
        double* gi = grads + (int64_t)i * gw;
        if (h->slot_ok[i]) {
          chain_rule(h, ts[i], mask, g.data() + (size_t)i * h->ntheta, gi);
        } else {
          for (int k = 0; k < h->ntheta; ++k) gi[k] = std::numeric_limits<double>::quiet_NaN();
        }
      }
    }
    return frc;
  }
  if (h->m != 0 && count > 1 && h->d <= CELL_PAR - CELL_PAR_LS) {
    if (!z) return fail(h, GPRX_EINVAL, "z (inducing inputs) is null for a sparse model");
    const int64_t nz = h->m * h->d;
    for (int64_t e = 0; e < (int64_t)count * nz; ++e)
      if (!std::isfinite(z[e])) return fail(h, GPRX_EINVAL, "z is not finite");
    std::vector<Theta> ts(count);
    for (int i = 0; i < count; ++i) {
      if (units[i] < 0 || units[i] >= h->n_units) return fail(h, GPRX_EINVAL, "unit out of range (call gprx_set_data first)");
      for (int k = 0; k < h->ntheta; ++k)
        if (!std::isfinite(theta[(int64_t)i * h->ntheta + k])) return fail(h, GPRX_EINVAL, "theta is not finite");
      ts[i] = decode_theta(h, theta + (int64_t)i * h->ntheta);
    }
    std::vector<double> elbo(count), g(grads ? (size_t)count * h->ntheta : 0), gzv(grads ? (size_t)count * nz : 0);
    std::vector<int> st(count);
    const int frc = sgpr_objective_batch(h, count, units, ts.data(), z, elbo.data(), grads ? g.data() : nullptr, grads ? gzv.data() : nullptr, st.data());
    if (frc != GPRX_OK && frc != GPRX_ENOTPD) return frc;
    for (int i = 0; i < count; ++i) {
      losses[i] = -(elbo[i] + log_prior(h, ts[i], mask));  // NaN for a failed cell
      if (!grads) continue;
      double* gi = grads + (int64_t)i * gw;
      if (st[i] != GPRX_OK) {
        for (int64_t k = 0; k < gw; ++k) gi[k] = std::numeric_limits<double>::quiet_NaN();
        continue;
      }
      chain_rule(h, ts[i], mask, g.data() + (size_t)i * h->ntheta, gi);
      double* gzi = gi + h->ntheta;
      for (int64_t e = 0; e < nz; ++e) gzi[e] = (mask & GPRX_TRAIN_Z) ? -gzv[(size_t)i * nz + e] : 0.0;
    }
    return frc;
  }
  // one cell after the other (a single cell, or d > 64): same contract as the batched paths -- a cell
  // whose matrix is not positive definite gets NaN, the others are still evaluated, the first failure is returned
  int first_error = GPRX_OK;
  for (int i = 0; i < count; ++i) {
    rc = objective_impl(h, units[i], theta + (int64_t)i * h->ntheta, z ? z + (int64_t)i * h->m * h->d : nullptr, mask, losses + i,
                        grads ? grads + (int64_t)i * gw : nullptr);
    if (rc == GPRX_ENOTPD) {
      losses[i] = std::numeric_limits<double>::quiet_NaN();
      if (grads)
        for (int64_t k = 0; k < gw; ++k) grads[(int64_t)i * gw + k] = std::numeric_limits<double>::quiet_NaN();
      if (!first_error) first_error = rc;
      continue;
    }
    if (rc) return rc;
  }
  return first_error;
}

static constexpr int PRED_TILE = 8192;
// test points per pass of ONE exact model's predict: the N x tile blocks Ks and V = L^-1 Ks stay at the 268 MB each they have at N = 4096,
// so a small model takes more points per pass (N = 1024: 13 passes of 7 692 points with four launches each spent 21 % of the predict outside
// the product; per-point results do not depend on the pass they fall into)
static inline int pred_tile_for(int64_t np) { return np <= 1024 ? 4 * PRED_TILE : (np <= 2048 ? 2 * PRED_TILE : PRED_TILE); }

// what one exact factorisation contributes to a prediction through the explicit inverse: alpha, L^-1, the kernel's
// hyperparameters (a device lengthscale vector, or a row of the cell-parameter table) and the variance offset
struct ExactPredictSrc {
  const double* alpha;
  const double* Xinv;
  const double* ls_dev;
  const double* cell_par;  // row of the batch's cell-parameter table ([0] variance, [8..] lengthscales) or nullptr
  double variance, base;   // base = variance (+ noise for predict_y)
};

// transposed formulation, test points along the rows: Kst = k(Xs, X) (ts x np), mean = Kst alpha (row dots),
// Vt = Kst L^-T as an NT GEMM -- both operands k-contiguous, the GEMM kernel's fastest case; op(B) = L^-T is
// upper triangular, so the K range of a tile ends at its last column and every tile row mixes short and long
// tiles (no tail of long tiles) -- and var = base - row sums of Vt^2.  h->Ks holds 2 x np x tile doubles.
static int exact_predict_inverse(gprx_handle h, const ExactPredictSrc& src, const double* xs_dev, int64_t ns, double* mean_dev, double* var_dev,
                                 int tile) {
  const int np = (int)h->np;
  const int64_t ld = h->np;
  hipStream_t st = h->stream;
  double* Vbuf = h->Ks.p + (size_t)h->np * tile;
  for (int64_t t0 = 0; t0 < ns; t0 += tile) {
    const int ts = (int)std::min<int64_t>(tile, ns - t0);
    const int tsp = (int)round_up(ts, NB);
    KmatArgs ka{xs_dev + t0 * h->d, h->X.p, src.ls_dev, h->Ks.p, ld, ts, (int)h->n, h->d, tsp, np, src.variance, 0.0, 0, 0.0, nullptr, 0};
    if (src.cell_par) {  // hyperparameters of a batch slot: straight from the device table (no upload, no synchronisation)
      ka.cell_par = src.cell_par;
      ka.diag_const = 1;
    }
    HIPCHK(h, launch_kmat(st, h->kid, with_form(ka, h)));
    hipLaunchKernelGGL(rowreduce_kernel, dim3((ts + 3) / 4), dim3(256), 0, st, (const double*)h->Ks.p, ld, src.alpha, ts, np, 0.0, 1.0, mean_dev + t0);
    // Vt is never stored: the GEMM's epilogue leaves the row sums of squares of its tiles (2 slabs per tile column), which
    // the final kernel adds in a fixed order -- 2 x 8 np tile bytes less HBM traffic per tile than storing and re-reading Vt
    // 64 x 64 tiles: operands by LDS-DMA and finer clipping of the triangular K range (measured at N = 4096, 100 000 points:
    // 3.65 M points/s = 61.2 TFLOP/s against 3.35 M with the 128 x 128 register-staged kernel)
    static const int ptile = getenv("GPRX_PREDICT_TILE") ? atoi(getenv("GPRX_PREDICT_TILE")) : 64;
    const int nparts = 2 * ((np + ptile - 1) / ptile);
    HIPCHK(h, launch_gemm(st, 0, 1, tsp, np, np, 1.0, h->Ks.p, ld, src.Xinv, ld, 0.0, Vbuf, ld, GEMM_B_UPPER, ptile, 1, 0, 0, 0, 1, 0, 0, 0, nullptr, 0,
                          Vbuf, (int64_t)tile));
    hipLaunchKernelGGL(rowsq_final_kernel, dim3((ts + 255) / 256), dim3(256), 0, st, (const double*)Vbuf, nparts, (int64_t)tile, ts, src.base, var_dev + t0);
  }
  HIPCHK(h, hipGetLastError());
  return GPRX_OK;
}

int gprx_predict_dev(gprx_handle h, const double* xs_dev, int64_t ns, double* mean_dev, double* var_dev, int include_noise) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (!h->factorized) return fail(h, GPRX_ESTATE, "gprx_predict before a successful gprx_factorize / gprx_objective");
  if (ns < 0 || (ns > 0 && (!xs_dev || !mean_dev || !var_dev))) return fail(h, GPRX_EINVAL, "null argument");
  hipStream_t st = h->stream;
  const int rows_per_chunk = 256;
  if (h->m != 0) return sgpr_predict_batch(h, 1, xs_dev, ns, mean_dev, var_dev, include_noise);  // cell block 0
  const int np = (int)h->np;
  const int64_t ld = h->np;
  const int tile = (int)std::min<int64_t>(pred_tile_for(h->np), round_up(ns, NB));
  // Many test points: V = L^-1 Ks as ONE triangular GEMM per tile against the explicit inverse (computed once
  // per factorisation, N^3/3 flops amortised over N* >= 2 N points) instead of the recursive solve's ~2 N/64
  // dependent launches per tile.  Few points: blocked forward substitution on L itself.
  // Measured at N = 4096 (tools/predict_sizes.py): the substitution path costs ~1.7 ms whatever the batch (2 N / 64
  // dependent launches), the inverse path 0.9 ms for L^-1 plus 0.3 us per point -- faster for every batch size; at larger
  // N the N^3 / 3 flops of L^-1 only pay from about N / 2 points on.  predict_path (gprx_set_tuning): 1 / 2 force a path.
  const int forced = h->predict_path;
  const bool use_inverse = forced == 1 || (forced != 2 && (h->have_linv || h->n <= 4096 || 2 * ns >= (int64_t)h->n));
  if ((rc = ensure(h, h->Ks, sizeof(double) * h->np * tile * (use_inverse ? 2 : 1)))) return rc;
  double* Vbuf = h->Ks.p + (use_inverse ? (size_t)h->np * tile : 0);
  if (use_inverse && !h->have_linv) {
    if ((rc = ensure(h, h->Xinv, sizeof(double) * h->np * ld))) return rc;
    if ((rc = ensure(h, h->Tmp, sizeof(double) * h->np * ld))) return rc;
    HIPCHK(h, hipMemsetAsync(h->Xinv.p, 0, sizeof(double) * h->np * ld, st));
    HIPCHK(h, trtri_lower(st, h->Kmat.p, ld, h->invD.p, h->Xinv.p, ld, h->Tmp.p, ld, np));
    h->have_linv = true;
  }
  const double base = h->variance + (include_noise ? h->noise : 0.0);
  if (use_inverse) {
    const ExactPredictSrc src{h->alpha.p, h->Xinv.p, h->invls.p, nullptr, h->variance, base};
    return exact_predict_inverse(h, src, xs_dev, ns, mean_dev, var_dev, tile);
  }
  const int nchunks = (np + rows_per_chunk - 1) / rows_per_chunk;
  if ((rc = ensure(h, h->pred, sizeof(double) * (size_t)nchunks * tile))) return rc;
  for (int64_t t0 = 0; t0 < ns; t0 += tile) {
    const int ts = (int)std::min<int64_t>(tile, ns - t0);
    const int tsp = (int)round_up(ts, NB);
    KmatArgs ka{h->X.p, xs_dev + t0 * h->d, h->invls.p, h->Ks.p, tile, (int)h->n, ts, h->d, np, tsp, h->variance, 0.0, 0, 0.0, nullptr, 0};
    HIPCHK(h, launch_kmat(st, h->kid, with_form(ka, h)));
    dim3 grid((ts + 255) / 256, nchunks);
    hipLaunchKernelGGL(colreduce_partial, grid, dim3(256), 0, st, h->Ks.p, (int64_t)tile, h->alpha.p, np, ts, rows_per_chunk, h->pred.p);
    hipLaunchKernelGGL(colreduce_final, dim3((ts + 255) / 256), dim3(256), 0, st, h->pred.p, nchunks, ts, 0.0, 1.0, 0, mean_dev + t0);
    HIPCHK(h, trsm_lower_left(st, h->Kmat.p, ld, h->invD.p, h->Ks.p, tile, np, tsp));
    hipLaunchKernelGGL(colreduce_partial, grid, dim3(256), 0, st, (const double*)h->Ks.p, (int64_t)tile, (const double*)nullptr, np, ts, rows_per_chunk,
                       h->pred.p);
    hipLaunchKernelGGL(colreduce_final, dim3((ts + 255) / 256), dim3(256), 0, st, h->pred.p, nchunks, ts, base, -1.0, 0, var_dev + t0);
  }
  HIPCHK(h, hipGetLastError());
  return GPRX_OK;
}

int gprx_predict(gprx_handle h, const double* xs, int64_t ns, double* mean, double* var, int include_noise) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (ns < 0 || (ns > 0 && (!xs || !mean || !var))) return fail(h, GPRX_EINVAL, "null argument");
  if (ns == 0) return GPRX_OK;
  if ((rc = ensure(h, h->xs, sizeof(double) * (ns * h->d + 2 * ns)))) return rc;
  double* dxs = h->xs.p;
  double* dmean = dxs + ns * h->d;
  double* dvar = dmean + ns;
  HIPCHK(h, hipMemcpyAsync(dxs, xs, sizeof(double) * ns * h->d, hipMemcpyHostToDevice, h->stream));
  if ((rc = gprx_predict_dev(h, dxs, ns, dmean, dvar, include_noise))) return rc;
  HIPCHK(h, hipMemcpyAsync(mean, dmean, sizeof(double) * ns, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipMemcpyAsync(var, dvar, sizeof(double) * ns, hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, wait_stream(h, h->stream));
  return GPRX_OK;
}

// ---- device memory helpers ---------------------------------------------------------------------
// Core of gprx_predict_batch: the test points are in device memory (xs_dev) and the results go to device memory
// (means_dev / vars_dev: (count, ns) row-major); asynchronous on the handle's stream after the batched factorisation.
static int predict_batch_core(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs_dev, int64_t ns,
                              double* means_dev, double* vars_dev, int include_noise) {
  int rc;
  hipStream_t st = h->stream;
  if (h->m == 0 && h->d <= CELL_PAR - CELL_PAR_LS) {
    // exact models: all factorisations by one batched launch sequence, then every slot predicts
    if ((rc = gprx_factorize_batch(h, count, units, thetas, 0, nullptr, nullptr))) return rc;
    if (ns == 0) return GPRX_OK;
    const bool use_inverse = h->predict_path != 2 && (h->n <= 4096 || 2 * ns >= (int64_t)h->n);
    if (!use_inverse) {
      for (int i = 0; i < count; ++i) {
        if ((rc = select_slot(h, i))) return rc;
        if ((rc = gprx_predict_dev(h, xs_dev, ns, means_dev + (int64_t)i * ns, vars_dev + (int64_t)i * ns, include_noise))) return rc;
      }
      return GPRX_OK;
    }
    // L^-1 of every slot by batched launches (trtri_lower with the cell index in its grids); each slot then predicts with
    // its alpha / L^-1 / row of the parameter table -- no per-cell upload or synchronisation
    const int np = (int)h->np;
    const int64_t ld = h->np, cs = h->cell_stride, gs = 2 * (int64_t)h->np * h->np;
    const int tile = (int)std::min<int64_t>(PRED_TILE, round_up(ns, NB));
    if ((rc = ensure(h, h->garena, sizeof(double) * (size_t)gs * count))) return rc;
    if ((rc = ensure(h, h->Ks, sizeof(double) * h->np * tile * 2))) return rc;
    for (int c = 0; c < count; ++c) HIPCHK(h, hipMemsetAsync(h->garena.p + (int64_t)c * gs, 0, sizeof(double) * h->np * ld, st));
    HIPCHK(h, trtri_lower(st, h->arena.p, ld, h->arena.p + h->off_invd, h->garena.p, ld, h->garena.p + (int64_t)np * ld, ld, np, count, cs, gs,
                          h->tune.update_tile ? h->tune.update_tile : 64));
    for (int i = 0; i < count; ++i) {
      const Theta& t = h->slot_theta[i];
      const double* cpar = h->cellpar.p + (int64_t)i * CELL_PAR;
      const ExactPredictSrc src{h->arena.p + (int64_t)i * cs + h->off_alpha, h->garena.p + (int64_t)i * gs, nullptr, cpar, t.variance,
                                t.variance + (include_noise ? t.noise : 0.0)};
      if ((rc = exact_predict_inverse(h, src, xs_dev, ns, means_dev + (int64_t)i * ns, vars_dev + (int64_t)i * ns, tile))) return rc;
    }
    h->have_linv = false;  // the single-cell views of the handle may point into the arena: their cached L^-1 is not this batch's
    return GPRX_OK;
  }
  if (h->m != 0 && count > 1 && h->d <= CELL_PAR - CELL_PAR_LS) {
    // sparse models (what gpras runs): every cell factorised by ONE batched launch sequence, then one batched predict
    if (!z) return fail(h, GPRX_EINVAL, "z (inducing inputs) is null for a sparse model");
    const int64_t nz = h->m * h->d;
    for (int64_t e = 0; e < (int64_t)count * nz; ++e)
      if (!std::isfinite(z[e])) return fail(h, GPRX_EINVAL, "z is not finite");
    std::vector<Theta> ts(count);
    for (int i = 0; i < count; ++i) {
      if (units[i] < 0 || units[i] >= h->n_units) return fail(h, GPRX_EINVAL, "unit out of range (call gprx_set_data first)");
      for (int k = 0; k < h->ntheta; ++k)
        if (!std::isfinite(thetas[(int64_t)i * h->ntheta + k])) return fail(h, GPRX_EINVAL, "theta is not finite");
      ts[i] = decode_theta(h, thetas + (int64_t)i * h->ntheta);
    }
    std::vector<double> elbo(count);
    std::vector<int> stv(count);
    if ((rc = sgpr_objective_batch(h, count, units, ts.data(), z, elbo.data(), nullptr, nullptr, stv.data()))) return rc;  // ENOTPD included
    if (ns == 0) return GPRX_OK;
    return sgpr_predict_batch(h, count, xs_dev, ns, means_dev, vars_dev, include_noise);
  }
  for (int i = 0; i < count; ++i) {
    if ((rc = objective_impl(h, units[i], thetas + (int64_t)i * h->ntheta, z ? z + (int64_t)i * h->m * h->d : nullptr, 0, nullptr, nullptr)))
      return rc;
    if ((rc = gprx_predict_dev(h, xs_dev, ns, means_dev + (int64_t)i * ns, vars_dev + (int64_t)i * ns, include_noise))) return rc;
  }
  return GPRX_OK;
}

int gprx_predict_batch_dev(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs_dev, int64_t ns,
                           double* means_dev, double* vars_dev, int include_noise) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (count <= 0 || !units || !thetas || ns < 0 || (ns > 0 && (!xs_dev || !means_dev || !vars_dev))) return fail(h, GPRX_EINVAL, "null argument");
  return predict_batch_core(h, count, units, thetas, z, xs_dev, ns, means_dev, vars_dev, include_noise);
}

int gprx_predict_batch(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs, int64_t ns,
                       double* means, double* vars, int include_noise) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (count <= 0 || !units || !thetas || ns < 0 || (ns > 0 && (!xs || !means || !vars))) return fail(h, GPRX_EINVAL, "null argument");
  // the test points go up ONCE; the (count, ns) results come back in slabs of cells so that the device staging stays small
  // at configs[3]'s size (100 000 points: 1.6 MB per cell)
  const int slab = (int)std::max<int64_t>(1, std::min<int64_t>(count, ((int64_t)1 << 27) / std::max<int64_t>(2 * ns, 1)));
  if ((rc = ensure(h, h->xs, sizeof(double) * (ns * h->d + 2 * ns * slab + 16)))) return rc;
  double* dxs = h->xs.p;
  double* dmean = dxs + ns * h->d;
  double* dvar = dmean + ns * slab;
  if (ns > 0) HIPCHK(h, hipMemcpyAsync(dxs, xs, sizeof(double) * ns * h->d, hipMemcpyHostToDevice, h->stream));
  for (int c0 = 0; c0 < count; c0 += slab) {
    const int cnt = std::min(slab, count - c0);
    if ((rc = predict_batch_core(h, cnt, units + c0, thetas + (int64_t)c0 * h->ntheta, z ? z + (int64_t)c0 * h->m * h->d : nullptr, dxs, ns, dmean, dvar,
                                 include_noise)))
      return rc;
    if (ns > 0) {
      HIPCHK(h, hipMemcpyAsync(means + (int64_t)c0 * ns, dmean, sizeof(double) * ns * cnt, hipMemcpyDeviceToHost, h->stream));
      HIPCHK(h, hipMemcpyAsync(vars + (int64_t)c0 * ns, dvar, sizeof(double) * ns * cnt, hipMemcpyDeviceToHost, h->stream));
    }
    HIPCHK(h, wait_stream(h, h->stream));
  }
  return GPRX_OK;
}

int gprx_predict_batch_t(gprx_handle h, int count, const int* units, const double* thetas, const double* z, const double* xs, int64_t ns,
                         double* means_t, double* vars_t, int include_noise) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  if (count <= 0 || !units || !thetas || ns < 0 || (ns > 0 && (!xs || !means_t || !vars_t))) return fail(h, GPRX_EINVAL, "null argument");
  // as gprx_predict_batch, with every slab of cells transposed on the device before it leaves: the host block is written in its final
  // (ns, count) layout -- whole when all cells fit one slab, by 2-D copies into the slab's columns otherwise
  int slab = (int)std::max<int64_t>(1, std::min<int64_t>(count, ((int64_t)1 << 26) / std::max<int64_t>(2 * ns, 1)));
  if (const char* e = getenv("GPRX_PREDICT_SLAB")) slab = std::max(1, std::min(count, atoi(e)));  // (tests: force the slab-by-slab copies)
  if ((rc = ensure(h, h->xs, sizeof(double) * (ns * h->d + 4 * ns * slab + 16)))) return rc;
  double* dxs = h->xs.p;
  double* dmean = dxs + ns * h->d;
  double* dvar = dmean + ns * slab;
  double* tmean = dvar + ns * slab;
  double* tvar = tmean + ns * slab;
  if (ns > 0) HIPCHK(h, hipMemcpyAsync(dxs, xs, sizeof(double) * ns * h->d, hipMemcpyHostToDevice, h->stream));
  for (int c0 = 0; c0 < count; c0 += slab) {
    const int cnt = std::min(slab, count - c0);
    if ((rc = predict_batch_core(h, cnt, units + c0, thetas + (int64_t)c0 * h->ntheta, z ? z + (int64_t)c0 * h->m * h->d : nullptr, dxs, ns, dmean, dvar,
                                 include_noise)))
      return rc;
    if (ns > 0) {
      launch_transpose_small(h->stream, dmean, cnt, ns, tmean);
      launch_transpose_small(h->stream, dvar, cnt, ns, tvar);
      HIPCHK(h, hipGetLastError());
      if (cnt == count) {
        HIPCHK(h, hipMemcpyAsync(means_t, tmean, sizeof(double) * ns * cnt, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(vars_t, tvar, sizeof(double) * ns * cnt, hipMemcpyDeviceToHost, h->stream));
      } else {
        HIPCHK(h, hipMemcpy2DAsync(means_t + c0, sizeof(double) * count, tmean, sizeof(double) * cnt, sizeof(double) * cnt, (size_t)ns, hipMemcpyDeviceToHost,
                                   h->stream));
        HIPCHK(h, hipMemcpy2DAsync(vars_t + c0, sizeof(double) * count, tvar, sizeof(double) * cnt, sizeof(double) * cnt, (size_t)ns, hipMemcpyDeviceToHost,
                                   h->stream));
      }
    }
    HIPCHK(h, wait_stream(h, h->stream));
  }
  return GPRX_OK;
}

int gprx_mem_info(int device, int64_t* free_bytes, int64_t* total_bytes) {
  if (!free_bytes || !total_bytes) return fail(nullptr, GPRX_EINVAL, "null argument");
  HIPCHK(nullptr, hipSetDevice(device));
  size_t f = 0, t = 0;
  HIPCHK(nullptr, hipMemGetInfo(&f, &t));
  *free_bytes = (int64_t)f;
  *total_bytes = (int64_t)t;
  return GPRX_OK;
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
  if (!out || bytes < 0) return fail(nullptr, GPRX_EINVAL, "bad argument");
  HIPCHK(nullptr, hipSetDevice(device));
  HIPCHK(nullptr, hipMalloc(out, (size_t)std::max<int64_t>(bytes, 16)));
  return GPRX_OK;
}
int gprx_dev_free(int device, void* ptr) {
  HIPCHK(nullptr, hipSetDevice(device));
  HIPCHK(nullptr, hipFree(ptr));
  return GPRX_OK;
}
int gprx_memcpy_h2d(int device, void* dst_dev, const void* src_host, int64_t bytes) {
  HIPCHK(nullptr, hipSetDevice(device));
  HIPCHK(nullptr, copy_sync(dst_dev, src_host, (size_t)bytes, hipMemcpyHostToDevice));
  return GPRX_OK;
}
int gprx_memcpy_d2h(int device, void* dst_host, const void* src_dev, int64_t bytes) {
  HIPCHK(nullptr, hipSetDevice(device));
  HIPCHK(nullptr, copy_sync(dst_host, src_dev, (size_t)bytes, hipMemcpyDeviceToHost));
  return GPRX_OK;
}

// ---- building blocks ----------------------------------------------------------------------------
int gprx_kmat(int device, int kernel_id, const double* a_dev, int64_t n1, const double* b_dev, int64_t n2, int d,
              const double* ls_host, double variance, double diag_add, double* out_dev, int64_t ld, int64_t n1p, int64_t n2p,
              int mode) {
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
}

int gprx_gemm(int device, int ta, int tb, int64_t m, int64_t n, int64_t k, double alpha, const double* a_dev, int64_t lda,
              const double* b_dev, int64_t ldb, double beta, double* c_dev, int64_t ldc, int flags, int tile) {
  if (!a_dev || !b_dev || !c_dev) return fail(nullptr, GPRX_EINVAL, "null argument");
  if (k % 16 || lda % 2 || ldb % 2) return fail(nullptr, GPRX_EINVAL, "k must be a multiple of 16, leading dimensions even");
  if (!((ta == 0 && tb == 1) || (ta == 0 && tb == 0) || (ta == 1 && tb == 0))) return fail(nullptr, GPRX_EINVAL, "unsupported transpose pair");
  if (tile != 0 && tile != 64 && tile != 128) return fail(nullptr, GPRX_EINVAL, "tile must be 0, 64 or 128");
  HIPCHK(nullptr, hipSetDevice(device));
  HIPCHK(nullptr, launch_gemm(util_stream(), ta, tb, (int)m, (int)n, (int)k, alpha, a_dev, lda, b_dev, ldb, beta, c_dev, ldc, flags, tile));
  HIPCHK(nullptr, hipStreamSynchronize(util_stream()));
  return GPRX_OK;
}

int gprx_potrf(int device, double* a_dev, int64_t lda, int64_t np, int64_t extra, double* inv_diag_dev, int* info_host) {
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
}

int gprx_gemm_splitk(int device, int ta, int tb, int64_t m, int64_t n, int64_t k, double alpha, const double* a_dev, int64_t lda,
                     const double* b_dev, int64_t ldb, double beta, double* c_dev, int64_t ldc, double* ws_dev, int kchunk, int cells,
                     int64_t cell_a, int64_t cell_b, int64_t cell_c, int64_t ws_cell, const double* alpha_tab_dev, int alpha_stride) {
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
}

int gprx_trsv_lower(int device, const double* l_dev, int64_t lda, const double* inv_diag_dev, double* b_dev, int64_t np, int transpose,
                    int batch, int64_t cs, double* work_dev) {
  if (const char* why = solve_probe_invalid(l_dev, lda, inv_diag_dev, np, batch, cs)) return fail(nullptr, GPRX_EINVAL, why);
  if (!b_dev || (work_dev && (!transpose || batch != 1))) return fail(nullptr, GPRX_EINVAL, "work is for the transposed solve of one system");
  HIPCHK(nullptr, hipSetDevice(device));
  HIPCHK(nullptr, trsv_lower(util_stream(), l_dev, lda, inv_diag_dev, b_dev, (int)np, transpose != 0, batch, cs, work_dev));
  HIPCHK(nullptr, hipStreamSynchronize(util_stream()));
  return GPRX_OK;
}

int gprx_trsm_lower_left(int device, const double* l_dev, int64_t lda, const double* inv_diag_dev, double* b_dev, int64_t ldb, int64_t n,
                         int64_t ncols, int cells, int64_t cs, const double* src_dev) {
  if (const char* why = solve_probe_invalid(l_dev, lda, inv_diag_dev, n, cells, cs)) return fail(nullptr, GPRX_EINVAL, why);
  if (!b_dev || off16(b_dev) || (src_dev && off16(src_dev))) return fail(nullptr, GPRX_EINVAL, "right-hand side must be given, 16-byte aligned");
  if (ncols <= 0 || ncols > (1 << 30) || ldb < ncols || odd(ldb)) return fail(nullptr, GPRX_EINVAL, "ldb must be even and at least ncols");
  if (src_dev && n != NB) return fail(nullptr, GPRX_EINVAL, "src is for n == 64 only");
  HIPCHK(nullptr, hipSetDevice(device));
  HIPCHK(nullptr, trsm_lower_left(util_stream(), l_dev, lda, inv_diag_dev, b_dev, ldb, (int)n, (int)ncols, cells, cs, src_dev));
  HIPCHK(nullptr, hipStreamSynchronize(util_stream()));
  return GPRX_OK;
}

int gprx_trtri_lower(int device, const double* l_dev, int64_t lda, const double* inv_diag_dev, double* x_dev, int64_t ldx, double* t_dev,
                     int64_t ldt, int64_t np, int cells, int64_t cs_l, int64_t cs_x, int tile) {
  if (const char* why = solve_probe_invalid(l_dev, lda, inv_diag_dev, np, cells, cs_l)) return fail(nullptr, GPRX_EINVAL, why);
  if (!x_dev || !t_dev || off16(x_dev) || off16(t_dev)) return fail(nullptr, GPRX_EINVAL, "X and T must be given, 16-byte aligned");
  if (ldx < np || ldt < np || odd(ldx) || odd(ldt) || odd(cs_x) || cs_x < 0) return fail(nullptr, GPRX_EINVAL, "ldx, ldt, cs_x must be even, rows at least np");
  if (tile != 0 && tile != 64 && tile != 128) return fail(nullptr, GPRX_EINVAL, "tile must be 0, 64 or 128");
  HIPCHK(nullptr, hipSetDevice(device));
  HIPCHK(nullptr, trtri_lower(util_stream(), l_dev, lda, inv_diag_dev, x_dev, ldx, t_dev, ldt, (int)np, cells, cs_l, cs_x, tile));
  HIPCHK(nullptr, hipStreamSynchronize(util_stream()));
  return GPRX_OK;
}

int gprx_transpose_inplace(int device, double* x_dev, int64_t ld, int64_t n, int cells, int64_t cs) {
  if (!x_dev || off16(x_dev)) return fail(nullptr, GPRX_EINVAL, "X must be given, 16-byte aligned");
  if (n <= 0 || n % 64 || n > (1 << 30) || ld < n || odd(ld) || cells < 1 || odd(cs) || cs < 0)
    return fail(nullptr, GPRX_EINVAL, "n must be a positive multiple of 64, ld and cs even");
  HIPCHK(nullptr, hipSetDevice(device));
  HIPCHK(nullptr, transpose_inplace(util_stream(), x_dev, ld, (int)n, cells, cs));
  HIPCHK(nullptr, hipStreamSynchronize(util_stream()));
  return GPRX_OK;
}

int gprx_alpha_from_inverse(int device, const double* x_dev, int64_t ldx, const double* beta_dev, double* part_dev, double* alpha_dev, int64_t np,
                            int cells, int64_t cs_x, int64_t cs_b, int64_t cs_a) {
  if (!x_dev || !beta_dev || !part_dev || !alpha_dev) return fail(nullptr, GPRX_EINVAL, "null argument");
  if (np <= 0 || np % NB || np > (1 << 30) || ldx < np || cells < 1 || cs_x < 0 || cs_b < 0 || cs_a < 0)
    return fail(nullptr, GPRX_EINVAL, "np must be a positive multiple of 64");
  HIPCHK(nullptr, hipSetDevice(device));
  HIPCHK(nullptr, alpha_from_inverse(util_stream(), x_dev, ldx, beta_dev, part_dev, alpha_dev, (int)np, cells, cs_x, cs_b, cs_a));
  HIPCHK(nullptr, hipStreamSynchronize(util_stream()));
  return GPRX_OK;
}

int gprx_reduce_probe(int device, int op, const double* m_dev, int64_t ldm, const double* w_dev, int64_t nrows, int64_t ncols, double base,
                      double scale, int accumulate, double* partial_dev, int rows_per_chunk, double* out_dev, int cells, int64_t m_cell,
                      int64_t w_cell, int64_t p_cell, int64_t out_cell, const double* base_tab_dev, const double* base_tab2_dev, int base_stride) {
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
  else if (k == "poison_workspace" && value >= 0 && value <= 1) t.poison_workspace = value;
  else if (k == "predict_path" && value >= 0 && value <= 2) predict_path = value;
  else if (k == "sgpr_fused" && value >= 0 && value <= 1) fused = value;
  else if (k == "sgpr_resident" && value >= 0 && value <= 1) resident = value;  // 0: sparse optimiser loops are stepped by the host
  else if (k == "wait_handover_us" && value >= 0) wait_handover_us() = value;  // (process-wide whichever entry point sets it)
  else if (k == "sgpr_groups_from" && value >= 0) sf_groups_from() = value;    // (process-wide; 0: the resident Adam loop never splits a batch into groups)
  else return false;
  return true;
}
}  // namespace

int gprx_set_tuning(const char* key, int value) {
  if (!key) return fail(nullptr, GPRX_EINVAL, "null key");
  if (!apply_tuning(potrf_tuning(), predict_path_tuning(), sgpr_fused_tuning(), sgpr_resident_tuning(), key, value)) return fail(nullptr, GPRX_EINVAL, "unknown tuning key or bad value");
  return GPRX_OK;
}

int gprx_set_handle_tuning(gprx_handle h, const char* key, int value) {
  if (!h || !key) return fail(h, GPRX_EINVAL, "null argument");
  const int fused_before = h->sgpr_fused;
  if (!apply_tuning(h->tune, h->predict_path, h->sgpr_fused, h->sgpr_resident, key, value)) return fail(h, GPRX_EINVAL, "unknown tuning key or bad value");
  if (hipSetDevice(h->device) == hipSuccess && hipStreamSynchronize(h->stream) == hipSuccess) drop_graphs(h);  // captured with the old schedule
  if (h->sgpr_fused != fused_before) {  // the cell blocks of the two sparse schedules differ (sgpr_batch_layout): the arena is rebuilt on the next call
    h->sarena_slots = 0;
    if (h->m != 0) h->factorized = false;
  }
  return GPRX_OK;
}

int gprx_mfma_f64_peak(int device, double* tflops) {
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
}

}  // extern "C"
