// GP path, part 1 of 6: the handle (gprx_ctx) and what every other part of the path needs from it -- parameter decoding and the
// per-cell argument checks, priors and the chain rule, the stream wait, graph capture, the resets of resident state, the
// environment switches and the process-wide tuning cells.  Host code only; included by gprx.hip alone, before gp_exact.h.
#pragma once

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
  std::vector<double> yhost;  // y as uploaded (unit-major, np apart): the held-out forms sum a cell's own y.y over its kept rows from it
  Buf hold;                   // device table of a batch's held-out row ranges (gp_sparse.h CellHolds): SF_HOLD_W doubles per cell
  int* info = nullptr;
  double* pin = nullptr;  // pinned host staging: [0..63] lengthscales up, [64..71] reductions down, [72] info (as int),
                          // [74] variance, [75] noise (graph replay reads them through the device block `gparams`)
  double* gparams = nullptr;            // device {variance, noise} for captured kernel-matrix builds
  std::map<int, hipGraphExec_t> graphs;  // unit -> captured single-stream exact factorisation
  std::map<std::pair<int, int>, hipGraphExec_t> sgraphs;  // (cells, with gradient [+ GRAPH_HELD: with the hold table]) -> captured sparse batch evaluation
  bool sgraph_off = false;                                // a capture failed once: this handle stays on eager launches
  std::map<std::pair<int, int>, hipGraphExec_t> rgraphs;  // (cells, optimiser [+ GRAPH_HELD]) -> captured step of the resident loop of the launch sequence
  int sgpr_resident = 1;                                  // sparse models: the optimiser loops stay on the device ("sgpr_resident" tuning key)
  int last_route = 0, last_host_waits = 0;                // gprx_last_optimizer_route
  int last_loeo = 0;                                      // gprx_last_loeo: the last gprx_loeo_batch ran its downdate kernel
  double loeo_ms[4] = {0, 0, 0, 0};                       // ... and its stage times (gprx.h)
  int last_loeo_blocked = 0, loeo_blocked_groups = 0;     // gprx_last_loeo_blocked: the last gprx_loeo_batch_blocked ran to the end, in so many groups
  double loeo_blocked_ms[6] = {0, 0, 0, 0, 0, 0};         // ... and its stage times (gprx.h)
  Buf joint_ws;                                           // gprx_predict_joint_batch_dev: covariance, factorisation scratch and info per cell (gp_joint.h)
  Buf loeo_ws;                                            // its workspace: one slot per (cell, event) of a group (gp_loeo_blocked.h)
  hipEvent_t loeo_ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};  // created by its first call
  int host_waits = 0;                                     // stream waits of the running optimiser call (wait_stream and the loops' own)
  int sgpr_fused = 1;                                     // M <= 64: the five-launch evaluation of sgpr_fused.h ("sgpr_fused" tuning key)
  int held_general = 0;                                   // the held forms also serve the general launch sequence ("held_general" handle tuning key)
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
// ---- environment switches: a plain read; every caller keeps the value in a function-local static, so a variable is read once per
// process (but GPRX_PREDICT_SLAB, which tests change between calls: gprx_predict_batch_t) ----
int env_int(const char* name, int dflt) {
  const char* e = getenv(name);
  return e ? atoi(e) : dflt;
}
bool no_graph() {  // GPRX_NO_GRAPH set (to anything): eager launches wherever a captured graph would be replayed
  static const bool v = getenv("GPRX_NO_GRAPH") != nullptr;
  return v;
}
bool fused_eval() {  // GPRX_FUSED_EVAL=0: an exact evaluation with gradient waits for the factorisation, then differentiates
  static const bool v = env_int("GPRX_FUSED_EVAL", 1) != 0;
  return v;
}
void fill_nan(double* p, int64_t n) { std::fill(p, p + n, std::numeric_limits<double>::quiet_NaN()); }

// acc + sum of y_i^2 of unit u over the rows [r0, r1) of the handle's data, added in row order: the one loop behind gprx_set_data's y.y of
// a unit and a held-out cell's own (its kept rows before and behind the range), so that a cell that holds a suffix out gets the bits of
// a handle that never had those rows
double yy_rows(gprx_handle h, int u, int64_t r0, int64_t r1, double acc) {
  const double* yu = h->yhost.data() + (size_t)u * h->np;
  for (int64_t i = r0; i < r1; ++i) acc += yu[i] * yu[i];
  return acc;
}

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
double ln_logpdf(double u) { return px_ln_logpdf(u); }

constexpr int CELL_RES = 4;  // result row of a batch cell: [0] sum log diag L, [1] |L^-1 y|^2, [2] info (int), [3] unused

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
  static const bool blocking = env_int("GPRX_WAIT_BLOCKING", 0) != 0;
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

// priors and softplus chain rule on the hyperparameter part of a gradient; loss = -(value + log prior)
void chain_rule(gprx_handle h, const Theta& t, int mask, const double* g, double* grad) {
  grad[0] = sgpr_asm_chain(g[0], t.variance, t.w_var, (mask & GPRX_TRAIN_VARIANCE) != 0);
  for (int k = 0; k < h->nlen; ++k)
    grad[1 + k] = sgpr_asm_chain(g[1 + k], t.ls[k], t.w_len[k], (mask & GPRX_TRAIN_LENGTHSCALE) != 0);
  grad[1 + h->nlen] = sgpr_asm_chain(g[1 + h->nlen], t.noise, t.w_noise, (mask & GPRX_TRAIN_NOISE) != 0);
}

// one stream capture at a time in the process (two concurrent thread-local captures on different handles disturbed each other)
std::mutex& capture_mutex() {
  static std::mutex m;
  return m;
}

// What `enqueue` puts on `st`, captured into an executable graph: lock, begin, enqueue, end, instantiate, destroy the graph.
// Relaxed capture mode: another host thread may call a legacy-stream API (hipMemset / hipMemcpy of another handle's set-up)
// while this capture runs; in the global and thread-local modes the runtime refuses that call ("operation would make the
// legacy stream depend on a capturing blocking stream") AND invalidates this capture.  The handle's streams are
// non-blocking, so no implicit dependency on the legacy stream exists that the capture could miss.
// rc: what enqueue returned; e: the first HIP failure; exec: the graph, null unless both are clean.  What a failure means is the
// caller's business (exact_factorize_replay returns it, sgpr_replay goes back to eager launches).
struct Captured { int rc = GPRX_OK; hipError_t e = hipSuccess; hipGraphExec_t exec = nullptr; };
template <class Enqueue>
Captured capture_graph(hipStream_t st, Enqueue enqueue) {
  std::lock_guard<std::mutex> lock(capture_mutex());
  Captured c;
  hipGraph_t graph = nullptr;
  if ((c.e = hipStreamBeginCapture(st, hipStreamCaptureModeRelaxed)) != hipSuccess) return c;
  c.rc = enqueue();
  c.e = hipStreamEndCapture(st, &graph);
  if (!c.rc && c.e == hipSuccess && graph) c.e = hipGraphInstantiate(&c.exec, graph, nullptr, nullptr, 0);
  if (graph) hipGraphDestroy(graph);
  return c;
}

template <class Map>
void drop_graph_map(Map& graphs) {
  for (auto& kv : graphs)
    if (kv.second) hipGraphExecDestroy(kv.second);
  graphs.clear();
}
// Graphs of the general sparse sequence that read the hold table (h->hold) have keys of their own: the second word of the key carries
// GRAPH_HELD.  They hold the table's ADDRESS (its contents are read at replay): whoever moves the buffer drops them.
constexpr int GRAPH_HELD = 2;
void drop_held_graphs(gprx_handle h) {
  for (auto* graphs : {&h->sgraphs, &h->rgraphs})
    for (auto it = graphs->begin(); it != graphs->end();) {
      if ((it->first.second & GRAPH_HELD) != 0) {
        if (it->second) hipGraphExecDestroy(it->second);
        it = graphs->erase(it);
      } else {
        ++it;
      }
    }
}
void drop_graphs(gprx_handle h) {
  drop_graph_map(h->graphs);
  drop_graph_map(h->sgraphs);
  drop_graph_map(h->rgraphs);
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

// the model that predict and the gradient work on from now on; `factorized`: its factors are resident already
void commit_current(gprx_handle h, int unit, const Theta& t, bool factorized) {
  h->factorized = factorized;
  h->cur_unit = unit;
  h->variance = t.variance;
  h->noise = t.noise;
  h->ls = t.ls;
}

// Nothing resident may be used again: the current factorisation, its L^-1, the batch slots and every captured graph.
// slots_emptied (new data): gprx_select_slot answers GPRX_EINVAL, "slot holds no factorisation"; otherwise (another distance
// form) the slots keep their unit and it answers GPRX_ESTATE.
void forget_factorizations(gprx_handle h, bool slots_emptied) {
  h->factorized = false;
  h->have_linv = false;
  std::fill(h->slot_ok.begin(), h->slot_ok.end(), 0);
  if (slots_emptied) std::fill(h->slot_unit.begin(), h->slot_unit.end(), -1);
  drop_graphs(h);
}

int& sgpr_fused_tuning() {
  static int v = 1;
  return v;
}
// 1: the optimiser loops of sparse models (d <= 64) stay on the device; 0: the host-stepped loop for all of them (one process can compare)
int& sgpr_resident_tuning() {
  static int v = 1;
  return v;
}

int check_handle(gprx_handle h) {
  if (!h) return fail(nullptr, GPRX_EINVAL, "null handle");
  hipError_t e = hipSetDevice(h->device);
  if (e != hipSuccess) return fail(h, GPRX_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(e));
  return GPRX_OK;
}

// ---- the per-cell arguments of every evaluation entry point, checked and decoded in one place (include/gprx.h states the order) ----
// one cell; z: its m x d inducing inputs, read for a sparse handle only
int decode_cell(gprx_handle h, int unit, const double* theta, const double* z, Theta& t) {
  if (!theta) return fail(h, GPRX_EINVAL, "theta is null");
  if (unit < 0 || unit >= h->n_units) return fail(h, GPRX_EINVAL, "unit out of range (call gprx_set_data first)");
  for (int k = 0; k < h->ntheta; ++k)
    if (!std::isfinite(theta[k])) return fail(h, GPRX_EINVAL, "theta is not finite");
  if (h->m != 0) {
    if (!z) return fail(h, GPRX_EINVAL, "z (inducing inputs) is null for a sparse model");
    for (int64_t e = 0; e < h->m * h->d; ++e)
      if (!std::isfinite(z[e])) return fail(h, GPRX_EINVAL, "z is not finite");
  }
  decode_theta_into(h, theta, t);
  return GPRX_OK;
}
// `count` cells into out[0 .. count): grown when shorter, never shrunk -- a caller that keeps `out` allocates nothing per call
int decode_cells(gprx_handle h, int count, const int* units, const double* theta, const double* z, std::vector<Theta>& out) {
  if ((int)out.size() < count) out.resize(count);
  const int64_t nz = h->m * h->d;
  int rc;
  for (int i = 0; i < count; ++i)
    if ((rc = decode_cell(h, units[i], theta ? theta + (int64_t)i * h->ntheta : nullptr, z ? z + i * nz : nullptr, out[i]))) return rc;
  return GPRX_OK;
}
}  // namespace
