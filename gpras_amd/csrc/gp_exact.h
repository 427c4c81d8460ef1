// GP path, part 2 of 6: the exact model -- the single, replayed, batched and one-workgroup-per-cell factorisations, the batch
// arena and its slots, the gradients, and the small kernels these launch.  Included by gprx.hip after gp_ctx.h.
#pragma once

namespace {
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

// ---- exact GP ------------------------------------------------------------------------------------
// K = k(X,X) + s I (lower tiles) with y appended as row np; potrf gives L and beta = L^-1 y in that
// row; alpha by the backward solve; red[0] = sum log diag L, red[1] = |beta|^2.
int ensure_event_pair(gprx_handle h, hipEvent_t (&ev)[2]) {
  if (ev[0]) return GPRX_OK;
  HIPCHK(h, hipEventCreate(&ev[0]));
  HIPCHK(h, hipEventCreate(&ev[1]));
  return GPRX_OK;
}
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
    if ((rc = ensure_event_pair(h, h->kev))) return rc;
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
  commit_current(h, unit, t, false);
  return GPRX_OK;
}

// Throughput mode (gprx_factorize_many with several cells): the ~250 launches of one single-stream fit are
// captured once per (handle, unit) into a hipGraph and replayed; only the pinned parameter block changes.
// Measured on MI355X with 16 cells of N = 4096 in flight: 784 fits/s eager, 800 fits/s replayed -- the limit is
// the device (4 hardware queues, each cell ~1.8x slower under 4-way sharing), the replay mainly frees the host.
int exact_factorize_replay(gprx_handle h, int unit, const Theta& t) {
  if (h->d > 64 || h->profiling || no_graph()) return exact_factorize_enqueue(h, unit, t, false);
  auto it = h->graphs.find(unit);
  if (it == h->graphs.end()) {
    // buffers must exist before capture: a first eager pass allocates them (and is a valid fit by itself)
    if (!h->Kmat.p || !h->invD.p || !h->alpha.p || !h->dstage.p) return exact_factorize_enqueue(h, unit, t, false);
    std::memcpy(h->pin, t.ls.data(), sizeof(double) * h->d);
    h->pin[74] = t.variance;
    h->pin[75] = t.noise;
    const Captured c = capture_graph(h->stream, [&] { return exact_factorize_enqueue(h, unit, t, false, true); });
    if (c.rc) return c.rc;
    HIPCHK(h, c.e);  // (a capture that fails is an error here: sgpr_replay, which has an eager form of the same call, carries on)
    it = h->graphs.emplace(unit, c.exec).first;
  }
  std::memcpy(h->pin, t.ls.data(), sizeof(double) * h->d);
  h->pin[74] = t.variance;
  h->pin[75] = t.noise;
  HIPCHK(h, hipGraphLaunch(it->second, h->stream));
  h->dag_used = false;  // a replayed fit is always the launch-per-panel schedule ("dag" applies to eager single factorisations only)
  commit_current(h, unit, t, false);
  return GPRX_OK;
}

void summarize_profile(gprx_handle h) {
  double gemm_ms = 0.0, gemm_flops = 0.0, panel_ms = 0.0, strip_ms = 0.0, strip_flops = 0.0;
  auto sum_marks = [&](const auto& marks, double& ms_sum, double& flops) {
    for (auto& mk : marks) {
      ms_sum += elapsed_ms(h->prof.pool[mk.first], h->prof.pool[mk.first + 1]);
      flops += mk.second;
    }
  };
  sum_marks(h->prof.gemm_marks, gemm_ms, gemm_flops);
  sum_marks(h->prof.strip_marks, strip_ms, strip_flops);
  for (auto idx : h->prof.panel_marks) panel_ms += elapsed_ms(h->prof.pool[idx], h->prof.pool[idx + 1]);
  h->prof_out[0] = gemm_ms;
  h->prof_out[1] = (double)h->prof.gemm_marks.size();
  h->prof_out[2] = gemm_flops;
  h->prof_out[3] = panel_ms;
  h->prof_out[4] = (double)h->prof.panel_marks.size();
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
  if ((rc = ensure_event_pair(h, h->bev))) return rc;
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
  // One launch sequence for all cells on the handle's stream.  (Tried and removed, DESIGN.md 7b.2: two groups of cells on two streams,
  // the panel launches of one overlapping the MFMA-bound updates of the other -- at N = 4096 +2.5 % at 32 cells, +3 % at 64, nothing at
  // 16, -5 % at 8: not worth per-launch timings that depend on what the other stream happens to run.)
  HIPCHK(h, hipEventRecord(h->bev[0], st));
  HIPCHK(h, hipMemcpyAsync(h->cellpar.p, par, sizeof(double) * CELL_PAR * count, hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemsetAsync(h->cellres.p, 0, sizeof(double) * CELL_RES * count, st));
  if (h->profiling) h->prof.reset();
  double* K0 = h->arena.p;
  const double* cpar = h->cellpar.p;
  double* cres = h->cellres.p;
  KmatArgs ka{h->X.p, h->X.p, nullptr, K0, ld, (int)h->n, (int)h->n, h->d, np, np, 0.0, 0.0, 1, 1.0, nullptr, 0};
  ka.cell_par = cpar;
  ka.out_stride = cs;
  // (under profiling the launch sequence is instrumented launch by launch; the cell kernel -- ONE launch -- is timed when the handle
  // forces it, "cell_kernel" = 1: gprx_last_cell_kernel)
  const bool cell_kernel = use_cell_kernel(h->tune, np, count) && (!h->profiling || h->tune.cell_kernel > 0);
  // (opt-in, GPRX_CELL_BUILD_K=1: the column-pair cell kernel evaluates K where it consumes it -- no build launch, nothing written but the
  // right-hand-side rows)
  const bool cell_builds_k = cell_kernel && potrf_cells_builds_k(h->kid, h->dist_form, np, h->d);
  if (h->profiling) {
    if ((rc = ensure_event_pair(h, h->kev))) return rc;
    HIPCHK(h, hipEventRecord(h->kev[0], st));
  }
  if (!cell_builds_k) HIPCHK(h, launch_kmat(st, h->kid, with_form(ka, h), count));
  if (h->profiling) {
    HIPCHK(h, hipEventRecord(h->kev[1], st));
    h->kmat_bytes = 8.0 * KM_T * KM_T * (double)(np / KM_T) * (np / KM_T + 1) / 2 * count;
  }
  // (the column-pair cell kernel carries the right-hand side as a vector: one row, of which it reads and writes the first np entries)
  // (so does the launch sequence's split panel: potrf_rows_kernel<..., YVEC>)
  const bool rhs_vector = !cell_kernel && potrf_rhs_vector_ok(h->tune, count);
  const bool beta_vector = rhs_vector || (cell_kernel && !cell_builds_k && potrf_cells_beta_vector(np, NB, false));
  hipLaunchKernelGGL(set_rhs_rows_batch_kernel, dim3(beta_vector ? 4 : 64, count), dim3(256), 0, st, K0 + (int64_t)np * ld, ld, (const double*)h->Y.p, cpar,
                     (int)h->n, np, beta_vector ? 1 : NB, cs);
  int* info0 = reinterpret_cast<int*>(cres + 2);
  if (cell_kernel) {
    // small matrices in many cells: one workgroup owns one cell from the first column to the last (potrf_cell.h)
    if (h->profiling) {
      if ((rc = ensure_event_pair(h, h->cev))) return rc;
      HIPCHK(h, hipEventRecord(h->cev[0], st));
    }
    if (cell_builds_k)
      HIPCHK(h, potrf_cells(st, K0, ld, np, NB, K0 + h->off_invd, info0, count, cs, 2 * CELL_RES, 0, h->X.p, cpar, (int)h->n, h->d));
    else
      HIPCHK(h, potrf_cells(st, K0, ld, np, NB, K0 + h->off_invd, info0, count, cs, 2 * CELL_RES));
    if (h->profiling) {
      HIPCHK(h, hipEventRecord(h->cev[1], st));
      h->cev_recorded = true;
      h->cell_cells = count;
      h->cell_flops = (double)np * np * np / 3.0 * count;  // algorithmic: N^3 / 3 per cell (the right-hand-side rows' N^2 not counted)
    }
  } else {
    HIPCHK(h, potrf_lower(st, K0, ld, np, rhs_vector ? 0 : NB, K0 + h->off_invd, info0, K0 + h->off_stage, h->profiling ? &h->prof : nullptr, nullptr, count, cs,
                          2 * CELL_RES, &h->tune, 0, rhs_vector ? K0 + (int64_t)np * ld : nullptr));
  }
  const double* beta = K0 + (int64_t)np * ld;
  if (with_alpha) hipLaunchKernelGGL(copy_row_batch_kernel, dim3((np + 255) / 256, count), dim3(256), 0, st, beta, K0 + h->off_alpha, np, cs);
  hipLaunchKernelGGL(logdet_quad_kernel, dim3(count), dim3(256), 0, st, (const double*)K0, ld, beta, np, cres, cs, CELL_RES);
  if (with_alpha) HIPCHK(h, trsv_lower(st, K0, ld, K0 + h->off_invd, K0 + h->off_alpha, np, true, count, cs));  // (else: exact_gradient_batch)
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
  commit_current(h, h->slot_unit[slot], t, true);
  h->have_linv = false;
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
  // K^-1 = X^T X (X = L^-1) on the lower tiles, as the TN product on LDS-DMA operands.  (Until round 3 X was transposed in place and
  // L^-T multiplied with itself as an NT product -- one more pass over X, 5.9 ms per 128 cells of N = 4096; the same sums in the same k
  // order, so the values are unchanged: DESIGN.md 7b.)
  HIPCHK(h, launch_gemm(st, 1, 0, np, np, np, 1.0, X0, ld, X0, ld, 0.0, T0, ld, GEMM_C_LOWER | GEMM_A_UPPER | GEMM_B_LOWER, 64, count, gs, gs, gs));
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
  for (int c = 0; c < count; ++c)
    if (h->slot_ok[c]) exact_gradient_collect(h, host.data() + (size_t)c * width, g + (size_t)c * h->ntheta);
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
  h->have_linv = false;  // (Xinv is not zeroed above its diagonal: a later predict forms L^-1 again)
  HIPCHK(h, launch_gemm(st, 1, 0, np, np, np, 1.0, h->Xinv.p, ld, h->Xinv.p, ld, 0.0, h->Tmp.p, ld, GEMM_C_LOWER | GEMM_A_UPPER | GEMM_B_LOWER, 64));
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
int exact_gradient(gprx_handle h, const Theta& t, double* g) {
  std::vector<double> host(2 + h->d);
  int rc;
  if ((rc = exact_gradient_enqueue(h, t, host.data(), false))) return rc;
  HIPCHK(h, wait_stream(h, h->stream));
  exact_gradient_collect(h, host.data(), g);
  return GPRX_OK;
}
}  // namespace
