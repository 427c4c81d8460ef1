// GP path, part 4 of 6: the two device-resident optimiser loops of sparse models (around the fused evaluation, around the general
// launch sequence) and the state layout, window and stop-flag reads they share.  Included by gprx.hip after gp_sparse.h.
#pragma once

namespace {
// ---- what the two resident optimiser loops below share ------------------------------------------------------------------------------
// steps between two reads of the stop flags
int resident_check_every() {
  static const int v = env_int("GPRX_ADAM_CHECK_EVERY", 0);
  return v > 0 ? v : 25;
}

// Grows the device state block of the resident loops.  The captured steps of sgpr_resident_general (h->rgraphs) hold addresses inside
// it: whoever reallocates it drops them (the stream is idle: every optimiser call ends with a synchronisation).
int ensure_adam_dev(gprx_handle h, size_t bytes) {
  if (h->adam_dev.bytes >= bytes) return GPRX_OK;
  drop_graph_map(h->rgraphs);
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
// holds (checked by the caller): cells that hold rows out carry their table row through every launch of every step -- each group of cells
// its own part of the table (sf_params_from) -- and the closing launch takes the cell's own row count and y.y from it.
int sgpr_resident_fused(gprx_handle h, int kind, int count, const int* units, double* theta, double* z, int mask, int max_iter, double* losses,
                        int* n_evals, int* batches, const CellHolds& holds = CellHolds{}) {
  const SgprLayout L = sgpr_batch_layout(h);
  int rc;
  if ((rc = ensure_sarena(h, count, L))) return rc;
  hipStream_t st = h->stream;
  std::vector<double> htab;  // (lives until the synchronisation behind the initial state)
  const bool held = holds.any(count);
  if (held) {
    hold_table(h, count, units, holds, htab);
    if ((rc = hold_upload(h, htab))) return rc;
  }
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
  p.hold = held ? h->hold.p : nullptr;
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
// holds (checked by the caller; "held_general" = 1): every opening of a residency uploads the table rows of the cells that still run, in
// their new slots; the stage-in, the Kuf build and the step kernel are then their twins of sgpr_held.hip, and the step is captured under a
// key of its own (GRAPH_HELD).  A residency in which no running cell holds a row takes the launches and graphs without the table -- as
// the host-stepped loop does, which hands the running cells' ranges to the held objective.
int sgpr_resident_general(gprx_handle h, int kind, int count, const int* units, double* theta, double* z, int mask, int max_iter, double* losses,
                          int* n_evals, int* batches, const CellHolds& holds = CellHolds{}) {
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
    // the running cells' ranges and units, in their slots of this residency
    std::vector<int64_t> a_lo(na, 0), a_hi(na, 0);
    std::vector<int> a_units(na);
    std::vector<double> htab;  // (lives until the synchronisation behind the stage-in)
    for (int j = 0; j < na; ++j) {
      a_units[j] = units[active[j]];
      if (holds.lo && holds.hi) {
        a_lo[j] = holds.lo[active[j]];
        a_hi[j] = holds.hi[active[j]];
      }
    }
    const CellHolds a_holds{a_lo.data(), a_hi.data()};
    const bool held = a_holds.any(na);
    if (held) {
      hold_table(h, na, a_units.data(), a_holds, htab);
      if ((rc = hold_upload(h, htab))) return rc;
    }
    const double* hold_dev = held ? h->hold.p : nullptr;
    Theta row_theta;
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
      decode_theta_into(h, theta + (size_t)i * nt, row_theta);
      sgpr_par_row(h, h->spin + sg.par + (size_t)j * CELL_PAR, units[i], row_theta);
      std::memcpy(h->spin + sg.z + (size_t)j * nz, z + (size_t)i * nz, sizeof(double) * nz);
    }
    std::memcpy(&hd[rs.o_yy], h->yy.data(), sizeof(double) * h->n_units);
    HIPCHK(h, hipMemcpyAsync(h->adam_dev.p, hd.data(), sizeof(double) * rs.n_dbl, hipMemcpyHostToDevice, st));
    HIPCHK(h, hipMemcpyAsync(ad.stale, hi.data(), sizeof(int) * rs.n_int, hipMemcpyHostToDevice, st));
    if ((rc = sgpr_stage_in_enqueue(h, na, L, hold_dev))) return rc;
    HIPCHK(h, hipGetLastError());
    ++h->host_waits;
    HIPCHK(h, hipStreamSynchronize(st));  // (the host vectors and the pinned rows are free again)
    const SgprStep sa = sgpr_step_params(h, L, reinterpret_cast<const int*>(rs.win + check_every));
    auto step_enqueue = [&]() -> int {
      int erc;
      if ((erc = sgpr_body_enqueue(h, na, L, true, ps, hold_dev))) return erc;
      HIPCHK(h, sgpr_launch_step(st, kind, sa, ad, na, hold_dev));
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
        if ((rc = sgpr_replay(h, h->rgraphs, {na, kind + (held ? GRAPH_HELD : 0)}, step_enqueue, &replayed))) return rc;
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
}  // namespace
