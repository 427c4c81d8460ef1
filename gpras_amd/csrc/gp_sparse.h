// GP path, part 3 of 6: the sparse model (SGPR) -- cell layout, arena and pinned staging, the fused five-launch evaluation and the
// general launch sequence (stage-in, body, stage-out), graph replay, the batched objective and predict.  After gp_exact.h.
#pragma once

namespace {
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

// ---- held-out rows (gprx_*_held: the folds of a cross-validation as cells of one batch) ----
// lo / hi: `count` values each; cell i's model does not see the training rows [lo[i], hi[i]) (lo == hi: it sees all).  A default-
// constructed value -- what every entry point without "_held" passes -- holds nothing.
struct CellHolds {
  const int64_t* lo = nullptr;
  const int64_t* hi = nullptr;
  bool any(int count) const {  // some cell holds at least one row
    if (!lo || !hi) return false;
    for (int i = 0; i < count; ++i)
      if (hi[i] != lo[i]) return true;
    return false;
  }
  CellHolds from(int cell0) const { return lo && hi ? CellHolds{lo + cell0, hi + cell0} : CellHolds{}; }
};

// The argument check of the held forms, before any device work: the handle is one the five fused launches serve -- or, with the handle
// tuning key "held_general" = 1, any sparse handle with d <= 64: the general launch sequence then masks the rows as well (sgpr_held.hip) --
// every range lies in [0, n] with lo <= hi, and every cell keeps a row.
int check_holds(gprx_handle h, int count, const int64_t* lo, const int64_t* hi) {
  const bool general = h->held_general != 0;
  if (!lo || !hi) return fail(h, GPRX_EINVAL, "hold_lo / hold_hi is null");
  if (h->m == 0) return fail(h, GPRX_EINVAL, "held-out rows: exact model (the held forms serve sparse models on the five fused launches)");
  if (!general && h->m > NB) return fail(h, GPRX_EINVAL, "held-out rows: more than 64 inducing points (the held forms serve M <= 64)");
  if (h->d > CELL_PAR - CELL_PAR_LS) return fail(h, GPRX_EINVAL, "held-out rows: more than 64 features (the held forms serve d <= 64)");
  if (!general && !sgpr_five_launches(h))
    return fail(h, GPRX_EINVAL, "held-out rows: \"sgpr_fused\" = 0 (the general launch sequence holds no rows out)");
  char msg[200];
  for (int i = 0; i < count; ++i) {
    if (lo[i] > hi[i]) {
      snprintf(msg, sizeof msg, "cell %d: hold_lo %lld > hold_hi %lld", i, (long long)lo[i], (long long)hi[i]);
      return fail(h, GPRX_EINVAL, msg);
    }
    if (lo[i] < 0 || hi[i] > h->n) {
      snprintf(msg, sizeof msg, "cell %d: held range [%lld, %lld) outside [0, %lld]", i, (long long)lo[i], (long long)hi[i], (long long)h->n);
      return fail(h, GPRX_EINVAL, msg);
    }
    if (hi[i] - lo[i] >= h->n) {
      snprintf(msg, sizeof msg, "cell %d: held range [%lld, %lld) keeps no row", i, (long long)lo[i], (long long)hi[i]);
      return fail(h, GPRX_EINVAL, msg);
    }
  }
  return GPRX_OK;
}

// The table the kernels read (SfParams::hold), SF_HOLD_W doubles per cell: [lo, hi, rows kept, y.y of the kept rows].  y.y is summed over
// the kept rows in row order with gprx_set_data's loop (yy_rows) -- not y.y of the unit minus the held part, which rounds differently:
// a cell that holds a suffix out gets the bits of a handle created on the rows in front of it.
void hold_table(gprx_handle h, int count, const int* units, const CellHolds& holds, std::vector<double>& tab) {
  tab.resize((size_t)count * SF_HOLD_W);
  for (int i = 0; i < count; ++i) {
    const int64_t lo = holds.lo[i], hi = holds.hi[i];
    double* row = &tab[(size_t)i * SF_HOLD_W];
    row[0] = (double)lo;
    row[1] = (double)hi;
    row[2] = (double)(h->n - (hi - lo));
    row[3] = yy_rows(h, units[i], hi, h->n, yy_rows(h, units[i], 0, lo, 0.0));
  }
}

// the table onto the device, in stream order; `tab` must live until the stream has passed the copy.  A table that outgrows its buffer
// moves: the captured sequences that read it are dropped first (the stream is idle between calls: every evaluation ends with a wait).
int hold_upload(gprx_handle h, const std::vector<double>& tab) {
  int rc;
  if (h->hold.bytes < sizeof(double) * tab.size()) {
    HIPCHK(h, hipStreamSynchronize(h->stream));
    drop_held_graphs(h);
  }
  if ((rc = ensure(h, h->hold, sizeof(double) * tab.size()))) return rc;
  HIPCHK(h, hipMemcpyAsync(h->hold.p, tab.data(), sizeof(double) * tab.size(), hipMemcpyHostToDevice, h->stream));
  return GPRX_OK;
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
  static int v = env_int("GPRX_SF_GROUPS_FROM", 17);
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
  if (p.hold) p.hold += (int64_t)cell0 * SF_HOLD_W;
  if (cell0 != 0) p.stamps = nullptr;
  return p;
}

int sgpr_fused_enqueue(gprx_handle h, int count, const SgprLayout& L, bool want_grad, const double* hold_dev = nullptr) {
  hipStream_t st = h->stream;
  const SgprStage sg = sgpr_stage(h, count, L);
  SfParams p = sgpr_fused_params(h, L, want_grad);
  p.hold = hold_dev;
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
// hold_dev (here and in the body): the batch's hold table on the device when a cell holds rows out -- the stage-in and the Kuf build are
// then their twins of sgpr_held.hip, which write the held entries of y and the held columns of P as exact zeros; every other launch is
// the one it always was.  Null: today's launches.
int sgpr_stage_in_enqueue(gprx_handle h, int count, const SgprLayout& L, const double* hold_dev = nullptr) {
  const int np = (int)h->np, m = (int)h->m, d = h->d;
  const SgprStage sg = sgpr_stage(h, count, L);
  double* A0 = h->sarena.p;
  static_assert(CELL_RES <= 256 && CELL_PAR <= 256, "sgpr_stage_in_kernel moves them with its first workgroup");
  if (hold_dev != nullptr) {
    HIPCHK(h, sgpr_launch_stage_in_held(h->stream, (std::max(np, m * d) + 255) / 256, count, (const double*)h->Y.p, np,
                                        (const double*)(h->spin + sg.par), CELL_PAR, h->cellpar.p, (const double*)(h->spin + sg.z), m * d, A0 + L.oZ,
                                        A0 + L.oY, L.ss, h->cellres.p, CELL_RES, hold_dev));
    return GPRX_OK;
  }
  hipLaunchKernelGGL(sgpr_stage_in_kernel, dim3((std::max(np, m * d) + 255) / 256, count), dim3(256), 0, h->stream, (const double*)h->Y.p, np,
                     (const double*)(h->spin + sg.par), CELL_PAR, h->cellpar.p, (const double*)(h->spin + sg.z), m * d, A0 + L.oZ, A0 + L.oY, L.ss,
                     h->cellres.p, CELL_RES);
  return GPRX_OK;
}

int sgpr_body_enqueue(gprx_handle h, int count, const SgprLayout& L, bool want_grad, const SgprParSrc& ps, const double* hold_dev = nullptr) {
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
  if (hold_dev != nullptr)
    HIPCHK(h, launch_kmat_pair_held(st, h->kid, with_form(kp, h), with_form(kq, h), count, hold_dev));
  else
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

int sgpr_batch_enqueue(gprx_handle h, int count, const SgprLayout& L, bool want_grad, const SgprParSrc& ps, const double* hold_dev = nullptr) {
  if (sgpr_five_launches(h)) return sgpr_fused_enqueue(h, count, L, want_grad, hold_dev);
  int rc;
  if (hold_dev != nullptr && ps.table == nullptr) return fail(h, GPRX_EINVAL, "held-out rows: d > 64");  // (check_holds refuses it first)
  if ((rc = sgpr_stage_in_enqueue(h, count, L, hold_dev))) return rc;
  if ((rc = sgpr_body_enqueue(h, count, L, want_grad, ps, hold_dev))) return rc;
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
  hipStream_t st = h->stream;
  *replayed = false;
  if (no_graph() || h->sgraph_off || h->profiling) return GPRX_OK;
  auto it = graphs.find(key);
  if (it == graphs.end()) {
    graphs.emplace(key, nullptr);
    return GPRX_OK;
  }
  if (it->second == nullptr) {
    // (capture_graph: relaxed mode, serialised over the process; a capture that fails anyway is abandoned and the handle stays on
    // eager launches)
    const Captured c = capture_graph(st, enqueue);
    if (c.rc || c.e != hipSuccess || !c.exec) {
      (void)hipGetLastError();
      h->err.clear();
      h->sgraph_off = true;
      graphs.erase(it);
      return GPRX_OK;
    }
    it->second = c.exec;
  }
  HIPCHK(h, hipGraphLaunch(it->second, st));
  *replayed = true;
  return GPRX_OK;
}

// elbo_out[c] (NaN if a Cholesky failed), g: count x ntheta constrained-parameter derivatives, gz: count x m x d (host);
// g / gz may be null (loss only).  status[c]: GPRX_OK / GPRX_ENOTPD.  holds: checked by the caller (check_holds); a batch in which no
// cell holds a row takes the launches without the table -- and, on the general sequence, the graphs without it: a held sequence is
// captured under a key of its own (GRAPH_HELD), and reads the table's contents, uploaded in front of every call, at replay.
int sgpr_objective_batch(gprx_handle h, int count, const int* units, const Theta* ts, const double* zs, double* elbo_out, double* g, double* gz,
                         int* status, const CellHolds& holds = CellHolds{}) {
  const SgprLayout L = sgpr_batch_layout(h);
  int rc;
  std::vector<double> htab;  // (lives until the wait below)
  const bool held = holds.any(count);
  if (held) {
    hold_table(h, count, units, holds, htab);
    if ((rc = hold_upload(h, htab))) return rc;
  }
  const double* hold_dev = held ? h->hold.p : nullptr;
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
      (rc = sgpr_replay(h, h->sgraphs, {count, (want_grad ? 1 : 0) + (held ? GRAPH_HELD : 0)},
                        [&] { return sgpr_batch_enqueue(h, count, L, want_grad, ps, hold_dev); }, &replayed)))
    return rc;
  if (!replayed && (rc = sgpr_batch_enqueue(h, count, L, want_grad, ps, hold_dev))) return rc;
  const double* hres = h->spin + sg.res;
  const double* hred = h->spin + sg.red;
  const double* hsum = h->spin + sg.sum;
  const double* hdz = h->spin + sg.dz;
  HIPCHK(h, wait_stream(h, st));
  h->factorized = false;  // (objective_impl sets it for a lone model: cell block 0 is then what gprx_predict reads)
  int first_error = GPRX_OK;
  for (int c = 0; c < count; ++c) {
    // (a cell that holds rows out: its own row count and y.y, the values its row of the table carries to the resident loop)
    const double nn = held ? htab[(size_t)c * SF_HOLD_W + 2] : (double)h->n;
    const double yy = held ? htab[(size_t)c * SF_HOLD_W + 3] : h->yy[units[c]];
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
    elbo_out[c] = sgpr_asm_elbo(nn, yy, v, s, red);  // (sgpr_asm.h: the resident Adam loop forms the same sums on the device)
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
}  // namespace
