// GP path: leave-one-event-out prediction of fitted sparse models (M <= 64) on their own training rows -- one batched factorisation, the
// head of the batched predict per tile of events, then the downdate kernel of sf_loeo.h per (event, cell).  After gp_predict.h.  The
// stages are functions of their own: gp_loeo_blocked.h (64 < M <= 320) runs the same ones around another downdate.
#pragma once

namespace {
// Argument errors of gprx_loeo_batch and gprx_loeo_batch_blocked, all found before any device work.  max_mp: the largest padded M the
// caller's downdate takes (NB: the one-workgroup kernel; LOEO_BLOCKED_MAX_MP: the blocked route).
int loeo_check(gprx_handle h, int count, const int* units, const double* thetas, const double* z, int n_events, const int64_t* ev_lo, const int64_t* ev_hi,
               const double* means, const double* vars, const int* status, int max_mp = NB) {
  if (count <= 0 || n_events <= 0 || !units || !thetas || !ev_lo || !ev_hi || !means || !vars || !status) return fail(h, GPRX_EINVAL, "null argument");
  if (h->m == 0) return fail(h, GPRX_EINVAL, "gprx_loeo_batch: exact model (the downdate serves sparse models with M <= 64)");
  if (h->mp > max_mp)
    return fail(h, GPRX_EINVAL, max_mp == NB ? "gprx_loeo_batch: more than 64 inducing points" : "gprx_loeo_batch_blocked: more than 320 inducing points");
  if (h->d > CELL_PAR - CELL_PAR_LS) return fail(h, GPRX_EINVAL, "gprx_loeo_batch: d > 64");
  if (!z) return fail(h, GPRX_EINVAL, "z (inducing inputs) is null for a sparse model");
  int64_t prev = 0;
  for (int e = 0; e < n_events; ++e) {
    if (ev_lo[e] < prev || ev_hi[e] > h->n) return fail(h, GPRX_EINVAL, "gprx_loeo_batch: event ranges must be sorted, disjoint and inside [0, N]");
    if (ev_hi[e] <= ev_lo[e]) return fail(h, GPRX_EINVAL, "gprx_loeo_batch: empty event range");
    if (ev_hi[e] - ev_lo[e] > SGPR_PRED_TILE) return fail(h, GPRX_EINVAL, "gprx_loeo_batch: an event is longer than one predict tile");
    prev = ev_hi[e];
  }
  return GPRX_OK;
}

// The stages both drivers share.  A call: factorize, stage, then per tile head + its own downdate, then finish.
struct LoeoRun {
  SgprLayout L;
  int mp = 0, m = 0, count = 0, n_events = 0;
  int64_t ss = 0, N = 0;
  double* A0 = nullptr;
  const double* cpar = nullptr;
  double *dmean = nullptr, *dvar = nullptr;  // device staging: [means count x N | vars count x N | event table | status]
  int *dtab = nullptr, *dstatus = nullptr;
  std::vector<int> tab, tile_first;          // event table (LOEO_EV ints per event); first event of every tile, then n_events
};

// one batched factorisation of the cells without a gradient (ENOTPD included); *ms: its host time
int loeo_factorize(gprx_handle h, int count, const int* units, const double* thetas, const double* z, double* ms) {
  int rc;
  const auto w0 = std::chrono::steady_clock::now();
  std::vector<Theta> ts;
  if ((rc = decode_cells(h, count, units, thetas, z, ts))) return rc;
  std::vector<double> elbo(count);
  std::vector<int> stv(count);
  if ((rc = sgpr_objective_batch(h, count, units, ts.data(), z, elbo.data(), nullptr, nullptr, stv.data()))) return rc;
  *ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - w0).count();
  return GPRX_OK;
}

// device staging, the tiles and the event table; outputs start as NaN, status as 0
int loeo_stage_run(gprx_handle h, LoeoRun& r, int count, int n_events, const int64_t* ev_lo, const int64_t* ev_hi) {
  int rc;
  hipStream_t st = h->stream;
  r.L = sgpr_batch_layout(h);
  r.mp = (int)h->mp;
  r.m = (int)h->m;
  r.count = count;
  r.n_events = n_events;
  r.ss = r.L.ss;
  r.N = h->n;
  r.A0 = h->sarena.p;
  r.cpar = h->cellpar.p;
  const int tile = SGPR_PRED_TILE;
  const int64_t N = r.N;
  const size_t out_doubles = 2 * (size_t)count * N;
  const size_t n_ints = (size_t)LOEO_EV * n_events + (size_t)count * n_events;
  if ((rc = ensure(h, h->xs, sizeof(double) * out_doubles + sizeof(int) * n_ints + 16))) return rc;
  r.dmean = h->xs.p;
  r.dvar = r.dmean + (size_t)count * N;
  r.dtab = reinterpret_cast<int*>(h->xs.p + out_doubles);
  r.dstatus = r.dtab + (size_t)LOEO_EV * n_events;
  // tiles: consecutive events packed while their span of rows fits one tile; every tile starts and ends on an event boundary
  r.tab.assign((size_t)LOEO_EV * n_events, 0);
  r.tile_first.clear();
  for (int e = 0; e < n_events;) {
    const int64_t t0 = ev_lo[e];
    r.tile_first.push_back(e);
    int j = e;
    while (j < n_events && ev_hi[j] - t0 <= tile) {
      r.tab[(size_t)LOEO_EV * j] = (int)(ev_lo[j] - t0);
      r.tab[(size_t)LOEO_EV * j + 1] = (int)(ev_hi[j] - ev_lo[j]);
      r.tab[(size_t)LOEO_EV * j + 2] = (int)ev_lo[j];
      ++j;
    }
    e = j;
  }
  r.tile_first.push_back(n_events);
  HIPCHK(h, hipMemcpyAsync(r.dtab, r.tab.data(), sizeof(int) * r.tab.size(), hipMemcpyHostToDevice, st));
  HIPCHK(h, hipMemsetAsync(r.dmean, 0xFF, sizeof(double) * out_doubles, st));  // (all bits set: a NaN) rows of no event keep it
  HIPCHK(h, hipMemsetAsync(r.dstatus, 0, sizeof(int) * (size_t)count * n_events, st));
  return GPRX_OK;
}

// the head of sgpr_predict_batch on the training rows [t0, t0 + tsz): Kus, t1 = L^-1 Kus, var = v - colsum(t1^2), t2 = LB^-1 t1 (left in
// every cell's Kus tile)
int loeo_head(gprx_handle h, const LoeoRun& r, int64_t t0, int tsz) {
  hipStream_t st = h->stream;
  const SgprLayout& L = r.L;
  const int mp = r.mp, tile = SGPR_PRED_TILE, count = r.count;
  const int64_t ss = r.ss;
  double* A0 = r.A0;
  const int rows_per_chunk = 256;
  const int nchunks = (mp + rows_per_chunk - 1) / rows_per_chunk;
  const int tsp = (int)round_up(tsz, NB);
  KmatArgs ka{A0 + L.oZ, h->X.p + t0 * h->d, nullptr, A0 + L.oKs, tile, r.m, tsz, h->d, mp, tsp, 0.0, 0.0, 0, 0.0, nullptr, 0};
  ka.cell_par = r.cpar;
  ka.out_stride = ss;
  ka.a_stride = ss;
  ka.diag_const = 1;
  HIPCHK(h, launch_kmat(st, h->kid, with_form(ka, h), count));
  const dim3 pgrid((tsz + 255) / 256, nchunks, count), fgrid((tsz + 255) / 256, count);
  HIPCHK(h, trsm_lower_left(st, A0 + L.oQm, mp, A0 + L.oInvDL, A0 + L.oKs, tile, mp, tsp, count, ss));
  hipLaunchKernelGGL(colreduce_partial, pgrid, dim3(256), 0, st, (const double*)(A0 + L.oKs), (int64_t)tile, (const double*)nullptr, mp, tsz,
                     rows_per_chunk, A0 + L.oPred, ss, (int64_t)0, ss);
  hipLaunchKernelGGL(colreduce_final, fgrid, dim3(256), 0, st, (const double*)(A0 + L.oPred), nchunks, tsz, 0.0, -1.0, 0, r.dvar + t0, ss, r.N, r.cpar,
                     (const double*)nullptr, CELL_PAR);
  HIPCHK(h, trsm_lower_left(st, A0 + L.oBm, mp, A0 + L.oInvDB, A0 + L.oKs, tile, mp, tsp, count, ss));
  return GPRX_OK;
}

// what both downdates read of a tile whose first event is e0
LoeoParams loeo_params(gprx_handle h, const LoeoRun& r, int e0, int include_noise) {
  LoeoParams lp{};
  lp.arena = r.A0;
  lp.ss = r.ss;
  lp.oKs = r.L.oKs;
  lp.oC = r.L.oBm + (int64_t)r.mp * r.mp;
  lp.ldk = SGPR_PRED_TILE;
  lp.cpar = r.cpar;
  lp.Y = h->Y.p;
  lp.np = (int)h->np;
  lp.events = r.dtab + (size_t)LOEO_EV * e0;
  lp.means = r.dmean;
  lp.vars = r.dvar;
  lp.out_stride = r.N;
  lp.status = r.dstatus + e0;
  lp.status_stride = r.n_events;
  lp.include_noise = include_noise ? 1 : 0;
  return lp;
}

// gaps between events back to NaN, `done` recorded, the copies out and one wait
int loeo_finish(gprx_handle h, const LoeoRun& r, const int64_t* ev_lo, const int64_t* ev_hi, hipEvent_t done, double* means, double* vars, int* status) {
  hipStream_t st = h->stream;
  const int64_t N = r.N;
  const int count = r.count, n_events = r.n_events;
  // rows between two events of one tile were written by the tile's variance launch: back to NaN
  for (int e = 0; e + 1 < n_events; ++e)
    if (ev_hi[e] < ev_lo[e + 1])
      HIPCHK(h, hipMemset2DAsync(r.dvar + ev_hi[e], sizeof(double) * N, 0xFF, sizeof(double) * (size_t)(ev_lo[e + 1] - ev_hi[e]), (size_t)count, st));
  HIPCHK(h, hipEventRecord(done, st));
  HIPCHK(h, hipMemcpyAsync(means, r.dmean, sizeof(double) * (size_t)count * N, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(vars, r.dvar, sizeof(double) * (size_t)count * N, hipMemcpyDeviceToHost, st));
  HIPCHK(h, hipMemcpyAsync(status, r.dstatus, sizeof(int) * (size_t)count * n_events, hipMemcpyDeviceToHost, st));
  HIPCHK(h, wait_stream(h, st));
  return GPRX_OK;
}

// means / vars: (count, N) host, row-major; status: (count, n_events) host, 0 or the 1-based failing pivot of chol(H).
int loeo_batch(gprx_handle h, int count, const int* units, const double* thetas, const double* z, int n_events, const int64_t* ev_lo, const int64_t* ev_hi,
               double* means, double* vars, int include_noise, int* status) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  h->last_loeo = 0;
  if ((rc = loeo_check(h, count, units, thetas, z, n_events, ev_lo, ev_hi, means, vars, status))) return rc;
  hipStream_t st = h->stream;
  if ((rc = loeo_factorize(h, count, units, thetas, z, &h->loeo_ms[0]))) return rc;
  LoeoRun r;
  if ((rc = loeo_stage_run(h, r, count, n_events, ev_lo, ev_hi))) return rc;
  HIPCHK(h, hipEventRecord(h->ev[0], st));
  for (size_t ti = 0; ti + 1 < r.tile_first.size(); ++ti) {
    const int e0 = r.tile_first[ti], e1 = r.tile_first[ti + 1];
    const int64_t t0 = ev_lo[e0];
    if ((rc = loeo_head(h, r, t0, (int)(ev_hi[e1 - 1] - t0)))) return rc;
    if (ti == 0) HIPCHK(h, hipEventRecord(h->ev[1], st));
    HIPCHK(h, sf_launch_loeo(st, loeo_params(h, r, e0, include_noise), e1 - e0, count));
    if (ti == 0) HIPCHK(h, hipEventRecord(h->ev[2], st));
  }
  if ((rc = loeo_finish(h, r, ev_lo, ev_hi, h->ev[3], means, vars, status))) return rc;
  float f = 0.f;
  HIPCHK(h, hipEventElapsedTime(&f, h->ev[0], h->ev[1]));
  h->loeo_ms[1] = f;
  HIPCHK(h, hipEventElapsedTime(&f, h->ev[1], h->ev[2]));
  h->loeo_ms[2] = f;
  HIPCHK(h, hipEventElapsedTime(&f, h->ev[0], h->ev[3]));
  h->loeo_ms[3] = f;
  h->last_loeo = 1;
  return GPRX_OK;
}
}  // namespace
