// GP path: leave-one-event-out prediction of fitted sparse models with up to 320 inducing points -- the stages of gp_loeo.h around a
// downdate that keeps H = I - t2 t2^T / s (mp x mp) of every (cell, event) in a workspace slot in device memory: the gram kernel of
// sf_loeo_blocked.hip, the batched Cholesky and triangular inverse over the slots of a group, c' and the apply kernel.  After gp_loeo.h.
#pragma once

namespace {
// Default cap of the workspace: the reference's largest inducing-point option under its usual event count -- 16 modes x 35 events at
// mp = 320, 560 slots of 2.95 MB = 1.65 GB -- still runs as ONE group; a larger batch splits into groups, each of which fills the chip
// many times over, so nothing is gained by holding more.
constexpr double LOEO_BLOCKED_WS_CAP = 2147483648.0;

struct LoeoSlotLayout {
  int64_t oH, oInvD, oP, oT, oStage, oU, oCp, oInfo, stride;  // doubles
};
LoeoSlotLayout loeo_slot_layout(int mp) {
  LoeoSlotLayout s{};
  int64_t o = 0;
  auto take = [&](int64_t n) {
    const int64_t at = o;
    o += n;
    return at;
  };
  s.oH = take((int64_t)mp * mp);
  s.oInvD = take((int64_t)mp * NB);
  s.oP = take((int64_t)mp * mp);
  s.oT = take((int64_t)mp * mp);         // scratch of trtri_lower
  s.oStage = take((int64_t)mp * STAGE_LD);  // staged diagonal blocks of potrf_lower
  s.oU = take(mp);
  s.oCp = take(mp);
  s.oInfo = take(2);
  s.stride = round_up(o, 2);  // (16-byte aligned slots: the GEMMs of the inverse take their operands by LDS-DMA)
  return s;
}

// The schedule of chol(H) over the slots, a function of mp ALONE: 0 = launch sequence with the fused panel, 1 = with the split panel,
// 2 = one workgroup per slot (potrf_cell.h).  potrf_lower's own pickers change route with the number of matrices (split panel from 24,
// cell kernel from 32 / 160 / 256), which would make a result's bits depend on how many events share its group.  Measured with
// tools/loeo_blocked_timing.py at 560 slots (Cholesky plus inverse): one workgroup per slot wins at every mp it serves
// -- mp = 128: 0.163 against 0.191 (fused) / 0.192 ms (split); 192: 0.333 / 0.416 / 0.407; 256: 0.562 / 0.702 / 0.671; 320: 0.888 /
// 1.105 / 1.052 -- and mp = 64 is one panel either way (0.058 / 0.057 ms).
int loeo_blocked_potrf_route(int mp) { return mp == NB ? 1 : 2; }
int& loeo_blocked_potrf_force() {  // "loeo_blocked_potrf" tuning key: -1 = the table above
  static int v = -1;
  return v;
}

int loeo_blocked_batch(gprx_handle h, int count, const int* units, const double* thetas, const double* z, int n_events, const int64_t* ev_lo,
                       const int64_t* ev_hi, double* means, double* vars, int include_noise, int max_slots, int* status) {
  int rc;
  if ((rc = check_handle(h))) return rc;
  h->last_loeo_blocked = 0;
  h->loeo_blocked_groups = 0;
  if ((rc = loeo_check(h, count, units, thetas, z, n_events, ev_lo, ev_hi, means, vars, status, LOEO_BLOCKED_MAX_MP))) return rc;
  if (max_slots < 0) return fail(h, GPRX_EINVAL, "gprx_loeo_batch_blocked: max_slots < 0");
  hipStream_t st = h->stream;
  const int mp = (int)h->mp;
  const LoeoSlotLayout S = loeo_slot_layout(mp);
  // events per group: a run of consecutive events of a tile whose count x events slots fit the cap
  const int64_t cap_slots = max_slots > 0 ? max_slots : (int64_t)(LOEO_BLOCKED_WS_CAP / (sizeof(double) * (double)S.stride));
  const int group_cap = (int)std::max<int64_t>(1, std::min<int64_t>(cap_slots / count, n_events));
  {  // the workspace, before any device work: GPRX_ENOMEM where it does not fit
    const size_t before = h->loeo_ws.bytes;
    if ((rc = ensure(h, h->loeo_ws, sizeof(double) * (size_t)S.stride * count * group_cap, "gprx_loeo_batch_blocked workspace"))) return rc;
    // once per allocation: the tiles of H above the diagonal are never written by this path and must not hold NaN patterns
    if (h->loeo_ws.bytes != before) HIPCHK(h, hipMemsetAsync(h->loeo_ws.p, 0, h->loeo_ws.bytes, st));
  }
  for (auto& ev : h->loeo_ev)
    if (!ev) HIPCHK(h, hipEventCreate(&ev));
  if ((rc = loeo_factorize(h, count, units, thetas, z, &h->loeo_blocked_ms[0]))) return rc;
  LoeoRun r;
  if ((rc = loeo_stage_run(h, r, count, n_events, ev_lo, ev_hi))) return rc;
  const int route = (loeo_blocked_potrf_force() >= 0 && !(loeo_blocked_potrf_force() == 2 && mp == NB)) ? loeo_blocked_potrf_force()
                                                                                                        : loeo_blocked_potrf_route(mp);
  PotrfTuning tune;  // (defaults: neither the handle's knobs nor the process-wide ones)
  tune.split_panel = route == 1 ? 1 : -1;
  tune.cell_kernel = -1;
  double* W0 = h->loeo_ws.p;
  int groups = 0;
  HIPCHK(h, hipEventRecord(h->loeo_ev[0], st));
  for (size_t ti = 0; ti + 1 < r.tile_first.size(); ++ti) {
    const int e0 = r.tile_first[ti], e1 = r.tile_first[ti + 1];
    const int64_t t0 = ev_lo[e0];
    if ((rc = loeo_head(h, r, t0, (int)(ev_hi[e1 - 1] - t0)))) return rc;
    if (ti == 0) HIPCHK(h, hipEventRecord(h->loeo_ev[1], st));
    for (int g0 = e0; g0 < e1; g0 += group_cap, ++groups) {
      const int g1 = std::min(e1, g0 + group_cap), gev = g1 - g0, slots = count * gev;
      const bool first = groups == 0;
      int longest = 0;
      for (int e = g0; e < g1; ++e) longest = std::max(longest, (int)(ev_hi[e] - ev_lo[e]));
      LoeoBlockedParams bp{};
      bp.base = loeo_params(h, r, g0, include_noise);
      bp.mp = mp;
      bp.group_events = gev;
      bp.ws = W0;
      bp.slot_stride = S.stride;
      bp.oH = S.oH;
      bp.oP = S.oP;
      bp.oU = S.oU;
      bp.oCp = S.oCp;
      bp.oInfo = S.oInfo;
      HIPCHK(h, sf_launch_loeo_gram(st, bp, count));
      if (first) HIPCHK(h, hipEventRecord(h->loeo_ev[2], st));
      int* info0 = reinterpret_cast<int*>(W0 + S.oInfo);
      if (route == 2)
        HIPCHK(h, potrf_cells(st, W0 + S.oH, mp, mp, 0, W0 + S.oInvD, info0, slots, S.stride, (int)(2 * S.stride)));
      else
        HIPCHK(h, potrf_lower(st, W0 + S.oH, mp, mp, 0, W0 + S.oInvD, info0, W0 + S.oStage, nullptr, nullptr, slots, S.stride, (int)(2 * S.stride), &tune));
      // (tile 64 whatever the number of slots: launch_gemm's own choice changes with it)
      HIPCHK(h, trtri_lower(st, W0 + S.oH, mp, W0 + S.oInvD, W0 + S.oP, mp, W0 + S.oT, mp, mp, slots, S.stride, S.stride, 64));
      if (first) HIPCHK(h, hipEventRecord(h->loeo_ev[3], st));
      HIPCHK(h, sf_launch_loeo_cprime(st, bp, count));
      HIPCHK(h, sf_launch_loeo_apply(st, bp, (longest + NB - 1) / NB, count));
      if (first) HIPCHK(h, hipEventRecord(h->loeo_ev[4], st));
    }
  }
  if ((rc = loeo_finish(h, r, ev_lo, ev_hi, h->loeo_ev[5], means, vars, status))) return rc;
  for (int s = 1; s <= 4; ++s) {
    float f = 0.f;
    HIPCHK(h, hipEventElapsedTime(&f, h->loeo_ev[s - 1], h->loeo_ev[s]));
    h->loeo_blocked_ms[s] = f;
  }
  float f = 0.f;
  HIPCHK(h, hipEventElapsedTime(&f, h->loeo_ev[0], h->loeo_ev[5]));
  h->loeo_blocked_ms[5] = f;
  h->loeo_blocked_groups = groups;
  h->last_loeo_blocked = 1;
  return GPRX_OK;
}
}  // namespace
