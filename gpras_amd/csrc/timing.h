// Event timing of a peak ensemble: per (member, cell) of ONE event the row of the peak, and per threshold the number of rows above it and
// the first of them.  With y[t] the value pca_ensemble_peaks_kernel forms at row t of a member:
//   t_peak      = the row of the first maximum by the rule of ens_take (a NaN is the maximum and sticks): np.argmax(y)
//   duration[j] = #{t : y[t] > thr[j]}          (strict, as the exceedance counts; a NaN row is not counted)
//   arrival[j]  = min{t : y[t] > thr[j]}, or the sentinel rows_e when no row exceeds
// in rows counted from the event's first.  They go out as one int32 block timing (members, n_maps, cells), n_maps = 1 + 2 n_thr: map 0
// t_peak, map 1 + j duration[j], map 1 + n_thr + j arrival[j]; consecutive threads write consecutive cells.  rows_e <= 2^31 - 2.
//
// pca_ensemble_timing_kernel: the mapping, staging, prefetch and per-row arithmetic of pca_ensemble_peaks_kernel (ensemble.h) with the
// integers carried beside pk -- per row and threshold one compare, one add and one minimum next to KMAX fmas and a division.  It writes
// peak (members, cells) too, bit for bit the peaks kernel's, so that a call that wants both walks the rows once.  Nothing is carried from
// one member to the next: the maps do not depend on the grouping.  The thresholds are kernel arguments (uniform: scalar registers).
// gfx950 (profiles/ensemble_resources.txt): no scratch in either instantiation, <64> at two waves per SIMD as the peaks kernel.
//
// field_member_timing_kernel: the same maps from a resident field (members * rows_e, cells), beside field_member_peaks_kernel: the last
// step of route="refield", and with one member the observed maps of the truth.
//
// member_timing_stats_kernel: statistics over the members of a contiguous range of maps, one thread per (map, cell), every loop in member
// order; integers throughout, so every result is exact.
#pragma once
#include "ensemble.h"

namespace gprx {

struct TimingArgs {
  EnsembleArgs e;  // e.peak may not be null
  int n_thr;
  double thr[ENS_TMAX];
  int* timing;  // (members, 1 + 2 n_thr, cells)
};

// what ens_take decides: whether row y replaces the running maximum pk
__device__ __forceinline__ bool tm_takes(double pk, double y, bool first) { return first || (!(pk != pk) && (y > pk || y != y)); }

// the integers of one member's walk
struct TimingState {
  int tpk, dur[ENS_TMAX], arr[ENS_TMAX];
  __device__ __forceinline__ void reset(int rows_e) {
    tpk = 0;
#pragma unroll
    for (int j = 0; j < ENS_TMAX; ++j) dur[j] = 0, arr[j] = rows_e;
  }
  // row t with value y; n_thr is uniform over the launch
  __device__ __forceinline__ void row(int t, double y, bool takes, int n_thr, const double* thr) {
    tpk = takes ? t : tpk;
#pragma unroll
    for (int j = 0; j < ENS_TMAX; ++j) {
      if (j >= n_thr) break;
      const bool ex = y > thr[j];
      dur[j] += ex ? 1 : 0;
      const int cand = ex ? t : arr[j];
      arr[j] = cand < arr[j] ? cand : arr[j];
    }
  }
  // the member's maps: map m of cell c at out[m * cells + c]
  __device__ __forceinline__ void store(int* out, int64_t cells, int64_t c, int n_thr) const {
    out[c] = tpk;
#pragma unroll
    for (int j = 0; j < ENS_TMAX; ++j) {
      if (j >= n_thr) break;
      out[(int64_t)(1 + j) * cells + c] = dur[j];
      out[(int64_t)(1 + n_thr + j) * cells + c] = arr[j];
    }
  }
};

template <int KMAX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void pca_ensemble_timing_kernel(TimingArgs q) {
  // (the walk of pca_ensemble_peaks_kernel, statement by statement; see there)
  constexpr int RSTEP = 256 / KMAX, NST = PCA_RB / RSTEP;
  __shared__ double sM[PCA_RB][KMAX];
  const EnsembleArgs& p = q.e;
  const int tid = threadIdx.x;
  const int64_t c = (int64_t)blockIdx.x * 256 + tid;
  const bool live = c < p.cells;
  const int k = p.k, n_thr = q.n_thr, rows_i = (int)p.rows_e;
  const int64_t n_maps = 1 + 2 * (int64_t)n_thr;
  double e[KMAX];
  const double wc = live ? p.w[c] : 1.0, b = live ? p.base[c] : 0.0, el = (live && p.depth_mode) ? p.elev[c] : 0.0;
#pragma unroll
  for (int kk = 0; kk < KMAX; ++kk) e[kk] = (live && kk < k) ? p.Eb[(int64_t)kk * p.lde + c] : 0.0;
  const int kk0 = tid % KMAX, r0 = tid / KMAX;
  const bool kok = kk0 < k;
  const double xsk = kok ? p.xs[kk0] : 0.0, xmk = kok ? p.xm[kk0] : 0.0;
  const int64_t s0 = (int64_t)blockIdx.y * p.group;
  const int64_t s1 = s0 + p.group < p.members ? s0 + p.group : p.members;
  double v[NST];
  auto fetch = [&](int64_t sm, int64_t t0) {
    const double* rows = p.scores + sm * p.rows_e * k;
#pragma unroll
    for (int i = 0; i < NST; ++i) {
      const int64_t t = t0 + r0 + i * RSTEP;
      v[i] = (kok && t < p.rows_e) ? rows[t * k + kk0] : 0.0;
    }
  };
  int64_t sm = s0, t0 = 0;
  if (sm < s1) fetch(sm, t0);
  double pk = 0.0;
  TimingState ts;
  ts.reset(rows_i);
  while (sm < s1) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NST; ++i) sM[r0 + i * RSTEP][kk0] = v[i] * xsk + xmk;
    __syncthreads();
    const bool last = t0 + PCA_RB >= p.rows_e;  // of this member
    const int64_t smn = last ? sm + 1 : sm, t0n = last ? 0 : t0 + PCA_RB;
    if (smn < s1) fetch(smn, t0n);
    const int nr = (int)((p.rows_e - t0 < PCA_RB) ? p.rows_e - t0 : PCA_RB);
    const int tb = (int)t0;
    for (int r = 0; r < nr; ++r) {
      double s = 0.0;
#pragma unroll
      for (int kk = 0; kk < KMAX; ++kk) s = __builtin_fma(sM[r][kk], e[kk], s);
      const double y = ens_finish(s, wc, b, el, p.depth_mode);
      const bool first = t0 == 0 && r == 0;
      ts.row(tb + r, y, tm_takes(pk, y, first), n_thr, q.thr);
      pk = ens_take(pk, y, first);
    }
    if (last) {
      if (live) {
        p.peak[sm * p.cells + c] = pk;
        ts.store(q.timing + sm * n_maps * p.cells, p.cells, c, n_thr);
      }
      ts.reset(rows_i);
    }
    sm = smn;
    t0 = t0n;
  }
}

// The last step of the refield route for the timing maps: member blockIdx.y of a resident field (members * rows_e, cells), one thread per
// cell.  peak (members, cells) may be null; where given it is field_member_peaks_kernel's.
struct FieldTimingArgs {
  const double* f;
  int64_t rows_e, cells;
  int n_thr;
  double thr[ENS_TMAX];
  double* peak;
  int* timing;  // (members, 1 + 2 n_thr, cells)
};
__global__ __launch_bounds__(256) void field_member_timing_kernel(FieldTimingArgs p) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= p.cells) return;
  const int64_t sm = blockIdx.y;
  const double* col = p.f + sm * p.rows_e * p.cells + c;
  TimingState ts;
  ts.reset((int)p.rows_e);
  double pk = 0.0;
  for (int64_t t = 0; t < p.rows_e; ++t) {
    const double y = col[t * p.cells];
    ts.row((int)t, y, tm_takes(pk, y, t == 0), p.n_thr, p.thr);
    pk = ens_take(pk, y, t == 0);
  }
  if (p.peak) p.peak[sm * p.cells + c] = pk;
  ts.store(p.timing + sm * (1 + 2 * (int64_t)p.n_thr) * p.cells, p.cells, c, p.n_thr);
}

constexpr int TM_LMAX = 8;  // levels of the distribution function per call

struct TimingStatsArgs {
  const int* timing;  // (members, n_maps, cells)
  int64_t members, cells;
  int n_maps, map0;   // the maps map0 .. map0 + gridDim.y - 1
  int rows_e, sentinel;
  int n_lev, n_rank;
  int level[TM_LMAX];
  int rank[ENS_RMAX];
  const int* obs;     // (n_sel, cells) or null
  int* cdf;           // (n_sel, n_lev, cells)
  int* n_valid;       // (n_sel, cells)
  long long* sum;     // (n_sel, cells)
  int* order;         // (n_sel, n_rank, cells)
  int *below, *equal; // (n_sel, cells), with obs
};

// One thread per (map, cell) with v_s = timing[s, map, c], s = 0 .. members - 1, values in [0, rows_e]:
//   cdf[l] = #{s : v_s <= level[l]};  n_valid = #{s : v_s != sentinel} and sum = the sum of v_s over those members (sentinel -1: none);
//   below = #{v_s < obs}, equal = #{v_s == obs};
//   order[j] = np.sort(v)[rank[j]] -- the smallest x with #{v_s <= x} >= rank[j] + 1, found by bisection on the value range [0, rows_e]:
//   ceil(log2(rows_e + 1)) passes over the members, every rank halving its own interval in each.  (The arrival maps' sentinel rows_e
//   is their largest value, so it sorts last.)
__global__ __launch_bounds__(256) void member_timing_stats_kernel(TimingStatsArgs p) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= p.cells) return;
  const int64_t m = blockIdx.y;
  const int64_t stride = (int64_t)p.n_maps * p.cells;
  const int* col = p.timing + (p.map0 + m) * p.cells + c;
  const bool has_obs = p.obs != nullptr;
  const int ob = has_obs ? p.obs[m * p.cells + c] : 0;
  int cnt[TM_LMAX];
#pragma unroll
  for (int l = 0; l < TM_LMAX; ++l) cnt[l] = 0;
  int valid = 0, below = 0, equal = 0;
  long long sum = 0;
  for (int64_t s = 0; s < p.members; ++s) {
    const int v = col[s * stride];
    const bool ok = v != p.sentinel;
    valid += ok ? 1 : 0;
    sum += ok ? (long long)v : 0ll;
    below += v < ob ? 1 : 0;
    equal += v == ob ? 1 : 0;
#pragma unroll
    for (int l = 0; l < TM_LMAX; ++l) {
      if (l >= p.n_lev) break;
      cnt[l] += v <= p.level[l] ? 1 : 0;
    }
  }
#pragma unroll
  for (int l = 0; l < TM_LMAX; ++l)
    if (l < p.n_lev) p.cdf[(m * p.n_lev + l) * p.cells + c] = cnt[l];
  p.n_valid[m * p.cells + c] = valid;
  p.sum[m * p.cells + c] = sum;
  if (has_obs) {
    p.below[m * p.cells + c] = below;
    p.equal[m * p.cells + c] = equal;
  }
  if (p.n_rank == 0) return;
  int lo[ENS_RMAX], hi[ENS_RMAX];
#pragma unroll
  for (int j = 0; j < ENS_RMAX; ++j) lo[j] = 0, hi[j] = p.rows_e;
  int passes = 0;
  while (((long long)1 << passes) < (long long)p.rows_e + 1) ++passes;
  for (int pass = 0; pass < passes; ++pass) {
    int mid[ENS_RMAX], le[ENS_RMAX];
#pragma unroll
    for (int j = 0; j < ENS_RMAX; ++j) mid[j] = lo[j] + ((hi[j] - lo[j]) >> 1), le[j] = 0;
    for (int64_t s = 0; s < p.members; ++s) {
      const int v = col[s * stride];
#pragma unroll
      for (int j = 0; j < ENS_RMAX; ++j) {
        if (j >= p.n_rank) break;
        le[j] += v <= mid[j] ? 1 : 0;
      }
    }
#pragma unroll
    for (int j = 0; j < ENS_RMAX; ++j) {
      if (j >= p.n_rank) break;
      if (le[j] >= p.rank[j] + 1) hi[j] = mid[j];
      else lo[j] = mid[j] + 1;
    }
  }
#pragma unroll
  for (int j = 0; j < ENS_RMAX; ++j)
    if (j < p.n_rank) p.order[(m * p.n_rank + j) * p.cells + c] = lo[j];
}

}  // namespace gprx
