// Peak ensembles: members of a joint predictive distribution pushed through the field chain of ONE event, reduced to the event's peak
// per (member, cell) without a field ever being written, and the statistics over the members.
//
// pca_ensemble_peaks_kernel.  A member is rows_e rows of EOF scores, member s in rows [s rows_e, (s + 1) rows_e) of the (members rows_e, k)
// block pca_reverse_kernel reads.  A thread owns one cell and keeps its e[kk], weight, base and elevation in registers; a workgroup owns
// 256 cells (blockIdx.x) and `group` consecutive members (blockIdx.y) and walks each member's rows in blocks of PCA_RB with the rows' mode
// values in LDS, as pca_reverse_kernel does.  Per row the operations are those of the chain in their order: the mode sum with one fma per
// mode in the order kk = 0, 1, ... over all KMAX terms (pca_reverse_kernel; the same KMAX is instantiated for the same k), s / w + base,
// the two steps of field_to_depth_kernel with contraction off, then the first maximum by the rule of metrics.h.  Nothing is carried
// from one member to the next, so peak[s, c] does not depend on the grouping.  Only peak (members, cells) is written: consecutive
// threads, consecutive cells.
//
// What bounds it: every fma takes one 8-byte LDS operand that all lanes of the wave share (a broadcast read).  A wave's read costs
// 2 LDS cycles per double (ds_read_b64, or 4 per ds_read_b128 of two), the CU's LDS serves one read at a time, and its four SIMDs
// together retire one wave-wide fp64 fma per cycle: the LDS reads cap the kernel at half the fp64 vector rate.  Measured at 3 010 rows x
// 100 000 cells, K = 50, 256 members: 0.24 of that rate in useful fmas.  gfx950: <64> 192 VGPRs, 16 KiB of LDS, two
// waves per SIMD; <16> 80 VGPRs, six waves; no scratch.
//
// member_cell_stats_kernel, member_area_kernel, member_area_sum_kernel: the statistics over the members, all in fixed orders.
//
// ensemble_normals_kernel: the standard normals of an event drawn by address (normals.h: Philox4x64-10, AS 241), in place of the host
// generator and its upload.  gfx950: 122 VGPRs, four waves per SIMD, no scratch, no LDS.
#pragma once
#include "gprx_common.h"
#include "normals.h"
#include "pca.h"

namespace gprx {

constexpr int ENS_TMAX = 8;     // thresholds per call
constexpr int ENS_RMAX = 8;     // order statistics per call
constexpr int ENS_SMAX = 4096;  // members the statistics take

struct EnsembleArgs {
  const double* scores;  // (members * rows_e, k)
  int64_t members, rows_e, cells;
  int k;
  const double* Eb;  // (k, lde)
  int64_t lde;
  const double *w, *base, *xm, *xs, *elev;
  int depth_mode;  // 0: none, 1: max(y - el, 0), 2: max((y + el) - el, 0)
  int group;       // members per workgroup
  double* peak;    // (members, cells)
};

// s / w + base, then the two steps of field_to_depth_kernel (contraction off, as there)
__device__ __forceinline__ double ens_finish(double s, double wc, double b, double el, int depth_mode) {
  double y = s / wc + b;
  if (depth_mode) {
    {
#pragma clang fp contract(off)
      if (depth_mode == 2) y = y + el;
      y = y - el;
    }
    y = y < 0.0 ? 0.0 : y;
  }
  return y;
}
// the first maximum; a NaN is taken as the maximum and sticks (metrics.h)
__device__ __forceinline__ double ens_take(double pk, double y, bool first) {
  const bool take = first || (!(pk != pk) && (y > pk || y != y));
  return take ? y : pk;
}

template <int KMAX>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2))) void pca_ensemble_peaks_kernel(EnsembleArgs p) {
  // staging: thread tid owns mode tid % KMAX of the rows tid / KMAX + i RSTEP of a block
  constexpr int RSTEP = 256 / KMAX, NST = PCA_RB / RSTEP;
  __shared__ double sM[PCA_RB][KMAX];
  const int tid = threadIdx.x;
  const int64_t c = (int64_t)blockIdx.x * 256 + tid;
  const bool live = c < p.cells;
  const int k = p.k;
  double e[KMAX];
  const double wc = live ? p.w[c] : 1.0, b = live ? p.base[c] : 0.0, el = (live && p.depth_mode) ? p.elev[c] : 0.0;
#pragma unroll
  for (int kk = 0; kk < KMAX; ++kk) e[kk] = (live && kk < k) ? p.Eb[(int64_t)kk * p.lde + c] : 0.0;
  const int kk0 = tid % KMAX, r0 = tid / KMAX;
  const bool kok = kk0 < k;
  const double xsk = kok ? p.xs[kk0] : 0.0, xmk = kok ? p.xm[kk0] : 0.0;
  const int64_t s0 = (int64_t)blockIdx.y * p.group;
  const int64_t s1 = s0 + p.group < p.members ? s0 + p.group : p.members;
  // the mode values of block (member sm, rows from t0) on their way to LDS: fetched while the block before is worked on
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
  while (sm < s1) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NST; ++i) sM[r0 + i * RSTEP][kk0] = v[i] * xsk + xmk;  // (modes >= k: zeros; rows past the event's end are not read)
    __syncthreads();
    const bool last = t0 + PCA_RB >= p.rows_e;  // of this member
    const int64_t smn = last ? sm + 1 : sm, t0n = last ? 0 : t0 + PCA_RB;
    if (smn < s1) fetch(smn, t0n);
    const int nr = (int)((p.rows_e - t0 < PCA_RB) ? p.rows_e - t0 : PCA_RB);
    for (int r = 0; r < nr; ++r) {
      double s = 0.0;
#pragma unroll
      for (int kk = 0; kk < KMAX; ++kk) s = __builtin_fma(sM[r][kk], e[kk], s);
      pk = ens_take(pk, ens_finish(s, wc, b, el, p.depth_mode), t0 == 0 && r == 0);
    }
    if (last && live) p.peak[sm * p.cells + c] = pk;
    sm = smn;
    t0 = t0n;
  }
}

// Draws into score rows: scores[(s rows_e + t) k + kk] = mean[kk, t] + W[kk, s, t], mean (k, rows_e), W (k, members, tp) = Zn Lc^T of the
// batched GEMM (its columns t >= rows_e belong to the identity padding of Lc and are dropped).  One plain addition per element.
__global__ __launch_bounds__(256) void ensemble_pack_kernel(const double* __restrict__ mean, const double* __restrict__ W, int64_t members, int64_t rows_e,
                                                            int64_t tp, int k, double* __restrict__ scores) {
  const int64_t total = members * rows_e * k;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int kk = (int)(i % k);
    const int64_t st = i / k, s = st / rows_e, t = st - s * rows_e;
    scores[i] = mean[(int64_t)kk * rows_e + t] + W[((int64_t)kk * members + s) * tp + t];
  }
}

// The standard normals of one event, made where they are used: zn (k, members, tp), zn[kk, sl, t] = the draw of address (seed, stream, event,
// mode kk, member member0 + sl, row t) of normals.h for t < rows_e, an exact zero beyond (those columns meet the identity padding of Lc).
// A thread owns one Philox block, four consecutive t of one (kk, sl) -- tp is a multiple of 64, so no block straddles a row -- and writes
// its 32 bytes with two 16-byte stores: consecutive lanes, consecutive 32 bytes.  Blocks wholly in the padding skip the generator.
// pair_offset = h > 0: the absolute member s >= h reads the counter of member s - h and flips the sign bit (-z bit for bit).  raw: the
// 64-bit words of the counter read instead of the normals, the sign flip left out.
struct NormalsArgs {
  uint64_t seed, stream;
  int64_t event, member0, members, pair_offset, rows_e, tp;
  int k, raw;
  unsigned long long* zn;  // (k, members, tp): doubles, or the words when raw
};
__global__ __launch_bounds__(256) void ensemble_normals_kernel(NormalsArgs p) {
  const int64_t bpr = p.tp >> 2;  // blocks per (mode, member) row
  const int64_t total = (int64_t)p.k * p.members * bpr;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i % bpr, ks = i / bpr, sl = ks % p.members, kk = ks / p.members;
    int64_t s = p.member0 + sl;
    const bool negate = p.pair_offset > 0 && s >= p.pair_offset;
    if (negate) s -= p.pair_offset;
    const int64_t t0 = b << 2;
    unsigned long long out[4] = {0ull, 0ull, 0ull, 0ull};
    if (t0 < p.rows_e) {
      uint64_t w[4];
      nrm_block(p.seed, p.stream, (uint64_t)p.event, (uint64_t)kk, (uint64_t)s, (uint64_t)t0, w);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (t0 + j >= p.rows_e) continue;
        if (p.raw) {
          out[j] = w[j];
        } else {
          const unsigned long long zb = (unsigned long long)__double_as_longlong(nrm_normal(w[j]));
          out[j] = negate ? zb ^ 0x8000000000000000ull : zb;
        }
      }
    }
    ulonglong2* dst = reinterpret_cast<ulonglong2*>(p.zn + (i << 2));  // (the block (kk, sl, b) starts at element 4 i; 16-byte aligned with zn)
    dst[0] = make_ulonglong2(out[0], out[1]);
    dst[1] = make_ulonglong2(out[2], out[3]);
  }
}
// z[i] = the normal of word w[i] by the same inline transform: the way in for words no draw reaches (the far tail r > 5 needs u < 1.4e-11)
__global__ __launch_bounds__(256) void ensemble_normal_transform_kernel(const unsigned long long* __restrict__ w, int64_t n, double* __restrict__ z) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) z[i] = nrm_normal((uint64_t)w[i]);
}

// The last step of the refield route: peak[s, c] = the first maximum over the rows_e rows of member s of a resident field
// (members * rows_e, cells), by the rule of metrics.h.
__global__ __launch_bounds__(256) void field_member_peaks_kernel(const double* __restrict__ f, int64_t rows_e, int64_t cells, double* __restrict__ peak) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  const int64_t sm = blockIdx.y;
  const double* col = f + sm * rows_e * cells + c;
  double pk = col[0];
  for (int64_t t = 1; t < rows_e; ++t) {
    const double y = col[t * cells];
    if (!(pk != pk) && (y > pk || y != y)) pk = y;
  }
  peak[sm * cells + c] = pk;
}

// The order-preserving 64-bit key of a double: ascending keys are ascending values, -0 before +0, every NaN last (np.sort's order).
__device__ __forceinline__ unsigned long long ens_key(double x) {
  if (x != x) return ~0ull;
  const unsigned long long u = (unsigned long long)__double_as_longlong(x);
  return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double ens_unkey(unsigned long long key) {
  const unsigned long long u = (key >> 63) ? (key & 0x7fffffffffffffffull) : ~key;
  return __longlong_as_double((long long)u);
}

struct MemberStatsArgs {
  const double* peak;  // (members, cells)
  int64_t members, cells;
  int n_thr, n_rank;
  double thr[ENS_TMAX];
  int rank[ENS_RMAX];
  int* exceed;    // (n_thr, cells)
  double* mean;   // (cells)
  double* std;    // (cells)
  double* order;  // (n_rank, cells)
};

// One thread per cell, every loop in member order s = 0 .. members - 1: the counts of peak > thr[j] (strict), the plain sum / members,
// the squared deviations from that mean in a second pass (each a rounded product, then a rounded addition: no fma) with
// std = sqrt(sum / members), and the order statistics by a bitwise binary search on the keys: 64 passes over the members, each rank
// keeping its own prefix -- at bit b a rank counts the members whose key agrees with its prefix above b and has bit b clear, and
// takes the 1 branch when its remaining rank is not among them.  The value found is one of the member's own values, exactly.
__global__ __launch_bounds__(256) void member_cell_stats_kernel(MemberStatsArgs p) {
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= p.cells) return;
  const double* col = p.peak + c;
  int cnt[ENS_TMAX];
#pragma unroll
  for (int j = 0; j < ENS_TMAX; ++j) cnt[j] = 0;
  double sum = 0.0;
  for (int64_t s = 0; s < p.members; ++s) {
    const double x = col[s * p.cells];
    sum += x;
#pragma unroll
    for (int j = 0; j < ENS_TMAX; ++j) cnt[j] += (j < p.n_thr && x > p.thr[j]) ? 1 : 0;
  }
  const double mu = sum / (double)p.members;
  double dev = 0.0;
  for (int64_t s = 0; s < p.members; ++s) {
#pragma clang fp contract(off)
    const double d = col[s * p.cells] - mu;
    const double d2 = d * d;
    dev = dev + d2;
  }
#pragma unroll
  for (int j = 0; j < ENS_TMAX; ++j)
    if (j < p.n_thr) p.exceed[(int64_t)j * p.cells + c] = cnt[j];
  p.mean[c] = mu;
  p.std[c] = sqrt(dev / (double)p.members);
  if (p.n_rank == 0) return;
  unsigned long long prefix[ENS_RMAX];
  int left[ENS_RMAX];
#pragma unroll
  for (int j = 0; j < ENS_RMAX; ++j) {
    prefix[j] = 0ull;
    left[j] = j < p.n_rank ? p.rank[j] : 0;
  }
  for (int bit = 63; bit >= 0; --bit) {
    const unsigned long long above = bit == 63 ? 0ull : (~0ull << (bit + 1));
    int zero[ENS_RMAX];
#pragma unroll
    for (int j = 0; j < ENS_RMAX; ++j) zero[j] = 0;
    for (int64_t s = 0; s < p.members; ++s) {
      const unsigned long long key = ens_key(col[s * p.cells]);
      const bool clear = !((key >> bit) & 1ull);
#pragma unroll
      for (int j = 0; j < ENS_RMAX; ++j) {
        if (j >= p.n_rank) break;  // (uniform: only the ranks asked for are counted)
        zero[j] += (clear && (key & above) == prefix[j]) ? 1 : 0;
      }
    }
#pragma unroll
    for (int j = 0; j < ENS_RMAX; ++j) {
      if (left[j] >= zero[j]) {
        left[j] -= zero[j];
        prefix[j] |= 1ull << bit;
      }
    }
  }
#pragma unroll
  for (int j = 0; j < ENS_RMAX; ++j)
    if (j < p.n_rank) p.order[(int64_t)j * p.cells + c] = ens_unkey(prefix[j]);
}

// part[(s, j), blockIdx.x] = sum over the workgroup's 256 cells of area[c] [peak[s, c] > thr[j]]: a wave's 64 lanes in the order of
// wave_sum_dpp, then the four waves in their order.  area null: every area is 1.0, the sum is an exact count.
struct MemberAreaArgs {
  const double* peak;
  const double* area;
  int64_t members, cells;
  int n_thr;
  double thr[ENS_TMAX];
  double* part;  // (members, n_thr, gridDim.x)
};
__global__ __launch_bounds__(256) void member_area_kernel(MemberAreaArgs p) {
  __shared__ double sred[ENS_TMAX][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t c = (int64_t)blockIdx.x * 256 + tid, sm = blockIdx.y;
  const bool live = c < p.cells;
  const double x = live ? p.peak[sm * p.cells + c] : 0.0;
  const double a = live ? (p.area ? p.area[c] : 1.0) : 0.0;
#pragma unroll
  for (int j = 0; j < ENS_TMAX; ++j) {
    if (j >= p.n_thr) break;
    const double r = wave_sum_dpp((live && x > p.thr[j]) ? a : 0.0);
    if (lane == 0) sred[j][wave] = r;
  }
  __syncthreads();
  if (tid < p.n_thr) p.part[(sm * p.n_thr + tid) * gridDim.x + blockIdx.x] = ((sred[tid][0] + sred[tid][1]) + sred[tid][2]) + sred[tid][3];
}
// wet_area[i] = sum over the workgroups of part[i, b], b ascending: one thread per (member, threshold)
__global__ __launch_bounds__(256) void member_area_sum_kernel(const double* __restrict__ part, int nblk, int64_t total, double* __restrict__ wet_area) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  double s = 0.0;
  for (int bq = 0; bq < nblk; ++bq) s += part[i * nblk + bq];
  wet_area[i] = s;
}

}  // namespace gprx
