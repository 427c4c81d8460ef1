// The numerics inside the reference's diagnostic plots (gpras/utils/plotting.py: performance_cdf :201-233, performance_scatterplot
// :155-198, map_detection_categories :716-859) on the device: a radix sort of fp64 keys, a rank gather, a scatter summary and the
// per-event detection codes.  DESIGN.md section 3.18.
//
// SORT.  LSD radix sort of 64-bit unsigned keys, 8 bits per pass, least significant byte first, ping-pong between two buffers.
//   key          a raw key, or bits(fabs(a[i] - b[i])) built where it is read (one subtraction and one sign clear, contraction off):
//                with the sign clear the unsigned order of the bit patterns is the numeric order, +inf after every finite value, every
//                NaN after +inf (where np.sort puts them), -0.0 becomes +0.0, and a denormal residual is an ordinary small key (fp64
//                denormals are never flushed).  No key array is materialised before the first executed pass: that pass reads the pair.
//   histograms   one sweep (dg_hist_kernel) builds the key and counts all eight digits: 8 x 256 counters in LDS per workgroup, flushed
//                with 64-bit integer global atomics (integer sums do not depend on the order: deterministic).  Residuals of one field
//                share their top bytes, so a wave first peels up to two wave-wide digit values (one LDS add for all their lanes)
//                before the remaining lanes add one by one.
//   pass skip    the host reads the 8 x 256 histogram; a pass whose digit has exactly ONE non-empty bin would move nothing and is
//                skipped.  With P executed passes the first one writes into the output when P is odd and into the workspace when P is
//                even, so that the last one always lands in the output; P = 0 copies (or builds) the keys into the output.
//   a pass       dg_count_kernel: the digit counts of every tile of DG_TILE consecutive keys, counts[digit][tile] (32-bit);
//                dg_scan_kernel: offs[digit][tile] = (keys of smaller digits, from the histogram) + (the digit's keys in earlier tiles),
//                64-bit, one workgroup per digit walking its row of tiles in ascending order;
//                dg_scatter_kernel: STABLE.  Wave w of a tile owns its keys [w * DG_TILE / 4, (w + 1) * DG_TILE / 4) in rounds of 64; the
//                rank of a key among the keys of its digit is (the digit's keys in earlier waves) + (in earlier rounds of its wave, a
//                running LDS counter per wave) + (in lower lanes of its round, by ballot matching on the 8 digit bits).  The tile is
//                reordered by digit in LDS and written out so that consecutive lanes write consecutive keys of a digit's run.
//   indices      every index and offset that scales with n is 64-bit; the counts of one tile and positions inside it are 32-bit.
//
// GATHER.  out[j] = sorted[ranks[j]] (the caller has checked the ranks).
//
// SCATTER SUMMARY of a pair (p, hf) of n values: the min and max over both arrays, NaN when any value is NaN (ndarray.min / max), and
// S = sum (p - hf)^2 in THIS order, fixed by n alone (no atomics; the grid follows from n, not from the device):
//   1. chunk c = i / DG_SUM_CHUNK (8192): thread t adds the squares of elements c * 8192 + j * 256 + t, j = 0 .. 31, to 0.0 in ascending j;
//   2. the 64 lanes of a wave by a balanced tree over adjacent lanes (gprx_common.h wave_sum_dpp), six levels;
//   3. the chunk's four waves as ((w0 + w1) + w2) + w3;
//   4. the chunk sums: thread t of ONE workgroup adds chunks t, t + 256, ... to 0.0 in ascending order, then steps 2 and 3 again.
// Depth of the tree, D(n) = 32 + 6 + 3 + ceil(ceil(n / 8192) / 256) + 6 + 3 additions on its longest path (dg_sum_depth below): every
// term is non-negative, so |S - exact sum of the rounded squares| <= D(n) * 2^-53 * S to first order.
//
// DETECTION.  truth and pred (rows, cells), E events as row ranges [lo, hi).  Per event and cell: the max over the event's rows
// ignoring NaN (an all-NaN column gives NaN: pandas DataFrame.max(axis=0), :765-766); a negative max is reported (the reference's
// ValueError, :776-777) BEFORE the threshold; a max below wet_threshold_depth becomes 0 (:780-781); code 1 Detected (t > 0, p > 0), 2 Miss
// (t > 0, p == 0), 3 False Alarm (t == 0, p > 0), 4 Correct Negative (t == 0, p == 0; 0 when not included), 0 when a NaN is compared
// (:792-802).  One thread per cell, rows in tiles of DG_RT loads.
#pragma once
#include "gprx_common.h"

namespace gprx {

constexpr int DG_NT = 256;                      // threads of every workgroup here
constexpr int DG_WAVES = DG_NT / 64;
constexpr int DG_KPT = 16;                      // keys per thread of a tile
constexpr int DG_TILE = DG_NT * DG_KPT;         // 4096 (gpras_amd/diagnostics.py: DG_TILE)
constexpr int DG_WCHUNK = DG_TILE / DG_WAVES;   // consecutive keys of one wave
constexpr int DG_ROUNDS = DG_WCHUNK / 64;       // = DG_KPT
constexpr int DG_BINS = 256;
constexpr int DG_PASSES = 8;
constexpr int DG_HIST_PT = 4;                   // keys per thread and iteration of the histogram sweep
constexpr int DG_SCAN_PT = 8;                   // tiles per thread and iteration of the scan
constexpr int DG_SUM_PT = 32;
constexpr int DG_SUM_CHUNK = DG_NT * DG_SUM_PT;  // 8192
constexpr int DG_RT = 16;                       // rows per tile of the detection kernel (gpras_amd/diagnostics.py: DG_RT)

inline int64_t dg_sum_depth(int64_t n) {
  const int64_t chunks = (n + DG_SUM_CHUNK - 1) / DG_SUM_CHUNK;
  return DG_SUM_PT + 6 + 3 + (chunks + DG_NT - 1) / DG_NT + 6 + 3;
}

// key i of the source: PAIR: bits(fabs(a[i] - b[i])); else the raw key
template <bool PAIR>
__device__ __forceinline__ uint64_t dg_key(const void* __restrict__ s0, const void* __restrict__ s1, int64_t i) {
#pragma clang fp contract(off)
  if constexpr (PAIR) {
    const double r = static_cast<const double*>(s0)[i] - static_cast<const double*>(s1)[i];
    return (uint64_t)__double_as_longlong(r) & 0x7fffffffffffffffull;
  } else {
    return static_cast<const uint64_t*>(s0)[i];
  }
}

// h[d] += 1 for every valid lane of the wave (other waves add to h at the same time)
__device__ __forceinline__ void dg_hist_add(unsigned int* h, unsigned int d, bool valid) {
  const int lane = threadIdx.x & 63;
  unsigned long long rest = __ballot(valid);
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    if (rest == 0) break;  // the same for the whole wave
    const int lead = __ffsll((long long)rest) - 1;
    const unsigned int dl = (unsigned int)__builtin_amdgcn_readlane((int)d, lead);
    const unsigned long long same = __ballot(valid && d == dl) & rest;
    if (lane == lead) atomicAdd(&h[dl], (unsigned int)__popcll(same));
    rest &= ~same;
  }
  if ((rest >> lane) & 1) atomicAdd(&h[d], 1u);
}

// inclusive scan over the 64 lanes of a wave
template <class T>
__device__ __forceinline__ T dg_wave_scan(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const T u = __shfl_up(v, off, 64);
    if (lane >= off) v += u;
  }
  return v;
}

// exclusive scan over the DG_NT threads of the workgroup; *total: the sum over all of them.  `wt`: DG_WAVES words of LDS, free to be
// written when every thread has entered; two barriers.
template <class T>
__device__ __forceinline__ T dg_block_scan(T v, T* wt, T* total) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const T inc = dg_wave_scan(v);
  if (lane == 63) wt[w] = inc;
  __syncthreads();
  T before = 0, all = 0;
#pragma unroll
  for (int k = 0; k < DG_WAVES; ++k) {
    const T t = wt[k];
    if (k < w) before += t;
    all += t;
  }
  __syncthreads();
  *total = all;
  return before + inc - v;
}

// ---- the histogram sweep: grid-stride, hist [8][256] zeroed before -----------------------------------------------------------------
template <bool PAIR>
__global__ __launch_bounds__(DG_NT) void dg_hist_kernel(const void* __restrict__ s0, const void* __restrict__ s1, int64_t n,
                                                        unsigned long long* __restrict__ hist) {
  __shared__ unsigned int h[DG_PASSES * DG_BINS];
  for (int i = threadIdx.x; i < DG_PASSES * DG_BINS; i += DG_NT) h[i] = 0;
  __syncthreads();
  const int64_t step = (int64_t)gridDim.x * DG_NT * DG_HIST_PT;
  for (int64_t base = (int64_t)blockIdx.x * DG_NT * DG_HIST_PT; base < n; base += step) {
    uint64_t key[DG_HIST_PT];
    bool valid[DG_HIST_PT];
#pragma unroll
    for (int k = 0; k < DG_HIST_PT; ++k) {
      const int64_t i = base + (int64_t)k * DG_NT + threadIdx.x;
      valid[k] = i < n;
      key[k] = valid[k] ? dg_key<PAIR>(s0, s1, i) : 0;
    }
#pragma unroll
    for (int k = 0; k < DG_HIST_PT; ++k)
#pragma unroll
      for (int p = 0; p < DG_PASSES; ++p) dg_hist_add(h + p * DG_BINS, (unsigned int)(key[k] >> (8 * p)) & 255u, valid[k]);
  }
  __syncthreads();
  for (int i = threadIdx.x; i < DG_PASSES * DG_BINS; i += DG_NT)
    if (h[i]) atomicAdd(&hist[i], (unsigned long long)h[i]);
}

// keys of the pair into out (the route with no executed pass)
__global__ __launch_bounds__(DG_NT) void dg_build_kernel(const void* __restrict__ a, const void* __restrict__ b, int64_t n, uint64_t* __restrict__ out) {
  const int64_t step = (int64_t)gridDim.x * DG_NT;
  for (int64_t i = (int64_t)blockIdx.x * DG_NT + threadIdx.x; i < n; i += step) out[i] = dg_key<true>(a, b, i);
}

// ---- one pass ------------------------------------------------------------------------------------------------------------------------
// grid (tiles): counts[d * tiles + tile]
template <bool PAIR>
__global__ __launch_bounds__(DG_NT) void dg_count_kernel(const void* __restrict__ s0, const void* __restrict__ s1, int64_t n, int shift, int64_t tiles,
                                                         unsigned int* __restrict__ counts) {
  __shared__ unsigned int h[DG_BINS];
  h[threadIdx.x] = 0;
  __syncthreads();
  const int64_t tile = blockIdx.x, base = tile * DG_TILE;
  uint64_t key[DG_KPT];
#pragma unroll
  for (int k = 0; k < DG_KPT; ++k) {
    const int64_t i = base + (int64_t)k * DG_NT + threadIdx.x;
    key[k] = i < n ? dg_key<PAIR>(s0, s1, i) : 0;
  }
#pragma unroll
  for (int k = 0; k < DG_KPT; ++k) dg_hist_add(h, (unsigned int)(key[k] >> shift) & 255u, base + (int64_t)k * DG_NT + threadIdx.x < n);
  __syncthreads();
  counts[(int64_t)threadIdx.x * tiles + tile] = h[threadIdx.x];
}

// grid (256): workgroup d turns row d of counts into row d of offs; hist: the 256 bins of this pass
__global__ __launch_bounds__(DG_NT) void dg_scan_kernel(const unsigned int* __restrict__ counts, int64_t tiles, const unsigned long long* __restrict__ hist,
                                                        unsigned long long* __restrict__ offs) {
  __shared__ unsigned long long wt[DG_WAVES];
  const int d = blockIdx.x;
  unsigned long long carry = 0;
  dg_block_scan<unsigned long long>((int)threadIdx.x < d ? hist[threadIdx.x] : 0ull, wt, &carry);  // the keys of smaller digits
  const unsigned int* row = counts + (int64_t)d * tiles;
  unsigned long long* orow = offs + (int64_t)d * tiles;
  for (int64_t t0 = 0; t0 < tiles; t0 += (int64_t)DG_NT * DG_SCAN_PT) {
    const int64_t first = t0 + (int64_t)threadIdx.x * DG_SCAN_PT;
    unsigned int c[DG_SCAN_PT];
    unsigned long long mine = 0;
#pragma unroll
    for (int j = 0; j < DG_SCAN_PT; ++j) {
      c[j] = first + j < tiles ? row[first + j] : 0u;
      mine += c[j];
    }
    unsigned long long all = 0;
    unsigned long long at = carry + dg_block_scan<unsigned long long>(mine, wt, &all);
#pragma unroll
    for (int j = 0; j < DG_SCAN_PT; ++j) {
      if (first + j < tiles) orow[first + j] = at;
      at += c[j];
    }
    carry += all;
  }
}

// grid (tiles): the stable scatter of one tile
template <bool PAIR>
__global__ __launch_bounds__(DG_NT) void dg_scatter_kernel(const void* __restrict__ s0, const void* __restrict__ s1, int64_t n, int shift, int64_t tiles,
                                                           const unsigned long long* __restrict__ offs, uint64_t* __restrict__ dst) {
  __shared__ uint64_t skeys[DG_TILE];
  __shared__ unsigned long long gbase[DG_BINS];  // where the digit's run of this tile starts in dst, minus where it starts in skeys
  __shared__ unsigned int wcnt[DG_WAVES][DG_BINS];
  __shared__ unsigned int wt[DG_WAVES];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int k = 0; k < DG_WAVES; ++k) wcnt[k][tid] = 0;
  const int64_t tile = blockIdx.x, base = tile * DG_TILE;
  const int cnt = (int)(n - base < DG_TILE ? n - base : DG_TILE);
  uint64_t key[DG_ROUNDS];
  unsigned int rank[DG_ROUNDS];
#pragma unroll
  for (int r = 0; r < DG_ROUNDS; ++r) {
    const int li = w * DG_WCHUNK + r * 64 + lane;
    key[r] = li < cnt ? dg_key<PAIR>(s0, s1, base + li) : 0;
  }
  __syncthreads();
  const unsigned long long lower = (1ull << lane) - 1ull;
#pragma unroll
  for (int r = 0; r < DG_ROUNDS; ++r) {
    const bool valid = w * DG_WCHUNK + r * 64 + lane < cnt;
    const unsigned int d = (unsigned int)(key[r] >> shift) & 255u;
    unsigned long long mask = __ballot(valid);  // the valid lanes with this lane's digit
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long bal = __ballot(valid && bit);
      mask &= bit ? bal : ~bal;
    }
    const unsigned int old = valid ? wcnt[w][d] : 0u;
    rank[r] = old + (unsigned int)__popcll(mask & lower);
    // every lane of the wave has read the counter before the digit's lowest lane moves it on, and the next round reads what was written
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (valid && (mask & lower) == 0) wcnt[w][d] = old + (unsigned int)__popcll(mask);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  __syncthreads();
  {  // thread = digit: where the digit's keys of every wave start in the reordered tile
    unsigned int c[DG_WAVES], tot = 0;
#pragma unroll
    for (int k = 0; k < DG_WAVES; ++k) {
      c[k] = wcnt[k][tid];
      tot += c[k];
    }
    unsigned int all = 0;
    unsigned int at = dg_block_scan<unsigned int>(tot, wt, &all);
    gbase[tid] = offs[(int64_t)tid * tiles + tile] - at;
#pragma unroll
    for (int k = 0; k < DG_WAVES; ++k) {
      wcnt[k][tid] = at;
      at += c[k];
    }
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < DG_ROUNDS; ++r)
    if (w * DG_WCHUNK + r * 64 + lane < cnt) skeys[wcnt[w][(unsigned int)(key[r] >> shift) & 255u] + rank[r]] = key[r];
  __syncthreads();
#pragma unroll
  for (int k = 0; k < DG_KPT; ++k) {
    const int li = k * DG_NT + tid;
    if (li < cnt) {
      const uint64_t v = skeys[li];
      const unsigned long long at = gbase[(unsigned int)(v >> shift) & 255u] + (unsigned long long)li;
      if (at < (unsigned long long)n) dst[at] = v;  // below n by construction: the comparison keeps a fault in the tables from becoming a stray store
    }
  }
}

// ---- rank gather ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(DG_NT) void dg_gather_kernel(const double* __restrict__ sorted, const int64_t* __restrict__ ranks, int64_t m,
                                                          double* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * DG_NT + threadIdx.x;
  if (j < m) out[j] = sorted[ranks[j]];
}

// ---- scatter summary -----------------------------------------------------------------------------------------------------------------
// the workgroup's (sum, min, max, NaN seen) from every thread's; thread 0 holds the result.  red: 3 * DG_WAVES doubles of LDS.
__device__ __forceinline__ void dg_summary_combine(double& acc, double& mn, double& mx, int& nan, double* red) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  acc = wave_sum_dpp(acc);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    mn = __builtin_fmin(mn, __shfl_xor(mn, off, 64));
    mx = __builtin_fmax(mx, __shfl_xor(mx, off, 64));
  }
  nan = __syncthreads_or(nan);
  if (lane == 0) {
    red[w] = acc;
    red[DG_WAVES + w] = mn;
    red[2 * DG_WAVES + w] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    acc = ((red[0] + red[1]) + red[2]) + red[3];
    for (int k = 0; k < DG_WAVES; ++k) {
      mn = __builtin_fmin(mn, red[DG_WAVES + k]);
      mx = __builtin_fmax(mx, red[2 * DG_WAVES + k]);
    }
  }
}

// grid (chunks): part[4 c] = the chunk's sum of squares, [4 c + 1] its min, [4 c + 2] its max (both NaN when it holds a NaN)
__global__ __launch_bounds__(DG_NT) void dg_summary_kernel(const double* __restrict__ p, const double* __restrict__ hf, int64_t n, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[3 * DG_WAVES];
  const int64_t base = (int64_t)blockIdx.x * DG_SUM_CHUNK;
  double acc = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
  int nan = 0;
#pragma unroll 8
  for (int j = 0; j < DG_SUM_PT; ++j) {
    const int64_t i = base + (int64_t)j * DG_NT + threadIdx.x;
    if (i < n) {
      const double a = p[i], b = hf[i];
      const double r = a - b;
      const double q = r * r;
      acc = acc + q;
      nan |= (a != a) || (b != b);
      mn = __builtin_fmin(mn, __builtin_fmin(a, b));
      mx = __builtin_fmax(mx, __builtin_fmax(a, b));
    }
  }
  dg_summary_combine(acc, mn, mx, nan, red);
  if (threadIdx.x == 0) {
    const double q = __builtin_nan("");
    part[4 * (int64_t)blockIdx.x] = acc;
    part[4 * (int64_t)blockIdx.x + 1] = nan ? q : mn;
    part[4 * (int64_t)blockIdx.x + 2] = nan ? q : mx;
  }
}

// one workgroup: res[0] = min, res[1] = max, res[2] = the sum of squares
__global__ __launch_bounds__(DG_NT) void dg_summary_final_kernel(const double* __restrict__ part, int64_t chunks, double* __restrict__ res) {
#pragma clang fp contract(off)
  __shared__ double red[3 * DG_WAVES];
  double acc = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
  int nan = 0;
  for (int64_t c = threadIdx.x; c < chunks; c += DG_NT) {
    const double s = part[4 * c], lo = part[4 * c + 1], hi = part[4 * c + 2];
    acc = acc + s;
    nan |= (lo != lo) || (hi != hi);
    mn = __builtin_fmin(mn, lo);
    mx = __builtin_fmax(mx, hi);
  }
  dg_summary_combine(acc, mn, mx, nan, red);
  if (threadIdx.x == 0) {
    const double q = __builtin_nan("");
    res[0] = nan ? q : mn;
    res[1] = nan ? q : mx;
    res[2] = acc;
  }
}

// ---- detection -------------------------------------------------------------------------------------------------------------------------
__global__ void dg_detect_init_kernel(int* first_negative) { *first_negative = 0x7fffffff; }

__device__ __forceinline__ double dg_nanmax(double m, double v) { return (v != v) ? m : ((m != m || v > m) ? v : m); }

// grid (cell strips, E).  ev: lo[E] then hi[E].  *first_negative: the smallest event index with a negative maximum.
__global__ __launch_bounds__(DG_NT) void dg_detect_kernel(const double* __restrict__ truth, const double* __restrict__ pred, int64_t cells,
                                                          const int64_t* __restrict__ ev, int E, double thr, int include_cn,
                                                          unsigned char* __restrict__ codes, int* first_negative) {
  const int64_t c = (int64_t)blockIdx.x * DG_NT + threadIdx.x;
  const int e = blockIdx.y;
  if (c >= cells) return;
  const int64_t lo = ev[e], hi = ev[E + e];
  double mt = __builtin_nan(""), mp = mt;
  int64_t r = lo;
  for (; r + DG_RT <= hi; r += DG_RT) {
    double vt[DG_RT], vp[DG_RT];
#pragma unroll
    for (int k = 0; k < DG_RT; ++k) {
      vt[k] = truth[(r + k) * cells + c];
      vp[k] = pred[(r + k) * cells + c];
    }
#pragma unroll
    for (int k = 0; k < DG_RT; ++k) {
      mt = dg_nanmax(mt, vt[k]);
      mp = dg_nanmax(mp, vp[k]);
    }
  }
  for (; r < hi; ++r) {
    mt = dg_nanmax(mt, truth[r * cells + c]);
    mp = dg_nanmax(mp, pred[r * cells + c]);
  }
  if (mt < 0.0 || mp < 0.0) atomicMin(first_negative, e);
  if (mt < thr) mt = 0.0;
  if (mp < thr) mp = 0.0;
  unsigned char code = 0;
  if (mt > 0.0 && mp > 0.0) code = 1;
  else if (mt > 0.0 && mp == 0.0) code = 2;
  else if (mt == 0.0 && mp > 0.0) code = 3;
  else if (mt == 0.0 && mp == 0.0) code = include_cn ? 4 : 0;
  codes[(int64_t)e * cells + c] = code;
}

}  // namespace gprx
