// Storm-event selection (production/pre_processing/event_selection.py:13-257) on the device, DESIGN.md section 3.19:
//   ev_pivot_kernel / ev_lengths_kernel    pivot(...).fillna(0) (:157-160) and groupby("event_id").max() (:36-42)
//   ev_block_keys_kernel / ev_knots_kernel the knots of get_return_period_function (:44-59), around the radix sort of diag.h
//   ev_rp_eval_kernel                      scipy's interp1d._call_linear, operation for operation
//   ev_colsum_* / ev_centre_kernel / ev_gather_scores_kernel / ev_standardise_kernel
//                                          the column passes around the GEMMs of the two PCAs and the StandardScaler (:162-167)
//   ev_fp_*                                the farthest-point loop (:173-180), incrementally, one launch per pick
// Wave size 64.  Every sum here has ONE order, fixed by the shape alone (tests/events_numpy.py restates it).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace gprx {

constexpr int EV_NT = 256;             // threads of a workgroup, four waves
constexpr int EV_SUM_CHUNK = 256;      // rows of one partial column sum
constexpr int EV_KNOT_NT = 1024;       // the one workgroup of the knot compaction
constexpr int EV_FP_MAX_BLOCKS = 1024; // workgroups of a selection launch: as many partial maxima
constexpr int EV_MAX_D = 64;           // columns of the score matrix
constexpr int EV_NONE = 0x7fffffff;    // the row of an empty partial maximum

// ---- 1. pivot ------------------------------------------------------------------------------------------------------------------------
// The three blocks (E, ld) arrive filled with one NaN pattern; row r of the long frame lands at (rank[r], hour[r]).  (event, hour) is
// unique, so no two rows write one element and the result does not depend on the order of the rows.
__global__ __launch_bounds__(EV_NT) void ev_pivot_kernel(int64_t rows, const int32_t* __restrict__ rank, const int32_t* __restrict__ hour,
                                                         const double* __restrict__ pe, const double* __restrict__ pc, const double* __restrict__ q, int64_t E,
                                                         int64_t H, int64_t ld, double* __restrict__ Ppe, double* __restrict__ Ppc, double* __restrict__ Pq,
                                                         int* __restrict__ bad) {
  const int64_t step = (int64_t)gridDim.x * EV_NT;
  for (int64_t r = (int64_t)blockIdx.x * EV_NT + threadIdx.x; r < rows; r += step) {
    const int64_t e = rank[r], h = hour[r];
    if (e < 0 || e >= E || h < 0 || h >= H) {
      *bad = 1;
      continue;
    }
    const int64_t off = e * ld + h;
    Ppe[off] = pe[r];
    Ppc[off] = pc[r];
    Pq[off] = q[r];
  }
}

// ---- 2. lengths and maxima -------------------------------------------------------------------------------------------------------------
// One wave per event.  An element that still holds NaN was not written: it becomes the 0 of fillna(0) and does not enter the maxima (a
// negative inflow maximum survives).  len[e] = the number of hours when they are exactly 0 .. len - 1, else -1.  mx (2, E): the maxima
// of precip-cum and of inflow.
__global__ __launch_bounds__(EV_NT) void ev_lengths_kernel(int64_t E, int64_t H, int64_t ld, double* __restrict__ Ppe, double* __restrict__ Ppc,
                                                           double* __restrict__ Pq, int32_t* __restrict__ len, double* __restrict__ mx) {
  const int lane = threadIdx.x & 63;
  const int64_t e = (int64_t)blockIdx.x * (EV_NT / 64) + (threadIdx.x >> 6);
  if (e >= E) return;  // (the whole wave)
  int cnt = 0, last = -1;
  double mpc = -INFINITY, mq = -INFINITY;
  for (int64_t h = lane; h < ld; h += 64) {
    const int64_t off = e * ld + h;
    const double a = Ppe[off], b = Ppc[off], c = Pq[off];
    if (h < H && a == a && b == b && c == c) {
      ++cnt;
      last = (int)h;
      mpc = fmax(mpc, b);
      mq = fmax(mq, c);
    } else {
      Ppe[off] = 0.0;
      Ppc[off] = 0.0;
      Pq[off] = 0.0;
    }
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    cnt += __shfl_xor(cnt, o);
    last = max(last, __shfl_xor(last, o));
    mpc = fmax(mpc, __shfl_xor(mpc, o));
    mq = fmax(mq, __shfl_xor(mq, o));
  }
  if (lane == 0) {
    len[e] = (cnt > 0 && last + 1 == cnt) ? cnt : -1;
    mx[e] = mpc;
    mx[E + e] = mq;
  }
}

// ---- 3. return periods -----------------------------------------------------------------------------------------------------------------
// the order-preserving map of a double onto an unsigned key (-0.0 counts as +0.0, as np.sort and np.unique compare them)
__device__ __forceinline__ uint64_t ev_key(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v + 0.0);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ev_unkey(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// keys[b] = key(max of v[b * ar .. min(E, (b + 1) * ar))): series[i : i + arrival_rate].max() (:45-48), the last block may be short
__global__ __launch_bounds__(EV_NT) void ev_block_keys_kernel(const double* __restrict__ v, int64_t E, int64_t ar, int64_t nb, uint64_t* __restrict__ keys) {
  const int64_t b = (int64_t)blockIdx.x * EV_NT + threadIdx.x;
  if (b >= nb) return;
  const int64_t lo = b * ar, hi = min(E, lo + ar);
  double m = v[lo];
  for (int64_t i = lo + 1; i < hi; ++i) m = fmax(m, v[i]);
  keys[b] = ev_key(m);
}

// sorted (nb) ascending keys.  np.sort(blocks)[::-1], ranks 1 .. nb, np.unique(..., return_index=True) (:49-52): ascending element i is
// descending position nb - 1 - i, and the FIRST descending occurrence of a value is the LAST ascending one, so the knot of a run of equal
// values is x = the value, y = (nb + 1) / (nb - i) at the run's last i.  One workgroup compacts the knots in order: a scan per 1024 keys
// and a running count.  *nk = the number of knots.
__global__ __launch_bounds__(EV_KNOT_NT) void ev_knots_kernel(const uint64_t* __restrict__ sorted, int64_t nb, double* __restrict__ xk, double* __restrict__ yk,
                                                              int64_t* __restrict__ nk) {
  __shared__ int wsum[EV_KNOT_NT / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int64_t carry = 0;
  for (int64_t base = 0; base < nb; base += EV_KNOT_NT) {
    const int64_t i = base + threadIdx.x;
    const int flag = (i < nb && (i == nb - 1 || sorted[i + 1] != sorted[i])) ? 1 : 0;
    int v = flag;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int t = __shfl_up(v, o);
      if (lane >= o) v += t;
    }
    if (lane == 63) wsum[wave] = v;
    __syncthreads();
    int before = 0, total = 0;
    for (int w = 0; w < EV_KNOT_NT / 64; ++w) {
      if (w < wave) before += wsum[w];
      total += wsum[w];
    }
    if (flag) {
      const int64_t pos = carry + before + v - 1;
      xk[pos] = ev_unkey(sorted[i]);
      yk[pos] = (double)(nb + 1) / (double)(nb - i);
    }
    carry += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) *nk = carry;
}

// scipy.interpolate.interp1d._call_linear with fill_value="extrapolate": searchsorted (left), clip to [1, nk - 1], then
// slope = (y_hi - y_lo) / (x_hi - x_lo); y = slope * (x - x_lo) + y_lo -- each operation rounded on its own.  nk >= 2.
__global__ __launch_bounds__(EV_NT) void ev_rp_eval_kernel(const double* __restrict__ xk, const double* __restrict__ yk, const int64_t* __restrict__ nk_p,
                                                           const double* __restrict__ v, int64_t n, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t i = (int64_t)blockIdx.x * EV_NT + threadIdx.x;
  if (i >= n) return;
  const int64_t nk = *nk_p;
  const double x = v[i];
  int64_t lo = 0, hi = nk;
  if (x != x) lo = nk;  // (searchsorted sorts NaN last)
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (xk[mid] < x)
      lo = mid + 1;
    else
      hi = mid;
  }
  const int64_t idx = min(max(lo, (int64_t)1), nk - 1);
  const double x_lo = xk[idx - 1], x_hi = xk[idx], y_lo = yk[idx - 1], y_hi = yk[idx];
  const double slope = (y_hi - y_lo) / (x_hi - x_lo);
  out[i] = slope * (x - x_lo) + y_lo;
}

// ---- 4. column passes of the PCA and of the scaler -----------------------------------------------------------------------------------
// grid (chunks, ceil(ncol / 64)), 64 threads: partial[c * ncol + j] = the sum over the rows r of chunk c, in order of r, of X[r][j]
// (shift null) or of (X[r][j] - shift[j])^2
__global__ __launch_bounds__(64) void ev_colsum_partial_kernel(const double* __restrict__ X, int64_t n, int64_t ncol, int64_t ld, const double* __restrict__ shift,
                                                               double* __restrict__ partial) {
#pragma clang fp contract(off)
  const int64_t j = (int64_t)blockIdx.y * 64 + threadIdx.x, c = blockIdx.x;
  if (j >= ncol) return;
  const int64_t r0 = c * EV_SUM_CHUNK, r1 = min(n, r0 + EV_SUM_CHUNK);
  const double s = shift ? shift[j] : 0.0;
  double acc = 0.0;
  for (int64_t r = r0; r < r1; ++r) {
    double x = X[r * ld + j];
    if (shift) {
      const double d = x - s;
      x = d * d;
    }
    acc += x;
  }
  partial[c * ncol + j] = acc;
}

// out[j] = (the sum of the partials in order of the chunk) / n; as_scale: its square root, 1 where that is 0 (a constant column)
__global__ __launch_bounds__(EV_NT) void ev_colsum_final_kernel(const double* __restrict__ partial, int64_t chunks, int64_t ncol, double n, int as_scale,
                                                                double* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t j = (int64_t)blockIdx.x * EV_NT + threadIdx.x;
  if (j >= ncol) return;
  double acc = 0.0;
  for (int64_t c = 0; c < chunks; ++c) acc += partial[c * ncol + j];
  double v = acc / n;
  if (as_scale) {
    v = __dsqrt_rn(v);
    if (v == 0.0) v = 1.0;
  }
  out[j] = v;
}

// Xc (Ep, ld) = X - mean over the H columns of the E rows, 0 in the padding columns and in the padding rows E .. Ep - 1 (the K of the
// covariance GEMM is a multiple of 16)
__global__ __launch_bounds__(EV_NT) void ev_centre_kernel(const double* __restrict__ X, int64_t E, int64_t Ep, int64_t H, int64_t ld,
                                                          const double* __restrict__ mean, double* __restrict__ Xc) {
  const int64_t total = Ep * ld, live = E * ld, step = (int64_t)gridDim.x * EV_NT;
  for (int64_t i = (int64_t)blockIdx.x * EV_NT + threadIdx.x; i < total; i += step) {
    const int64_t j = i % ld;
    Xc[i] = (i < live && j < H) ? X[i] - mean[j] : 0.0;
  }
}

// S (E, 2k) = [T[:, 0:k], T[:, kp:kp + k]] of the two GEMM outputs T (E, 2 kp): np.concatenate([pcs1, pcs2], axis=1) (:164)
__global__ __launch_bounds__(EV_NT) void ev_gather_scores_kernel(const double* __restrict__ T, int64_t E, int k, int kp, double* __restrict__ S) {
  const int64_t d = 2 * k, total = E * d, step = (int64_t)gridDim.x * EV_NT;
  for (int64_t i = (int64_t)blockIdx.x * EV_NT + threadIdx.x; i < total; i += step) {
    const int64_t r = i / d, c = i % d;
    S[i] = T[r * 2 * kp + (c < k ? c : kp + c - k)];
  }
}

// StandardScaler (:165-167): S = (S - mean) / scale, two operations
__global__ __launch_bounds__(EV_NT) void ev_standardise_kernel(double* __restrict__ S, int64_t E, int d, const double* __restrict__ mean,
                                                               const double* __restrict__ scale) {
#pragma clang fp contract(off)
  const int64_t total = E * d, step = (int64_t)gridDim.x * EV_NT;
  for (int64_t i = (int64_t)blockIdx.x * EV_NT + threadIdx.x; i < total; i += step) {
    const int c = (int)(i % d);
    S[i] = (S[i] - mean[c]) / scale[c];
  }
}

// ---- 5. farthest-point selection -------------------------------------------------------------------------------------------------------
// mind[r]: the squared distance of candidate r to its nearest selected row; -1 marks a selected row.  Squared distances are direct
// differences summed over the columns in order.  The largest wins, the lowest row on a tie.
__device__ __forceinline__ bool ev_better(double v, int i, double bv, int bi) { return v > bv || (v == bv && i < bi); }

// all threads of the workgroup (EV_NT) leave with the workgroup's best pair
__device__ __forceinline__ void ev_block_argmax(double& v, int& i, double* sv, int* si) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    const double ov = __shfl_xor(v, o);
    const int oi = __shfl_xor(i, o);
    if (ev_better(ov, oi, v, i)) {
      v = ov;
      i = oi;
    }
  }
  __syncthreads();  // (sv and si may still be read from the previous call)
  if ((threadIdx.x & 63) == 0) {
    sv[threadIdx.x >> 6] = v;
    si[threadIdx.x >> 6] = i;
  }
  __syncthreads();
  v = sv[0];
  i = si[0];
#pragma unroll
  for (int w = 1; w < EV_NT / 64; ++w)
    if (ev_better(sv[w], si[w], v, i)) {
      v = sv[w];
      i = si[w];
    }
}

__device__ __forceinline__ double ev_sqdist(const double* __restrict__ a, const double* __restrict__ b, int d) {
#pragma clang fp contract(off)
  double acc = 0.0;
  for (int j = 0; j < d; ++j) {
    const double t = a[j] - b[j];
    acc += t * t;
  }
  return acc;
}

__global__ __launch_bounds__(EV_NT) void ev_fp_fill_kernel(double* __restrict__ mind, int64_t n) {
  const int64_t step = (int64_t)gridDim.x * EV_NT;
  for (int64_t r = (int64_t)blockIdx.x * EV_NT + threadIdx.x; r < n; r += step) mind[r] = INFINITY;
}

__global__ __launch_bounds__(EV_NT) void ev_fp_mark_kernel(double* __restrict__ mind, const int32_t* __restrict__ sel, int64_t ns) {
  const int64_t s = (int64_t)blockIdx.x * EV_NT + threadIdx.x;
  if (s < ns) mind[sel[s]] = -1.0;
}

// mind of every candidate against the initial selection, and the partial maxima (pv, pi) of this launch's workgroups
__global__ __launch_bounds__(EV_NT) void ev_fp_init_kernel(const double* __restrict__ S, int64_t n, int d, const int32_t* __restrict__ sel, int64_t ns,
                                                           double* __restrict__ mind, double* __restrict__ pv, int* __restrict__ pi) {
  __shared__ double sv[EV_NT / 64];
  __shared__ int si[EV_NT / 64];
  double bv = -1.0;
  int bi = EV_NONE;
  const int64_t step = (int64_t)gridDim.x * EV_NT;
  for (int64_t r = (int64_t)blockIdx.x * EV_NT + threadIdx.x; r < n; r += step) {
    double m = mind[r];
    if (m < 0.0) continue;
    const double* a = S + r * d;
    for (int64_t s = 0; s < ns; ++s) m = fmin(m, ev_sqdist(a, S + (int64_t)sel[s] * d, d));
    mind[r] = m;
    if (ev_better(m, (int)r, bv, bi)) {
      bv = m;
      bi = (int)r;
    }
  }
  ev_block_argmax(bv, bi, sv, si);
  if (threadIdx.x == 0) {
    pv[blockIdx.x] = bv;
    pi[blockIdx.x] = bi;
  }
}

// Pick `it`: the winner among the G partial maxima of the previous launch (every workgroup finds it for itself), recorded by workgroup 0
// with its one square root; then the min-update of this workgroup's rows against the winner and their new partial maximum, into the
// OTHER pair of partial buffers.  The launches of all picks are enqueued at once; a kernel boundary orders them, no workgroup waits for
// another.
__global__ __launch_bounds__(EV_NT) void ev_fp_step_kernel(const double* __restrict__ S, int64_t n, int d, double* __restrict__ mind,
                                                           const double* __restrict__ pv_in, const int* __restrict__ pi_in, int G,
                                                           double* __restrict__ pv_out, int* __restrict__ pi_out, int32_t* __restrict__ picks,
                                                           double* __restrict__ pick_dist, int it) {
  __shared__ double sv[EV_NT / 64];
  __shared__ int si[EV_NT / 64];
  __shared__ double w[EV_MAX_D];
  double wv = -1.0;
  int wi = EV_NONE;
  for (int g = threadIdx.x; g < G; g += EV_NT)
    if (ev_better(pv_in[g], pi_in[g], wv, wi)) {
      wv = pv_in[g];
      wi = pi_in[g];
    }
  ev_block_argmax(wv, wi, sv, si);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    picks[it] = wi == EV_NONE ? -1 : wi;
    pick_dist[it] = wi == EV_NONE ? -1.0 : __dsqrt_rn(wv);
  }
  double bv = -1.0;
  int bi = EV_NONE;
  if (wi != EV_NONE) {  // (the same in every thread)
    if (threadIdx.x < d) w[threadIdx.x] = S[(int64_t)wi * d + threadIdx.x];
    __syncthreads();
    const int64_t step = (int64_t)gridDim.x * EV_NT;
    for (int64_t r = (int64_t)blockIdx.x * EV_NT + threadIdx.x; r < n; r += step) {
      double m = mind[r];
      if (r == wi) {
        mind[r] = -1.0;
        continue;
      }
      if (m < 0.0) continue;
      m = fmin(m, ev_sqdist(S + r * d, w, d));
      mind[r] = m;
      if (ev_better(m, (int)r, bv, bi)) {
        bv = m;
        bi = (int)r;
      }
    }
  }
  ev_block_argmax(bv, bi, sv, si);
  if (threadIdx.x == 0) {
    pv_out[blockIdx.x] = bv;
    pi_out[blockIdx.x] = bi;
  }
}

}  // namespace gprx
