// HmsPreProcessor (gpras/preprocess.py:1165-1320) on the device: the features of the "Upskill HEC-HMS" formulations.
//
//   x (rows, n_features) lives on the device column-major (X[c * ldx + t]); a C-order input is uploaded in row chunks and
//   transposed (hms_transpose_kernel).  Every reduction below has a fixed order that depends on the row count only, never on
//   the grid, so two fits give the same bits.
//   1. colmean:   input_mean over ALL columns (:1226), and IncrementalPCA's own column mean of the centred precip block.
//   2. centre2:   X2 = (x[:, precip] - input_mean) - colmean, the PCA input, in the layout its product needs: (p, ld2) "feature
//                 major" for the covariance C = X2^T X2 (rows >= p), (rows, ld2) row-major for the Gram G = X2 X2^T (rows < p).
//                 The product itself is the fp64 MFMA GEMM of gemm_f64.h (lower triangle, split-K, slabs summed in a fixed order).
//   3. project:   one thread per row: the bc block and x_precip eofs^T of the once-centred precip block (:1251-1254), 32 modes
//                 per workgroup row of the grid, and the row mean avg_precip; j ascends in every sum.
//   4. api:       the antecedent precipitation index (:1284-1294): out[t] = sum_{i=0}^{min(t, W-1)} w[i] a[t-i], a causal Toeplitz
//                 product, i ascending for every output.
//   5. colstats / standardise: x_mean, and x_std over the entries that are not exactly zero (:1260-1261); (f - x_mean) / x_std
//                 (:1280) written row-major.
#pragma once
#include "gprx_common.h"

namespace gprx {

// C-order chunk S (rows, cols) -> X[c * ldx + t0 + r]; 32 x 32 tiles through LDS (odd row stride: no bank conflicts)
__global__ __launch_bounds__(256) void hms_transpose_kernel(const double* __restrict__ S, int64_t rows, int64_t cols, double* __restrict__ X,
                                                            int64_t ldx) {
  __shared__ double tile[32][33];
  const int64_t r0 = (int64_t)blockIdx.x * 32, c0 = (int64_t)blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    const int64_t r = r0 + k, c = c0 + tx;
    if (r < rows && c < cols) tile[k][tx] = S[r * cols + c];
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int64_t c = c0 + k, r = r0 + tx;
    if (r < rows && c < cols) X[c * ldx + r] = tile[tx][k];
  }
}

// Fixed-order sum of 256 values, one per thread; the total is returned to every thread.
__device__ __forceinline__ double hms_block_sum(double v, double* red) {
  const int tid = threadIdx.x;
  __syncthreads();  // a previous use of red is over
  red[tid] = v;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] = red[tid] + red[tid + h];
    __syncthreads();
  }
  return red[0];
}

// out[j] = sum_t (X[c * ldx + t] - sub[c]) / rows with c = idx ? idx[j] : j (sub may be null).  One workgroup per column; thread
// tid sums t = tid + 256 (4 m + q) into four accumulators, combined (s0 + s1) + (s2 + s3), then the fixed tree of hms_block_sum.
__global__ __launch_bounds__(256) void hms_colmean_kernel(const double* __restrict__ X, int64_t ldx, int64_t rows, const int64_t* __restrict__ idx,
                                                          const double* __restrict__ sub, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int64_t j = blockIdx.x;
  const int64_t c = idx ? idx[j] : j;
  const double m = sub ? sub[c] : 0.0;
  const double* col = X + c * ldx;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  int64_t t = threadIdx.x;
  for (; t + 768 < rows; t += 1024) {
    s0 += col[t] - m;
    s1 += col[t + 256] - m;
    s2 += col[t + 512] - m;
    s3 += col[t + 768] - m;
  }
  if (t < rows) s0 += col[t] - m;
  if (t + 256 < rows) s1 += col[t + 256] - m;
  if (t + 512 < rows) s2 += col[t + 512] - m;
  const double s = hms_block_sum((s0 + s1) + (s2 + s3), red);
  if (threadIdx.x == 0) out[j] = s / (double)rows;
}

constexpr int HMS_COV = 0, HMS_GRAM = 1;

// X2 = (X[:, pc] - mu[pc]) - m2, zero beyond rows / p (the K padding of the products).  HMS_COV: X2[j * ld2 + t], grid (ld2 / 256, p);
// HMS_GRAM: X2[t * ld2 + j], grid (ld2 / 256, rows).  Padding rows of X2 are cleared by the host.
__global__ __launch_bounds__(256) void hms_centre2_kernel(const double* __restrict__ X, int64_t ldx, int64_t rows, const int64_t* __restrict__ pc,
                                                          int64_t p, const double* __restrict__ mu, const double* __restrict__ m2, int route,
                                                          double* __restrict__ X2, int64_t ld2) {
#pragma clang fp contract(off)
  const int64_t fast = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (fast >= ld2) return;
  const int64_t t = route == HMS_COV ? fast : (int64_t)blockIdx.y;
  const int64_t j = route == HMS_COV ? (int64_t)blockIdx.y : fast;
  double v = 0.0;
  if (t < rows && j < p) {
    const int64_t c = pc[j];
    v = (X[c * ldx + t] - mu[c]) - m2[j];
  }
  X2[route == HMS_COV ? j * ld2 + t : t * ld2 + j] = v;
}

// One thread per row t; blockIdx.y = block of 32 modes.  F is column-major (feature c at F[c * ldf + t]):
//   F[n_bc + i]  = sum_j (X[pc_j, t] - mup_j) Et[j][i]       (x_precip eofs^T, :1254; Et (p, ke_pad) zero beyond ke)
// and in the first mode block also
//   F[b]          = X[bc_b, t] - mub_b                         (x_bc, :1231)
//   F[n_bc + ke]  = sum_j (X[pc_j, t] - mup_j) / p             (avg_precip, :1251)
// nonfinite[0] becomes 1 when some avg_precip is not finite (the API then keeps the zero tail of its weights: 0 * inf = NaN).
constexpr int HMS_MB = 32;
__global__ __launch_bounds__(256) void hms_project_kernel(const double* __restrict__ X, int64_t ldx, int64_t rows, const int64_t* __restrict__ pc,
                                                          const double* __restrict__ mup, int64_t p, const double* __restrict__ Et, int64_t ke_pad,
                                                          int ke, const int64_t* __restrict__ bc, const double* __restrict__ mub, int64_t n_bc,
                                                          double* __restrict__ F, int64_t ldf, int* __restrict__ nonfinite) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t >= rows) return;  // no barriers below
  const int mb = blockIdx.y;
  double acc[HMS_MB];
#pragma unroll
  for (int i = 0; i < HMS_MB; ++i) acc[i] = 0.0;
  double rs = 0.0;
  const double* e = Et + mb * HMS_MB;
  for (int64_t j = 0; j < p; ++j) {
    const double v = X[pc[j] * ldx + t] - mup[j];
    rs += v;
#pragma unroll
    for (int i = 0; i < HMS_MB; ++i) acc[i] = fma(v, e[j * ke_pad + i], acc[i]);
  }
#pragma unroll
  for (int i = 0; i < HMS_MB; ++i)
    if (mb * HMS_MB + i < ke) F[(n_bc + mb * HMS_MB + i) * ldf + t] = acc[i];
  if (mb != 0) return;
  const double a = rs / (double)p;
  F[(n_bc + ke) * ldf + t] = a;
  if (!isfinite(a)) nonfinite[0] = 1;  // every writer writes the same value
  for (int64_t b = 0; b < n_bc; ++b) F[b * ldf + t] = X[bc[b] * ldx + t] - mub[b];
}

// Antecedent precipitation index.  A workgroup (one wave) owns HMS_API_BT consecutive outputs, a thread HMS_API_R consecutive ones
// in registers together with the HMS_API_R values of `a` they need at the current lag; one lag costs one broadcast read of w,
// HMS_API_R FMAs and one LDS read of the value of `a` that shifts in.  The lags stream through LDS in chunks of HMS_API_CL.  Lags
// i >= n_w weigh 0; indices t - i < 0 read 0 (an exact no-op: the weights are finite).  Lags beyond min(lags, t0 + BT) reach no
// output of the block.  The blocks with the most lags are dispatched first.
// R = 4, not 8: a thread's lags run one after another (4 cycles per wave-wide fp64 FMA), so the last block's thread sets the
// critical path at lags x R x 4 cycles; the LDS traffic per FMA (1 / R) is still well below the LDS rate at R = 4.
constexpr int HMS_API_R = 4, HMS_API_NT = 64, HMS_API_BT = HMS_API_R * HMS_API_NT, HMS_API_CL = 512, HMS_API_G = 8;
// LDS index of `a` offset o: threads read offsets HMS_API_R apart, so one pad per HMS_API_R makes the stride odd (5 doubles):
// the 32 lanes of a ds_read_b64 group then hit 32 distinct bank pairs
__host__ __device__ constexpr int hms_api_pad(int o) { return o + o / HMS_API_R; }
__global__ __launch_bounds__(HMS_API_NT) void hms_api_kernel(const double* __restrict__ a, int64_t n, const double* __restrict__ w, int64_t n_w,
                                                             int64_t lags, double* __restrict__ out) {
  __shared__ double sa[hms_api_pad(HMS_API_BT + HMS_API_CL)];
  __shared__ double sw[HMS_API_CL];
  const int64_t nblk = (n + HMS_API_BT - 1) / HMS_API_BT;
  const int64_t t0 = (nblk - 1 - (int64_t)blockIdx.x) * HMS_API_BT;
  const int tid = threadIdx.x;
  const int64_t tb = t0 + (int64_t)HMS_API_R * tid;
  double acc[HMS_API_R], av[HMS_API_R];
#pragma unroll
  for (int r = 0; r < HMS_API_R; ++r) {
    acc[r] = 0.0;
    av[r] = tb + r < n ? a[tb + r] : 0.0;  // av[r] = a[tb + r - i] at lag i
  }
  const int64_t L = lags < t0 + HMS_API_BT ? lags : t0 + HMS_API_BT;
  const int ob = HMS_API_R * tid + HMS_API_CL - 1;
  for (int64_t i0 = 0; i0 < L; i0 += HMS_API_CL) {
    const int cl = (int)(L - i0 < HMS_API_CL ? L - i0 : HMS_API_CL);
    const int64_t base = t0 - i0 - HMS_API_CL;  // sa offset o holds a[base + o]
    __syncthreads();                            // the previous chunk is read
    for (int o = tid; o < HMS_API_BT + HMS_API_CL; o += HMS_API_NT) {
      const int64_t s = base + o;
      sa[hms_api_pad(o)] = (s >= 0 && s < n) ? a[s] : 0.0;
    }
    for (int o = tid; o < cl; o += HMS_API_NT) sw[o] = i0 + o < n_w ? w[i0 + o] : 0.0;
    __syncthreads();
    // groups of HMS_API_G lags; the LDS reads of the next group are issued before the FMAs of this one (one wave per SIMD
    // leaves nothing else to hide their latency)
    const int ng = cl / HMS_API_G;
    double wn[HMS_API_G], an[HMS_API_G];
#pragma unroll
    for (int q = 0; q < HMS_API_G; ++q) {
      wn[q] = ng > 0 ? sw[q] : 0.0;
      an[q] = ng > 0 ? sa[hms_api_pad(ob - q)] : 0.0;
    }
    for (int g = 0; g < ng; ++g) {
      double wc[HMS_API_G], ac[HMS_API_G];
#pragma unroll
      for (int q = 0; q < HMS_API_G; ++q) {
        wc[q] = wn[q];
        ac[q] = an[q];
      }
      if (g + 1 < ng) {
        const int l1 = (g + 1) * HMS_API_G;
#pragma unroll
        for (int q = 0; q < HMS_API_G; ++q) {
          wn[q] = sw[l1 + q];
          an[q] = sa[hms_api_pad(ob - l1 - q)];
        }
      }
#pragma unroll
      for (int q = 0; q < HMS_API_G; ++q) {
#pragma unroll
        for (int r = 0; r < HMS_API_R; ++r) acc[r] = fma(wc[q], av[r], acc[r]);
#pragma unroll
        for (int r = HMS_API_R - 1; r > 0; --r) av[r] = av[r - 1];
        av[0] = ac[q];  // a[tb - (i0 + l) - 1], l = g G + q
      }
    }
    for (int l = ng * HMS_API_G; l < cl; ++l) {  // the last lags of the chunk, one at a time
      const double wi = sw[l];
#pragma unroll
      for (int r = 0; r < HMS_API_R; ++r) acc[r] = fma(wi, av[r], acc[r]);
#pragma unroll
      for (int r = HMS_API_R - 1; r > 0; --r) av[r] = av[r - 1];
      av[0] = sa[hms_api_pad(ob - l)];
    }
  }
#pragma unroll
  for (int r = 0; r < HMS_API_R; ++r)
    if (tb + r < n) out[tb + r] = acc[r];
}

// x_mean[c] = sum / rows; x_std[c] = np.std over the entries != 0 (ddof 0; none: NaN).  One workgroup per feature column.
__global__ __launch_bounds__(256) void hms_colstats_kernel(const double* __restrict__ F, int64_t ldf, int64_t rows, double* __restrict__ xm,
                                                           double* __restrict__ xs) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const double* col = F + (int64_t)blockIdx.x * ldf;
  double s = 0.0, snz = 0.0, cnt = 0.0;
  for (int64_t t = threadIdx.x; t < rows; t += 256) {
    const double v = col[t];
    s += v;
    if (v != 0.0) {
      snz += v;
      cnt += 1.0;
    }
  }
  const double tot = hms_block_sum(s, red);
  const double tnz = hms_block_sum(snz, red);
  const double n_nz = hms_block_sum(cnt, red);
  const double m = tnz / n_nz;
  double q = 0.0;
  for (int64_t t = threadIdx.x; t < rows; t += 256) {
    const double v = col[t];
    if (v != 0.0) {
      const double d = v - m;
      q += d * d;
    }
  }
  const double tq = hms_block_sum(q, red);
  if (threadIdx.x == 0) {
    xm[blockIdx.x] = tot / (double)rows;
    xs[blockIdx.x] = n_nz > 0.0 ? sqrt(tq / n_nz) : NAN;
  }
}

// out[t * nf + c] = (F[c * ldf + t] - xm[c]) / xs[c], one thread per output element
__global__ __launch_bounds__(256) void hms_standardise_kernel(const double* __restrict__ F, int64_t ldf, int64_t rows, int64_t nf,
                                                              const double* __restrict__ xm, const double* __restrict__ xs, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * nf) return;
  const int64_t t = e / nf, c = e % nf;
  out[e] = (F[c * ldf + t] - xm[c]) / xs[c];
}

}  // namespace gprx
