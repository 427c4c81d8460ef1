// Fitting the EOF preprocessor on the device: PreProcessor.fit (gpras/preprocess.py:947-1007) with the single-batch
// IncrementalPCA it calls (n_samples <= n_wet cells: one partial_fit, one SVD).
//
//   1. colstats:   one pass over x (rows, cells): per cell max / min of g(x) (g = x - e for wse, the depth max(x - e, 0) for
//                  depth), the wetness class of _classify_depths (:1128-1133) and the column mean of the PCA input (x, or
//                  the depth) in numpy's pairwise order and one division: the reference's x[:, ~dry] is a Fortran-order
//                  copy, so its x.mean(axis=0) reduces every column as one contiguous run (pairwise_sum), and
//                  input_mean is bit-identical only in that order.
//   2. compact:    Xc1[t, j] = (v(x[t, c_j]) - mu_j) * w_j over the wet cells c_j (:980-986: subtract, then weight), then
//                  IncrementalPCA's own centring Xc2 = Xc1 - colmean(Xc1) (partial_fit, first batch; the same pairwise
//                  order), one thread per column.
//   3. Gram:       G = Xc2 Xc2^T with the fp64 MFMA GEMM (lower triangle, split-K), slabs summed in a fixed order and mirrored.
//   4. eigh(G) = U diag(lambda) U^T, on the host (numpy) or on the device (eig_jacobi.h); the SVD of Xc2 is U diag(sqrt(lambda)) V^T.
//   5. components: E = diag(lambda^-1/2) U_k^T Xc2 (GEMM, K = n_samples), then svd_flip(u_based_decision=False): every row
//                  is turned so that its entry of largest magnitude (lowest index on ties) is positive.
//   6. projection: Z = Xc1 E^T (:1005 projects the matrix centred once).
#pragma once
#include <vector>

#include "gprx_common.h"

namespace gprx {

// wetness classes, as _classify_depths leaves them: 0 = "" (max == threshold exactly, or NaN), 1 = AD, 2 = TF, 3 = AF
constexpr int PCAFIT_WSE = 0, PCAFIT_DEPTH = 1, PCAFIT_VELOCITY = 2;

__device__ __forceinline__ double pcafit_depth(double x, double e) {
#pragma clang fp contract(off)
  double d = x - e;
  return d < 0.0 ? 0.0 : d;  // d[d < 0] = 0: a NaN stays a NaN
}

// numpy's pairwise summation of a contiguous run (pairwise_sum in loops_utils.h): runs of <= 128 are leaves (< 8 values: in
// order from 0; else 8 interleaved accumulators, combined ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the rest in
// order); longer runs split at n2 = n / 2 - (n / 2) % 8.  The split tree depends on the row count only: the host lists it in
// post order (pcafit_pairwise_ops) as leaves {first row, count} and additions {-1, 0}, and each thread keeps its stack of
// partial sums in LDS (column threadIdx.x, PCAFIT_STACK deep).
constexpr int PCAFIT_STACK = 16;
template <class F>
__device__ __forceinline__ double pcafit_pairwise(F val, const int2* __restrict__ ops, int nops, double* stk) {
#pragma clang fp contract(off)
  int sp = 0;
  for (int o = 0; o < nops; ++o) {
    const int2 op = ops[o];
    if (op.x < 0) {
      stk[(sp - 2) * 256] = stk[(sp - 2) * 256] + stk[(sp - 1) * 256];
      --sp;
      continue;
    }
    const int s0 = op.x, n = op.y;
    double res;
    if (n < 8) {
      res = 0.0;
      for (int i = 0; i < n; ++i) res += val(s0 + i);
    } else {
      double r0 = val(s0), r1 = val(s0 + 1), r2 = val(s0 + 2), r3 = val(s0 + 3), r4 = val(s0 + 4), r5 = val(s0 + 5), r6 = val(s0 + 6),
             r7 = val(s0 + 7);
      int i = 8;
      for (; i < n - (n % 8); i += 8) {
        r0 += val(s0 + i);
        r1 += val(s0 + i + 1);
        r2 += val(s0 + i + 2);
        r3 += val(s0 + i + 3);
        r4 += val(s0 + i + 4);
        r5 += val(s0 + i + 5);
        r6 += val(s0 + i + 6);
        r7 += val(s0 + i + 7);
      }
      res = ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7));
      for (; i < n; ++i) res += val(s0 + i);
    }
    stk[sp * 256] = res;
    ++sp;
  }
  return stk[0];
}

// One thread per cell.  x: (rows, cells) row-major.  cls: class per cell; mean: column mean of the PCA input.
__global__ __launch_bounds__(256) void pcafit_colstats_kernel(const double* __restrict__ x, int64_t rows, int64_t cells,
                                                              const double* __restrict__ elev, int mode, double thr, const int2* __restrict__ ops,
                                                              int nops, unsigned char* __restrict__ cls, double* __restrict__ mean) {
#pragma clang fp contract(off)
  __shared__ double stk[PCAFIT_STACK * 256];
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cells) return;
  const double e = (mode == PCAFIT_VELOCITY) ? 0.0 : elev[c];
  const double* col = x + c;
  double mx = -INFINITY, mn = INFINITY;
  bool nan = false;
  // every row is visited exactly once by the summation: max / min / NaN ride along (they are order-free)
  auto val = [&](int t) {
    double v = col[(int64_t)t * cells];
    const double g = (mode == PCAFIT_DEPTH) ? pcafit_depth(v, e) : v - e;
    if (mode == PCAFIT_DEPTH) v = g;
    nan |= g != g;
    mx = g > mx ? g : mx;
    mn = g < mn ? g : mn;
    return v;
  };
  const double s = pcafit_pairwise(val, ops, nops, stk + threadIdx.x);
  unsigned char k = 2;  // velocity: every cell TF
  if (mode != PCAFIT_VELOCITY) {
    k = 0;
    if (!nan) {  // numpy's max / min propagate NaN, and every comparison with NaN is false
      if (mx < thr) k = 1;
      if (mx > thr) k = 2;
      if (mn > thr) k = 3;
    }
  }
  cls[c] = k;
  mean[c] = s / (double)rows;
}

// One thread per compacted column j < ldc (padding columns j >= n_wet get zeros).  idx: wet cell of column j; mu: column means
// over ALL cells (colstats); w: weights over all cells or null (unweighted: no multiply, as the reference skips it).
// Writes xc1 (rows, ldc) = (v - mu) w and xc2 (rows, ldc) = xc1 - colmean(xc1); m2 (ldc) receives colmean(xc1).
__global__ __launch_bounds__(256) void pcafit_compact_kernel(const double* __restrict__ x, int64_t rows, int64_t cells,
                                                             const int64_t* __restrict__ idx, int64_t n_wet, int64_t ldc,
                                                             const double* __restrict__ elev, int mode, const double* __restrict__ mu,
                                                             const double* __restrict__ w, const int2* __restrict__ ops, int nops,
                                                             double* __restrict__ xc1, double* __restrict__ xc2, double* __restrict__ m2) {
#pragma clang fp contract(off)
  __shared__ double stk[PCAFIT_STACK * 256];
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= ldc) return;
  if (j >= n_wet) {
    for (int64_t t = 0; t < rows; ++t) {
      xc1[t * ldc + j] = 0.0;
      xc2[t * ldc + j] = 0.0;
    }
    m2[j] = 0.0;
    return;
  }
  const int64_t c = idx[j];
  const double e = (mode == PCAFIT_DEPTH) ? elev[c] : 0.0, m = mu[c];
  const double wc = w ? w[c] : 1.0;
  for (int64_t t = 0; t < rows; ++t) {
    double v = x[t * cells + c];
    if (mode == PCAFIT_DEPTH) v = pcafit_depth(v, e);
    v = v - m;
    if (w) v = v * wc;
    xc1[t * ldc + j] = v;
  }
  // IncrementalPCA: col_mean = (0 + nansum(X, 0)) / n_samples over the (Fortran-order) weighted matrix, then X -= col_mean
  const double s = pcafit_pairwise([&](int t) { return xc1[(int64_t)t * ldc + j]; }, ops, nops, stk + threadIdx.x);
  const double m2j = (0.0 + s) / (double)rows;
  m2[j] = m2j;
  for (int64_t t = 0; t < rows; ++t) xc2[t * ldc + j] = xc1[t * ldc + j] - m2j;
}

// G (n, n) from the lower-triangle split-K slabs ws[z] (n, n): G[i][j] = G[j][i] = sum_z ws[z][i][j] for i >= j, z ascending.
__global__ __launch_bounds__(256) void pcafit_gram_reduce_kernel(const double* __restrict__ ws, int nsplit, int n, double* __restrict__ G) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n * n) return;
  const int i = (int)(e / n), j = (int)(e % n);
  if (j > i) return;
  double s = 0.0;
  for (int z = 0; z < nsplit; ++z) s += ws[(int64_t)z * n * n + e];
  G[(int64_t)i * n + j] = s;
  G[(int64_t)j * n + i] = s;
}

// A (k, rows_p) = diag(lambda^-1/2) U_k^T from the device eigenpairs: U (rows, rows) with eigenvectors in columns and lam ascending,
// so row i of A takes column rows - 1 - i; the K padding [rows, rows_p) is zero.  The arithmetic of the host path: s = 1 / sqrt(lambda), u s.
__global__ __launch_bounds__(256) void pcafit_scale_u_kernel(const double* __restrict__ U, const double* __restrict__ lam, int64_t rows, int64_t rows_p,
                                                             int k, double* __restrict__ A) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)k * rows_p) return;
  const int64_t i = e / rows_p, t = e % rows_p;
  double v = 0.0;
  if (t < rows) {
    const int64_t c = rows - 1 - i;
    const double s = 1.0 / sqrt(lam[c]);
    v = U[t * rows + c] * s;
  }
  A[e] = v;
}

// svd_flip(u_based_decision=False) on the rows of E (k, lde), over the first `cols` entries: one workgroup per row finds the
// first index of max |E[r][.]| (np.argmax) and multiplies the row by np.sign of that entry.
__global__ __launch_bounds__(256) void pcafit_sign_flip_kernel(double* __restrict__ E, int64_t lde, int64_t cols) {
  __shared__ double sv[256];
  __shared__ int64_t si[256];
  double* row = E + (int64_t)blockIdx.x * lde;
  const int tid = threadIdx.x;
  double best = -1.0;
  int64_t bi = -1;
  for (int64_t c = tid; c < cols; c += 256) {
    const double a = fabs(row[c]);
    if (a > best) {  // strides ascend within a thread: the first maximum is kept
      best = a;
      bi = c;
    }
  }
  sv[tid] = best;
  si[tid] = bi;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) {
      const double b = sv[tid + h];
      const int64_t i2 = si[tid + h];
      if (i2 >= 0 && (b > sv[tid] || (b == sv[tid] && (si[tid] < 0 || i2 < si[tid])))) {
        sv[tid] = b;
        si[tid] = i2;
      }
    }
    __syncthreads();
  }
  const int64_t arg = si[0];
  if (arg < 0) return;
  const double piv = row[arg];
  const double sgn = piv > 0.0 ? 1.0 : (piv < 0.0 ? -1.0 : 0.0);
  __syncthreads();  // every thread has read the pivot before any thread changes the row
  if (sgn == 1.0) return;
  for (int64_t c = tid; c < cols; c += 256) row[c] = row[c] * sgn;
}

// post-order program of numpy's pairwise summation over n rows (see pcafit_pairwise); depth: values on the stack so far
inline void pcafit_pairwise_ops(int s0, int n, int depth, std::vector<int2>& ops, int& max_depth) {
  if (n <= 128) {
    ops.push_back(make_int2(s0, n));
    max_depth = depth + 1 > max_depth ? depth + 1 : max_depth;
    return;
  }
  int n2 = n / 2;
  n2 -= n2 % 8;
  pcafit_pairwise_ops(s0, n2, depth, ops, max_depth);
  pcafit_pairwise_ops(s0 + n2, n - n2, depth + 1, ops, max_depth);
  ops.push_back(make_int2(-1, 0));
}

}  // namespace gprx
