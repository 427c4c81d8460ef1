// The covariance route of PreProcessor.fit: more samples than wet cells (n_samples > n_wet), where the reference's IncrementalPCA
// runs one batch of more rows than columns (n_samples <= 5 n_wet) or several batches.  With n_components = None it keeps all n_wet
// components in every partial_fit, so nothing is truncated and the multi-batch fit equals the PCA of the whole centred matrix up to
// rounding: the eigendecomposition of C = Xc2^T Xc2 (n_wet x n_wet) gives its eigenvalues and, as eigenvectors, its components.
//
// The one-thread-per-cell kernels of pca_fit.h walk every row in one dependent chain; a tall x has few cells and many rows, so the
// statistics and the centring here are parallel over rows, in an order that is still fixed by the row count alone:
//
//   0. operation list: numpy reduces a long contiguous column in pieces of np.getbufsize() = 8192 elements, each piece in its pairwise
//                  tree (pcafit_pairwise_ops), and adds the piece sums left to right (pcafit_chunked_ops).  Up to 8192 rows this is the
//                  single tree of the Gram route.  The list is a program for the stack machine of pcafit_pairwise.
//   1. leaf pass:  one thread per (leaf, column): the leaf's sum exactly as a leaf of pcafit_pairwise forms it, and for the statistics
//                  the leaf's max / min / NaN flag of g(x).  Lanes of a wave read consecutive cells of one row.
//   2. combine:    one thread per column replays the operation list over the leaf sums (<= rows / 64 loads) and reduces max / min /
//                  NaN (order-free): the class of _classify_depths and mean = s / n; for the second centring (0 + s) / n.
//   3. compaction: Xc1 = (v - mu) w elementwise over (rows, ldc), padding columns zero.
//   4. centring:   m2 = colmean(Xc1) by the same leaf / combine pair: fixed order, two fits give the same bits.  It is NOT scikit-learn's
//                  incremental mean of several batches bit for bit (that one merges batch means by counts); the difference is a
//                  rounding of the mean, inside the bounds of the fit's error model.
//                  Xc2^T = (Xc1 - m2)^T is written cell-major (round_up(n_wet, 16), round_up(rows, 16)) with zero padding, through a
//                  padded LDS tile: rows of Xc1 are read along the cells, rows of Xc2^T are written along the samples.
//   5. covariance: gram_lower on Xc2^T (K = rows), the split-K reduction and mirroring of the Gram route.
//   6. components: the k leading eigenvectors as rows, svd_flip (pcafit_sign_flip_kernel), Z = Xc1 E^T.
//
// "pcafit_rowsplit" = 0 runs steps 1-4 with pcafit_colstats_kernel / pcafit_compact_kernel on the same operation list: same bits.
#pragma once
#include <vector>

#include "pca_fit.h"

namespace gprx {

constexpr int PCAFIT_PIECE = 8192;  // np.getbufsize(): elements per buffered piece of a reduction
constexpr int PCAFIT_LEAF_COLS = 64, PCAFIT_LEAF_GROUP = 4;  // a workgroup of the leaf pass: 64 columns x 4 leaves

// post-order program of numpy's sum of one contiguous column of n rows: per piece its pairwise tree, then (all but the first) the
// addition that folds it into the running sum
inline void pcafit_chunked_ops(int64_t n, std::vector<int2>& ops, int& max_depth) {
  for (int64_t s0 = 0; s0 < n; s0 += PCAFIT_PIECE) {
    const int len = (int)(n - s0 < PCAFIT_PIECE ? n - s0 : PCAFIT_PIECE);
    pcafit_pairwise_ops((int)s0, len, s0 ? 1 : 0, ops, max_depth);
    if (s0) ops.push_back(make_int2(-1, 0));
  }
}

// the sum of one leaf {s0, n <= 128}: the arithmetic of a leaf of pcafit_pairwise
template <class F>
__device__ __forceinline__ double pcafit_leaf_sum(F val, int s0, int n) {
#pragma clang fp contract(off)
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
  return res;
}

// Leaf pass.  x: (rows, ld) row-major, `cols` columns used; leaves: {first row, count} in the order of the operation list.  Workgroup
// b covers columns 64 (b % ncb) ... and leaves 4 (b / ncb) ...; lsum / lmax / lmin / lnan: (nleaves, cols).
// STATS: x is the raw input, the summed value is the PCA input (x, or the depth) and max / min / NaN of g(x) ride along as in
// pcafit_colstats_kernel; otherwise x is summed as it is and lmax / lmin / lnan are not touched.
template <bool STATS>
__global__ __launch_bounds__(256) void pcafit_leaf_kernel(const double* __restrict__ x, int64_t ld, int64_t cols, const double* __restrict__ elev,
                                                          int mode, const int2* __restrict__ leaves, int64_t nleaves, int64_t ncb,
                                                          double* __restrict__ lsum, double* __restrict__ lmax, double* __restrict__ lmin,
                                                          unsigned char* __restrict__ lnan) {
#pragma clang fp contract(off)
  const int64_t b = blockIdx.x;
  const int64_t c = (b % ncb) * PCAFIT_LEAF_COLS + (threadIdx.x & (PCAFIT_LEAF_COLS - 1));
  const int64_t leaf = (b / ncb) * PCAFIT_LEAF_GROUP + (threadIdx.x / PCAFIT_LEAF_COLS);
  if (c >= cols || leaf >= nleaves) return;
  const int2 lf = leaves[leaf];
  const double* col = x + c;
  if constexpr (STATS) {
    const double e = (mode == PCAFIT_VELOCITY) ? 0.0 : elev[c];
    double mx = -INFINITY, mn = INFINITY;
    bool nan = false;
    auto val = [&](int t) {
      double v = col[(int64_t)t * ld];
      const double g = (mode == PCAFIT_DEPTH) ? pcafit_depth(v, e) : v - e;
      if (mode == PCAFIT_DEPTH) v = g;
      nan |= g != g;
      mx = g > mx ? g : mx;
      mn = g < mn ? g : mn;
      return v;
    };
    lsum[leaf * cols + c] = pcafit_leaf_sum(val, lf.x, lf.y);
    lmax[leaf * cols + c] = mx;
    lmin[leaf * cols + c] = mn;
    lnan[leaf * cols + c] = nan ? 1 : 0;
  } else {
    lsum[leaf * cols + c] = pcafit_leaf_sum([&](int t) { return col[(int64_t)t * ld]; }, lf.x, lf.y);
  }
}

// Combine pass, one thread per column: the stack machine of pcafit_pairwise with a load of the next leaf sum where that one sums a leaf.
// STATS: cls / mean as pcafit_colstats_kernel writes them; otherwise mean = (0 + s) / rows, IncrementalPCA's col_mean.
template <bool STATS>
__global__ __launch_bounds__(256) void pcafit_combine_kernel(const double* __restrict__ lsum, const double* __restrict__ lmax,
                                                             const double* __restrict__ lmin, const unsigned char* __restrict__ lnan, int64_t cols,
                                                             int64_t rows, const int2* __restrict__ ops, int nops, int mode, double thr,
                                                             unsigned char* __restrict__ cls, double* __restrict__ mean) {
#pragma clang fp contract(off)
  __shared__ double stk_all[PCAFIT_STACK * 256];
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= cols) return;
  double* stk = stk_all + threadIdx.x;
  double mx = -INFINITY, mn = INFINITY;
  bool nan = false;
  int sp = 0;
  int64_t leaf = 0;
  for (int o = 0; o < nops; ++o) {
    if (ops[o].x < 0) {
      stk[(sp - 2) * 256] = stk[(sp - 2) * 256] + stk[(sp - 1) * 256];
      --sp;
      continue;
    }
    const int64_t at = leaf * cols + c;
    stk[sp * 256] = lsum[at];
    if constexpr (STATS) {
      const double a = lmax[at], b = lmin[at];
      nan |= lnan[at] != 0;
      mx = a > mx ? a : mx;
      mn = b < mn ? b : mn;
    }
    ++leaf;
    ++sp;
  }
  const double s = stk[0];
  if constexpr (STATS) {
    unsigned char k = 2;  // velocity: every cell TF
    if (mode != PCAFIT_VELOCITY) {
      k = 0;
      if (!nan) {
        if (mx < thr) k = 1;
        if (mx > thr) k = 2;
        if (mn > thr) k = 3;
      }
    }
    cls[c] = k;
    mean[c] = s / (double)rows;
  } else {
    mean[c] = (0.0 + s) / (double)rows;
  }
}

// Compaction, elementwise: xc1 (rows, ldc) = (v(x[t, c_j]) - mu) w over the wet cells, zeros in the padding columns; the arithmetic of
// pcafit_compact_kernel.  Grid: (column blocks of 256, row lanes); a row lane strides over the rows.
__global__ __launch_bounds__(256) void pcafit_compact_rows_kernel(const double* __restrict__ x, int64_t rows, int64_t cells,
                                                                  const int64_t* __restrict__ idx, int64_t n_wet, int64_t ldc,
                                                                  const double* __restrict__ elev, int mode, const double* __restrict__ mu,
                                                                  const double* __restrict__ w, double* __restrict__ xc1) {
#pragma clang fp contract(off)
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= ldc) return;
  if (j >= n_wet) {
    for (int64_t t = blockIdx.y; t < rows; t += gridDim.y) xc1[t * ldc + j] = 0.0;
    return;
  }
  const int64_t c = idx[j];
  const double e = (mode == PCAFIT_DEPTH) ? elev[c] : 0.0, m = mu[c];
  const double wc = w ? w[c] : 1.0;
  for (int64_t t = blockIdx.y; t < rows; t += gridDim.y) {
    double v = x[t * cells + c];
    if (mode == PCAFIT_DEPTH) v = pcafit_depth(v, e);
    v = v - m;
    if (w) v = v * wc;
    xc1[t * ldc + j] = v;
  }
}

// dst (r2, ldt) cell-major = (src - m2)^T of src (rows, lds) over its first n columns (m2 null: src is centred already), zeros for
// j in [n, r2) and t in [rows, ldt).  32 x 32 tiles through LDS (odd row stride: no bank conflicts): the read runs along the cells of
// a row of src, the write along the samples of a row of dst.  Grid: (ceil(ldt / 32), ceil(r2 / 32)).
__global__ __launch_bounds__(256) void pcafit_centre_t_kernel(const double* __restrict__ src, int64_t rows, int64_t lds, int64_t n,
                                                              const double* __restrict__ m2, double* __restrict__ dst, int64_t r2, int64_t ldt) {
#pragma clang fp contract(off)
  __shared__ double tile[32][33];
  const int64_t t0 = (int64_t)blockIdx.x * 32, j0 = (int64_t)blockIdx.y * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int k = ty; k < 32; k += 8) {
    const int64_t t = t0 + k, j = j0 + tx;
    double v = 0.0;
    if (t < rows && j < n) {
      v = src[t * lds + j];
      if (m2) v = v - m2[j];
    }
    tile[k][tx] = v;
  }
  __syncthreads();
  for (int k = ty; k < 32; k += 8) {
    const int64_t j = j0 + k, t = t0 + tx;
    if (j < r2 && t < ldt) dst[j * ldt + t] = tile[tx][k];
  }
}

// E (k, lde): row i = the eigenvector of the (i + 1)-th largest eigenvalue, from the device eigenpairs U (n, n) with eigenvectors in
// columns and ascending eigenvalues: E[i][j] = U[j][n - 1 - i]; the padding [n, lde) is zero.
__global__ __launch_bounds__(256) void pcafit_gather_v_kernel(const double* __restrict__ U, int64_t n, int k, double* __restrict__ E, int64_t lde) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)k * lde) return;
  const int64_t i = e / lde, j = e % lde;
  E[e] = j < n ? U[j * n + (n - 1 - i)] : 0.0;
}

}  // namespace gprx
