// Symmetric eigensolver on the device: parallel two-sided block Jacobi in fp64.
//
//   A (n, n) symmetric, row-major with leading dimension lda, is driven to diagonal form by orthogonal similarity transforms; V
//   accumulates them.  The indices are cut into m = ceil(n / EIG_B) blocks of width EIG_B = 32 (the last one may be narrower).  A
//   sweep is the round-robin tournament over the block pairs (eig_rr_pair: m - 1 rounds of m / 2 disjoint pairs for even m, m rounds
//   with one bye each for odd m); a round is three batched launches, the pair index in the grid:
//     1. eig_pair_solve_kernel   one workgroup per pair (I, J): gathers the w x w submatrix A[I u J, I u J] (w <= 64, lower
//                                triangle, mirrored) into LDS and diagonalises it there by cyclic Jacobi with a parallel rotation
//                                ordering (the same tournament over the w indices: w / 2 disjoint rotations per step, applied
//                                as one pass over 2 x 2 blocks), accumulating Q.  The columns of Q are brought to unit length
//                                and ordered by ascending eigenvalue; Q (64 x 64, zero padded) and the eigenvalues go to the workspace.
//     2. eig_apply_kernel<false> columns: A[:, I u J] <- A[:, I u J] Q and V[:, I u J] <- V[:, I u J] Q in place; a workgroup
//                                owns 64 rows of one pair, strip and Q in LDS, the product on v_mfma_f64_16x16x4_f64 (K = 64).
//     3. eig_apply_kernel<true>  rows: A[I u J, :] <- Q^T A[I u J, :], 64 columns per workgroup; launched after the column phase
//                                of the whole round.  The pair's own diagonal block is written as diag(eigenvalues) exactly.
//   After every sweep eig_off_rows_kernel / eig_off_total_kernel reduce off(A)^2 (strict lower triangle, doubled) and the squared
//   diagonal in a fixed order, and the host reads those two numbers.  Stop: off(A)_F <= n eps ||A||_F, also tested before the first
//   sweep (a diagonal input takes none).  30 sweeps without that, or a non-finite norm, end the run without a result.
//   eig_rank_kernel / eig_sign_kernel / eig_permute_kernel sort the eigenvalues ascending (ties by index), turn every eigenvector
//   so that its entry of largest magnitude (lowest index on ties) is positive and write both out.
// No atomics, and no summation whose order depends on the grid: two runs give the same bits.
#pragma once
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <vector>

#include "gprx_common.h"

namespace gprx {

constexpr int EIG_B = 32;          // block width
constexpr int EIG_W = 2 * EIG_B;   // rows of a pair problem, tile of the two update phases
constexpr int EIG_LD = EIG_W + 1;  // LDS row stride of the 64 x 64 images
constexpr int EIG_MAX_SWEEPS = 30;
constexpr int EIG_INNER_SWEEPS = 30;
constexpr size_t EIG_PAIR_SMEM = sizeof(double) * (2 * EIG_W * EIG_LD + 2 * EIG_B + 256 + EIG_W) + sizeof(int) * EIG_W;
constexpr size_t EIG_APPLY_SMEM = sizeof(double) * (2 * EIG_W * EIG_LD);

// Pair `k` (0 <= k < mm / 2) of round `t` (0 <= t < mm - 1) of the round-robin tournament over mm players, mm even: player
// mm - 1 stays, the others turn.  Every unordered pair meets once in mm - 1 rounds, nobody twice in a round.  x < y.
__host__ __device__ inline void eig_rr_pair(int mm, int t, int k, int& x, int& y) {
  int a, b;
  if (k == 0) {
    a = mm - 1;
    b = t;
  } else {
    a = (t + k) % (mm - 1);
    b = (t - k + (mm - 1)) % (mm - 1);
  }
  x = a < b ? a : b;
  y = a < b ? b : a;
}

// one block pair of a round: start and width of both index ranges (wj = 0: the block alone, m = 1)
struct EigPair {
  int i0, wi, j0, wj;
};
__device__ __forceinline__ int eig_gidx(const EigPair& p, int a) { return a < p.wi ? p.i0 + a : p.j0 + (a - p.wi); }

// upper triangle <- lower triangle
__global__ __launch_bounds__(256) void eig_mirror_kernel(double* __restrict__ A, int64_t lda, int n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n * n) return;
  const int i = (int)(e / n), j = (int)(e % n);
  if (j > i) A[(int64_t)i * lda + j] = A[(int64_t)j * lda + i];
}

__global__ __launch_bounds__(256) void eig_identity_kernel(double* __restrict__ V, int64_t ldv, int n) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n * n) return;
  const int i = (int)(e / n), j = (int)(e % n);
  V[(int64_t)i * ldv + j] = i == j ? 1.0 : 0.0;
}

// sum of the 256 values of a workgroup in a fixed tree; every thread gets it
__device__ __forceinline__ double eig_block_sum(double v, double* __restrict__ red, int tid) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (tid < h) red[tid] = red[tid] + red[tid + h];
    __syncthreads();
  }
  return red[0];
}

// ---- 1. pair solve ----------------------------------------------------------------------------------------------------------
// Qw: (pairs, 64, 64) row-major, column c = eigenvector of the c-th smallest eigenvalue, zero outside w x w; lamw: (pairs, 64).
// Vone non-null (m = 1, one workgroup, the block is the whole matrix): the kernel is the whole sweep: it writes V = Q to Vone (w, ldv)
// and diag(eigenvalues) over A, and Qw / lamw are not touched.
__global__ __launch_bounds__(256) void eig_pair_solve_kernel(double* __restrict__ A, int64_t lda, const EigPair* __restrict__ pairs,
                                                             double* __restrict__ Qw, double* __restrict__ lamw, double* __restrict__ Vone,
                                                             int64_t ldv) {
#pragma clang fp contract(off)
  extern __shared__ double eig_smem[];
  double* S = eig_smem;                  // [64][EIG_LD]
  double* Q = S + EIG_W * EIG_LD;        // [64][EIG_LD]
  double* cs = Q + EIG_W * EIG_LD;       // c, s of the step's rotations [2][32]
  double* red = cs + 2 * EIG_B;          // [256]
  double* lam = red + 256;               // [64]
  int* rank = reinterpret_cast<int*>(lam + EIG_W);  // [64]
  const int tid = threadIdx.x;
  const EigPair pr = pairs[blockIdx.x];
  const int w = pr.wi + pr.wj;
  const int we = (w + 1) & ~1;  // players of the rotation tournament (an odd w gets a dummy index w: its rotations are skipped)
  for (int e = tid; e < EIG_W * EIG_W; e += 256) {
    const int a = e >> 6, b = e & 63;
    double v = 0.0;
    if (a < w && b < w) {
      const int ga = eig_gidx(pr, a), gb = eig_gidx(pr, b);
      v = ga >= gb ? A[(int64_t)ga * lda + gb] : A[(int64_t)gb * lda + ga];
    }
    S[a * EIG_LD + b] = v;
    Q[a * EIG_LD + b] = a == b ? 1.0 : 0.0;
  }
  __syncthreads();
  const int half = we >> 1;
  for (int sweep = 0; sweep < EIG_INNER_SWEEPS && w > 1; ++sweep) {
    // off(S)^2 against eps^2 ||S||_F^2
    double off = 0.0, all = 0.0;
    for (int e = tid; e < EIG_W * EIG_W; e += 256) {
      const int a = e >> 6, b = e & 63;
      const double v = S[a * EIG_LD + b];
      all += v * v;
      if (a != b) off += v * v;
    }
    off = eig_block_sum(off, red, tid);
    all = eig_block_sum(all, red, tid);
    if (!(off > (DBL_EPSILON * DBL_EPSILON) * all)) break;  // converged, or not finite
    // Threshold Jacobi: entries below 1 % of the root-mean-square off-diagonal entry are left for a later sweep.  Inside a cluster
    // of equal eigenvalues the entries are of second order but their rotation angles are arbitrary, and rotating them scrambles
    // the first-order entries: without the threshold a 64 x 64 block of c I + u u^T + w w^T converges linearly (30 sweeps are not enough).
    const double thr2 = 1e-4 * off / (double)(w * (w - 1));
    for (int t = 0; t < we - 1; ++t) {
      if (tid < half) {
        int p, q;
        eig_rr_pair(we, t, tid, p, q);
        double c = 1.0, s = 0.0;
        if (q < w) {
          const double apq = S[q * EIG_LD + p];
          if (apq != 0.0 && apq * apq >= thr2) {
            const double tau = (S[q * EIG_LD + q] - S[p * EIG_LD + p]) / (2.0 * apq);
            const double tt = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
            c = 1.0 / sqrt(1.0 + tt * tt);
            s = tt * c;
          }
        }
        cs[tid] = c;
        cs[EIG_B + tid] = s;
      }
      __syncthreads();
      // S <- J^T S J over the 2 x 2 blocks (rotation k, rotation l); block (k, l) with k < l is computed as block (l, k) and
      // written transposed, so S stays symmetric bit for bit
      for (int e = tid; e < half * half; e += 256) {
        const int k = e / half, l = e % half;
        const int kh = k > l ? k : l, kl = k > l ? l : k;
        int ph, qh, pl, ql;
        eig_rr_pair(we, t, kh, ph, qh);
        eig_rr_pair(we, t, kl, pl, ql);
        const double ch = cs[kh], sh = cs[EIG_B + kh], cl = cs[kl], sl = cs[EIG_B + kl];
        double b00, b01, b10, b11;
        if (kh == kl) {
          const double app = S[ph * EIG_LD + ph], aqq = S[qh * EIG_LD + qh], apq = S[qh * EIG_LD + ph];
          if (sh != 0.0) {
            const double tt = sh / ch;
            b00 = app - tt * apq;
            b11 = aqq + tt * apq;
            b01 = b10 = 0.0;
          } else {
            b00 = app;
            b11 = aqq;
            b01 = b10 = apq;
          }
        } else {
          // a thread reads only the block it writes: for k < l the entries of block (l, k) from their mirror images
          double a00, a01, a10, a11;
          if (k >= l) {
            a00 = S[ph * EIG_LD + pl], a01 = S[ph * EIG_LD + ql], a10 = S[qh * EIG_LD + pl], a11 = S[qh * EIG_LD + ql];
          } else {
            a00 = S[pl * EIG_LD + ph], a01 = S[ql * EIG_LD + ph], a10 = S[pl * EIG_LD + qh], a11 = S[ql * EIG_LD + qh];
          }
          const double r00 = cl * a00 - sl * a01, r01 = sl * a00 + cl * a01, r10 = cl * a10 - sl * a11, r11 = sl * a10 + cl * a11;
          b00 = ch * r00 - sh * r10;
          b01 = ch * r01 - sh * r11;
          b10 = sh * r00 + ch * r10;
          b11 = sh * r01 + ch * r11;
        }
        if (k >= l) {
          S[ph * EIG_LD + pl] = b00;
          S[ph * EIG_LD + ql] = b01;
          S[qh * EIG_LD + pl] = b10;
          S[qh * EIG_LD + ql] = b11;
        } else {
          S[pl * EIG_LD + ph] = b00;
          S[ql * EIG_LD + ph] = b01;
          S[pl * EIG_LD + qh] = b10;
          S[ql * EIG_LD + qh] = b11;
        }
      }
      // Q <- Q J
      for (int e = tid; e < w * half; e += 256) {
        const int i = e / half, l = e % half;
        int p, q;
        eig_rr_pair(we, t, l, p, q);
        const double c = cs[l], s = cs[EIG_B + l];
        if (s != 0.0) {
          const double qp = Q[i * EIG_LD + p], qq = Q[i * EIG_LD + q];
          Q[i * EIG_LD + p] = c * qp - s * qq;
          Q[i * EIG_LD + q] = s * qp + c * qq;
        }
      }
      __syncthreads();
    }
  }
  // ascending eigenvalues, ties by index; the columns of Q are brought back to unit length (c^2 + s^2 = 1 holds to rounding only,
  // and the error of several hundred rotations accumulates in the length of a column, not in the angle between two)
  if (tid < EIG_W) lam[tid] = tid < w ? S[tid * EIG_LD + tid] : 0.0;
  __syncthreads();
  if (tid < w) {
    double nrm = 0.0;
    for (int i = 0; i < w; ++i) nrm += Q[i * EIG_LD + tid] * Q[i * EIG_LD + tid];
    cs[tid] = 1.0 / sqrt(nrm);
    const double v = lam[tid];
    int r = 0;
    for (int j = 0; j < w; ++j) {
      const double u = lam[j];
      r += (u < v || (u == v && j < tid)) ? 1 : 0;
    }
    rank[tid] = r;
  }
  __syncthreads();
  if (Vone) {
    for (int e = tid; e < w * w; e += 256) {
      const int i = e / w, c = e % w;
      Vone[(int64_t)i * ldv + c] = Q[i * EIG_LD + c] * cs[c];  // unsorted, as the diagonal: the finishing pass orders both
      A[(int64_t)i * lda + c] = i == c ? lam[i] : 0.0;  // w = n, the block starts at 0
    }
    return;
  }
  double* qo = Qw + (int64_t)blockIdx.x * EIG_W * EIG_W;
  double* lo = lamw + (int64_t)blockIdx.x * EIG_W;
  for (int e = tid; e < EIG_W * EIG_W; e += 256) qo[e] = 0.0;
  if (tid < EIG_W) lo[tid] = 0.0;
  __syncthreads();
  for (int e = tid; e < w * w; e += 256) {
    const int i = e / w, c = e % w;
    qo[i * EIG_W + rank[c]] = Q[i * EIG_LD + c] * cs[c];
  }
  if (tid < w) lo[rank[tid]] = lam[tid];
}

// ---- 2. / 3. the update phases --------------------------------------------------------------------------------------------------
// ROWS = false: X[r0 .. r0 + 64, I u J] <- X[...] Q for X = A (blockIdx.y < strips) and X = V (blockIdx.y >= strips).
// ROWS = true:  A[I u J, c0 .. c0 + 64] <- Q^T A[...]; entries of the pair's own diagonal block become diag(lamw).
// MFMA layout (v_mfma_f64_16x16x4_f64): lane (g = lane >> 4, r = lane & 15) supplies L[row r][k = 4 j + g] and R[k][col r] to
// instruction j of a 16-deep group and holds C[g + 4 q][r] in acc[q].  Wave (wm, wn) owns the 32 x 32 quarter of the 64 x 64 tile.
template <bool ROWS>
__global__ __launch_bounds__(256) void eig_apply_kernel(double* __restrict__ A, int64_t lda, double* __restrict__ V, int64_t ldv, int n, int strips,
                                                        const EigPair* __restrict__ pairs, const double* __restrict__ Qw,
                                                        const double* __restrict__ lamw) {
  extern __shared__ double eig_smem[];
  double* sX = eig_smem;              // ROWS: [k][col]; else [row][k]
  double* sQ = sX + EIG_W * EIG_LD;   // [k][c]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1, g = lane >> 4, r = lane & 15;
  const EigPair pr = pairs[blockIdx.x];
  const int w = pr.wi + pr.wj;
  int strip = (int)blockIdx.y;
  double* X = A;
  int64_t ldx = lda;
  if (!ROWS && strip >= strips) {
    strip -= strips;
    X = V;
    ldx = ldv;
  }
  const int o0 = strip * EIG_W;  // first row (columns phase) / first column (rows phase) of the strip
  const double* q = Qw + (int64_t)blockIdx.x * EIG_W * EIG_W;
  for (int e = tid; e < EIG_W * EIG_W; e += 256) {
    const int a = e >> 6, b = e & 63;
    sQ[a * EIG_LD + b] = q[e];
    double v = 0.0;
    if (ROWS) {  // a: index within the pair, b: column of the strip
      if (a < w && o0 + b < n) v = X[(int64_t)eig_gidx(pr, a) * ldx + o0 + b];
    } else {  // a: row of the strip, b: index within the pair
      if (b < w && o0 + a < n) v = X[(int64_t)(o0 + a) * ldx + eig_gidx(pr, b)];
    }
    sX[a * EIG_LD + b] = v;
  }
  __syncthreads();
  d4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
  for (int kb = 0; kb < EIG_W / 16; ++kb) {
    double fa[2][4], fb[2][4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = kb * 16 + 4 * j + g;
#pragma unroll
      for (int a = 0; a < 2; ++a) {
        const int row = wm * 32 + a * 16 + r;
        fa[a][j] = ROWS ? sQ[k * EIG_LD + row] : sX[row * EIG_LD + k];
      }
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const int col = wn * 32 + b * 16 + r;
        fb[b][j] = ROWS ? sX[k * EIG_LD + col] : sQ[k * EIG_LD + col];
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a][j], fb[b][j], acc[a][b], 0, 0, 0);
  }
  const double* lw = lamw + (int64_t)blockIdx.x * EIG_W;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int qq = 0; qq < 4; ++qq) {
        const int row = wm * 32 + a * 16 + g + 4 * qq, col = wn * 32 + b * 16 + r;
        double v = acc[a][b][qq];
        if (ROWS) {
          const int gc = o0 + col;
          if (row >= w || gc >= n) continue;
          int pc = -1;  // position of column gc within the pair, if it belongs to it
          if (gc >= pr.i0 && gc < pr.i0 + pr.wi) pc = gc - pr.i0;
          if (gc >= pr.j0 && gc < pr.j0 + pr.wj) pc = pr.wi + gc - pr.j0;
          if (pc >= 0) v = pc == row ? lw[row] : 0.0;
          X[(int64_t)eig_gidx(pr, row) * ldx + gc] = v;
        } else {
          if (col >= w || o0 + row >= n) continue;
          X[(int64_t)(o0 + row) * ldx + eig_gidx(pr, col)] = v;
        }
      }
}

// ---- the stop rule ----------------------------------------------------------------------------------------------------------------
// part[i] = sum_{j < i} A[i][j]^2, part[n + i] = A[i][i]^2: one workgroup per row, fixed tree
__global__ __launch_bounds__(256) void eig_off_rows_kernel(const double* __restrict__ A, int64_t lda, int n, double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int i = (int)blockIdx.x, tid = threadIdx.x;
  const double* row = A + (int64_t)i * lda;
  double s = 0.0;
  for (int j = tid; j < i; j += 256) s += row[j] * row[j];
  s = eig_block_sum(s, red, tid);
  if (tid == 0) {
    part[i] = s;
    part[n + i] = row[i] * row[i];
  }
}
// out[0] = off(A)_F^2 = 2 sum part[0 .. n), out[1] = sum of the squared diagonal: one workgroup
__global__ __launch_bounds__(256) void eig_off_total_kernel(const double* __restrict__ part, int n, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double red[256];
  const int tid = threadIdx.x;
  double s = 0.0, d = 0.0;
  for (int i = tid; i < n; i += 256) {
    s += part[i];
    d += part[n + i];
  }
  s = eig_block_sum(s, red, tid);
  d = eig_block_sum(d, red, tid);
  if (tid == 0) {
    out[0] = 2.0 * s;
    out[1] = d;
  }
}

// ---- sort and sign --------------------------------------------------------------------------------------------------------------
// rank[i] = position of A[i][i] in ascending order, ties by index
__global__ __launch_bounds__(256) void eig_rank_kernel(const double* __restrict__ A, int64_t lda, int n, int* __restrict__ rank) {
  const int i = (int)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double v = A[(int64_t)i * lda + i];
  int r = 0;
  for (int j = 0; j < n; ++j) {
    const double u = A[(int64_t)j * lda + j];
    r += (u < v || (u == v && j < i)) ? 1 : 0;
  }
  rank[i] = r;
}
// sgn[c] = -1 when the entry of largest magnitude of column c of V (lowest row on ties) is negative, else 1
__global__ __launch_bounds__(256) void eig_sign_kernel(const double* __restrict__ V, int64_t ldv, int n, double* __restrict__ sgn) {
  const int c = (int)blockIdx.x * 256 + threadIdx.x;
  if (c >= n) return;
  double best = -1.0, piv = 0.0;
  for (int i = 0; i < n; ++i) {
    const double v = V[(int64_t)i * ldv + c], a = fabs(v);
    if (a > best) {
      best = a;
      piv = v;
    }
  }
  sgn[c] = piv < 0.0 ? -1.0 : 1.0;
}
// lam[rank[c]] = A[c][c]; Vout[:, rank[c]] = sgn[c] V[:, c]
__global__ __launch_bounds__(256) void eig_permute_kernel(const double* __restrict__ A, int64_t lda, const double* __restrict__ V, int64_t ldw, int n,
                                                          const int* __restrict__ rank, const double* __restrict__ sgn, double* __restrict__ lam,
                                                          double* __restrict__ Vout, int64_t ldv) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)n * n) return;
  const int i = (int)(e / n), c = (int)(e % n);
  const int rc = rank[c];
  Vout[(int64_t)i * ldv + rc] = sgn[c] * V[(int64_t)i * ldw + c];
  if (i == 0) lam[rc] = A[(int64_t)c * lda + c];
}

// ---- host driver ----------------------------------------------------------------------------------------------------------------
// the pairs of every round of a sweep over m blocks of n indices, round after round; rounds[r] = first pair of round r
inline void eig_schedule(int n, std::vector<EigPair>& pairs, std::vector<int>& rounds) {
  const int m = (n + EIG_B - 1) / EIG_B;
  auto width = [&](int blk) { return blk * EIG_B + EIG_B <= n ? EIG_B : n - blk * EIG_B; };
  pairs.clear();
  rounds.assign(1, 0);
  if (m == 1) {
    pairs.push_back(EigPair{0, n, 0, 0});
    rounds.push_back(1);
    return;
  }
  const int mm = (m + 1) & ~1;
  for (int t = 0; t < mm - 1; ++t) {
    for (int k = 0; k < mm / 2; ++k) {
      int x, y;
      eig_rr_pair(mm, t, k, x, y);
      if (y >= m) continue;  // the bye of an odd block count
      pairs.push_back(EigPair{x * EIG_B, width(x), y * EIG_B, width(y)});
    }
    rounds.push_back((int)pairs.size());
  }
}

// device workspace of one run, in doubles: working V (n, n), Q and eigenvalues of a round's pairs, row partials, the two norms,
// signs, ranks, the pair table
struct EigLayout {
  size_t v, qw, lamw, part, norms, sgn, rank, pairs, total;
};
inline EigLayout eig_layout(int n) {
  const size_t m = (size_t)(n + EIG_B - 1) / EIG_B, mm = (m + 1) & ~(size_t)1;
  const size_t per_round = m == 1 ? 1 : mm / 2, all_pairs = m == 1 ? 1 : (mm - 1) * (mm / 2);
  EigLayout l;
  size_t o = 0;
  auto take = [&](size_t doubles) {
    const size_t at = o;
    o += (doubles + 15) / 16 * 16;
    return at;
  };
  l.v = take((size_t)n * n);
  l.qw = take(per_round * EIG_W * EIG_W);
  l.lamw = take(per_round * EIG_W);
  l.part = take(2 * (size_t)n);
  l.norms = take(2);
  l.sgn = take((size_t)n);
  l.rank = take(((size_t)n + 1) / 2);
  l.pairs = take(all_pairs * 2);  // an EigPair is 16 bytes
  l.total = o;
  return l;
}
inline size_t eig_jacobi_workspace_bytes_impl(int n) { return sizeof(double) * eig_layout(n).total; }

// A (n, lda): symmetric input, lower triangle read, overwritten.  V (n, ldv): eigenvectors in columns, lam (n): ascending eigenvalues.
// All device pointers; ws: eig_jacobi_workspace_bytes(n).  Synchronises the stream once per sweep.  sweeps, off_rel = off(A)_F / ||A||_F
// at the end.  Returns hipSuccess and *status = 0 (converged) or 1 (sweep cap reached or a non-finite norm: lam and V are not written).
inline hipError_t eig_jacobi_run_impl(hipStream_t st, int n, double* A, int64_t lda, double* V, int64_t ldv, double* lam, double* ws, int* sweeps,
                                      double* off_rel, int* status) {
  hipError_t e;
  // kernels with more than 64 KiB of LDS need the raised dynamic-LDS limit: set once per device, as sf_launch_mid does
  static bool attr_set[64] = {};
  int dev = 0;
  if ((e = hipGetDevice(&dev)) != hipSuccess) return e;
  if (dev < 0 || dev >= 64 || !attr_set[dev]) {
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(eig_pair_solve_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)EIG_PAIR_SMEM)) != hipSuccess)
      return e;
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(eig_apply_kernel<false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)EIG_APPLY_SMEM)) != hipSuccess)
      return e;
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(eig_apply_kernel<true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)EIG_APPLY_SMEM)) != hipSuccess)
      return e;
    if (dev >= 0 && dev < 64) attr_set[dev] = true;
  }
  const EigLayout l = eig_layout(n);
  double *W = ws + l.v, *Qw = ws + l.qw, *lamw = ws + l.lamw, *part = ws + l.part, *norms = ws + l.norms, *sgn = ws + l.sgn;
  int* rank = reinterpret_cast<int*>(ws + l.rank);
  EigPair* dpairs = reinterpret_cast<EigPair*>(ws + l.pairs);
  std::vector<EigPair> pairs;
  std::vector<int> rounds;
  eig_schedule(n, pairs, rounds);
  if ((e = hipMemcpyAsync(dpairs, pairs.data(), sizeof(EigPair) * pairs.size(), hipMemcpyHostToDevice, st)) != hipSuccess) return e;
  const unsigned nn = (unsigned)(((int64_t)n * n + 255) / 256);
  const int strips = (n + EIG_W - 1) / EIG_W;
  hipLaunchKernelGGL(eig_mirror_kernel, dim3(nn), dim3(256), 0, st, A, lda, n);
  hipLaunchKernelGGL(eig_identity_kernel, dim3(nn), dim3(256), 0, st, W, (int64_t)n, n);
  *sweeps = 0;
  *status = 1;
  double h[2] = {0.0, 0.0}, fro2 = 0.0;
  for (int sweep = 0;; ++sweep) {
    hipLaunchKernelGGL(eig_off_rows_kernel, dim3((unsigned)n), dim3(256), 0, st, (const double*)A, lda, n, part);
    hipLaunchKernelGGL(eig_off_total_kernel, dim3(1), dim3(256), 0, st, (const double*)part, n, norms);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if ((e = hipMemcpyAsync(h, norms, sizeof(h), hipMemcpyDeviceToHost, st)) != hipSuccess) return e;
    if ((e = hipStreamSynchronize(st)) != hipSuccess) return e;
    if (sweep == 0) fro2 = h[0] + h[1];  // ||A||_F^2 of the input: orthogonal similarity keeps it
    *sweeps = sweep;
    *off_rel = fro2 > 0.0 ? std::sqrt(h[0] / fro2) : h[0];
    if (!std::isfinite(h[0]) || !std::isfinite(fro2)) return hipSuccess;
    const double thr = (double)n * DBL_EPSILON;
    if (h[0] <= thr * thr * fro2) break;
    if (sweep == EIG_MAX_SWEEPS) return hipSuccess;
    for (size_t rd = 0; rd + 1 < rounds.size(); ++rd) {
      const int np = rounds[rd + 1] - rounds[rd];
      if (np == 0) continue;
      const EigPair* pp = dpairs + rounds[rd];
      if (n <= EIG_B) {  // m = 1: the pair solve alone
        hipLaunchKernelGGL(eig_pair_solve_kernel, dim3(1), dim3(256), EIG_PAIR_SMEM, st, A, lda, pp, Qw, lamw, W, (int64_t)n);
        continue;
      }
      hipLaunchKernelGGL(eig_pair_solve_kernel, dim3((unsigned)np), dim3(256), EIG_PAIR_SMEM, st, A, lda, pp, Qw, lamw, (double*)nullptr,
                         (int64_t)0);
      hipLaunchKernelGGL(eig_apply_kernel<false>, dim3((unsigned)np, (unsigned)(2 * strips)), dim3(256), EIG_APPLY_SMEM, st, A, lda, W, (int64_t)n, n,
                         strips, pp, (const double*)Qw, (const double*)lamw);
      hipLaunchKernelGGL(eig_apply_kernel<true>, dim3((unsigned)np, (unsigned)strips), dim3(256), EIG_APPLY_SMEM, st, A, lda, W, (int64_t)n, n, strips,
                         pp, (const double*)Qw, (const double*)lamw);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  const unsigned nb = (unsigned)((n + 255) / 256);
  hipLaunchKernelGGL(eig_rank_kernel, dim3(nb), dim3(256), 0, st, (const double*)A, lda, n, rank);
  hipLaunchKernelGGL(eig_sign_kernel, dim3(nb), dim3(256), 0, st, (const double*)W, (int64_t)n, n, sgn);
  hipLaunchKernelGGL(eig_permute_kernel, dim3(nn), dim3(256), 0, st, (const double*)A, lda, (const double*)W, (int64_t)n, n, (const int*)rank,
                     (const double*)sgn, lam, V, ldv);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  *status = 0;
  return hipSuccess;
}

}  // namespace gprx
