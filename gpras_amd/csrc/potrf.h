// Blocked right-looking Cholesky (lower, in place, row-major) for gfx950.
//
// Per 64-column panel two launches:
//   1. potrf_panel_kernel  -- factor the 64 x 64 diagonal block AND solve every row below it
//      (L21 = A21 L11^-T, including the right-hand-side rows appended under the matrix) in one
//      launch.  A workgroup owns 128 panel rows: the 64 rows of the diagonal block -- every workgroup
//      re-factors it redundantly, so no inter-workgroup hand-off exists -- plus 64 rows of A21.
//      The 128 x 64 panel lives in the MFMA accumulators (wave w: rows 32 w .. 32 w + 31).  Work
//      proceeds in 8-column sub-panels: the sub-panel's columns go accumulators -> LDS, each thread
//      factors the 8 x 8 diagonal sub-block (register math) and solves its own row, then the
//      columns right of the sub-panel are updated on MFMA (rows x 8 times (64 x 8)^T) with the
//      operands read once from LDS and no read-modify-write of C; two barriers per sub-panel.  One
//      extra workgroup carries the 64 identity rows, which come out as L11^-1 (inverse of the
//      diagonal block, used by the triangular solves).
//   2. gemm_f64 (NT, C_LOWER, alpha = -1, beta = 1) -- trailing update A22 -= L21 L21^T on MFMA.
#pragma once
#include <cstdlib>
#include <utility>
#include <vector>

#include "chain64.h"
#include "gemm_f64.h"
#include "gprx_common.h"

namespace gprx {

// GPRX_PANEL_ACC (development builds, tools/panel_acc.sh): phase durations of panel workgroup 0 (a rows workgroup) summed over
// every panel launch of a factorisation -- [0] launches, [1] loads, [2] sub-panel 0, [3] sub-panels 1-3, [4] sub-panels 4-7,
// [5] stores (shader clocks)
#ifdef GPRX_PANEL_ACC
__device__ unsigned long long g_panel_acc[8];
#define PACC_DECL unsigned long long pacc_prev_ = 0;
#define PACC(i)                                                                                                       \
  {                                                                                                                   \
    if ((i) == 5) __builtin_amdgcn_s_waitcnt(0);                                                                      \
    const unsigned long long t_ = __builtin_amdgcn_s_memtime();                                                       \
    if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0 && gridDim.x > 2) {                                    \
      if ((i) > 0) atomicAdd(&g_panel_acc[i], t_ - pacc_prev_);                                                       \
      else atomicAdd(&g_panel_acc[0], 1ull);                                                                          \
    }                                                                                                                 \
    pacc_prev_ = t_;                                                                                                  \
  }
#else
#define PACC_DECL
#define PACC(i)
#endif
#ifdef GPRX_PANEL_STAMPS
__device__ unsigned long long g_panel_stamps[64];
#define PSTAMP(i)                                                                                                     \
  if (threadIdx.x == 0) {                                                                                             \
    if (blockIdx.x == 0) g_panel_stamps[i] = __builtin_amdgcn_s_memtime();                                            \
    if (blockIdx.x == gridDim.x / 2 && (i) < 6) g_panel_stamps[32 + (i)] = __builtin_amdgcn_s_memtime();               \
    if (blockIdx.x == gridDim.x - 2 && (i) < 6) g_panel_stamps[48 + (i)] = __builtin_amdgcn_s_memtime();               \
  }
#else
#define PSTAMP(i)
#endif

// RT = 16-row tiles per wave: 128 rows per workgroup.  (RT = 4, 256-row workgroups that leave CUs to other cells' GEMMs: a measured
// dead end, removed -- DESIGN.md 3.2.)
constexpr int RT = 2;
constexpr int PANEL_WG_ROWS = 64 * RT;             // rows held by one panel workgroup (rows 0..63 = the diagonal block)
constexpr int PANEL_OWN_ROWS = PANEL_WG_ROWS - NB;  // rows of A21 per panel workgroup
// (PSUB, the LDS row stride of the 8-column sub-panel buffers, lives in chain64.h)

// State shared by the unrolled sub-panel steps.
struct PanelCtx {
  double* sIn;    // [rows][9]  current sub-panel, as updated so far (written from the accumulators)
  double* sX;     // [rows][9]  current sub-panel, solved (MFMA operands of the trailing update)
  double* out;    // this thread's output row (global memory or the diagonal-block staging area); nullptr: none
  double* inv_diag;
  double* rinv_out;  // last workgroup: the 64 reciprocal pivots, stored behind the staged diagonal block
  int ident;      // >= 0: this thread carries identity row `ident` (last workgroup)
  int tid, wave, g, r;
  int zero_above;  // diagonal-block rows: entries right of the diagonal are zero
  int bad;
};

// One 8-column sub-panel.  acc[rt][kt]: this wave's 16 RT rows x 64 columns in MFMA C/D layout
// (lane (g, r) holds rows 16 RT w + 16 rt + g + 4 q, column 16 kt + r).
template <int P>
__device__ __forceinline__ void panel_step(d4 (&acc)[RT][4], PanelCtx& c) {
  constexpr int WROWS = 16 * RT;                 // rows per wave
  constexpr int PWG_ROWS = PANEL_WG_ROWS;
  constexpr int C0 = 8 * P;
  constexpr int KT = C0 / 16;      // tile column holding this sub-panel
  constexpr int HALF = P & 1;      // which 8 columns of that tile
  if constexpr (P == 1) { PSTAMP(10) }
  // A: accumulators -> LDS (only the lanes that hold these 8 columns)
  if ((c.r >> 3) == HALF) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) c.sIn[(WROWS * c.wave + 16 * rt + c.g + 4 * q) * PSUB + (c.r & 7)] = acc[rt][KT][q];
  }
  __syncthreads();
  if constexpr (P == 1) { PSTAMP(11) }
  // B: every thread factors the 8 x 8 diagonal sub-block (rows C0 .. C0+7 of the diagonal block)
  double l[8][8], rinv[8];
#pragma unroll
  for (int j = 0; j < 8; ++j)
#pragma unroll
    for (int k = 0; k <= j; ++k) l[j][k] = c.sIn[(C0 + j) * PSUB + k];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    double s = l[j][j];
#pragma unroll
    for (int m = 0; m < j; ++m) s = __builtin_fma(-l[j][m], l[j][m], s);
    if (!(s > 0.0)) {
      if (c.bad == 0) c.bad = C0 + j + 1;
      s = 1.0;
    }
    const double ri = rsqrt_f64(s);
    rinv[j] = ri;
    l[j][j] = s * ri;
#pragma unroll
    for (int i = j + 1; i < 8; ++i) {
      double t = l[i][j];
#pragma unroll
      for (int m = 0; m < j; ++m) t = __builtin_fma(-l[i][m], l[j][m], t);
      l[i][j] = t * ri;
    }
  }
  if (c.rinv_out && c.tid == 0) {  // reciprocal pivots for potrf_rows_kernel (split panel): exactly the values used here
#pragma unroll
    for (int j = 0; j < 8; ++j) c.rinv_out[C0 + j] = rinv[j];
  }
  if constexpr (P == 1) { PSTAMP(12) }
  if (c.tid < PWG_ROWS) {
    // own row: x = a[C0 .. C0+7] L_dd^-T
    double x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      double t = c.sIn[c.tid * PSUB + k];
#pragma unroll
      for (int m = 0; m < k; ++m) t = __builtin_fma(-x[m], l[k][m], t);
      x[k] = (C0 + k > c.zero_above) ? 0.0 : t * rinv[k];
    }
    if constexpr (P == 1) { PSTAMP(16) }
#pragma unroll
    for (int k = 0; k < 8; ++k) c.sX[c.tid * PSUB + k] = x[k];
    if constexpr (P == 1) { PSTAMP(17) }
    // solved values leave through memory directly (64 contiguous bytes per row and sub-panel): no 66-KiB output
    // image in LDS, so several panel workgroups -- of this or of other cells -- fit on one CU beside GEMM tiles
    if (c.out) {
#pragma unroll
      for (int k = 0; k < 8; k += 2) *reinterpret_cast<d2*>(c.out + C0 + k) = d2{x[k], x[k + 1]};
    }
    if (c.ident >= 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) c.inv_diag[(C0 + k) * NB + c.ident] = x[k];  // identity row i -> column i of L11^-1
    }
  }
  if constexpr (P == 1) { PSTAMP(13) }
  __syncthreads();
  if constexpr (P == 1) { PSTAMP(14) }
  // C: trailing columns [C0 + 8, 64) of this wave's rows: acc -= X_rows (32 x 8) * X_diag(16 kt .. +15, 8)^T
  if constexpr (C0 + 8 < NB) {
    constexpr int KT0 = (C0 + 8) / 16;
    double fa[RT][2], fb[4][2];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) fa[rt][ks] = -c.sX[(WROWS * c.wave + 16 * rt + c.r) * PSUB + 4 * ks + c.g];
#pragma unroll
    for (int kt = KT0; kt < 4; ++kt) {
      const int kk = kt * 16 + c.r;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) fb[kt][ks] = (kk >= C0 + 8) ? c.sX[kk * PSUB + 4 * ks + c.g] : 0.0;
    }
    // the tile column that the next sub-panel reads goes first; the rest may still be in the MFMA pipe
    // while the next sub-panel's factorisation runs on the VALU
#pragma unroll
    for (int kt = KT0; kt < 4; ++kt)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        acc[rt][kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[rt][0], fb[kt][0], acc[rt][kt], 0, 0, 0);
        acc[rt][kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[rt][1], fb[kt][1], acc[rt][kt], 0, 0, 0);
      }
  }
  // the solved values return to the accumulators of the lanes that hold these columns: the panel leaves through
  // one coalesced store pass at the end (16 lanes = one 128-byte line) instead of 16-byte stores scattered over 64
  // rows per instruction -- 4096 write requests per workgroup that the L2 had to merge.  Issued after the MFMAs so
  // that the LDS reads run under them (the MFMA on this tile column added exact zeros to the solved columns).
  if ((c.r >> 3) == HALF) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[rt][KT][q] = c.sX[(WROWS * c.wave + 16 * rt + c.g + 4 * q) * PSUB + (c.r & 7)];
  }
  if constexpr (P == 1) { PSTAMP(15) }
}

// A points at the diagonal block (c, c).  rows_below = rows under the block to solve.
// Workgroup rows 0..63 = the diagonal block (every workgroup factors it redundantly), rows 64..127 =
// this workgroup's 64 rows of A21 (or, in the last workgroup, the 64 identity rows -> L11^-1).
//
// In-place hazard: every workgroup reads the diagonal block, so none of them may overwrite it during
// this launch (a late-dispatched workgroup would read L11 instead of A11).  The last workgroup writes
// L11 to `stage_out` instead, and copies the PREVIOUS panel's staged block (`prev_stage`, prev_pw x
// prev_pw) to its place `prev_dst` in the matrix -- all readers of that block finished with the
// previous launch.  potrf_lower flushes the final block with copy_block_kernel.
__device__ __forceinline__ void flush_staged_block(const double* __restrict__ prev_stage, double* __restrict__ prev_dst, int64_t lda,
                                                   int prev_pw, int tid) {
  if (!prev_stage) return;
  const int chunks = prev_pw / 2;  // 16-byte chunks per row
  for (int e = tid; e < prev_pw * chunks; e += 256) {
    const int row = e / chunks, cc = e % chunks;
    *reinterpret_cast<d2*>(prev_dst + (int64_t)row * lda + 2 * cc) = *reinterpret_cast<const d2*>(prev_stage + row * prev_pw + 2 * cc);
  }
}

__global__ __launch_bounds__(256) void copy_block_kernel(const double* __restrict__ stage, double* __restrict__ dst, int64_t lda, int pw,
                                                         int64_t cs) {
  flush_staged_block(stage + (int64_t)blockIdx.x * cs, dst + (int64_t)blockIdx.x * cs, lda, pw, threadIdx.x);
}

// (two workgroups per CU; compiled for three it spills without gain -- DESIGN.md 3.2)
template <bool FUSE_K64>
__global__ __launch_bounds__(256, 2) void potrf_panel_kernel(double* __restrict__ A, int64_t lda, int rows_below, int nchunks,
                                                          double* __restrict__ inv_diag, int* __restrict__ info, int col0,
                                                          double* __restrict__ stage_out, const double* __restrict__ prev_stage,
                                                          double* __restrict__ prev_dst, int prev_pw, int64_t cs, int info_stride,
                                                          double* __restrict__ yv, int y_left) {
  constexpr int PWG_ROWS = PANEL_WG_ROWS;
  constexpr int PANEL_ROWS = PANEL_OWN_ROWS;
  constexpr int WROWS = 16 * RT;
#ifndef GPRX_PANEL_NO_SETPRIO
  // the panel is the dependent chain: its waves outrank the bulk update's waves they share SIMDs with (instruction issue is
  // arbitrated by priority, then age -- MI355X_MICROARCH.md, two waves per SIMD).  Measured: N = 16384 29.79 -> 29.46 ms,
  // N = 8192 6.46 -> 6.30 ms, N = 4096 2.17 -> 2.15 ms (tools/setprio_probe.sh): small, consistent, free.
  __builtin_amdgcn_s_setprio(3);
#endif
  {
    // batched: blockIdx.y = cell; every per-cell pointer lives in one cell block, `cs` doubles apart
    const int64_t off = (int64_t)blockIdx.y * cs;
    A += off;
    inv_diag += off;
    stage_out += off;
    if (prev_stage) prev_stage += off;
    if (prev_dst) prev_dst += off;
    info += (int64_t)blockIdx.y * info_stride;
  }
  __shared__ __attribute__((aligned(16))) double sIn[PWG_ROWS * PSUB];
  __shared__ __attribute__((aligned(16))) double sX[PWG_ROWS * PSUB];
  PanelCtx c;
  c.sIn = sIn;
  c.sX = sX;
  c.inv_diag = inv_diag;
  c.tid = threadIdx.x;
  const int lane = c.tid & 63;
  c.wave = c.tid >> 6;
  c.g = lane >> 4;
  c.r = lane & 15;
  c.zero_above = c.tid < NB ? c.tid : (1 << 30);
  c.bad = 0;
  const bool last = (int)blockIdx.x == nchunks;
  c.rinv_out = last ? stage_out + NB * NB : nullptr;
  if (last) flush_staged_block(prev_stage, prev_dst, lda, prev_pw, c.tid);
  // where this thread's solved row goes (thread t < PWG_ROWS owns workgroup row t)
  c.out = nullptr;
  c.ident = -1;
  if (c.tid < NB) {
    if (last) c.out = stage_out + c.tid * NB;  // the factored diagonal block is staged (in-place hazard, see above)
  } else if (c.tid < PWG_ROWS) {
    if (last && c.tid < 2 * NB) c.ident = c.tid - NB;  // (rows of A21 leave through the final store pass)
  }
  PSTAMP(0)
  PACC_DECL
  PACC(0)

  // ---- load straight into the accumulator layout: 16 RT loads per lane, all in flight ----
  // Every load is unconditional (rows outside the matrix read row 0 of the diagonal block instead) and the
  // triangle / padding / identity masks are applied afterwards with selects: with the conditions around the
  // loads the compiler emitted a branch and a full wait per load, i.e. 32 serialised memory round trips.
  d4 acc[RT][4];
  {
    const double* rowp[RT][4];
    bool valid[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int wrow = WROWS * c.wave + 16 * rt + c.g + 4 * q;  // workgroup row
        const int idx = (int)blockIdx.x * PANEL_ROWS + (wrow - NB);
        const bool diag = wrow < NB;
        const bool ok = diag || (!last && idx < rows_below);
        const int64_t mrow = diag ? wrow : (ok ? NB + idx : 0);
        rowp[rt][q] = A + mrow * lda + c.r;
        valid[rt][q] = ok;
      }
    d4 upd[FUSE_K64 ? RT : 1][4];
    if constexpr (FUSE_K64) {
      // The K = 64 update that the schedule would launch between the previous panel and this one (these 64 columns, every
      // row from the diagonal block down, by the 64 columns left of them), applied here to the rows this workgroup holds: one
      // dependent launch less per odd panel (~9 us of a lone matrix's chain).  Operation for operation what gemm_f64 does
      // (accumulators from zero, stages of 16 along k, instruction j of a stage takes k = k0 + 4 g + j; C + (-1) * sum with one
      // rounding), so the factor is the same bit for bit as with the separate launch.  factor_range fuses every pair of panels,
      // for a lone matrix and for batched cells alike: only a 64-column outer block still makes that launch.
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) upd[rt][kt] = d4{0.0, 0.0, 0.0, 0.0};
      const double* arow[RT];
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const int wrow = WROWS * c.wave + 16 * rt + c.r;  // A operand: lane (g, r) supplies row r of the tile, k = 4 g + j
        const int idx = (int)blockIdx.x * PANEL_ROWS + (wrow - NB);
        const bool diag = wrow < NB;
        const bool ok = diag || (!last && idx < rows_below);
        arow[rt] = A + (diag ? wrow : (ok ? NB + idx : 0)) * lda - NB + 4 * c.g;
      }
      const double* brow = A + (int64_t)c.r * lda - NB + 4 * c.g;  // B operand: rows of the diagonal block (row 16 kt + r)
#pragma unroll
      for (int k0 = 0; k0 < NB; k0 += 16) {
        double fa[RT][4], fb[4][4];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          const d2 lo = *reinterpret_cast<const d2*>(arow[rt] + k0), hi = *reinterpret_cast<const d2*>(arow[rt] + k0 + 2);
          fa[rt][0] = lo.x; fa[rt][1] = lo.y; fa[rt][2] = hi.x; fa[rt][3] = hi.y;
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          const double* bp = brow + (int64_t)(16 * kt) * lda + k0;
          const d2 lo = *reinterpret_cast<const d2*>(bp), hi = *reinterpret_cast<const d2*>(bp + 2);
          fb[kt][0] = lo.x; fb[kt][1] = lo.y; fb[kt][2] = hi.x; fb[kt][3] = hi.y;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) upd[rt][kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[rt][j], fb[kt][j], upd[rt][kt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) acc[rt][kt][q] = rowp[rt][q][kt * 16];
    if constexpr (FUSE_K64) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const double v = -1.0 * upd[rt][kt][q];
            acc[rt][kt][q] = __builtin_fma(1.0, acc[rt][kt][q], v);
          }
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int wrow = WROWS * c.wave + 16 * rt + c.g + 4 * q;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          const int col = kt * 16 + c.r;
          double v = valid[rt][q] ? acc[rt][kt][q] : 0.0;
          if (wrow < NB) {
            v = (col > wrow) ? 0.0 : v;
          } else if (last) {
            v = (col == wrow - NB) ? 1.0 : 0.0;
          }
          acc[rt][kt][q] = v;
        }
      }
  }
  PSTAMP(1)
  PACC(1)

  panel_step<0>(acc, c);
  PSTAMP(2)
  PACC(2)
  panel_step<1>(acc, c);
  panel_step<2>(acc, c);
  panel_step<3>(acc, c);
  PSTAMP(3)
  PACC(3)
  panel_step<4>(acc, c);
  panel_step<5>(acc, c);
  panel_step<6>(acc, c);
  panel_step<7>(acc, c);
  PSTAMP(4)
  PACC(4)
  if (!last) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int wrow = WROWS * c.wave + 16 * rt + c.g + 4 * q;
        const int idx = (int)blockIdx.x * PANEL_ROWS + (wrow - NB);
        if (wrow >= NB && idx < rows_below) {
          double* dst = A + (int64_t)(NB + idx) * lda + c.r;
#pragma unroll
          for (int kt = 0; kt < 4; ++kt) dst[kt * 16] = acc[rt][kt][q];
        }
      }
  }
  if (last && c.tid == 0 && c.bad != 0) atomicCAS(info, 0, col0 + c.bad);
  if (yv != nullptr && last) {
    // Right-hand side as a vector (potrf_rows_kernel<..., YVEC>): beta_j = L11^-1 y_j by the diagonal workgroup itself, from the inverse
    // its identity rows have just stored (every wave's stores acknowledged, then the barrier; nobody read those lines before).  Row a of
    // the inverse times y_j: four partial sums of 16 terms, added in a fixed order.
    yv += (int64_t)blockIdx.y * cs;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    double* sv = sIn;         // (the sub-panel buffers are free now)
    double* sred = sIn + NB;
    static_assert(PWG_ROWS * PSUB >= NB + 256, "the sub-panel buffer holds y_j and the partial sums");
    const int a = c.tid & 63, qq = c.tid >> 6;
    if (FUSE_K64 && y_left) {
      // Right panel of a rows pair (potrf_rows_pair_kernel): its 64 rows B = L(c .. c + 63, c - 64 .. c - 1) were solved by the chunk
      // workgroup of the left panel's diagonal launch, which carries no y, so y_j -= B beta_{j-1} happens here, before beta_j is formed.
      // Row a of B times beta_{j-1}: four partial sums of 16 terms (k ascending), added in order of k, then taken off y_j[a].
      const double* brow = A + (int64_t)a * lda - NB + 16 * qq;
      const double* bl = yv - NB + 16 * qq;
      double sum = 0.0;
#pragma unroll
      for (int i = 0; i < 16; ++i) sum = __builtin_fma(brow[i], bl[i], sum);
      sred[c.tid] = sum;
      __syncthreads();
      if (c.tid < NB) sv[c.tid] = yv[c.tid] - (((sred[c.tid] + sred[64 + c.tid]) + sred[128 + c.tid]) + sred[192 + c.tid]);
    } else {
      if (c.tid < NB) sv[c.tid] = yv[c.tid];
    }
    __syncthreads();
    const double* row = inv_diag + a * NB + 16 * qq;
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) sum = __builtin_fma(row[i], sv[16 * qq + i], sum);
    sred[c.tid] = sum;
    __syncthreads();
    if (c.tid < NB) yv[c.tid] = ((sred[c.tid] + sred[64 + c.tid]) + sred[128 + c.tid]) + sred[192 + c.tid];
  }
  PSTAMP(5)
  PACC(5)
}

// ---- split panel (many cells per launch): rows only ---------------------------------------------------
// potrf_panel_kernel launched with ONE workgroup per cell factors the diagonal block (staged L11, L11^-1 and the
// 64 reciprocal pivots); this kernel then solves the rows below it, 128 rows per workgroup and no redundant
// factorisation.  The arithmetic per row -- substitution order, the MFMA updates of the columns right of each
// 8-column sub-panel and their order -- is that of potrf_panel_kernel with the operands it would have recomputed,
// so the results are bit-identical; the registers that held the 8 x 8 factor are free and a launch has half as
// many workgroups.
// L11 is not copied to LDS: the 8 x 8 diagonal sub-block and the pivots come through scalar loads from the staged block
// (uniform addresses: s_load into SGPRs that v_fma_f64 takes directly), the MFMA operands straight from it (L1 / L2 resident):
// 18 KB of LDS and 116 VGPRs, four workgroups per CU instead of three.  The kernel is bound by its own dependent chain (8 sub-panels
// x (LDS round trip, 44-FMA substitution, MFMA update)), not by bandwidth (3.3 TB/s) -- rows in flight per CU are what counts:
// -0.5 ms per 128-cell step at N = 4096.  Measured without effect: 256-row workgroups, scalar loads alone.
// A wave substitutes its OWN 32 rows (lanes < 32), so nothing crosses waves and the two barriers of a sub-panel are
// wave-scope fences: the four waves of a workgroup drift apart and overlap their phases (another -0.3 ms).  (Removed, DESIGN.md 3.3
// and 7c.1: the form with an L11 image in LDS, 44 broadcast reads per row and sub-panel and workgroup barriers -- 81 against 68 us
// per launch -- and the rows by one MFMA tile product against L11^-1 -- 206 against 207 us batched, 2.70 against 2.15 ms lone.)
constexpr int ROWS_WG = 64 * RT;
__device__ __forceinline__ void wave_sync_lds() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <int P>
__device__ __forceinline__ void rows_step(d4 (&acc)[RT][4], double* __restrict__ sIn, double* __restrict__ sX, int tid, int wave, int g, int r,
                                          const double* __restrict__ gstage) {
  constexpr int C0 = 8 * P;
  constexpr int KT = C0 / 16;
  constexpr int HALF = P & 1;
  constexpr int WROWS = 16 * RT;
  if ((r >> 3) == HALF) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) sIn[(WROWS * wave + 16 * rt + g + 4 * q) * PSUB + (r & 7)] = acc[rt][KT][q];
  }
  wave_sync_lds();
  const int srow = WROWS * wave + (tid & 63);
  if ((tid & 63) < WROWS) {
    double x[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      double t = sIn[srow * PSUB + k];
#pragma unroll
      for (int m = 0; m < k; ++m) t = __builtin_fma(-x[m], gstage[(C0 + k) * NB + C0 + m], t);
      x[k] = t * gstage[NB * NB + C0 + k];
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) sX[srow * PSUB + k] = x[k];
  }
  wave_sync_lds();
  if constexpr (C0 + 8 < NB) {
    constexpr int KT0 = (C0 + 8) / 16;
    double fa[RT][2], fb[4][2];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) fa[rt][ks] = -sX[(WROWS * wave + 16 * rt + r) * PSUB + 4 * ks + g];
#pragma unroll
    for (int kt = KT0; kt < 4; ++kt) {
      const int kk = kt * 16 + r;
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) fb[kt][ks] = (kk >= C0 + 8) ? gstage[kk * NB + C0 + 4 * ks + g] : 0.0;
    }
#pragma unroll
    for (int kt = KT0; kt < 4; ++kt)
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        acc[rt][kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[rt][0], fb[kt][0], acc[rt][kt], 0, 0, 0);
        acc[rt][kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[rt][1], fb[kt][1], acc[rt][kt], 0, 0, 0);
      }
  }
  if ((r >> 3) == HALF) {  // solved values back into the accumulators (see potrf_panel_kernel): one coalesced store pass at the end
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) acc[rt][KT][q] = sX[(WROWS * wave + 16 * rt + g + 4 * q) * PSUB + (r & 7)];
  }
}

// A21: first row below the diagonal block (rows_below rows, lda); stage: this panel's staged L11 (64 x 64) followed by
// the 64 reciprocal pivots.  grid = (ceil(rows_below / ROWS_WG), cells).
// FUSE_K64: as in potrf_panel_kernel -- the K = 64 update of these 64 columns by the 64 columns left of them (which the schedule
// would launch between the previous panel and this one) is applied to this workgroup's rows on their way in: with many cells per
// launch that update is HBM-bound (16 bytes of C traffic per 128 flops), and this kernel reads and writes the very same columns
// anyway.  Operation for operation the general NT kernel's arithmetic (accumulators from zero, stages of 16 along k, instruction j
// takes k = k0 + 4 g + j, C + (-1) * sum with one rounding): bit-identical to the separate launch.
// YVEC (round 4): the right-hand side of the cell travels as a VECTOR instead of a 64-row tile below the matrix (one useful row of 64:
// T^2 / 2 tile products of a factorisation with T block columns, 4.5 % of the flops at N = 4096).  yv points at this panel's 64 entries
// of it -- beta_j = L11^-1 y_j, written by the diagonal workgroup at its end (a launch of its own for it: same sums, removed) -- followed by the
// entries of the rows below, which this kernel updates: y_i -= sum_c L(i, c) beta_j[c], the 64 products of a row summed over the tile
// columns in a lane (k t ascending) and then over the 16 lanes that hold the row (xor 1, 2, 4, 8): a fixed order.
//
// rows_pass is the body: one workgroup's 128 rows (from row0 of A21 on) against one panel.  Of the cell's right-hand side yv + ycell, the
// panel's beta_j starts at entry ybeta and the entries that belong to A21's rows at entry yrows.  potrf_rows_pair_kernel runs it twice on
// the same rows, for the two panels of a pair:
//   X_L2   the A operand of the K = 64 update (the left panel's solved rows) was stored by THIS wave a moment ago: 16-byte sc1 loads, served
//          by the XCD's L2 past the CU's L1 (which may still hold the lines as they were before the solve);
//   NT_IN  the rows' own columns are read once and NT_OUT their solved values are not read again in this launch: non-temporal accesses
//          (measured: 348 -> 338 us per pair launch at 256 cells of N = 4096; the bytes fetched stay what they were);
//   Y_OUT  the updated entries of y are not stored but kept for the second pass, in the padding word of the rows' sub-panel lines in LDS
//          (column 8 of PSUB = 9, which no sub-panel step touches; a wave's own rows, so wave-scope fences do); Y_IN takes them from there.
__device__ __forceinline__ d2 ld2_l2(__amdgpu_buffer_rsrc_t rs, unsigned voff, unsigned soff) {
  typedef unsigned int u4v __attribute__((ext_vector_type(4)));
  const u4v v = __builtin_amdgcn_raw_buffer_load_b128(rs, voff, soff, 16);  // aux 16 = sc1
  d2 out;
  __builtin_memcpy(&out, &v, 16);
  return out;
}
// v of lane (own index ^ M), M < 32: the exchange pattern is an immediate (ds_swizzle, bit mode), so no lane-address register lives
// through the kernel as with __shfl_xor
template <int M>
__device__ __forceinline__ double lane_xor(double v) {
  int w[2];
  __builtin_memcpy(w, &v, 8);
  w[0] = __builtin_amdgcn_ds_swizzle(w[0], (M << 10) | 0x1f);
  w[1] = __builtin_amdgcn_ds_swizzle(w[1], (M << 10) | 0x1f);
  __builtin_memcpy(&v, w, 8);
  return v;
}
template <bool FUSE_K64, bool YVEC, bool X_L2, bool Y_IN, bool Y_OUT, bool NT_IN = false, bool NT_OUT = false>
__device__ __forceinline__ void rows_pass(double* __restrict__ A21, int64_t lda, int rows_below, int row0, const double* __restrict__ stage,
                                          double* __restrict__ yv, int64_t ycell, int ybeta, int yrows, double* __restrict__ sIn,
                                          double* __restrict__ sX) {
  constexpr int WROWS = 16 * RT;
  // (the wave index as a scalar, the lane index from the execution mask: every wave-dependent address term lives in SGPRs)
  const int lane = __lane_id(), wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), tid = 64 * wave + lane, g = lane >> 4, r = lane & 15;
  // own rows -> accumulator layout, every load unconditional (rows past the end re-read the workgroup's first row and are masked)
  d4 acc[RT][4];
  {
    // (a row's address = the workgroup's first row, which exists -- a scalar -- plus a 32-bit byte offset: one register per row, not two)
    const char* wg0 = reinterpret_cast<const char*>(A21 + (int64_t)row0 * lda);
    unsigned rowp[RT][4];
    bool valid[RT][4];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int lrow = WROWS * wave + 16 * rt + g + 4 * q;
        valid[rt][q] = row0 + lrow < rows_below;
        rowp[rt][q] = ((unsigned)(valid[rt][q] ? lrow : 0) * (unsigned)lda + r) * 8u;
      }
    d4 upd[FUSE_K64 ? RT : 1][4];
    if constexpr (FUSE_K64) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) upd[rt][kt] = d4{0.0, 0.0, 0.0, 0.0};
      const double* arow[RT];
      // (X_L2: descriptor at the workgroup's first row, which exists; per-lane byte offsets within its 128 rows.  Rows past the end read
      // that first row and are masked below, as the plain form reads row 0.)
      [[maybe_unused]] __amdgpu_buffer_rsrc_t xrs;
      [[maybe_unused]] unsigned xoff[RT];
      if constexpr (X_L2) xrs = __builtin_amdgcn_make_buffer_rsrc(A21 + (int64_t)row0 * lda - NB, 0, 0xffffffff, 0x00020000);
#pragma unroll
      for (int rt = 0; rt < RT; ++rt) {
        const int idx = row0 + WROWS * wave + 16 * rt + r;  // A operand: lane (g, r) supplies row r of the tile, k = 4 g + j
        arow[rt] = A21 + (int64_t)(idx < rows_below ? idx : 0) * lda - NB + 4 * g;
        if constexpr (X_L2) xoff[rt] = ((unsigned)(idx < rows_below ? idx - row0 : 0) * (unsigned)lda + 4u * g) * 8u;
      }
      const double* brow = A21 - (int64_t)NB * lda + (int64_t)r * lda - NB + 4 * g;  // B operand: the diagonal block's rows, previous 64 columns
#pragma unroll
      for (int k0 = 0; k0 < NB; k0 += 16) {
        double fa[RT][4], fb[4][4];
#pragma unroll
        for (int rt = 0; rt < RT; ++rt) {
          d2 lo, hi;
          if constexpr (X_L2) {
            lo = ld2_l2(xrs, xoff[rt], 8u * k0);
            hi = ld2_l2(xrs, xoff[rt], 8u * k0 + 16u);
          } else {
            lo = *reinterpret_cast<const d2*>(arow[rt] + k0);
            hi = *reinterpret_cast<const d2*>(arow[rt] + k0 + 2);
          }
          fa[rt][0] = lo.x; fa[rt][1] = lo.y; fa[rt][2] = hi.x; fa[rt][3] = hi.y;
        }
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          const double* bp = brow + (int64_t)(16 * kt) * lda + k0;
          const d2 lo = *reinterpret_cast<const d2*>(bp), hi = *reinterpret_cast<const d2*>(bp + 2);
          fb[kt][0] = lo.x; fb[kt][1] = lo.y; fb[kt][2] = hi.x; fb[kt][3] = hi.y;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int kt = 0; kt < 4; ++kt) upd[rt][kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[rt][j], fb[kt][j], upd[rt][kt], 0, 0, 0);
      }
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          const double* src = reinterpret_cast<const double*>(wg0 + rowp[rt][q] + kt * 128);
          acc[rt][kt][q] = NT_IN ? __builtin_nontemporal_load(src) : *src;
        }
    if constexpr (FUSE_K64) {
#pragma unroll
      for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const double v = -1.0 * upd[rt][kt][q];
            acc[rt][kt][q] = __builtin_fma(1.0, acc[rt][kt][q], v);
          }
    }
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) acc[rt][kt][q] = valid[rt][q] ? acc[rt][kt][q] : 0.0;
  }
  rows_step<0>(acc, sIn, sX, tid, wave, g, r, stage);
  rows_step<1>(acc, sIn, sX, tid, wave, g, r, stage);
  rows_step<2>(acc, sIn, sX, tid, wave, g, r, stage);
  rows_step<3>(acc, sIn, sX, tid, wave, g, r, stage);
  rows_step<4>(acc, sIn, sX, tid, wave, g, r, stage);
  rows_step<5>(acc, sIn, sX, tid, wave, g, r, stage);
  // (YVEC: beta_j and this lane group's entries of y are requested before the last two sub-panel steps -- their latency hides behind
  // those -- and only stored at the end; not earlier, the registers are needed)
  double ybj[YVEC ? 4 : 1], yold[YVEC ? RT : 1][4];
  [[maybe_unused]] int yrow0 = row0;
  if constexpr (YVEC) {
    yv += ycell;
    asm volatile("" : "+s"(yrow0));  // (the addresses of the y entries are formed here, not at the top beside the rows' own)
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) ybj[kt] = yv[ybeta + 16 * kt + r];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int idx = yrow0 + WROWS * wave + 16 * rt + g + 4 * q;
        yold[rt][q] = Y_IN ? sIn[(WROWS * wave + 16 * rt + g + 4 * q) * PSUB + 8] : yv[yrows + (idx < rows_below ? idx : 0)];
      }
  }
  rows_step<6>(acc, sIn, sX, tid, wave, g, r, stage);
  rows_step<7>(acc, sIn, sX, tid, wave, g, r, stage);
#pragma unroll
  for (int rt = 0; rt < RT; ++rt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int idx = row0 + WROWS * wave + 16 * rt + g + 4 * q;
      if (idx < rows_below) {
        double* dst = A21 + (int64_t)idx * lda + r;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
          if constexpr (NT_OUT) __builtin_nontemporal_store(acc[rt][kt][q], dst + kt * 16);
          else dst[kt * 16] = acc[rt][kt][q];
        }
      }
    }
  if constexpr (YVEC) {
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        double sum = acc[rt][0][q] * ybj[0];
#pragma unroll
        for (int kt = 1; kt < 4; ++kt) sum = __builtin_fma(acc[rt][kt][q], ybj[kt], sum);
        sum += lane_xor<1>(sum);
        sum += lane_xor<2>(sum);
        sum += lane_xor<4>(sum);
        sum += lane_xor<8>(sum);
        const int idx = yrow0 + WROWS * wave + 16 * rt + g + 4 * q;
        if constexpr (Y_OUT) {
          if (r == 0) sIn[(WROWS * wave + 16 * rt + g + 4 * q) * PSUB + 8] = yold[rt][q] - sum;
        } else {
          if (r == 0 && idx < rows_below) yv[yrows + idx] = yold[rt][q] - sum;
        }
      }
  }
}

// (four workgroups per CU; three with the accumulators of the K = 64 update: 168 registers)
template <bool FUSE_K64, bool YVEC>
__global__ __launch_bounds__(256, FUSE_K64 ? 3 : 4) void potrf_rows_kernel(double* __restrict__ A21, int64_t lda, int rows_below,
                                                                           const double* __restrict__ stage, int64_t cs, double* __restrict__ yv) {
  __shared__ __attribute__((aligned(16))) double sIn[ROWS_WG * PSUB];
  __shared__ __attribute__((aligned(16))) double sX[ROWS_WG * PSUB];
  const int64_t off = (int64_t)blockIdx.y * cs;
  rows_pass<FUSE_K64, YVEC, false, false, false>(A21 + off, lda, rows_below, blockIdx.x * ROWS_WG, stage + off, yv, off, 0, NB, sIn, sX);
}

// The rows below a PAIR of panels (columns c .. c + 63 and c + 64 .. c + 127) in one launch: what potrf_rows_kernel<false> at c and
// potrf_rows_kernel<true> at c + 64 do, back to back on the same 128 rows, every operation in the same order -- the same bits.  The fused
// kernel's A operand is the left panel's solved rows X, which the same rows' workgroup stored one launch earlier; with 256 cells x ~2000
// rows x 512 B gone past in between it came from HBM.  Here the wave reads it back right after storing it: plain stores leave the lines in
// this XCD's L2, every wave waits for its own stores (a wave's A operand is its own 32 rows: nothing crosses waves, no workgroup barrier),
// and the loads are sc1, past the L1.  X is NOT kept in registers or LDS: its accumulators are dead once stored, so the register peak is the
// fused rows kernel's and three workgroups fit a CU.
// A21: row c + 128, column c (rows_below rows); stage, stage2: the two panels' staged blocks; yv: the right-hand side from entry c on
// (beta_c, beta_{c+64}, then the rows' entries, which stay in registers between the two updates).  grid = (ceil(rows_below / ROWS_WG), cells).
template <bool YVEC>
__global__ __launch_bounds__(256, 3) void potrf_rows_pair_kernel(double* __restrict__ A21, int64_t lda, int rows_below,
                                                                 const double* __restrict__ stage, const double* __restrict__ stage2, int64_t cs,
                                                                 double* __restrict__ yv) {
  __shared__ __attribute__((aligned(16))) double sIn[ROWS_WG * PSUB];
  __shared__ __attribute__((aligned(16))) double sX[ROWS_WG * PSUB];
  const int64_t off = (int64_t)blockIdx.y * cs;
  const int row0 = blockIdx.x * ROWS_WG;
  rows_pass<false, YVEC, false, false, true, true, false>(A21 + off, lda, rows_below, row0, stage + off, yv, off, 0, 2 * NB, sIn, sX);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's stores of X have reached the L2
  wave_sync_lds();                                   // (and its entries of y the padding words)
  // (the second pass forms its addresses anew: shared with the first pass's they would stay live through it, which spills)
  int row0b = row0;
  asm volatile("" : "+s"(row0b));
  rows_pass<true, YVEC, true, true, false, true, true>(A21 + off + NB, lda, rows_below, row0b, stage2 + off, yv, off, NB, 2 * NB, sIn, sX);
}

// staging area: STAGE_LD doubles per matrix column; the panel at column c stages its diagonal block (64 x 64, row-major) at
// c * STAGE_LD and its 64 reciprocal pivots right behind it.  (129: the stride that also held the 128 x 128 block of the retired
// 128-column panel; kept so that no workspace layout moves.)
constexpr int STAGE_LD = 129;

// Optional per-launch timing of the two kernels of the factorisation (HIP events on the launch stream).
struct PotrfProfile {
  std::vector<hipEvent_t> pool;
  size_t used = 0;
  std::vector<std::pair<size_t, double>> gemm_marks;   // launches of the main GEMM kernel (bulk HEAD / TAIL updates and in-block updates with K > 128):
                                                       // (index of start event, algorithmic flops)
  std::vector<std::pair<size_t, double>> strip_marks;  // short-K in-block updates (K <= 128: the 64 x 64 GEMM with C prefetch)
  std::vector<size_t> panel_marks;
  hipEvent_t next() {
    if (used == pool.size()) {
      hipEvent_t e;
      hipEventCreate(&e);
      pool.push_back(e);
    }
    return pool[used++];
  }
  void reset() {
    used = 0;
    gemm_marks.clear();
    strip_marks.clear();
    panel_marks.clear();
  }
  ~PotrfProfile() {
    for (auto e : pool) hipEventDestroy(e);
  }
};

// run-time tuning knobs (gprx_set_tuning): 0 = default heuristics
struct PotrfTuning {
  int outer_block = 0;   // multiple of 128
  int update_tile = 0;   // tile of the TAIL GEMM: 64 or 128
  int no_lookahead = 0;  // 1: everything on the main stream (debugging)
  int split_panel = 0;   // 1: always the split panel (diagonal workgroup + rows kernel), -1: never, 0: from 24 cells per launch on
  int poison_workspace = 0;  // testing: the gradient's L^-1 workspace starts as NaN patterns (nothing may depend on its old contents)
  int cell_kernel = 0;   // batched cells: 1 = always one workgroup per cell (potrf_cell.h), -1 never, 0 = for np <= 1024 and >= 256 cells
  int rhs_vector = 0;    // batched cells, split panel: -1 = the right-hand side always rides as a 64-row tile; 0 / 1 = as a vector where the schedule knows it
  int dag = 0;           // lone matrices: 1 = the tile-DAG factorisation (potrf_dag.h); 0 / -1 = the launch-per-panel schedule (default)
  int rows_pair = 1;     // batched cells, split panel: 1 = one rows launch per pair of panels (potrf_rows_pair_kernel, default); 0 = one per panel (A/B runs, tests)
};
inline PotrfTuning& potrf_tuning() {
  static PotrfTuning t = [] {
    PotrfTuning v;
    if (const char* e = getenv("GPRX_OUTER_BLOCK")) v.outer_block = atoi(e);  // experiments without recompiling callers
    if (const char* e = getenv("GPRX_UPDATE_TILE")) v.update_tile = atoi(e);
    if (const char* e = getenv("GPRX_SPLIT_PANEL")) v.split_panel = atoi(e);
    if (const char* e = getenv("GPRX_DAG")) v.dag = atoi(e);
    if (const char* e = getenv("GPRX_RHS_VECTOR")) v.rhs_vector = atoi(e);
    if (const char* e = getenv("GPRX_CELL_KERNEL")) v.cell_kernel = atoi(e);
    if (const char* e = getenv("GPRX_ROWS_PAIR")) v.rows_pair = atoi(e) != 0;
    return v;
  }();
  return t;
}

// Stream and events of the look-ahead schedule (owned by the caller, reused across factorisations).
struct PotrfStreams {
  hipStream_t aux = nullptr;
  hipEvent_t block_done = nullptr, tail_done = nullptr;
  hipError_t init() {
    hipError_t e = hipStreamCreateWithFlags(&aux, hipStreamNonBlocking);  // normal priority (see gprx_create)
    if (e != hipSuccess) return e;
    if ((e = hipEventCreateWithFlags(&block_done, hipEventDisableTiming)) != hipSuccess) return e;
    return hipEventCreateWithFlags(&tail_done, hipEventDisableTiming);
  }
  void destroy() {
    if (aux) hipStreamDestroy(aux);
    if (block_done) hipEventDestroy(block_done);
    if (tail_done) hipEventDestroy(tail_done);
    aux = nullptr;
    block_done = tail_done = nullptr;
  }
};

// Split panel (the diagonal workgroup, then a rows-only kernel) or fused panel?  The split pays one more dependent launch per panel and
// wins once a fused launch would fill the chip with redundant factorisations (measured at N = 4096: -2 % at 16 cells per launch, +5 % at
// 32); bit-identical either way.  "split_panel": 1 = always, -1 = never, 0 = from 24 cells per launch on.
inline bool potrf_split_panel(const PotrfTuning& tune, int batch) { return tune.split_panel ? tune.split_panel > 0 : batch >= 24; }

// Can potrf_lower carry ONE right-hand side as a vector (yvec; then extra = 0) under this tuning and batch size?  Only the split panel of
// batched cells knows the form (the diagonal workgroup + potrf_rows_kernel<..., YVEC>); a lone or small-batch factorisation (fused panel)
// keeps the 64-row tile, whose arithmetic is the one single calls are bit-identical in.
// "rhs_vector": 1 / 0 = where possible (default), -1 = never.
inline bool potrf_rhs_vector_ok(const PotrfTuning& tune, int batch) { return tune.rhs_vector >= 0 && batch > 1 && potrf_split_panel(tune, batch); }

// Factor the (np x np) matrix in place; `extra` rows below it are carried as right-hand sides.
// inv_diag: np/64 blocks of 64 x 64.  info (device int) must be zeroed by the caller.
//
// Two-level right-looking schedule with look-ahead.  Panels are 64 columns wide (one launch factors the diagonal block and
// solves all rows below it; a 128-column kernel was measured slower -- 203 us per 128 columns against 173 us, its MFMA updates
// serialise behind the scalar factor chain -- and removed).
// Outer blocks are `ob` columns (1024 up to n = 4096, else 512, measured): the bulk trailing updates
// run with K = ob, i.e. n / ob passes over the trailing matrix instead of n / 64; inside a block the panels are combined
// recursively (see factor_range).  For each outer block J = columns [C, C + w):
//   main stream: its panels and in-block updates;
//                then HEAD(J): the update of the NEXT block's columns by block J (K = w);
//   aux stream : TAIL(J): the update of every column right of the next block (K = w, the bulk of the
//                flops), overlapping the next block's panel chain on the main stream.
// Order: TAIL(J) waits for HEAD(J) to be enqueued behind block J (event) and follows TAIL(J-1)
// (stream order); HEAD(J) waits for TAIL(J-1), the last writer of the next block's columns.
// (Tried and removed, DESIGN.md 7b.6: splitting the K >= 256 updates by columns over a third stream so that the chain carries only
// the 64 columns the next panel needs -- N = 4096 2.17 -> 2.66 ms, it loses at every size.)
// diag_stage: scratch of np * STAGE_LD doubles (staged diagonal blocks and reciprocal pivots, see potrf_panel_kernel)
// col_base: added to the failing-pivot index reported through `info` (the matrix is a diagonal block of a larger one).
// batch > 1: `batch` matrices at A + c * cs (inv_diag and diag_stage likewise: all live in cell blocks `cs` doubles apart),
// info words info_stride ints apart; every launch carries the cell index in blockIdx.y.
// yvec (see potrf_rhs_vector_ok, which the caller asks first): the one right-hand side as a vector of np entries per cell; it is an
// error where the schedule is the fused panel, which has no such form.
inline hipError_t potrf_lower(hipStream_t st, double* A, int64_t lda, int np, int extra, double* inv_diag, int* info,
                              double* diag_stage, PotrfProfile* prof = nullptr, PotrfStreams* ps = nullptr, int batch = 1, int64_t cs = 0,
                              int info_stride = 0, const PotrfTuning* tune_in = nullptr, int col_base = 0, double* yvec = nullptr) {
  const double* prev_stage = nullptr;
  double* prev_dst = nullptr;
  auto mark_gemm = [&](hipStream_t s, int ncols_lower, int rows_rect, int ncols, int k, bool strip = false) {
    if (!prof) return;
    // algorithmic flops: 2 K per updated element (lower triangle incl. diagonal of the square part + rectangle)
    const double elems = 0.5 * (double)ncols_lower * (ncols_lower + 1) + (double)rows_rect * ncols;
    (strip ? prof->strip_marks : prof->gemm_marks).push_back({prof->used, 2.0 * k * elems * batch});
    hipEventRecord(prof->next(), s);
  };
  auto mark_end = [&](hipStream_t s) {
    if (prof) hipEventRecord(prof->next(), s);
  };
  const int total_rows = np + extra;
  const PotrfTuning& tune = tune_in ? *tune_in : potrf_tuning();  // a handle's own knobs, or the process defaults
  if (tune.no_lookahead) ps = nullptr;
  const int ob = tune.outer_block ? tune.outer_block : (np > 4096 ? 512 : 1024);  // measured: N=2048/4096 -> 1024, N=8192/16384 -> 512
  // bulk-update tile: batched cells fill the chip with 64 x 64 tiles already (4 workgroups per CU hide the C
  // read-modify-write; measured 1529 vs 1513 fits/s at 16 cells of N = 4096); a single matrix lets launch_gemm choose
  // (a single matrix too since the 64 x 64 kernel takes its operands by LDS-DMA: N = 16384 30.7 ms against 32.4 ms with the
  // 128 x 128 tile, whose ragged row counts keep it on the register-staged kernel)
  const int bulk_tile = tune.update_tile ? tune.update_tile : 64;
  bool tail_pending = false;
  hipError_t err = hipSuccess;
  const bool split_panel = potrf_split_panel(tune, batch);
  if (yvec && !split_panel) return hipErrorInvalidValue;  // only the split panel carries the right-hand side as a vector
  const bool rows_pair = split_panel && batch > 1 && tune.rows_pair != 0;
  // one panel: factor the diagonal block at column c and solve every row below it.  fuse: the K = 64 update of these 64 columns by the
  // 64 columns left of them happens inside the panel kernel (one dependent launch less; same arithmetic as the general NT kernel)
  // pair (rows_pair): 1 = the left panel of a pair, 2 = its right panel.  The left panel's launch solves only the 64 rows B that the right
  // diagonal block needs (one chunk workgroup in its fused-panel role beside the diagonal workgroup -- the launch is chip-idle anyway; the
  // role repeats the rows kernel's substitution operand for operand, so B has the same bits); the right panel's diagonal launch is today's
  // (with the right-hand side as a vector it first takes B beta_c off its 64 entries of y, which the chunk role does not carry), and ONE
  // rows launch then solves the rows from c + 128 down for both panels (potrf_rows_pair_kernel).
  auto panel = [&](int c, bool fuse = false, int pair = 0) {
    const int rows_below = total_rows - c - NB;
    double* Acc = A + (int64_t)c * lda + c;
    if (prof) {
      prof->panel_marks.push_back(prof->used);
      hipEventRecord(prof->next(), st);
    }
    double* stage_out = diag_stage + (int64_t)c * STAGE_LD;
    double* invd = inv_diag + (int64_t)(c / NB) * NB * NB;
    // fused: every workgroup factors the diagonal block and solves its 64 rows.  split: one workgroup per cell, the `last` role of the
    // panel kernel alone (L11 staged, L11^-1, pivots; right-hand side as a vector: beta_j = L11^-1 y_j at its end) ...
    double* yv = yvec ? yvec + c : nullptr;
    const int own_rows = split_panel ? (pair == 1 ? NB : 0) : rows_below;
    const int nchunks = (own_rows + PANEL_OWN_ROWS - 1) / PANEL_OWN_ROWS;
    const auto diag = fuse ? potrf_panel_kernel<true> : potrf_panel_kernel<false>;
    hipLaunchKernelGGL(diag, dim3(nchunks + 1, batch), dim3(256), 0, st, Acc, lda,
                       own_rows, nchunks, invd, info, col_base + c, stage_out, prev_stage, prev_dst, NB, cs, info_stride, yv, (int)(pair == 2 && yv));
    // ... then the rows below it, 128 per workgroup (and L21 beta_j off the entries of y below)
    if (pair == 2) {
      if (rows_below > 0) {
        const auto rows = yv ? potrf_rows_pair_kernel<true> : potrf_rows_pair_kernel<false>;
        hipLaunchKernelGGL(rows, dim3((rows_below + ROWS_WG - 1) / ROWS_WG, batch), dim3(256), 0, st, Acc + (int64_t)NB * lda - NB, lda, rows_below,
                           (const double*)(stage_out - (int64_t)NB * STAGE_LD), (const double*)stage_out, cs, yv ? yv - NB : nullptr);
      }
    } else if (split_panel && rows_below > 0 && pair == 0) {
      const auto rows = fuse ? (yv ? potrf_rows_kernel<true, true> : potrf_rows_kernel<true, false>)
                             : (yv ? potrf_rows_kernel<false, true> : potrf_rows_kernel<false, false>);
      hipLaunchKernelGGL(rows, dim3((rows_below + ROWS_WG - 1) / ROWS_WG, batch), dim3(256), 0, st, Acc + (int64_t)NB * lda, lda, rows_below,
                         (const double*)stage_out, cs, yv);
    }
    prev_stage = stage_out;
    prev_dst = Acc;
    if (prof) hipEventRecord(prof->next(), st);
  };
  // an update on the main stream: columns [c1, c1 + n) and every row from c1 down, by the k columns [c0, c0 + k) factored before
  auto update = [&](int c0, int k, int c1, int n, int tile) {
    const int rows = total_rows - c1;
    const double* L21 = A + (int64_t)c1 * lda + c0;
    double* A22 = A + (int64_t)c1 * lda + c1;
    mark_gemm(st, n, rows - n, n, k, k <= 128);  // K <= 128 runs the 64 x 64 GEMM with C prefetch, longer K the main GEMM kernel
    // (K = 64 gets here only with a 64-column outer block, GPRX_OUTER_BLOCK=64 -- a pair of panels fuses it, wider ranges split at
    // K >= 128 -- and runs on 64 x 64 tiles whatever `tile` says, as it did when it had a launch function of its own; the single-stage
    // 64 KiB kernel that function could select is retired)
    hipError_t e = launch_gemm(st, 0, 1, rows, n, k, -1.0, L21, lda, L21, lda, 1.0, A22, lda, GEMM_C_LOWER, k == NB ? 64 : tile, batch, cs, cs, cs);
    mark_end(st);
    if (e != hipSuccess && err == hipSuccess) err = e;
  };
  // Inside an outer block the panels are combined recursively: factor the left half, update the right half with
  // it (K = half the width), factor the right half.  The block's columns are rewritten log2(w / 64) times
  // instead of w / 64 times (a K = 64 update moves 16 bytes of C per 128 flops -- right-looking K = 64 strips were HBM-bound once
  // many cells are batched, 23 against 43 TFLOP/s, and are removed: DESIGN.md 3.2), and most in-block flops run at K >= 128.
  auto factor_range = [&](auto&& self, int c0, int w) -> void {
    if (w <= NB) {
      panel(c0);
      return;
    }
    const int h = ((w / NB + 1) / 2) * NB;
    if (h == NB && w - h == NB && rows_pair) {
      panel(c0, false, 1);
      panel(c0 + h, true, 2);
      return;
    }
    self(self, c0, h);
    if (h == NB && w - h == NB) {
      // the K = 64 update of the right panel rides in its own kernel (split panels too since round 3: the update is HBM-bound there; the
      // separate launch was kept for A/B runs until its measurements were in).  Wider ranges split at K >= 128.
      panel(c0 + h, true);
      return;
    }
    update(c0, h, c0 + h, w - h, 64);
    self(self, c0 + h, w - h);
  };
  for (int C = 0; C < np; C += ob) {
    const int w = (np - C < ob) ? np - C : ob;
    factor_range(factor_range, C, w);
    if (err != hipSuccess) return err;
    const int R = C + w;  // first column right of this block
    if (R >= np) break;
    const int wn = (np - R < ob) ? np - R : ob;     // width of the next block
    // HEAD(J): columns [R, R + wn), rows [R, total_rows); the last writer of these columns is TAIL(J-1) on the aux stream
    if (ps && tail_pending) hipStreamWaitEvent(st, ps->tail_done, 0);
    update(C, w, R, wn, batch > 1 ? bulk_tile : 64);
    if (err != hipSuccess) return err;
    if (ps) hipEventRecord(ps->block_done, st);
    // TAIL(J): columns [R + wn, np), rows [R + wn, total_rows)
    const int R2 = R + wn;
    if (R2 < np) {
      hipStream_t ts = ps ? ps->aux : st;
      if (ps) hipStreamWaitEvent(ts, ps->block_done, 0);
      const int rows = total_rows - R2, cols = np - R2;
      const double* Lrow = A + (int64_t)R2 * lda + C;  // L[R2:, C:C+w]
      mark_gemm(ts, cols, rows - cols, cols, w);
      hipError_t e = launch_gemm(ts, 0, 1, rows, cols, w, -1.0, Lrow, lda, Lrow, lda, 1.0, A + (int64_t)R2 * lda + R2, lda, GEMM_C_LOWER,
                                   bulk_tile, batch, cs, cs, cs);
      mark_end(ts);
      if (e != hipSuccess) return e;
      if (ps) {
        hipEventRecord(ps->tail_done, ts);
        tail_pending = true;
      }
    }
  }
  // the last panel's diagonal block is still staged
  if (prev_stage) hipLaunchKernelGGL(copy_block_kernel, dim3(batch), dim3(256), 0, st, prev_stage, prev_dst, lda, NB, cs);
  // everything later on `st` must see the aux stream's last update
  if (ps && tail_pending) hipStreamWaitEvent(st, ps->tail_done, 0);
  return hipGetLastError();
}

}  // namespace gprx
