// Leave-one-event-out downdate of fitted sparse models (sf_loeo.h): one workgroup per (event, cell) around the 64 x 64 chain.
#include "sgpr_fused_dev.h"

#include <limits>

#include "sf_loeo.h"
#include "sf_loeo_dev.h"

namespace gprx {

// MFMA layout as chain_step's: wave w owns row band w (rows 16 w .. 16 w + 15), lane (g = lane >> 4, r = lane & 15) holds C[16 w + g + 4 q][16 kt + r];
// instruction j of k stage ks takes k = 16 ks + 4 g + j.
__global__ __launch_bounds__(256) void sf_loeo_kernel(LoeoParams p) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  double* sT = smem;                  // a 64-column chunk of t2
  double* sH = sT + NB * SM_LD;       // H (lower triangle), then Lh^-1
  double* sIn = sH + NB * SM_LD;      // chain buffers; pass B: the column partials of mean and variance
  double* sX = sIn + 2 * NB * PSUB;
  double* sy = sX + 2 * NB * PSUB;    // [64] y of the chunk
  double* sb = sy + NB;               // [64] c - u / s
  double* sc = sb + NB;               // [64] c'
  double* part = sc + NB;             // [4][64]
  const int ev = blockIdx.x, cell = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
  const int col0 = p.events[LOEO_EV * ev], len = p.events[LOEO_EV * ev + 1], orow = p.events[LOEO_EV * ev + 2];
  const double* par = p.cpar + (int64_t)cell * CELL_PAR;
  const double inv_s = par[3], s_add = p.include_noise ? par[1] : 0.0;
  const int unit = (int)par[2];
  const double* A = p.arena + (int64_t)cell * p.ss;
  const double* T = A + p.oKs + col0;
  const double* y = p.Y + (int64_t)unit * p.np + orow;
  double* mean = p.means + (int64_t)cell * p.out_stride + orow;
  double* var = p.vars + (int64_t)cell * p.out_stride + orow;
  const int urow = tid & 63, uq = tid >> 6;

  // ---- pass A: S = t2 t2^T (the tiles on and below the diagonal), u = t2 y ----
  d4 accS[4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) accS[kt] = d4{0.0, 0.0, 0.0, 0.0};
  double upart = 0.0;
  for (int c0 = 0; c0 < len; c0 += NB) {
    const int nc = min(NB, len - c0);
    __syncthreads();  // the previous chunk's readers are done
    loeo_stage(T, p.ldk, c0, nc, sT, tid);
    if (tid < NB) sy[tid] = tid < nc ? y[c0 + tid] : 0.0;
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 16 * ks + 4 * g + j;
        const double a = sT[(16 * wave + r) * SM_LD + k];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
          if (kt <= wave) accS[kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sT[(16 * kt + r) * SM_LD + k], accS[kt], 0, 0, 0);
      }
#pragma unroll
    for (int i = 0; i < 16; ++i) upart = __builtin_fma(sT[urow * SM_LD + 16 * uq + i], sy[16 * uq + i], upart);
  }
  part[uq * NB + urow] = upart;
  // H = I - S / s
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = 16 * wave + g + 4 * q, col = 16 * kt + r;
      if (kt <= wave) sH[row * SM_LD + col] = __builtin_fma(-accS[kt][q], inv_s, row == col ? 1.0 : 0.0);
    }
  __syncthreads();
  if (tid < NB) {
    const double u = ((part[tid] + part[NB + tid]) + part[2 * NB + tid]) + part[3 * NB + tid];
    sb[tid] = __builtin_fma(-u, inv_s, A[p.oC + tid]);
  }
  // ---- Lh = chol(H); the identity rows of the chain come out as Lh^-T ----
  d4 acc[2][4];
  const int bad = sf_chain(sH, SM_LD, sIn, sX, acc, tid);
  __syncthreads();
  if (tid == 0) p.status[(int64_t)cell * p.status_stride + ev] = bad;
  if (bad != 0) {  // (uniform over the workgroup: every thread factors the same 8 x 8 blocks)
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    for (int j = tid; j < len; j += 256) {
      mean[j] = qnan;
      var[j] = qnan;
    }
    return;
  }
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = 16 * wave + g + 4 * q, col = 16 * kt + r;
      sH[col * SM_LD + row] = acc[1][kt][q];  // Lh^-1 = (acc[1])^T
    }
  __syncthreads();
  {  // c' = Lh^-1 (c - u / s)
    double sum = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) sum = __builtin_fma(sH[urow * SM_LD + 16 * uq + i], sb[16 * uq + i], sum);
    part[uq * NB + urow] = sum;
  }
  __syncthreads();
  if (tid < NB) sc[tid] = ((part[tid] + part[NB + tid]) + part[2 * NB + tid]) + part[3 * NB + tid];

  // ---- pass B: W = Lh^-1 t2 (Lh^-1 is lower triangular: row band w needs the k stages 0 .. w), mean and colsum(W^2) ----
  double* pmean = sIn;            // [16][64]: partial of (wave, g) for every column
  double* pvar = sIn + 16 * NB;
  static_assert(2 * 16 * NB <= 2 * 2 * NB * PSUB, "the column partials fit into the chain's sub-panel buffers");
  for (int c0 = 0; c0 < len; c0 += NB) {
    const int nc = min(NB, len - c0);
    __syncthreads();  // the previous chunk's readers are done (the first pass: sc is published)
    loeo_stage(T, p.ldk, c0, nc, sT, tid);
    __syncthreads();
    d4 w[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) w[kt] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
      if (ks <= wave) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = 16 * ks + 4 * g + j;
          const double a = sH[(16 * wave + r) * SM_LD + k];
#pragma unroll
          for (int kt = 0; kt < 4; ++kt) w[kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sT[k * SM_LD + 16 * kt + r], w[kt], 0, 0, 0);
        }
      }
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      double pm = 0.0, pv = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        pm = __builtin_fma(w[kt][q], sc[16 * wave + g + 4 * q], pm);
        pv = __builtin_fma(w[kt][q], w[kt][q], pv);
      }
      pmean[(4 * wave + g) * NB + 16 * kt + r] = pm;
      pvar[(4 * wave + g) * NB + 16 * kt + r] = pv;
    }
    __syncthreads();
    if (tid < nc) {
      double m = 0.0, v = 0.0;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        m += pmean[e * NB + tid];
        v += pvar[e * NB + tid];
      }
      mean[c0 + tid] = m;
      var[c0 + tid] = (var[c0 + tid] + v) + s_add;  // (the noise last: predict_y is predict_f + s to the bit)
    }
  }
}
constexpr size_t SF_LOEO_SMEM = sizeof(double) * (2 * NB * SM_LD + 2 * 2 * NB * PSUB + 3 * NB + 4 * NB);

hipError_t sf_launch_loeo(hipStream_t st, const LoeoParams& p, int events, int cells) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(sf_loeo_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)SF_LOEO_SMEM);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  hipLaunchKernelGGL(sf_loeo_kernel, dim3(events, cells), dim3(256), SF_LOEO_SMEM, st, p);
  return hipGetLastError();
}

}  // namespace gprx
