// Leave-one-event-out downdate of fitted sparse models with up to 320 inducing points (sf_loeo.h, LoeoBlockedParams): the kernels around
// the batched Cholesky and triangular inverse -- H = I - t2 t2^T / s per 64 x 64 tile, c' = P (c - u / s), and W = P t2 with the column
// sums of W c' and W^2.  fp64 MFMA on 64 x 64 tiles, 256 threads, LDS rows 65 doubles apart.
#include "sgpr_fused_dev.h"

#include <limits>

#include "sf_loeo.h"
#include "sf_loeo_dev.h"

namespace gprx {

namespace {
struct LoeoSlot {
  int col0, len, orow;
  const double* A;   // the cell's block of the arena
  const double* par; // its row of the cell-parameter table
  double* slot;
};
__device__ __forceinline__ LoeoSlot loeo_slot(const LoeoBlockedParams& p, int ev, int cell) {
  LoeoSlot s;
  s.col0 = p.base.events[LOEO_EV * ev];
  s.len = p.base.events[LOEO_EV * ev + 1];
  s.orow = p.base.events[LOEO_EV * ev + 2];
  s.A = p.base.arena + (int64_t)cell * p.base.ss;
  s.par = p.base.cpar + (int64_t)cell * CELL_PAR;
  s.slot = p.ws + ((int64_t)cell * p.group_events + ev) * p.slot_stride;
  return s;
}
}  // namespace

// MFMA layout as sf_loeo_kernel's: wave w owns rows 16 w .. 16 w + 15 of the tile, lane (g = lane >> 4, r = lane & 15) holds
// C[16 w + g + 4 q][16 kt + r]; instruction j of k stage ks takes k = 16 ks + 4 g + j.

// ---- H = I - t2 t2^T / s, tile (bi, bj) with bj <= bi; the workgroups of the first tile column also form u = t2 y for their band ----
__global__ __launch_bounds__(256) void loeo_gram_kernel(LoeoBlockedParams p) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  int bi = 0;
  while ((bi + 1) * (bi + 2) / 2 <= (int)blockIdx.x) ++bi;
  const int bj = (int)blockIdx.x - bi * (bi + 1) / 2;
  double* sA = smem;                                 // rows of band bi, a 64-column chunk of the event
  double* sB = bi == bj ? sA : sA + NB * SM_LD;      // rows of band bj
  double* sy = smem + 2 * NB * SM_LD;                // [64] y of the chunk
  double* part = sy + NB;                            // [4][64]
  const int ev = blockIdx.y, cell = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
  const LoeoSlot s = loeo_slot(p, ev, cell);
  const double inv_s = s.par[3];
  const int unit = (int)s.par[2];
  const double* T = s.A + p.base.oKs + s.col0;
  const double* y = p.base.Y + (int64_t)unit * p.base.np + s.orow;
  const int urow = tid & 63, uq = tid >> 6;
  const bool with_u = bj == 0;
  if (blockIdx.x == 0 && tid == 0) *reinterpret_cast<int*>(s.slot + p.oInfo) = 0;

  d4 acc[4];
#pragma unroll
  for (int kt = 0; kt < 4; ++kt) acc[kt] = d4{0.0, 0.0, 0.0, 0.0};
  double upart = 0.0;
  for (int c0 = 0; c0 < s.len; c0 += NB) {  // from the EVENT's first column on: the bits do not depend on its place in the tile
    const int nc = min(NB, s.len - c0);
    __syncthreads();  // the previous chunk's readers are done
    loeo_stage(T + (int64_t)bi * NB * p.base.ldk, p.base.ldk, c0, nc, sA, tid);
    if (bi != bj) loeo_stage(T + (int64_t)bj * NB * p.base.ldk, p.base.ldk, c0, nc, sB, tid);
    if (with_u && tid < NB) sy[tid] = tid < nc ? y[c0 + tid] : 0.0;
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int k = 16 * ks + 4 * g + j;
        const double a = sA[(16 * wave + r) * SM_LD + k];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) acc[kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sB[(16 * kt + r) * SM_LD + k], acc[kt], 0, 0, 0);
      }
    if (with_u) {
#pragma unroll
      for (int i = 0; i < 16; ++i) upart = __builtin_fma(sA[urow * SM_LD + 16 * uq + i], sy[16 * uq + i], upart);
    }
  }
  double* H = s.slot + p.oH + (int64_t)bi * NB * p.mp + bj * NB;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = 16 * wave + g + 4 * q, col = 16 * kt + r;
      H[(int64_t)row * p.mp + col] = __builtin_fma(-acc[kt][q], inv_s, (bi == bj && row == col) ? 1.0 : 0.0);
    }
  if (with_u) {
    part[uq * NB + urow] = upart;
    __syncthreads();
    if (tid < NB) s.slot[p.oU + bi * NB + tid] = ((part[tid] + part[NB + tid]) + part[2 * NB + tid]) + part[3 * NB + tid];
  }
}
constexpr size_t LOEO_GRAM_SMEM = sizeof(double) * (2 * NB * SM_LD + NB + 4 * NB);

// ---- c' = P (c - u / s), one row band per workgroup: every row is one sum per lane over k = lane, lane + 64, ..., then over the lanes ----
__global__ __launch_bounds__(256) void loeo_cprime_kernel(LoeoBlockedParams p) {
  __shared__ double sb[LOEO_BLOCKED_MAX_MP];
  __shared__ double sRed[NB * SM_LD];
  const int ib = blockIdx.x, ev = blockIdx.y, cell = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const LoeoSlot s = loeo_slot(p, ev, cell);
  const double inv_s = s.par[3];
  const int kend = (ib + 1) * NB;
  for (int k = tid; k < kend; k += 256) sb[k] = __builtin_fma(-s.slot[p.oU + k], inv_s, s.A[p.base.oC + k]);
  __syncthreads();
  const double* P = s.slot + p.oP;
  for (int rl = 0; rl < 16; ++rl) {
    const int row = 16 * wave + rl, grow = ib * NB + row;
    double sum = 0.0;
    for (int kb = 0; kb <= ib; ++kb) {
      const int k = kb * NB + lane;
      const double v = P[(int64_t)grow * p.mp + k];
      sum = __builtin_fma(k <= grow ? v : 0.0, sb[k], sum);  // (the diagonal tile through a mask: P is lower triangular)
    }
    sRed[row * SM_LD + lane] = sum;
  }
  __syncthreads();
  if (tid < NB) {
    double sum = 0.0;
    for (int l = 0; l < NB; ++l) sum += sRed[tid * SM_LD + l];
    s.slot[p.oCp + ib * NB + tid] = sum;
  }
}

// ---- W = P t2 for one 64-column chunk of an event, row band after row band; mean = W^T c', var += colsum(W^2) (+ s, last) ----
// The tile of band kb of t2 is staged again for every (ib, kb), out of L2: a variant that kept the chunk of every band resident in LDS
// (possible up to mp = 192) was measured slower, 151 KB of LDS leave one workgroup per CU, and is gone.
__global__ __launch_bounds__(256) void loeo_apply_kernel(LoeoBlockedParams p) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const int nb = p.mp / NB;
  double* sP = smem;                       // a tile of P; after a band's products: the column partials of mean and variance
  double* sT = sP + NB * SM_LD;            // a tile of t2
  double* scp = sT + NB * SM_LD;           // [mp] c'
  double* pmean = sP;                      // [16][64]: partial of (wave, g) for every column
  double* pvar = sP + 16 * NB;
  static_assert(2 * 16 * NB <= NB * SM_LD, "the column partials fit into the tile of P");
  const int ev = blockIdx.y, cell = blockIdx.z, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g = lane >> 4, r = lane & 15;
  const LoeoSlot s = loeo_slot(p, ev, cell);
  const int c0 = NB * (int)blockIdx.x;
  if (c0 >= s.len) return;
  const int nc = min(NB, s.len - c0);
  double* mean = p.base.means + (int64_t)cell * p.base.out_stride + s.orow + c0;
  double* var = p.base.vars + (int64_t)cell * p.base.out_stride + s.orow + c0;
  const int bad = *reinterpret_cast<const int*>(s.slot + p.oInfo);
  if (bad != 0) {  // (uniform over the workgroup) chol(H) stopped at pivot `bad`: the event's rows are NaN in this cell
    if (blockIdx.x == 0 && tid == 0) p.base.status[(int64_t)cell * p.base.status_stride + ev] = bad;
    const double qnan = std::numeric_limits<double>::quiet_NaN();
    if (tid < nc) {
      mean[tid] = qnan;
      var[tid] = qnan;
    }
    return;
  }
  const double s_add = p.base.include_noise ? s.par[1] : 0.0;
  const double* T = s.A + p.base.oKs + s.col0;
  const double* P = s.slot + p.oP;
  for (int k = tid; k < p.mp; k += 256) scp[k] = s.slot[p.oCp + k];
  double m_acc = 0.0, v_acc = 0.0;  // of column tid (tid < 64), over the bands in ascending order
  for (int ib = 0; ib < nb; ++ib) {
    d4 w[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) w[kt] = d4{0.0, 0.0, 0.0, 0.0};
    for (int kb = 0; kb <= ib; ++kb) {
      __syncthreads();  // the previous tile's readers (and the readers of the previous band's partials) are done
      {
        const double* Pt = P + (int64_t)ib * NB * p.mp + kb * NB;
        double v[16];
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int q = tid + 256 * e, i = q >> 6, j = q & 63;
          v[e] = Pt[(int64_t)i * p.mp + j];
        }
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int q = tid + 256 * e, i = q >> 6, j = q & 63;
          sP[i * SM_LD + j] = (kb < ib || j <= i) ? v[e] : 0.0;  // (P is lower triangular: its diagonal tiles through a mask)
        }
      }
      loeo_stage(T + (int64_t)kb * NB * p.base.ldk, p.base.ldk, c0, nc, sT, tid);
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = 16 * ks + 4 * g + j;
          const double a = sP[(16 * wave + r) * SM_LD + k];
#pragma unroll
          for (int kt = 0; kt < 4; ++kt) w[kt] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, sT[k * SM_LD + 16 * kt + r], w[kt], 0, 0, 0);
        }
    }
    __syncthreads();  // every wave has read the last tile of P: its place takes the partials
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      double pm = 0.0, pv = 0.0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        pm = __builtin_fma(w[kt][q], scp[ib * NB + 16 * wave + g + 4 * q], pm);
        pv = __builtin_fma(w[kt][q], w[kt][q], pv);
      }
      pmean[(4 * wave + g) * NB + 16 * kt + r] = pm;
      pvar[(4 * wave + g) * NB + 16 * kt + r] = pv;
    }
    __syncthreads();
    if (tid < NB) {
      double m = 0.0, v = 0.0;
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        m += pmean[e * NB + tid];
        v += pvar[e * NB + tid];
      }
      m_acc += m;
      v_acc += v;
    }
  }
  if (tid < nc) {
    mean[tid] = m_acc;
    var[tid] = (var[tid] + v_acc) + s_add;  // (the noise last: predict_y is predict_f + s to the bit)
  }
}
inline size_t loeo_apply_smem(int mp) { return sizeof(double) * ((size_t)2 * NB * SM_LD + mp); }

hipError_t sf_launch_loeo_gram(hipStream_t st, const LoeoBlockedParams& p, int cells) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(loeo_gram_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)LOEO_GRAM_SMEM);
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  const int nb = p.mp / NB;
  hipLaunchKernelGGL(loeo_gram_kernel, dim3(nb * (nb + 1) / 2, p.group_events, cells), dim3(256), LOEO_GRAM_SMEM, st, p);
  return hipGetLastError();
}

hipError_t sf_launch_loeo_cprime(hipStream_t st, const LoeoBlockedParams& p, int cells) {
  hipLaunchKernelGGL(loeo_cprime_kernel, dim3(p.mp / NB, p.group_events, cells), dim3(256), 0, st, p);
  return hipGetLastError();
}

hipError_t sf_launch_loeo_apply(hipStream_t st, const LoeoBlockedParams& p, int chunks, int cells) {
  static bool attr_set = false;
  if (!attr_set) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(loeo_apply_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       (int)loeo_apply_smem(LOEO_BLOCKED_MAX_MP));
    if (e != hipSuccess) return e;
    attr_set = true;
  }
  if (p.mp % NB != 0 || p.mp < NB || p.mp > LOEO_BLOCKED_MAX_MP || chunks <= 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(loeo_apply_kernel, dim3(chunks, p.group_events, cells), dim3(256), loeo_apply_smem(p.mp), st, p);
  return hipGetLastError();
}

}  // namespace gprx
