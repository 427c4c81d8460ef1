// Tile-level building blocks shared by the one-workgroup-per-cell Cholesky (potrf_cell.h) and the opt-in tile-DAG scheduler
// (potrf_dag.h): the write-through / L1-bypassing buffer accessors, the chain's sub-panel step on [64 diagonal rows | 64 identity rows]
// (chain_step: L(k,k) and L(k,k)^-1 in one workgroup) and the 64 x 64 x 64 tile product on swizzled LDS stage images (dag_mma64).
// Round 4: split out of potrf_dag.h so that the product path (the cell kernel) does not include the scheduler (task queue, version
// counters, persistent kernel, and its panel task dag_panel), which is an opt-in of its own.
#pragma once
#include "gemm_f64.h"
#include "chain64.h"
#include "gprx_common.h"
#include "potrf.h"

namespace gprx {

constexpr int DAG_T_LD = NB + 2;       // LDS row stride of the 64 x 64 operand image of the chain (16-byte aligned rows)
constexpr int DAG_SMEM = 2 * NB * NB;  // doubles: workers: A block | B block (4 stage images each); chain: sIn | sX | sT (52 KB of it)
static_assert(2 * PANEL_WG_ROWS * PSUB + NB * DAG_T_LD <= DAG_SMEM, "the chain's buffers fit into the workers' LDS");

// every shared word goes through GLOBAL (never flat) agent-scope accesses; every handed-off double through buffer accesses with
// the sc1 bit (aux 16): stores write through, loads bypass the CU's L1.  Addresses = descriptor base + per-lane byte offset
// (one VGPR) + wave-uniform byte offset (SGPR): no 64-bit per-lane pointers, so the address arithmetic costs no registers.
typedef __attribute__((address_space(1))) int gint;
__device__ __forceinline__ int ld_agent(const int* p) { return __hip_atomic_load((gint*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void st_agent(int* p, int v) { __hip_atomic_store((gint*)p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
typedef unsigned int u4v __attribute__((ext_vector_type(4)));
typedef unsigned int u2v __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t dag_rsrc(const double* base) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<double*>(base), 0, 0xffffffff, 0x00020000);
}
// SC1 = false: plain (cached) accesses for data no other workgroup touches (potrf_cell.h)
template <bool SC1 = true>
__device__ __forceinline__ d2 ld2_sc1(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff = 0) {
  const u4v v = __builtin_amdgcn_raw_buffer_load_b128(r, voff, soff, SC1 ? 16 : 0);
  d2 out;
  __builtin_memcpy(&out, &v, 16);
  return out;
}
template <bool SC1 = true>
__device__ __forceinline__ void st2_sc1(__amdgpu_buffer_rsrc_t r, unsigned voff, d2 v, unsigned soff = 0) {
  u4v raw;
  __builtin_memcpy(&raw, &v, 16);
  __builtin_amdgcn_raw_buffer_store_b128(raw, r, voff, soff, SC1 ? 16 : 0);
}
template <bool SC1 = true>
__device__ __forceinline__ double ld1_sc1(__amdgpu_buffer_rsrc_t r, unsigned voff, unsigned soff = 0) {
  const u2v v = __builtin_amdgcn_raw_buffer_load_b64(r, voff, soff, SC1 ? 16 : 0);
  double out;
  __builtin_memcpy(&out, &v, 8);
  return out;
}
template <bool SC1 = true>
__device__ __forceinline__ void st1_sc1(__amdgpu_buffer_rsrc_t r, unsigned voff, double v, unsigned soff = 0) {
  u2v raw;
  __builtin_memcpy(&raw, &v, 8);
  __builtin_amdgcn_raw_buffer_store_b64(raw, r, voff, soff, SC1 ? 16 : 0);
}
// The 64 x 64 inverse block from its LDS image sT (row c, column m; rows DAG_T_LD apart) to memory, 16 bytes per lane and instruction.
// ALL eight values are read first, the eight stores are issued back to back, and the data registers are kept alive until the stores have
// completed (s_waitcnt vmcnt(0), then an empty asm that still names them).  Round 4: written as a loop { read 16 bytes from LDS; store
// them } the compiler reused the first data register for the next LDS address immediately after each buffer_store_dwordx4 -- it
// inserts no wait state there when the store takes its offset from an SGPR -- and on gfx950 the store unit had not always read its
// data by then: with two workgroups per CU the LOW DWORD of the first double of a store came out as that address in 7-50 % of the
// cells of the workgroups that became resident second (relative error ~5e-7 in a few entries of L(j,j)^-1, differently on every
// run; found with tools/cell_check.hip, which compares the factors of two kernels element by element at full load).
template <bool SC1>
__device__ __forceinline__ void store_inverse_block(__amdgpu_buffer_rsrc_t ri, const double* __restrict__ sT, int tid) {
  d2 iv[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int q = tid + 256 * e;  // 2048 chunks of 16 bytes
    iv[e] = *reinterpret_cast<const d2*>(sT + (q >> 5) * (NB + 2) + 2 * (q & 31));
  }
#pragma unroll
  for (int e = 0; e < 8; ++e) st2_sc1<SC1>(ri, (unsigned)tid * 16u, iv[e], (unsigned)e * 4096u);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
#pragma unroll
  for (int e = 0; e < 8; ++e) asm volatile("" ::"v"(iv[e].x), "v"(iv[e].y));
}
__device__ __forceinline__ void drain_stores() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// ---- workers -------------------------------------------------------------------------------------------------------------
// acc (this wave's 32 x 32 quarter of a 64 x 64 tile) += A B^T over one 64-deep block; ia / ib: the operands' four stage
// images [64 rows][16 k] in LDS, chunks XOR-swizzled (gemm_f64.h kc_swz)
__device__ __forceinline__ void dag_mma64(d4 (&acc)[2][2], const double* __restrict__ ia, const double* __restrict__ ib, int wm, int wn, int g,
                                          int r, int swz) {
#pragma unroll
  for (int s = 0; s < 4; ++s) {
    const double* pa = ia + s * (NB * GEMM_BK);
    const double* pb = ib + s * (NB * GEMM_BK);
    double fa[2][4], fb[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
      const int row = wm * 32 + a * 16 + r;
      const d2 lo = *reinterpret_cast<const d2*>(pa + row * GEMM_BK + 2 * ((2 * g) ^ swz));
      const d2 hi = *reinterpret_cast<const d2*>(pa + row * GEMM_BK + 2 * ((2 * g + 1) ^ swz));
      fa[a][0] = lo.x; fa[a][1] = lo.y; fa[a][2] = hi.x; fa[a][3] = hi.y;
    }
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int col = wn * 32 + b * 16 + r;
      const d2 lo = *reinterpret_cast<const d2*>(pb + col * GEMM_BK + 2 * ((2 * g) ^ swz));
      const d2 hi = *reinterpret_cast<const d2*>(pb + col * GEMM_BK + 2 * ((2 * g + 1) ^ swz));
      fb[b][0] = lo.x; fb[b][1] = lo.y; fb[b][2] = hi.x; fb[b][3] = hi.y;
    }
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f64_16x16x4f64(fa[a][jj], fb[b][jj], acc[a][b], 0, 0, 0);
  }
}

// a matrix in 64 x 64 tiles (tile (i, j) at A + 64 i lda + 64 j) and the inverses of its diagonal blocks (64 x 64 each, in block order)
struct TileCtx {
  double* A;
  int64_t lda;
  const double* inv_diag;
};

}  // namespace gprx
