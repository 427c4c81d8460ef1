// Depth-frequency maps of a weighted storm catalogue: per cell and depth level the rate at which the level is
// exceeded, accumulated event by event from the events' peak blocks, and its inversion to the depth at a given rate.
//
// freq_accumulate_kernel<LCAP>.  One pass over peak (S, cells).  A workgroup of four waves owns a tile of FREQ_TILE = 64 consecutive cells:
// lane c of every wave is tile cell c, wave w takes the members s = w, w + 4, ... (four loads in flight per lane; a wave reads 512
// consecutive bytes of a member row).  Per member the bin  b = #{ l : d_l < x }  by a binary search with a uniform trip count over the
// levels in LDS (padded with +inf to a power of two above L; a NaN compares false everywhere: b = 0, and it is counted for nan_members
// beside the histogram).  The histogram of a cell has L + 1 bins of 16 bits (S <= 4096), bin-major, two cells to a 32-bit word: bin b
// of tile cell c is half c / 32 of word  b 32 + (c mod 32)  -- the lanes of each half of a wave hit 32 distinct banks whatever their
// bins, and the two halves are served in different LDS cycles.  The four waves count into it with integer LDS adds of 1 or 1 << 16: no
// half can carry into the other (a bin holds at most 4096), and integer adds commute, so the counts do not depend on the order.
// Then wave w walks its quarter of the levels from the top with the running suffix sum  n = #{ s : x_s > d_l } = sum of the bins above l
// (started from the bins above its quarter) and performs, contraction off,
//   t = (double)n / (double)S,  u = w_e t,  rate[l, c] = rate[l, c] + u
// -- three rounded operations; a level with n = 0 is skipped (u = +0 changes no bit: rate is never -0).  Loads and stores of rate are
// 512 consecutive bytes per wave.  A cell's state depends on its own column alone: not on its tile-mates or the grid.  No
// floating-point atomics, no global atomics, plain vector stores, nothing carried between workgroups.
// LCAP = 64: 10 KiB of LDS; LCAP = 256: 36 KiB, four workgroups per compute unit.
//
// freq_invert_kernel.  One thread per cell: one coalesced walk over the L levels counts, for all targets,  k = #{ l : rate[l, c] >= p };
// then r_{k-1}, r_k are read back by index (neighbouring cells have neighbouring k) and the depth follows the definition, contraction off:
//   k = 0: -inf;  k = L: +inf;  step: d_{k-1};  linear: d_{k-1} + (d_k - d_{k-1}) ((r_{k-1} - p) / (r_{k-1} - r_k)).
// A cell with nan_members > 0: depth NaN, bracket -1 (the flag convention of member_verify_kernel).
#pragma once
#include "gprx_common.h"

namespace gprx {

constexpr int FREQ_LMAX = 256;   // levels
constexpr int FREQ_SMAX = 4096;  // members of one event: a 16-bit bin holds them
constexpr int FREQ_PMAX = 16;    // targets per inversion
constexpr int FREQ_TILE = 64;    // cells of a workgroup's tile: one per lane

struct FreqAccumulateArgs {
  const double* peak;    // (members, cells)
  const double* levels;  // (n_levels) on the device, strictly increasing
  int64_t members, cells;
  int n_levels;
  double weight;
  double* rate;      // (n_levels, cells)
  int* nan_members;  // (cells)
};

struct FreqInvertArgs {
  const double* rate;      // (n_levels, cells)
  const int* nan_members;  // (cells)
  const double* levels;    // (n_levels) on the device
  int64_t cells;
  int n_levels, n_aep, interp;  // interp: 0 linear, 1 step
  double aep[FREQ_PMAX];
  double* depth;  // (n_aep, cells)
  int* bracket;   // (n_aep, cells)
};

// the slots of the padded level table: the smallest power of two above n_levels
__host__ __device__ inline int freq_padded_levels(int n_levels) {
  int lp = 2;
  while (lp <= n_levels) lp <<= 1;
  return lp;
}

template <int LCAP>
__global__ __launch_bounds__(256) void freq_accumulate_kernel(FreqAccumulateArgs p) {
  constexpr int HALF = FREQ_TILE / 2;
  __shared__ double sLev[2 * LCAP];
  __shared__ unsigned sHist[(LCAP + 1) * HALF];
  __shared__ int sNan[FREQ_TILE];
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const int L = p.n_levels, LP = freq_padded_levels(L), S = (int)p.members;
  const int64_t cell = (int64_t)blockIdx.x * FREQ_TILE + lane;
  const bool live = cell < p.cells;
  for (int i = (int)tid; i < LP; i += 256) sLev[i] = i < L ? p.levels[i] : __longlong_as_double(0x7ff0000000000000ll);
  for (int i = (int)tid; i < (L + 1) * HALF; i += 256) sHist[i] = 0u;
  if (tid < (unsigned)FREQ_TILE) sNan[tid] = 0;
  __syncthreads();
  const unsigned word = lane & (unsigned)(HALF - 1), one = lane < (unsigned)HALF ? 1u : 0x10000u;
  if (live) {
    const double* col = p.peak + cell;
    int nans = 0;
    for (int s0 = (int)wave; s0 < S; s0 += 16) {
      double x[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int s = s0 + 4 * j;
        x[j] = s < S ? col[(int64_t)s * p.cells] : 0.0;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (s0 + 4 * j >= S) break;
        int b = 0;
        for (int step = LP >> 1; step; step >>= 1) b += sLev[b + step - 1] < x[j] ? step : 0;
        nans += x[j] != x[j] ? 1 : 0;
        atomicAdd(&sHist[(unsigned)b * HALF + word], one);
      }
    }
    if (nans) atomicAdd(&sNan[lane], nans);
  }
  __syncthreads();
  if (!live) return;
  if (wave == 0 && sNan[lane]) p.nan_members[cell] += sNan[lane];
  const unsigned shift = lane < (unsigned)HALF ? 0u : 16u;
  const int quarter = (L + 3) >> 2, lo = (int)wave * quarter, hi = min(L, lo + quarter);
  if (lo >= hi) return;
  int n = 0;
  for (int b = L; b > hi; --b) n += (int)((sHist[(unsigned)b * HALF + word] >> shift) & 0xffffu);
  const double members = (double)S, w = p.weight;
  double* rate = p.rate + cell;
  for (int l = hi - 1; l >= lo; --l) {
    n += (int)((sHist[(unsigned)(l + 1) * HALF + word] >> shift) & 0xffffu);
    if (n) {
#pragma clang fp contract(off)
      const double t = (double)n / members;
      const double u = w * t;
      const int64_t at = (int64_t)l * p.cells;
      rate[at] = rate[at] + u;
    }
  }
}

__global__ __launch_bounds__(256) void freq_invert_kernel(FreqInvertArgs p) {
  __shared__ double sLev[FREQ_LMAX];
  const int L = p.n_levels;
  for (int i = (int)threadIdx.x; i < L; i += 256) sLev[i] = p.levels[i];
  __syncthreads();
  const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (c >= p.cells) return;
  const double* col = p.rate + c;
  int k[FREQ_PMAX];
#pragma unroll
  for (int j = 0; j < FREQ_PMAX; ++j) k[j] = 0;
  for (int l = 0; l < L; ++l) {
    const double r = col[(int64_t)l * p.cells];
#pragma unroll
    for (int j = 0; j < FREQ_PMAX; ++j) k[j] += (j < p.n_aep && r >= p.aep[j]) ? 1 : 0;
  }
  const bool flagged = p.nan_members[c] > 0;
#pragma unroll
  for (int j = 0; j < FREQ_PMAX; ++j) {
    if (j >= p.n_aep) break;
    const int kj = k[j];
    double depth;
    if (flagged) depth = __longlong_as_double(0x7ff8000000000000ll);
    else if (kj == 0) depth = __longlong_as_double(0xfff0000000000000ll);
    else if (kj == L) depth = __longlong_as_double(0x7ff0000000000000ll);
    else if (p.interp) depth = sLev[kj - 1];
    else {
#pragma clang fp contract(off)
      const double r_lo = col[(int64_t)(kj - 1) * p.cells], r_hi = col[(int64_t)kj * p.cells];
      const double a = r_lo - p.aep[j];
      const double b = r_lo - r_hi;
      const double f = a / b;
      const double g = sLev[kj] - sLev[kj - 1];
      const double gf = g * f;
      depth = sLev[kj - 1] + gf;
    }
    p.depth[(int64_t)j * p.cells + c] = depth;
    p.bracket[(int64_t)j * p.cells + c] = flagged ? -1 : kj;
  }
}

}  // namespace gprx
