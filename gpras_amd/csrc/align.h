// Per-event temporal clipping (gpras/preprocess.py:89-155: DataBuilder._align_datasets, get_cutoff, _delta_cols_norm) on the device.
//
// The input is 1-4 blocks (ptr, cols, ld) that share `rows`; side by side they are the reference's `combo`, (rows, C).  Nothing is
// concatenated: virtual column c belongs to the block whose column range holds it.  Columns [cols, ld) of a block are never read.
//
//   scan:         first = the first row that holds a NaN in any column, `rows` when none does (:138-140); an integer minimum.
//                 T' = first rows are used, nd = T' - 1 difference rows.
//   normalisers:  n_c = sum_t |a[t+1, c] - a[t, c]|, t = 0 .. nd-1 in ascending order, one thread per column (numpy's order for
//                 sum(axis=0) of a C-ordered array, :152); 0 becomes 1 (:153).
//   row sums:     q[t, c] = |a[t+1, c] - a[t, c]| / n_c, a division (:154); r_t = sum_c q[t, c] (:142) in THIS order, fixed by the
//                 virtual column index alone:
//                   1. wave strip w = c / 64: the 64 values (0.0 for c >= C) by a balanced tree over adjacent lanes,
//                      (((q0 + q1) + (q2 + q3)) + ...), six levels (gprx_common.h wave_sum_dpp);
//                   2. strip s = c / 256: its four wave strips as ((w0 + w1) + w2) + w3;
//                   3. r_t = (((s0 + s1) + s2) + ...) over the strips in ascending order (al_combine_kernel).
//                 No floating-point atomics; the grid, the CU count and the block boundaries do not enter.
//   finish:       total = r_0 + r_1 + ... sequentially, u_t = r_t / total, cum = the sequential running sum of u (:142-143);
//                 stop = the first t with cum_t > threshold, start = the first t with cum_t > 10e-4, 0 when there is none (numpy's
//                 argmax of an all-False vector, :145-146; an all-constant block gives 0 / 0 = NaN and hence (0, 0)).
//
// Three sweeps read the field: the scan (rows x C), the normalisers (T' x C) and the row sums (a tile of AL_RT difference rows reads
// AL_RT + 1 rows).  Loads are 8 bytes per lane with consecutive lanes on consecutive columns.  Contraction is off: the differences,
// divisions and sums are IEEE operations in the order above, so two calls give the same bits.
#pragma once
#include "gprx_common.h"

namespace gprx {

constexpr int AL_NT = 256;       // threads of a workgroup = columns of a strip
constexpr int AL_WAVES = AL_NT / 64;
constexpr int AL_RT = 32;        // rows of a scan tile, difference rows of a row-sum tile
constexpr int AL_FC = 1024;      // rows the finish kernel stages in LDS at a time
constexpr int AL_MAX_BLOCKS = 4;
constexpr int AL_NO_NAN = 0x7fffffff;

struct AlBlocks {
  const double* p[AL_MAX_BLOCKS];
  int64_t ld[AL_MAX_BLOCKS];
  int64_t c0[AL_MAX_BLOCKS + 1];  // first virtual column of block b; C from the number of blocks on
  int64_t rows;
};

// The column of virtual index c < C: its first element; *ld its pitch.  Constant indices only: the struct stays in scalar registers.
__device__ __forceinline__ const double* al_column(const AlBlocks& B, int64_t c, int64_t* ld) {
  const double* p = B.p[0];
  int64_t l = B.ld[0], off = c;
#pragma unroll
  for (int b = 1; b < AL_MAX_BLOCKS; ++b)
    if (c >= B.c0[b]) {
      p = B.p[b];
      l = B.ld[b];
      off = c - B.c0[b];
    }
  *ld = l;
  return p + off;
}

__global__ void al_init_kernel(int* first, int rows) { *first = rows; }

// grid (strips, row tiles).  *first starts as `rows`.
__global__ __launch_bounds__(AL_NT) void al_scan_kernel(AlBlocks B, int* first) {
  const int64_t c = (int64_t)blockIdx.x * AL_NT + threadIdx.x, C = B.c0[AL_MAX_BLOCKS];
  const bool active = c < C;
  int64_t ld = 0;
  const double* col = active ? al_column(B, c, &ld) : nullptr;
  const int64_t tiles = (B.rows + AL_RT - 1) / AL_RT;
  for (int64_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
    const int64_t t0 = tile * AL_RT;
    // a NaN above this tile is known already: this tile and the later ones cannot lower it (one value for the whole wave: the lanes meet again below)
    if (t0 >= __builtin_amdgcn_readfirstlane(*reinterpret_cast<volatile int*>(first))) break;
    const int nr = (int)(B.rows - t0 < AL_RT ? B.rows - t0 : AL_RT);
    int bad = AL_NO_NAN;
    if (active) {
#pragma unroll 8
      for (int r = 0; r < nr; ++r) {
        const double v = col[(t0 + r) * ld];
        if (v != v && bad == AL_NO_NAN) bad = (int)(t0 + r);
      }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const int o = __shfl_xor(bad, off, 64);
      bad = o < bad ? o : bad;
    }
    if ((threadIdx.x & 63) == 0 && bad != AL_NO_NAN) atomicMin(first, bad);
  }
}

// One thread per column; nrm (C).
__global__ __launch_bounds__(AL_NT) void al_norm_kernel(AlBlocks B, const int* first, double* nrm) {
#pragma clang fp contract(off)
  const int64_t c = (int64_t)blockIdx.x * AL_NT + threadIdx.x;
  if (c >= B.c0[AL_MAX_BLOCKS]) return;
  const int64_t Tp = *first;
  int64_t ld;
  const double* col = al_column(B, c, &ld);
  double acc = 0.0, prev = col[0];
  for (int64_t t = 1; t < Tp; t += 8) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = t + i < Tp ? col[(t + i) * ld] : 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (t + i < Tp) {
        acc += fabs(v[i] - prev);
        prev = v[i];
      }
  }
  nrm[c] = acc == 0.0 ? 1.0 : acc;
}

// grid (strips, row tiles); part (strips, pitch): the strip's sum of every difference row.
__global__ __launch_bounds__(AL_NT) void al_rowsum_kernel(AlBlocks B, const int* first, const double* nrm, double* part, int64_t pitch) {
#pragma clang fp contract(off)
  __shared__ double wsum[AL_WAVES][AL_RT];
  const int64_t c = (int64_t)blockIdx.x * AL_NT + threadIdx.x, nd = (int64_t)*first - 1;
  const bool active = c < B.c0[AL_MAX_BLOCKS];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  int64_t ld = 0;
  const double* col = active ? al_column(B, c, &ld) : nullptr;
  const double n = active ? nrm[c] : 1.0;
  for (int64_t tile = blockIdx.y; tile * AL_RT < nd; tile += gridDim.y) {
    const int64_t t0 = tile * AL_RT;
    const int nr = (int)(nd - t0 < AL_RT ? nd - t0 : AL_RT);  // the same for the whole workgroup
    double prev = active ? col[t0 * ld] : 0.0;
    for (int r = 0; r < nr; r += 8) {
      double v[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) v[i] = active && r + i < nr ? col[(t0 + r + i + 1) * ld] : 0.0;
#pragma unroll
      for (int i = 0; i < 8; ++i)
        if (r + i < nr) {
          const double q = active ? fabs(v[i] - prev) / n : 0.0;
          prev = v[i];
          const double s = wave_sum_dpp(q);  // every lane of the wave is here: r, i and nr are uniform
          if (lane == 0) wsum[wave][r + i] = s;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < nr) {
      double s = wsum[0][threadIdx.x];
#pragma unroll
      for (int w = 1; w < AL_WAVES; ++w) s += wsum[w][threadIdx.x];
      part[(int64_t)blockIdx.x * pitch + t0 + threadIdx.x] = s;
    }
    __syncthreads();
  }
}

// One thread per difference row: the strips in ascending order.
__global__ __launch_bounds__(AL_NT) void al_combine_kernel(const int* first, const double* part, int64_t pitch, int64_t strips, double* r) {
#pragma clang fp contract(off)
  const int64_t t = (int64_t)blockIdx.x * AL_NT + threadIdx.x, nd = (int64_t)*first - 1;
  if (t >= nd) return;
  double acc = part[t];
  for (int64_t s = 1; s < strips; s += 8) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = s + i < strips ? part[(s + i) * pitch + t] : 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (s + i < strips) acc += v[i];
  }
  r[t] = acc;
}

// One workgroup.  r (nd) in; curve (nd) out; res: start, stop, T'.  The sequential sums run in thread 0 over rows staged in LDS.
__global__ __launch_bounds__(AL_NT) void al_finish_kernel(const int* first, const double* r, double threshold, double* curve, int64_t* res) {
#pragma clang fp contract(off)
  __shared__ double buf[AL_FC];
  __shared__ double total_s;
  const int64_t Tp = *first, nd = Tp - 1;
  double total = 0.0;
  for (int64_t t0 = 0; t0 < nd; t0 += AL_FC) {
    const int n = (int)(nd - t0 < AL_FC ? nd - t0 : AL_FC);
    for (int i = threadIdx.x; i < n; i += AL_NT) buf[i] = r[t0 + i];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < n; ++i) total += buf[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) total_s = total;
  __syncthreads();
  total = total_s;
  double cum = 0.0;
  int64_t start = 0, stop = 0;
  bool have_start = false, have_stop = false;
  for (int64_t t0 = 0; t0 < nd; t0 += AL_FC) {
    const int n = (int)(nd - t0 < AL_FC ? nd - t0 : AL_FC);
    for (int i = threadIdx.x; i < n; i += AL_NT) buf[i] = r[t0 + i] / total;
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < n; ++i) {
        cum += buf[i];
        buf[i] = cum;
        if (!have_start && cum > 10e-4) {
          have_start = true;
          start = t0 + i;
        }
        if (!have_stop && cum > threshold) {
          have_stop = true;
          stop = t0 + i;
        }
      }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += AL_NT) curve[t0 + i] = buf[i];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    res[0] = start;
    res[1] = stop;
    res[2] = Tp;
  }
}

// dst (n, ldd) = rows [start, start + n) of src (., lds), columns [cols, ldd) set to 0.  grid (column tiles, groups of 8 rows).
__global__ __launch_bounds__(AL_NT) void al_clip_kernel(const double* src, int64_t lds, int64_t cols, int64_t start, int64_t n, double* dst, int64_t ldd) {
  const int64_t j = (int64_t)blockIdx.x * AL_NT + threadIdx.x;
  if (j >= ldd) return;
  const bool in = j < cols;
  for (int64_t r0 = (int64_t)blockIdx.y * 8; r0 < n; r0 += (int64_t)gridDim.y * 8) {
    double v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = in && r0 + i < n ? src[(start + r0 + i) * lds + j] : 0.0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
      if (r0 + i < n) dst[(r0 + i) * ldd + j] = v[i];
  }
}

}  // namespace gprx
