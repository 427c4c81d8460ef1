// The pseudo-surface low-fidelity model (gpras/preprocess.py:454-697) on the device: rating curves, the centerline fit and the
// water-surface field of PseudoSurfaceDataBuilder.get_lf_plan_data (:581-599).
//
//   1. spline:    RatingCurve.predict (:511-513): a cubic B-spline in FITPACK's form (knots t[0..nt), coefficients c[0..nt-4)).  One
//                 thread per argument; knots and coefficients in LDS.  The interval l (t[l] <= x < t[l+1]) is found by binary search
//                 and clamped to [3, nt - 5], so arguments outside the fitted range are evaluated with the end pieces (FITPACK's
//                 default ext = 0).  The four non-zero basis functions come from the Cox - de Boor recurrence in the order of
//                 FITPACK's fpbspl, the value is their sum with the coefficients, j ascending.
//   2. fit:       _set_centerline_interpolater (:643-667): w[c] = median over the kept rows r of (us[r] - wse[r, c]) / (us[r] - ds[r]).
//                 A workgroup owns PSF_COLS adjacent columns, a thread one of them and every PSF_ROWS-th row, so that a wave-wide
//                 load covers one contiguous segment of PSF_COLS doubles in each of 64 / PSF_COLS rows.  The median is SELECTED, never sorted: eight passes of a
//                 radix select over the order-preserving 64-bit key of the ratio, 8 bits per pass with a 256-bin histogram per
//                 column in LDS, find the element of rank (n - 1) / 2; for an even n its upper neighbour is that same value (ties)
//                 or the smallest larger one (one more pass).  The ratio is formed again in every pass: nothing of size R x C is
//                 written.  Counts are integers, so the result does not depend on the launch shape.  A NaN ratio in a kept row
//                 makes the column NaN (np.median); infinities order as the ends.
//   3. surface:   out[t, c] = max(max(us[t] - (us[t] - ds[t]) * w[idx[c]], elev[c]), fluvial[t, c])  (:592-597) with np.maximum's
//                 NaN rule.  A thread owns two adjacent cells (16 B loads and stores when the row pitch allows) and PS_RT rows, for
//                 which idx, elev and the two weights stay in registers; w lives in LDS.  Columns [cells, ldo) of out are zeroed
//                 (the padding that gprx_pca_transform_dev needs finite).  The same kernel serves interpolate_centerline (:634-637:
//                 idx = identity, no floors) and interpolate_surface (:639-641: values gathered from a (T, C) block).
#pragma once
#include "gprx_common.h"

namespace gprx {

constexpr int PS_MAX_KNOTS = 64 + 8;  // interior knots + 2 x (degree + 1) boundary knots

__global__ __launch_bounds__(256) void ps_spline_kernel(const double* __restrict__ x, int64_t n, const double* __restrict__ t, const double* __restrict__ c,
                                                        int nt, double* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ double st[PS_MAX_KNOTS], sc[PS_MAX_KNOTS];
  for (int i = threadIdx.x; i < nt; i += 256) {
    st[i] = t[i];
    sc[i] = i < nt - 4 ? c[i] : 0.0;
  }
  __syncthreads();
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < n; e += (int64_t)gridDim.x * 256) {
    const double xv = x[e];
    int lo = 3, hi = nt - 5;  // the largest l in [3, nt - 5] with t[l] <= x (l = 3 when there is none; a NaN ends there too)
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (st[mid] <= xv)
        lo = mid;
      else
        hi = mid - 1;
    }
    const int l = lo;
    double h[4] = {1.0, 0.0, 0.0, 0.0}, hh[3];
#pragma unroll
    for (int j = 1; j <= 3; ++j) {
#pragma unroll
      for (int i = 0; i < j; ++i) hh[i] = h[i];
      h[0] = 0.0;
#pragma unroll
      for (int i = 1; i <= j; ++i) {
        const double tli = st[l + i], tlj = st[l + i - j];
        if (tli == tlj) {
          h[i] = 0.0;
        } else {
          const double f = hh[i - 1] / (tli - tlj);
          h[i - 1] = h[i - 1] + f * (tli - xv);
          h[i] = f * (xv - tlj);
        }
      }
    }
    double sp = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) sp = sp + sc[l - 3 + j] * h[j];
    out[e] = sp;
  }
}

// ---- centerline fit ------------------------------------------------------------------------------------------------------------
// 4 columns x 256 rows per step: the kernel is bound by the loads in flight, not by bytes, so many waves and many workgroups
// (C / 4) beat wider row segments (DESIGN.md section 3.14 has the measured shapes)
constexpr int PSF_COLS = 4, PSF_NT = 1024, PSF_ROWS = PSF_NT / PSF_COLS;

// order-preserving key of a double: a < b  <=>  key(a) < key(b) (-0 before +0)
__device__ __forceinline__ unsigned long long ps_key(double v) {
  const unsigned long long b = (unsigned long long)__double_as_longlong(v);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double ps_unkey(unsigned long long k) {
  const unsigned long long b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
  return __longlong_as_double((long long)b);
}

// keep[r] != 0: the row takes part (us_q > 0 or ds_q > 0, :657); n_keep of them (>= 1).  w[c], c < C.
__global__ __launch_bounds__(PSF_NT) void ps_fit_kernel(const double* __restrict__ wse, int64_t R, int64_t C, const double* __restrict__ us,
                                                        const double* __restrict__ ds, const unsigned char* __restrict__ keep, unsigned n_keep,
                                                        double* __restrict__ w) {
#pragma clang fp contract(off)
  __shared__ unsigned hist[PSF_COLS][256];
  __shared__ unsigned long long prefix[PSF_COLS], above[PSF_COLS];
  __shared__ unsigned rank[PSF_COLS], n_eq[PSF_COLS], has_nan[PSF_COLS];
  const int tid = threadIdx.x, lc = tid % PSF_COLS, lr = tid / PSF_COLS;
  const int64_t c = (int64_t)blockIdx.x * PSF_COLS + lc;
  const bool live = c < C;
  const unsigned k1 = (n_keep - 1) / 2, k2 = n_keep / 2;
  if (tid < PSF_COLS) {
    prefix[tid] = 0;
    rank[tid] = k1;
    has_nan[tid] = 0;
    above[tid] = ~0ull;
  }
  for (int pass = 0; pass < 8; ++pass) {
    const int shift = 56 - 8 * pass, above_shift = pass == 0 ? 63 : shift + 8;  // (pass 0 has no leading bits to compare)
    for (int i = tid; i < PSF_COLS * 256; i += PSF_NT) (&hist[0][0])[i] = 0;
    __syncthreads();
    const unsigned long long pre = prefix[lc];
    bool nan_seen = false;
    if (live) {
#pragma unroll 8
      for (int64_t r = lr; r < R; r += PSF_ROWS) {
        // the four loads do not wait for one another (a skipped row costs its loads, not a second round trip)
        const bool kept = keep[r] != 0;
        const double u = us[r], d = ds[r], x = wse[r * C + c];
        const double q = (u - x) / (u - d);
        if (kept && q != q) nan_seen = true;
        const unsigned long long k = ps_key(q);
        // pass 0 sees every kept element; later passes those whose leading bits equal the prefix found so far
        if (kept && (pass == 0 || (k >> above_shift) == (pre >> above_shift))) atomicAdd(&hist[lc][(unsigned)(k >> shift) & 255u], 1u);
      }
    }
    if (pass == 0 && nan_seen) has_nan[lc] = 1;  // every writer writes the same value
    __syncthreads();
    if (tid < PSF_COLS) {
      unsigned want = rank[tid], b = 0;
      for (; b < 255; ++b) {
        const unsigned cnt = hist[tid][b];
        if (want < cnt) break;
        want -= cnt;
      }
      rank[tid] = want;  // rank of the sought element among those of bin b
      n_eq[tid] = hist[tid][b];
      prefix[tid] = prefix[tid] | ((unsigned long long)b << shift);
    }
    __syncthreads();
  }
  // prefix = key of the element of rank k1; n_eq elements equal it, and the sought one is number rank[] among them.
  // Even n: the element of rank k2 = k1 + 1 is the same value when another equal element follows, else the smallest larger key.
  const bool need_next = live && k2 != k1 && !has_nan[lc] && rank[lc] + 1 >= n_eq[lc];
  if (need_next) {
    const unsigned long long pre = prefix[lc];
    unsigned long long best = ~0ull;
#pragma unroll 8
    for (int64_t r = lr; r < R; r += PSF_ROWS) {
      const bool kept = keep[r] != 0;
      const double u = us[r], d = ds[r], x = wse[r * C + c];
      const unsigned long long k = ps_key((u - x) / (u - d));
      if (kept && k > pre && k < best) best = k;
    }
    atomicMin(&above[lc], best);
  }
  __syncthreads();
  if (tid < PSF_COLS && (int64_t)blockIdx.x * PSF_COLS + tid < C) {
    const double a = ps_unkey(prefix[tid]);
    double m = a;
    if (k2 != k1) {
      const double b = rank[tid] + 1 < n_eq[tid] ? a : ps_unkey(above[tid]);
      m = (a + b) / 2.0;
    }
    w[(int64_t)blockIdx.x * PSF_COLS + tid] = has_nan[tid] ? __longlong_as_double(0x7ff8000000000000ll) : m;
  }
}

// ---- surface ---------------------------------------------------------------------------------------------------------------------
constexpr int PS_RT = 8, PS_NT = 256;
constexpr int PS_W_LDS = 8192;  // weights kept in LDS up to this many centerline cells (64 KiB); beyond it they are read through L2

// np.maximum: the first operand when it is not smaller or is NaN, else the second (a NaN on either side comes out)
__device__ __forceinline__ double ps_max(double a, double b) { return (a >= b || a != a) ? a : b; }

struct PsSurfaceArgs {
  const double* us;       // (T) upstream / downstream water-surface elevation of the rows of this call; null with `cl`
  const double* ds;
  const double* w;        // (C) centerline weights
  const double* cl;       // (T, C) centerline values to gather instead of us - (us - ds) w (interpolate_surface); may be null
  const int* idx;         // (cells rounded up to even) nearest centerline cell; null: identity (interpolate_centerline)
  const double* elev;     // (cells rounded up to even) floor; may be null
  const double* fluvial;  // (T, ldf) second floor; may be null
  double* out;            // (T, ldo); columns [cells, ldo) are set to 0
  int64_t T, cells, C, ldf, ldo;
};

// VF / VO: 16-byte loads of fluvial / stores of out (base 16-byte aligned and an even pitch)
template <bool VF, bool VO>
__global__ __launch_bounds__(PS_NT) void ps_surface_kernel(PsSurfaceArgs a) {
#pragma clang fp contract(off)
  extern __shared__ double sw[];
  const bool w_lds = a.w && a.C <= PS_W_LDS;
  if (w_lds) {
    for (int64_t i = threadIdx.x; i < a.C; i += PS_NT) sw[i] = a.w[i];
    __syncthreads();
  }
  const int64_t pairs = (a.ldo + 1) / 2, ctiles = (pairs + PS_NT - 1) / PS_NT, rtiles = (a.T + PS_RT - 1) / PS_RT;
  for (int64_t tile = blockIdx.x; tile < ctiles * rtiles; tile += gridDim.x) {
    const int64_t c0 = 2 * ((tile % ctiles) * PS_NT + threadIdx.x), t0 = (tile / ctiles) * PS_RT;
    if (c0 >= a.ldo) continue;  // no barriers below
    const bool in0 = c0 < a.cells, in1 = c0 + 1 < a.cells, st1 = c0 + 1 < a.ldo;
    int i0 = 0, i1 = 0;
    double e0 = 0.0, e1 = 0.0, w0 = 0.0, w1 = 0.0;
    if (in0) {  // idx and elev are allocated to an even count: the pair is readable whenever its first cell exists
      if (a.idx) {
        const int2 ii = *reinterpret_cast<const int2*>(a.idx + c0);
        i0 = ii.x;
        i1 = in1 ? ii.y : 0;
      } else {
        i0 = (int)c0;
        i1 = in1 ? (int)c0 + 1 : 0;
      }
      if (a.elev) {
        const double2 ee = *reinterpret_cast<const double2*>(a.elev + c0);
        e0 = ee.x;
        e1 = ee.y;
      }
      if (a.w) {
        w0 = w_lds ? sw[i0] : a.w[i0];
        w1 = w_lds ? sw[i1] : a.w[i1];
      }
    }
    const int nr = (int)(a.T - t0 < PS_RT ? a.T - t0 : PS_RT);
    double f0[PS_RT], f1[PS_RT];
    if (a.fluvial && in0) {
#pragma unroll
      for (int r = 0; r < PS_RT; ++r) {
        if (r >= nr) break;
        const double* p = a.fluvial + (t0 + r) * a.ldf + c0;
        if (VF && in1) {
          const double2 v = *reinterpret_cast<const double2*>(p);
          f0[r] = v.x;
          f1[r] = v.y;
        } else {
          f0[r] = p[0];
          f1[r] = in1 ? p[1] : 0.0;
        }
      }
    }
#pragma unroll
    for (int r = 0; r < PS_RT; ++r) {
      if (r >= nr) break;
      const int64_t t = t0 + r;
      double v0 = 0.0, v1 = 0.0;
      if (in0) {
        if (a.cl) {
          v0 = a.cl[t * a.C + i0];
          v1 = in1 ? a.cl[t * a.C + i1] : 0.0;
        } else {
          const double u = a.us[t], rg = u - a.ds[t];
          v0 = u - rg * w0;
          v1 = u - rg * w1;
        }
        if (a.elev) {
          v0 = ps_max(v0, e0);
          v1 = ps_max(v1, e1);
        }
        if (a.fluvial) {
          v0 = ps_max(v0, f0[r]);
          v1 = ps_max(v1, f1[r]);
        }
        if (!in1) v1 = 0.0;
      }
      double* o = a.out + t * a.ldo + c0;
      if (VO && st1) {
        *reinterpret_cast<double2*>(o) = make_double2(v0, v1);
      } else {
        o[0] = v0;
        if (st1) o[1] = v1;
      }
    }
  }
}

}  // namespace gprx
