// LF-to-HF mesh resampling (gpras/preprocess.py:163-174, :363-377, :433-451) on the device: one stream kernel that builds the
// (T, n_out) field on the high-fidelity cells from a (T, n_src) output block of the low-fidelity plan.
//
//   gather:    out[t, j] = src[t, idx[j]]                                   (vals[:, hf_resampler], :173; vals[:, lf_resampler], :373)
//   floor:     v = src[t, idx[j]]; out = v < elev[j] ? elev[j] : v          (the mask vals < cell_elevations, :375-376: a NaN value
//              stays, a NaN elevation never wins)
//   velocity:  out = sqrt(vx vx + vy vy) of the two gathered operands       (:367-373; the reference squares before it gathers, the
//              same operations per element)
//   linear:    acc = ((0.0 + c0 z0) + c1 z1) + c2 z2 with z_v = src[t, idx[v][j]], the weights c_v of the host
//              (scipy's LinearNDInterpolator, operation by operation, :445-447); with elevations
//              out = (acc < elev || acc != acc) ? elev : acc (:449-450), without out = acc.  A point outside the hull is stored as
//              vertices (0, 0, 0) with NaN weights: acc is NaN whatever the row holds and nothing is read out of range.
//
// A thread owns two adjacent output cells (16-byte stores when the pitch and the base allow, 8-byte loads of idx, 16-byte loads of
// the weights and elevations: those arrays are allocated to an even count) and the RS_RT x rs_groups(NV) rows of a tile, for which the
// indices, weights and elevations stay in registers.  The rows go in groups of RS_RT: the gathered loads of a group are issued
// before its first result is formed.  The grid strides over tiles, column tiles fastest, so that the workgroups in flight read the
// same source rows through L2.  Columns [n_out, ldo) of out are zeroed (the padding that gprx_pca_transform_dev needs finite).
// Contraction is off: the products and sums are the reference's IEEE operations in the reference's order.
#pragma once
#include "gprx_common.h"

namespace gprx {

constexpr int64_t RS_MAX_SRC = (int64_t)1 << 28;  // source cells per row: a cell's byte offset in its row fits 32 bits
constexpr int RS_RT = 8, RS_NT = 256;
// A tile is 2 RS_NT columns x rs_groups(NV) groups of RS_RT rows.  Four groups for the linear form, whose 44 bytes of indices,
// weights and elevation per cell are then read once per 32 rows; one for the others (12 bytes per cell at most), which measured
// slower with four.
constexpr int rs_groups(int nv) { return nv == 3 ? 4 : 1; }

struct RsArgs {
  const double* src;   // (T, lds)
  const double* src2;  // (T, lds) second velocity component; velocity instantiation only
  const int* idx;      // NV planes of `ce` indices in [0, n_src)
  const double* w;     // NV planes of `ce` weights; linear instantiation only
  const double* elev;  // (ce) floor; may be null
  double* out;         // (T, ldo); columns [n_out, ldo) are set to 0
  int64_t T, n_out, ce, lds, ldo;
};

// NV: vertices per output cell (1: nearest, 3: linear).  VEL: velocity magnitude (NV = 1).  VO: 16-byte stores of out.
template <int NV, bool VEL, bool VO>
__global__ __launch_bounds__(RS_NT) void rs_kernel(RsArgs a) {
#pragma clang fp contract(off)
  constexpr int RS_RG = rs_groups(NV);
  static_assert(NV == 1 || (NV == 3 && !VEL), "nearest, velocity or linear");
  const int64_t pairs = (a.ldo + 1) / 2, ctiles = (pairs + RS_NT - 1) / RS_NT, rtiles = (a.T + RS_RT * RS_RG - 1) / (RS_RT * RS_RG);
  for (int64_t tile = blockIdx.x; tile < ctiles * rtiles; tile += gridDim.x) {
    // the row tile is the same for the whole wave: read as a scalar it keeps every row base in scalar registers (the 64-bit
    // division runs on the vector unit, which hides the uniformity from the compiler)
    const int64_t tr = __builtin_amdgcn_readfirstlane((int)(tile / ctiles));
    const int64_t c0 = 2 * ((tile - tr * ctiles) * RS_NT + threadIdx.x), tile_t0 = tr * (RS_RT * RS_RG);
    if (c0 >= a.ldo) continue;  // no barriers below
    const bool in0 = c0 < a.n_out, in1 = c0 + 1 < a.n_out, st1 = c0 + 1 < a.ldo;
    unsigned i0[NV], i1[NV];  // byte offsets into a source row (n_src <= RS_MAX_SRC: below 2^31)
    double w0[NV], w1[NV], e0 = 0.0, e1 = 0.0;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      i0[v] = i1[v] = 0;
      w0[v] = w1[v] = 0.0;
    }
    if (in0) {  // the per-cell arrays are allocated to an even count: the pair is readable whenever its first cell exists
#pragma unroll
      for (int v = 0; v < NV; ++v) {
        const int2 ii = *reinterpret_cast<const int2*>(a.idx + v * a.ce + c0);
        i0[v] = 8u * (unsigned)ii.x;
        i1[v] = in1 ? 8u * (unsigned)ii.y : 0u;
        if constexpr (NV == 3) {
          const double2 ww = *reinterpret_cast<const double2*>(a.w + v * a.ce + c0);
          w0[v] = ww.x;
          w1[v] = ww.y;
        }
      }
      if (a.elev) {
        const double2 ee = *reinterpret_cast<const double2*>(a.elev + c0);
        e0 = ee.x;
        e1 = ee.y;
      }
    }
#pragma unroll 1  // one group's loads in flight: more would cost the waves that hide them
    for (int g = 0; g < RS_RG; ++g) {
      // The group's number goes through an empty asm statement: seen as a loop counter it lets the compiler turn every gathered
      // address into a 64-bit vector induction variable of its own (strength reduction), 2 registers per load in flight.
      int gs = g;
      asm volatile("" : "+s"(gs));
      const int64_t t0 = tile_t0 + (int64_t)gs * RS_RT;
      if (t0 >= a.T) break;
      const int nr = (int)(a.T - t0 < RS_RT ? a.T - t0 : RS_RT);
      constexpr int NS = VEL ? 2 : NV;  // gathered operands per cell
      double z0[RS_RT][NS], z1[RS_RT][NS];
      if (in0) {
#pragma unroll
        for (int r = 0; r < RS_RT; ++r) {
          if (r >= nr) break;
          const char* p = reinterpret_cast<const char*>(a.src + (t0 + r) * a.lds);  // wave-uniform row base + 32-bit byte offset
#pragma unroll
          for (int v = 0; v < NV; ++v) {
            z0[r][v] = *reinterpret_cast<const double*>(p + i0[v]);
            z1[r][v] = *reinterpret_cast<const double*>(p + i1[v]);
          }
          if constexpr (VEL) {
            const char* q = reinterpret_cast<const char*>(a.src2 + (t0 + r) * a.lds);
            z0[r][1] = *reinterpret_cast<const double*>(q + i0[0]);
            z1[r][1] = *reinterpret_cast<const double*>(q + i1[0]);
          }
        }
      }
#pragma unroll
      for (int r = 0; r < RS_RT; ++r) {
        if (r >= nr) break;
        double v0 = 0.0, v1 = 0.0;
        if (in0) {
          if constexpr (VEL) {
            v0 = sqrt(z0[r][0] * z0[r][0] + z0[r][1] * z0[r][1]);
            v1 = sqrt(z1[r][0] * z1[r][0] + z1[r][1] * z1[r][1]);
          } else if constexpr (NV == 3) {
            v0 = ((0.0 + w0[0] * z0[r][0]) + w0[1] * z0[r][1]) + w0[2] * z0[r][2];
            v1 = ((0.0 + w1[0] * z1[r][0]) + w1[1] * z1[r][1]) + w1[2] * z1[r][2];
            if (a.elev) {
              v0 = (v0 < e0 || v0 != v0) ? e0 : v0;
              v1 = (v1 < e1 || v1 != v1) ? e1 : v1;
            }
          } else {
            v0 = z0[r][0];
            v1 = z1[r][0];
            if (a.elev) {
              v0 = v0 < e0 ? e0 : v0;
              v1 = v1 < e1 ? e1 : v1;
            }
          }
          if (!in1) v1 = 0.0;
        }
        double* o = a.out + (t0 + r) * a.ldo + c0;
        if (VO && st1) {
          *reinterpret_cast<double2*>(o) = make_double2(v0, v1);
        } else {
          o[0] = v0;
          if (st1) o[1] = v1;
        }
      }
    }
  }
}

}  // namespace gprx
