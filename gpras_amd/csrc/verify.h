// Verification of a peak ensemble against the peak that happened: per cell the members of peak (members, cells)
// sorted on chip, then one walk in rank order for the CRPS of the empirical distribution, the rank counts of the observation and the
// order statistics asked for.
//
// member_verify_kernel<KEYS>.  A workgroup owns a tile of C = KEYS / Sp consecutive cells, Sp = the members rounded up to a power of two
// (at least 32), and holds the C x Sp keys (ens_key of ensemble.h; the slots past the members hold the largest key) in LDS, cell-major:
// key i of tile cell c at  c Sp + (i ^ swz(c)),  swz(c) = (c max(1, 32 / C)) mod 32.  There is no padding -- the XOR takes its place:
//   * the load writes, per member, C consecutive cells (a coalesced row segment): the lanes differ in c alone, so in swz(c) -> other banks;
//   * a compare-exchange stage gives consecutive lanes consecutive cells of one pair (i, i ^ j), then the next pair: 32 lanes are
//     32 cells of one pair (C >= 32), or C cells x 32 / C consecutive pairs, whose i run through 32 / C consecutive values once j >= 32 / C
//     -- the low bits from i, the high bits from swz(c): 32 distinct 8-byte banks.  (C < 32 and j < 32 / C: the run of i has gaps, 2-way.)
//     The partner's address is the own address ^ j: Sp is a power of two, a row starts at a multiple of it;
//   * the walk gives lane c cell c: at step i the lanes read (i ^ swz(c)), again distinct banks.
// The bitonic network runs over all KEYS / 2 pairs per stage with all 256 threads and a barrier per stage; equal keys are never told apart
// afterwards, so the network not being stable does not show.  After it, lane c < C walks its column once, i = 0, 1, ...:
//   x = x_(i), w = x > y ? (S - i) - 0.5 : i + 0.5, acc = acc + |x - y| w (a rounded product, then a rounded addition: contraction off),
//   below += x < y, equal += x == y;  crps = (2 acc) / ((double)S (double)S).
// A cell with a NaN member (the last key of the column is then the NaN key) or a NaN observation gets crps = NaN, below = equal = -1; its
// order statistics still follow the key order.  Infinities follow the formula: |inf - inf| is a NaN and makes the CRPS one, the counts stay
// counts.  A cell's outputs depend on its own column and observation alone: not on its tile-mates, on C or on the grid.  No atomics,
// nothing carried between tiles, plain vector stores.
//
// KEYS = 4096 (32 KiB of LDS, five workgroups per compute unit) serves Sp <= 2048, KEYS = 8192 (64 KiB, two) serves Sp = 4096 with the two
// cells a tile then still has.  Only C of the 256 threads walk, so it is the other resident workgroups' sorting that fills the compute
// unit meanwhile: hence the smaller tile wherever it leaves at least two cells.
#pragma once
#include "ensemble.h"

namespace gprx {

struct MemberVerifyArgs {
  const double* peak;  // (members, cells)
  const double* obs;   // (cells)
  int64_t members, cells;
  int log_sp;  // Sp = 1 << log_sp, 32 <= Sp <= 4096
  int n_rank;
  int rank[ENS_RMAX];
  double* crps;   // (cells)
  int* below;     // (cells)
  int* equal;     // (cells)
  double* order;  // (n_rank, cells)
};

// Sp = 1 << verify_log_sp: the members rounded up to a power of two, at least 32 (the XOR of the layout spans 32 keys); the keys of a tile
inline int verify_log_sp(int64_t members) {
  int log_sp = 5;
  while (((int64_t)1 << log_sp) < members) ++log_sp;
  return log_sp;
}
inline int verify_tile_keys(int log_sp) { return log_sp == 12 ? 8192 : 4096; }

template <int KEYS>
__global__ __launch_bounds__(256) void member_verify_kernel(MemberVerifyArgs p) {
  __shared__ unsigned long long sK[KEYS];
  constexpr int LOG_KEYS = KEYS == 8192 ? 13 : 12;
  static_assert(KEYS == (1 << LOG_KEYS), "the tile is 4096 or 8192 keys");
  const unsigned tid = threadIdx.x;
  const unsigned log_sp = (unsigned)p.log_sp, sp = 1u << log_sp;
  const unsigned log_c = LOG_KEYS - log_sp, C = 1u << log_c;  // 2 <= C <= 256
  const unsigned spread = C >= 32u ? 1u : 32u / C;
  const int64_t c0 = (int64_t)blockIdx.x * C;
  const int S = (int)p.members;
  // load: slot (member i, tile cell c) by thread tid of round it, consecutive threads consecutive cells
  for (unsigned e = tid; e < (unsigned)KEYS; e += 256u) {
    const unsigned c = e & (C - 1u), i = e >> log_c;
    const int64_t cell = c0 + c;
    unsigned long long key = ~0ull;
    if ((int)i < S && cell < p.cells) key = ens_key(p.peak[(int64_t)i * p.cells + cell]);
    sK[(c << log_sp) + (i ^ ((c * spread) & 31u))] = key;
  }
  __syncthreads();
  for (unsigned k = 2u; k <= sp; k <<= 1) {
    for (unsigned j = k >> 1; j; j >>= 1) {
#pragma unroll 4
      for (unsigned pr = tid; pr < (unsigned)(KEYS / 2); pr += 256u) {
        const unsigned c = pr & (C - 1u), q = pr >> log_c;
        const unsigned i = ((q & ~(j - 1u)) << 1) | (q & (j - 1u));  // bit j clear; the partner is i | j
        const unsigned a = (c << log_sp) + (i ^ ((c * spread) & 31u)), b = a ^ j;
        const unsigned long long ka = sK[a], kb = sK[b];
        const bool up = (i & k) == 0u;
        if ((ka > kb) == up) {
          sK[a] = kb;
          sK[b] = ka;
        }
      }
      __syncthreads();
    }
  }
  if (tid >= C) return;
  const int64_t cell = c0 + tid;
  if (cell >= p.cells) return;
  const unsigned long long* col = sK + (tid << log_sp);
  const unsigned sw = (tid * spread) & 31u;
  const double y = p.obs[cell];
  double acc = 0.0;
  int below = 0, equal = 0;
  for (int i = 0; i < S; ++i) {
#pragma clang fp contract(off)
    const double x = ens_unkey(col[(unsigned)i ^ sw]);
    const double w = x > y ? (double)(S - i) - 0.5 : (double)i + 0.5;
    const double t = fabs(x - y) * w;
    acc = acc + t;
    below += x < y ? 1 : 0;
    equal += x == y ? 1 : 0;
  }
  const bool bad = y != y || col[(unsigned)(S - 1) ^ sw] == ~0ull;
  const double ss = (double)S * (double)S;
  p.crps[cell] = bad ? __longlong_as_double(0x7ff8000000000000ll) : (2.0 * acc) / ss;
  p.below[cell] = bad ? -1 : below;
  p.equal[cell] = bad ? -1 : equal;
#pragma unroll
  for (int j = 0; j < ENS_RMAX; ++j)
    if (j < p.n_rank) p.order[(int64_t)j * p.cells + cell] = ens_unkey(col[(unsigned)p.rank[j] ^ sw]);
}

}  // namespace gprx
