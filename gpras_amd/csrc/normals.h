// Standard normals by address: the SAME source on the host and on the device (GPRX_HD, as px_math.h), so that a draw computed on the host
// and the same draw computed inside a kernel agree -- bit for bit wherever only + - * / take part.
//
// Philox4x64-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11; Random123's definition, the generator
// behind numpy.random.Philox).  One round on the counter (c0, c1, c2, c3) with the key (k0, k1):
//   hi0:lo0 = M0 c0,  hi1:lo1 = M1 c2  (128-bit products);  c <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0);  then k0 += W0, k1 += W1;
// ten rounds.  numpy.random.Philox(counter=[c0 - 1, c1, c2, c3], key=[k0, k1]).random_raw(4) gives the same four words (numpy increments
// the counter before its first block).  gfx950 has no 64-bit multiplier: the product is plain C++ (__umul64hi there, unsigned __int128
// on the host) and the compiler builds it from 32-bit multiplies.
//
// The addressing (include/gprx.h, gprx_pca_normals_dev): counter = (t >> 2, member, mode, event), key = (seed, stream); the draw of row t
// is word t & 3 of that block.
//
// Uniform: u = ((w >> 12) + 0.5) 2^-52 -- exact in fp64, symmetric about 1/2, inside [2^-53, 1 - 2^-53], so never 0 or 1; q = u - 0.5
// and 1 - u are exact too.  ~w gives 1 - u.
//
// Normal: Wichura's algorithm AS 241, PPND16 (Applied Statistics 37 (1988) 477-484), restated with contraction off: every operation is
// rounded once, the polynomials in Horner form from the highest coefficient down.  |q| <= 0.425: r = 0.180625 - q q, z = q A(r) / B(r);
// else r = sqrt(-px_log(min(u, 1 - u))), z = C(r - 1.6) / D(r - 1.6) for r <= 5, E(r - 5) / F(r - 5) beyond, negated for q < 0.  The
// central branch holds + - * / only; the tails go through px_log and sqrt.  z(~w) = -z(w) exactly.
#pragma once
#include <cstdint>

#include "px_math.h"

namespace gprx {

constexpr uint64_t PHILOX_M0 = 0xD2E7470EE14C6C93ull, PHILOX_M1 = 0xCA5A826395121157ull;
constexpr uint64_t PHILOX_W0 = 0x9E3779B97F4A7C15ull, PHILOX_W1 = 0xBB67AE8584CAA73Bull;

GPRX_HD uint64_t nrm_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * (unsigned __int128)b) >> 64);
#endif
}

// w[0..3]: the block of counter (c0, c1, c2, c3) under key (k0, k1)
GPRX_HD void philox4x64_10(uint64_t c0, uint64_t c1, uint64_t c2, uint64_t c3, uint64_t k0, uint64_t k1, uint64_t (&w)[4]) {
#pragma unroll
  for (int round = 0; round < 10; ++round) {
    const uint64_t hi0 = nrm_mulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
    const uint64_t hi1 = nrm_mulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += PHILOX_W0;
    k1 += PHILOX_W1;
  }
  w[0] = c0, w[1] = c1, w[2] = c2, w[3] = c3;
}

// the block that holds row t of (event, mode, member): the draw of row t is w[t & 3]
GPRX_HD void nrm_block(uint64_t seed, uint64_t stream, uint64_t event, uint64_t mode, uint64_t member, uint64_t t, uint64_t (&w)[4]) {
  philox4x64_10(t >> 2, member, mode, event, seed, stream, w);
}

GPRX_HD double nrm_uniform(uint64_t w) { return ((double)(w >> 12) + 0.5) * 0x1p-52; }

GPRX_HD double nrm_ppnd16(double u) {
#pragma clang fp contract(off)
  const double q = u - 0.5;
  if (__builtin_fabs(q) <= 0.425) {
    const double r = 0.180625 - q * q;
    double a = 2.5090809287301226727e3, b = 5.2264952788528545610e3;
    a = a * r + 3.3430575583588128105e4, b = b * r + 2.8729085735721942674e4;
    a = a * r + 6.7265770927008700853e4, b = b * r + 3.9307895800092710610e4;
    a = a * r + 4.5921953931549871457e4, b = b * r + 2.1213794301586595867e4;
    a = a * r + 1.3731693765509461125e4, b = b * r + 5.3941960214247511077e3;
    a = a * r + 1.9715909503065514427e3, b = b * r + 6.8718700749205790830e2;
    a = a * r + 1.3314166789178437745e2, b = b * r + 4.2313330701600911252e1;
    a = a * r + 3.3871328727963666080e0, b = b * r + 1.0;
    return q * a / b;
  }
  const double r = sqrt(-px_log(q < 0.0 ? u : 1.0 - u));
  double z;
  if (r <= 5.0) {
    const double x = r - 1.6;
    double c = 7.74545014278341407640e-4, d = 1.05075007164441684324e-9;
    c = c * x + 2.27238449892691845833e-2, d = d * x + 5.47593808499534494600e-4;
    c = c * x + 2.41780725177450611770e-1, d = d * x + 1.51986665636164571966e-2;
    c = c * x + 1.27045825245236838258e0, d = d * x + 1.48103976427480074590e-1;
    c = c * x + 3.64784832476320460504e0, d = d * x + 6.89767334985100004550e-1;
    c = c * x + 5.76949722146069140550e0, d = d * x + 1.67638483018380384940e0;
    c = c * x + 4.63033784615654529590e0, d = d * x + 2.05319162663775882187e0;
    c = c * x + 1.42343711074968357734e0, d = d * x + 1.0;
    z = c / d;
  } else {
    const double x = r - 5.0;
    double e = 2.01033439929228813265e-7, f = 2.04426310338993978564e-15;
    e = e * x + 2.71155556874348757815e-5, f = f * x + 1.42151175831644588870e-7;
    e = e * x + 1.24266094738807843860e-3, f = f * x + 1.84631831751005468180e-5;
    e = e * x + 2.65321895265761230930e-2, f = f * x + 7.86869131145613259100e-4;
    e = e * x + 2.96560571828504891230e-1, f = f * x + 1.48753612908506148525e-2;
    e = e * x + 1.78482653991729133580e0, f = f * x + 1.36929880922735805310e-1;
    e = e * x + 5.46378491116411436990e0, f = f * x + 5.99832206555887937690e-1;
    e = e * x + 6.65790464350110377720e0, f = f * x + 1.0;
    z = e / f;
  }
  return q < 0.0 ? -z : z;
}

GPRX_HD double nrm_normal(uint64_t w) { return nrm_ppnd16(nrm_uniform(w)); }

}  // namespace gprx
