// batch_rcp.hpp -- the refined double reciprocals of four (or two) float divisors from ONE reciprocal seed.
//
// Plain C++ (host and device): the fused kernels read it through device_math.hpp (norm2_leq0_fast), and
// tests/host/batch_rcp_harness.cpp runs the same code on the CPU with seeds of its own choosing.
//
// What it is for.  device_math.hpp divides by a float d through r = 1/(double)d refined to ~2^-53 and
// q = (float)fma((double)n, r, +0.0).  The seed of r (v_rcp_f64) is the dearest instruction of the dual stage, and a lane
// owns four pixels, i.e. four divisors.  Montgomery's batch inversion forms the four reciprocals from one seed:
//     ab = a b,  cd = c d,  P = ab cd,  r = refined 1/P,
//     1/a = (r cd) b,  1/b = (r cd) a,  1/c = (r ab) d,  1/d = (r ab) c.
// Per four divisors: 9 products, 1 seed, 4 fma  instead of  4 seeds, 16 fma.  The pair form (P = a b, 1/a = r b, 1/b = r a) takes
// 3 products, 1 seed, 4 fma per two divisors and needs fewer registers; it is the one the kernels use (device_math.hpp).
//
// Error of r_i against 1/d_i (u = 2^-53, every operation rounds to nearest, nothing over- or underflows -- see "Range"):
//   * ab and cd are exact: two 24-bit significands give at most 48 bits.
//   * P = RN(ab cd) = ab cd (1 + e1), |e1| <= u.
//   * Newton.  With y = (1 + t) / P:  e = RN(1 - P y) = -t (1 + h), |h| <= u (one rounding: fma), and
//     y' = RN(y + y e) = (1 - t^2 - t h (1 + t)) (1 + k) / P, |k| <= u.  A seed with |t0| <= 2^-21 (v_rcp_f64 is good to about
//     2^-23; the CPU harness perturbs an exact seed by +-2^-23 on top of its own rounding) gives |t1| <= 2^-42 + 2^-52.9, then
//     |t2| <= u + 2^-83.  So r = (1 + e2) / P with |e2| <= u (1 + 2^-30).
//   * r cd (or r ab) rounds once (e3), the product with the partner divisor once more (e4), |e3|, |e4| <= u.
//   r_i = (1 + e2)(1 + e3)(1 + e4) / ((1 + e1) d_i):   |r_i d_i - 1| <= 4 u (1 + 2^-29) < 2^-50.99.
//   The pair form has no e1 (P = a b is exact) and no e3:  |r_i d_i - 1| <= 2 u (1 + 2^-29) < 2^-51.99.
// The quotient (float)fma((double)n, r_i, +0.0) rounds the product once more in double: its total relative error is below
// 5 u (1 + 2^-28) = 2^-50.67 for four divisors, 2^-51.41 for two (the single reciprocal of device_math.hpp: 2 u = 2^-52).
//
// Why that suffices.  Let q = n / d for floats n, d, and let m be a rounding boundary of the float format next to q: the midpoint
// of two neighbouring floats.  For a normal quotient, m = M 2^em with an odd M < 2^25, n = N 2^en, d = D 2^ed with N, D < 2^24;
// n = m d is impossible (M D would need 25 significant bits at least, N has 24), and n - m d is a non-zero multiple of
// 2^(em+ed), the last place of the product, while |m d| < 2^49 2^(em+ed).  So |q - m| > 2^-49 |m|, and a double within
// 2^-50.67 of q (relative) lies on the same side of every boundary as q: it rounds to RN(n / d).  A quotient that is itself a
// float is at least half a float ulp (2^-25 relative) from every boundary.  Subnormal quotients have boundaries m = M 2^-150 with
// fewer bits in M, and the same argument gives a wider gap -- EXCEPT that n = m d then has solutions (n = 2^-149, d = 2: the
// quotient 2^-150 is exactly a tie).  No reciprocal method rounds an exact tie reliably unless r_i is exactly 1 / d_i.  The single
// reciprocal of device_math.hpp is exact for a power of two and so rounds those ties like the division; this one in general is
// not, and rounds about one in eight of them the other way (the CPU harness counts them and leaves them out).  Such a tie needs
// a quotient below 2^-126 in magnitude whose numerator's significand is a multiple of the divisor's: with the prox of
// norm2_leq0_fast, a gradient component more than 2^100 times smaller than its pixel's norm.  They are outside the guarantee
// here.  Signed zeros: +-0 times r_i plus +0.0 is +0.
//
// Range.  Callers clamp the divisors to [2^-48, 2^63] (norm2_leq0_fast: norms of the mid path), so ab, cd lie in [2^-96, 2^126],
// P in [2^-192, 2^252], r in [2^-252, 2^192], r cd and r ab in [2^-126, 2^96]: all normal doubles, no scaling needed.  Divisors
// must be positive finite floats in that range; zeros, infinities and NaNs are the callers' business.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PH_BATCH_RCP_HD __host__ __device__
#else
#define PH_BATCH_RCP_HD
#endif

namespace prost_hip {

// two Newton steps on a reciprocal seed y of p (seed: |p y - 1| <= 2^-21)
PH_BATCH_RCP_HD inline double rcp_newton2_from(double p, double y) {
  double e = __builtin_fma(-p, y, 1.0);
  y = __builtin_fma(y, e, y);
  e = __builtin_fma(-p, y, 1.0);
  y = __builtin_fma(y, e, y);
  return y;
}

// r[i] ~ 1 / d[i] for four divisors; seed(p) returns an estimate of 1 / p for a double p (the device passes v_rcp_f64)
template <class Seed>
PH_BATCH_RCP_HD inline void rcp_refined4(float d0, float d1, float d2, float d3, Seed seed, double& r0, double& r1, double& r2, double& r3) {
  const double a = (double)d0, b = (double)d1, c = (double)d2, d = (double)d3;
  const double ab = a * b, cd = c * d;
  const double p = ab * cd;
  const double r = rcp_newton2_from(p, seed(p));
  const double rab = r * cd, rcd = r * ab;        // 1 / (a b), 1 / (c d)
  r0 = rab * b; r1 = rab * a;
  r2 = rcd * d; r3 = rcd * c;
}

// the same for two divisors
template <class Seed>
PH_BATCH_RCP_HD inline void rcp_refined2(float d0, float d1, Seed seed, double& r0, double& r1) {
  const double a = (double)d0, b = (double)d1;
  const double p = a * b;
  const double r = rcp_newton2_from(p, seed(p));
  r0 = r * b; r1 = r * a;
}

}  // namespace prost_hip
