// batch_rcp_harness.cpp -- the batched reciprocal of prost_amd/csrc/batch_rcp.hpp against the host's float division, without a GPU.
//
//   batch_rcp_harness LOG2_RANDOM_QUADRUPLES
// For quadruples of divisors d0..d3 in [2^-48, 2^63] and numerators n0..n3 it forms r0..r3 with rcp_refined4 (and with
// rcp_refined2 on (d0, d1) and (d2, d3)) and compares (float)fma((double)n_i, r_i, 0.0) with n_i / d_i in float, bit for bit.
// Build with -ffp-contract=off: the header counts roundings.  The seed of 1 / P is the host's own quotient 1.0 / P times
// (1 + s 2^-23), s = -1 and +1 for every case (and 0 for the directed ones): the worst seeds the device's v_rcp_f64 may return.
// Both forms run on every case.  Prints one line per class, "class cases mismatches", then the exact ties of a SUBNORMAL quotient
// (batch_rcp.hpp: outside the guarantee), which are kept out of the classes:
//   "tie_pow2 cases shared single"  the divisor is a power of two: the single reciprocal (device_math.hpp: rcp_refined) is exact
//                                   there and rounds the tie like the division -- `single` mismatches, must be 0 -- while the
//                                   shared ones do not always: `shared` mismatches, reported (`extremes` meets these cases:
//                                   normal numerators over 2^63)
//   "ties N"                        any other divisor: neither form is exact there; left out
// The first mismatches go to stderr.
//
// Classes:
//   random    exponents of the divisors uniform over the clamped range (2^63 itself included), numerators random finite bit patterns
//   extremes  every quadruple from {2^-48, next(2^-48), 2^63, prev(2^63), 1, 3, prev(2), 2^20 + 1} with numerators +-0, the
//             smallest and largest subnormal, the smallest normal, the largest float, 1, 3 and random ones
//   equal     all four divisors equal
//   ulp       four divisors one ulp apart
//   zero      numerators +0 and -0
//   subnormal quotients in the subnormal range and just below it (2^-152 .. 2^-126)
//   boundary  the numerators nearest to m d for random 25-bit midpoints m
//   worst     n, m, d with |n - m d| ONE unit of the product's last place (M D = +-1 mod 2^25): the closest a quotient of floats
//             comes to a rounding boundary, 2^-49 .. 2^-47 relative
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "batch_rcp.hpp"

namespace {

struct Seed {
  double f;       // 1 + s 2^-23
  double operator()(double p) const { return (1.0 / p) * f; }
};

uint32_t bits_of(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }
float float_of(uint32_t u) { float x; std::memcpy(&x, &u, 4); return x; }

struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 0x9E3779B97F4A7C15ull + 0x2545F4914F6CDD1Dull) {}
  uint64_t next() { s ^= s >> 12; s ^= s << 25; s ^= s >> 27; return s * 0x2545F4914F6CDD1Dull; }
  uint32_t u32() { return (uint32_t)(next() >> 32); }
  // a divisor in [2^-48, 2^63]: exponent uniform over -48 .. 63, 2^63 without a fraction
  float divisor() {
    const uint32_t r = u32();
    const int e = -48 + (int)(r % 112u);
    const uint32_t frac = e == 63 ? 0u : (u32() & 0x7FFFFFu);
    return float_of(((uint32_t)(e + 127) << 23) | frac);
  }
  float numerator() {      // any finite float, zeros and subnormals included
    uint32_t u = u32();
    if (((u >> 23) & 0xFFu) == 0xFFu) u &= ~(1u << 23);
    return float_of(u);
  }
};

enum Class { kRandom, kExtremes, kEqual, kUlp, kZero, kSub, kBoundary, kWorst, kClasses };
const char* const kNames[kClasses] = {"random", "extremes", "equal", "ulp", "zero", "subnormal", "boundary", "worst"};
struct Tally {      // one per thread
  uint64_t cases[kClasses] = {}, bad[kClasses] = {}, ties = 0, pow2 = 0, pow2_shared = 0, pow2_single = 0;
};
std::atomic<int> g_printed{0};

// the exact quotient is a rounding boundary (possible for subnormal quotients only)
bool exact_tie(float n, float d, float q) {
  const float up = std::nextafterf(q, INFINITY), dn = std::nextafterf(q, -INFINITY);
  const double m1 = 0.5 * ((double)q + (double)up), m2 = 0.5 * ((double)q + (double)dn);     // exact: neighbours differ in the last place
  return m1 * (double)d == (double)n || m2 * (double)d == (double)n;                          // <= 25 x 24 bits: exact products
}

void compare(Tally& t, Class c, const char* form, const float (&d)[4], int i, float n, double r, double seedf) {
  const float want = n / d[i];
  if (n != 0.0f && std::fabs(want) < 0x1p-126f && exact_tie(n, d[i], want)) {
    if ((bits_of(d[i]) & 0x7FFFFFu) != 0u) { t.ties++; return; }
    const double dd = (double)d[i], rs = prost_hip::rcp_newton2_from(dd, (1.0 / dd) * seedf);      // rcp_refined with this seed
    t.pow2++;
    t.pow2_shared += bits_of((float)__builtin_fma((double)n, r, 0.0)) != bits_of(want);
    t.pow2_single += bits_of((float)__builtin_fma((double)n, rs, 0.0)) != bits_of(want);
    return;
  }
  const float got = (float)__builtin_fma((double)n, r, 0.0);
  t.cases[c]++;
  // bit for bit; a zero numerator gives +0 whatever its sign (fma(+-0, r, +0.0) = +0: the value the kernels want), n / d keeps the sign
  const bool same = n == 0.0f ? bits_of(got) == 0u : bits_of(got) == bits_of(want);
  if (!same) {
    t.bad[c]++;
    if (g_printed++ < 20)
      std::fprintf(stderr, "%s %s seed %a: d = {%a, %a, %a, %a}, i = %d, n = %a: got %a, want %a\n", kNames[c], form, seedf, d[0], d[1], d[2], d[3], i, n, got, want);
  }
}

void check(Tally& t, Class c, const float (&d)[4], const float (&n)[4], bool exact_seed_too, bool pair_too) {
  static const double kSeeds[3] = {1.0 - 0x1p-23, 1.0 + 0x1p-23, 1.0};
  for (int s = 0; s < (exact_seed_too ? 3 : 2); s++) {
    const Seed seed{kSeeds[s]};
    double r[4];
    prost_hip::rcp_refined4(d[0], d[1], d[2], d[3], seed, r[0], r[1], r[2], r[3]);
    for (int i = 0; i < 4; i++) compare(t, c, "four", d, i, n[i], r[i], kSeeds[s]);
    if (pair_too) {
      prost_hip::rcp_refined2(d[0], d[1], seed, r[0], r[1]);
      prost_hip::rcp_refined2(d[2], d[3], seed, r[2], r[3]);
      for (int i = 0; i < 4; i++) compare(t, c, "pair", d, i, n[i], r[i], kSeeds[s]);
    }
  }
}

// the float neighbours below / above an exact double value v (v itself if it is a float)
void bracket(double v, float& lo, float& hi) {
  const float c = (float)v;
  if ((double)c == v) { lo = hi = c; return; }
  if ((double)c < v) { lo = c; hi = std::nextafterf(c, INFINITY); }
  else { hi = c; lo = std::nextafterf(c, -INFINITY); }
}

uint32_t inverse_mod_2_25(uint32_t d) {       // d odd
  uint32_t x = d;
  for (int k = 0; k < 5; k++) x *= 2u - d * x;
  return x & 0x1FFFFFFu;
}

void random_part(Tally& t, uint64_t count, unsigned tid) {
  Rng g(1000 + tid);
  for (uint64_t k = 0; k < count; k++) {
    float d[4], n[4];
    for (int i = 0; i < 4; i++) { d[i] = g.divisor(); n[i] = g.numerator(); }
    check(t, kRandom, d, n, false, true);
  }
}

void directed_part(Tally& t, unsigned tid, unsigned threads) {
  Rng g(77 + tid);
  // extremes
  const float dv[8] = {0x1p-48f, std::nextafterf(0x1p-48f, 1.0f), 0x1p63f, std::nextafterf(0x1p63f, 1.0f), 1.0f, 3.0f, std::nextafterf(2.0f, 1.0f), 0x1p20f + 1.0f};
  const float nfix[10] = {0.0f, -0.0f, 0x1p-149f, -0x1p-149f, float_of(0x007FFFFFu), 0x1p-126f, float_of(0x7F7FFFFFu), 1.0f, 3.0f, -float_of(0x7F7FFFFFu)};
  for (unsigned q = tid; q < 4096u; q += threads) {
    const float d[4] = {dv[q & 7u], dv[(q >> 3) & 7u], dv[(q >> 6) & 7u], dv[(q >> 9) & 7u]};
    for (int a = 0; a < 16; a++) {
      float n[4];
      for (int i = 0; i < 4; i++) n[i] = a < 10 ? nfix[(a + i) % 10] : g.numerator();
      check(t, kExtremes, d, n, true, true);
    }
  }
  const unsigned per = (1u << 16) / threads + 1u;
  for (unsigned k = 0; k < per; k++) {
    float d[4], n[4];
    // equal
    d[0] = d[1] = d[2] = d[3] = g.divisor();
    for (int i = 0; i < 4; i++) n[i] = g.numerator();
    check(t, kEqual, d, n, true, true);
    // one ulp apart (kept inside the clamped range)
    float b = g.divisor();
    if (b > 0x1p62f) b = 0x1p62f;
    for (int i = 0; i < 4; i++) { d[i] = b; b = std::nextafterf(b, INFINITY); n[i] = g.numerator(); }
    check(t, kUlp, d, n, true, true);
  }
  const unsigned per2 = (1u << 20) / threads + 1u;
  for (unsigned k = 0; k < per2; k++) {
    float d[4], n[4];
    for (int i = 0; i < 4; i++) { d[i] = g.divisor(); n[i] = (g.u32() & 1u) ? 0.0f : -0.0f; }
    check(t, kZero, d, n, true, true);
    // quotient = a random value of magnitude 2^-152 .. 2^-126: the numerator nearest to quotient * divisor, where that is a float
    for (int i = 0; i < 4; i++) {
      const int e = -152 + (int)(g.u32() % 26u);
      const double qv = std::ldexp(1.0 + (double)(g.u32() & 0x7FFFFFu) * 0x1p-23, e) * ((g.u32() & 1u) ? -1.0 : 1.0);
      n[i] = (float)(qv * (double)d[i]);
    }
    check(t, kSub, d, n, true, true);
  }
  const unsigned per3 = (1u << 21) / threads + 1u;
  for (unsigned k = 0; k < per3; k++) {
    float d[4], nlo[4], nhi[4];
    // boundary: m = M 2^e with an odd 25-bit M, e so that m is a midpoint of normal floats and m d stays finite
    for (int i = 0; i < 4; i++) {
      d[i] = g.divisor();
      const uint32_t M = (1u << 24) | (g.u32() & 0xFFFFFEu) | 1u;
      int dexp; (void)std::frexp(d[i], &dexp);                     // d = f 2^dexp, f in [0.5, 1)
      const int lo_e = -126 - 24, hi_e = 126 - 24 - (dexp > 0 ? dexp : 0);     // m >= 2^-126; m d < 2^127
      const int e = lo_e + (int)(g.u32() % (uint32_t)(hi_e - lo_e + 1));
      const double sgn = (g.u32() & 1u) ? -1.0 : 1.0;
      bracket(sgn * std::ldexp((double)M, e) * (double)d[i], nlo[i], nhi[i]);     // 25 x 24 bits: exact
    }
    check(t, kBoundary, d, nlo, false, true);
    check(t, kBoundary, d, nhi, false, true);
    // worst: M D = +-1 (mod 2^25) with M an odd 25-bit number
    float n[4];
    for (int i = 0; i < 4; i++) {
      uint32_t D, M;
      do {
        D = (1u << 23) | (g.u32() & 0x7FFFFEu) | 1u;
        M = inverse_mod_2_25(D);
        if (g.u32() & 1u) M = (1u << 25) - M;
      } while (M < (1u << 24));
      const int de = -48 - 23 + (int)(g.u32() % 111u);             // d = D 2^de in [2^-48, 2^63)
      d[i] = (float)std::ldexp((double)D, de);
      const int me = -40 - (de > 0 ? de : 0) + (int)(g.u32() % 60u);     // m = M 2^me >= 2^-16; m d < 2^24 2^25 2^20
      const double prod = std::ldexp((double)M, me) * (double)d[i];
      const double sp = (g.u32() & 1u) ? -prod : prod;
      float lo, hi;
      bracket(sp, lo, hi);
      n[i] = std::fabs((double)lo - sp) < std::fabs((double)hi - sp) ? lo : hi;
    }
    check(t, kWorst, d, n, false, true);
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s LOG2_RANDOM_QUADRUPLES\n", argv[0]); return 2; }
  const int lg = std::atoi(argv[1]);
  if (lg < 0 || lg > 34) return 2;
  const uint64_t total = 1ull << lg;
  unsigned threads = std::thread::hardware_concurrency();
  threads = threads < 1u ? 1u : threads > 8u ? 8u : threads;
  std::vector<Tally> tally(threads);
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < threads; t++) {
    const uint64_t a = total * t / threads, b = total * (t + 1) / threads;
    pool.emplace_back([=, &tally] { directed_part(tally[t], t, threads); random_part(tally[t], b - a, t); });
  }
  for (auto& th : pool) th.join();
  uint64_t bad = 0, ties = 0;
  for (int c = 0; c < kClasses; c++) {
    uint64_t n = 0, m = 0;
    for (const Tally& t : tally) { n += t.cases[c]; m += t.bad[c]; }
    std::printf("%s %llu %llu\n", kNames[c], (unsigned long long)n, (unsigned long long)m);
    bad += m;
  }
  uint64_t p2 = 0, p2s = 0, p21 = 0;
  for (const Tally& t : tally) { ties += t.ties; p2 += t.pow2; p2s += t.pow2_shared; p21 += t.pow2_single; }
  std::printf("tie_pow2 %llu %llu %llu\n", (unsigned long long)p2, (unsigned long long)p2s, (unsigned long long)p21);
  std::printf("ties %llu\n", (unsigned long long)ties);
  return bad == 0 ? 0 : 1;
}
