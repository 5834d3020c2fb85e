// epi_conjquad_harness.cpp -- include/prost/prox/epi_conjquad.hpp on the host, stand-alone (plain g++, no HIP), meant to be built with
// -fsanitize=address,undefined -ffp-contract=off.  Usage: epi_conjquad_harness <step cap>; the cap has to be the header's own (the
// test passes what prost_hip_epi_conjquad_step_cap answers, so the two cannot drift apart unnoticed).
//
// Cases are built from their answers in long double: a boundary point P of phi* on the chosen piece, z0 = P + s n along the outward
// unit normal n (vertex: any direction of the normal cone; inside: z0 = P at or above the boundary), so the projection of z0 is P and
// no solver is involved in the truth.  Coefficients are values a float holds; z0 is rounded to T once.  Every case has to be within
//   max(4 e_T, 32 eps_T) max(1, |z0|_inf)
// of P, e_T being the relative error of the piece's own closed form evaluated in T at the true answer (the halfspace projection of
// the rounded z0 for a ray, t = q (y - b)^2 - c at the rounded y for the arc, 0 for the vertex and inside).  No case may reach the
// cap.  Prints one line per (case family, T) that ends in `within`, the largest step count, and `ok`.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "prost/prox/epi_conjquad.hpp"

namespace ecq = prost::epi_conjquad;
typedef long double L;

struct Case {
  int region;
  float a, b, c, alpha, beta;      // +-infinity allowed for alpha / beta
  L z0[2], P[2];
};

static const L kInf = std::numeric_limits<L>::infinity();

// the case whose answer is P: x = the slope on the arc / the direction at the vertex, d = distance in y from the contact point along
// a ray (inside: offset of y from b, either sign), s = distance along the outward normal (inside: height above the boundary)
static Case build(int region, float a, float b, float c, float alpha, float beta, L x, L d, L s) {
  Case k;
  k.region = region; k.a = a; k.b = b; k.c = c; k.alpha = alpha; k.beta = beta;
  const L la = a, lb = b, lc = c;
  const bool hl = (L)alpha > -kInf, hr = (L)beta < kInf;
  const L al = hl ? (L)alpha : 0, be = hr ? (L)beta : 0;
  const L ya = hl ? 2 * la * al + lb : -kInf, yb = hr ? 2 * la * be + lb : kInf;
  const L fa = (la * al + lb) * al + lc, fb = (la * be + lb) * be + lc;
  L slope = 0, py = 0, pt = 0;
  if (region == ecq::kLeft) { slope = al; py = ya - d; pt = al * py - fa; }
  else if (region == ecq::kRight) { slope = be; py = yb + d; pt = be * py - fb; }
  else if (region == ecq::kVertex) { slope = x; py = lb; pt = -lc; }
  else if (region == ecq::kArc) { slope = x; py = 2 * la * x + lb; pt = la * x * x - lc; }
  else {
    py = lb + d;
    if (py <= ya) pt = al * py - fa;
    else if (py >= yb) pt = be * py - fb;
    else pt = (py - lb) * (py - lb) / (4 * la) - lc;
    pt += s;
  }
  const L norm = std::sqrt(slope * slope + 1), move = region == ecq::kInside ? 0 : s;
  k.P[0] = py; k.P[1] = pt;
  k.z0[0] = py + move * slope / norm; k.z0[1] = pt - move / norm;
  return k;
}

static std::vector<Case> family(const char* name, L S, std::mt19937_64& rng) {
  std::vector<Case> v;
  std::uniform_real_distribution<double> U(0.0, 1.0);
  std::normal_distribution<double> N(0.0, 1.0);
  const float A4[4] = {0.0f, 1e-6f, 1.0f, 1e3f};
  const float inf = std::numeric_limits<float>::infinity();
  if (!std::strcmp(name, "random")) {
    for (int i = 0; i < 4000; i++) {
      const int region = i % 5;
      float a = A4[(i / 5) % 4];
      if (region == ecq::kVertex) a = 0;
      if (region == ecq::kArc && a == 0) a = 1;
      float lo = (float)(2 * N(rng)), hi = (float)(2 * N(rng));
      if (hi < lo) std::swap(lo, hi);
      if (!(hi > lo)) hi = lo + 0.5f;
      if (region != ecq::kVertex && region != ecq::kArc && U(rng) < 0.1) hi = lo;
      float alpha = lo, beta = hi;
      L x = (L)lo + ((L)hi - (L)lo) * U(rng);
      if (a > 0 && region != ecq::kLeft && U(rng) < 0.15) { alpha = -inf; if (region == ecq::kArc && U(rng) < 0.5) x = (L)lo - 3 * U(rng); }
      if (a > 0 && region != ecq::kRight && U(rng) < 0.15) { beta = inf; if (region == ecq::kArc && U(rng) < 0.5) x = (L)hi + 3 * U(rng); }
      const L d = S * U(rng) * (region == ecq::kInside ? (U(rng) < 0.5 ? -3 : 3) : 1);
      v.push_back(build(region, a, (float)(S * N(rng)), (float)(S * N(rng)), alpha, beta, x, d, 2 * S * U(rng)));
    }
  } else if (!std::strcmp(name, "alpha_eq_beta")) {
    for (int i = 0; i < 4; i++) {
      v.push_back(build(ecq::kLeft, A4[i], 0.5f * (float)S, -0.25f * (float)S, 0.75f, 0.75f, 0, S, 2 * S));
      v.push_back(build(ecq::kRight, A4[i], 0.5f * (float)S, -0.25f * (float)S, 0.75f, 0.75f, 0, S, 2 * S));
      v.push_back(build(ecq::kLeft, A4[i], 0.5f * (float)S, -0.25f * (float)S, 0.75f, 0.75f, 0, 0, S));
      v.push_back(build(ecq::kInside, A4[i], 0.5f * (float)S, -0.25f * (float)S, 0.75f, 0.75f, 0, -S, S));
    }
  } else if (!std::strcmp(name, "infinite")) {
    for (int i = 1; i < 4; i++) {
      const L xs[3] = {-4, 0.5, 7};
      for (L x : xs) v.push_back(build(ecq::kArc, A4[i], 0.5f * (float)S, 0.25f * (float)S, -inf, inf, x, 0, 1.5 * S));
      v.push_back(build(ecq::kArc, A4[i], -(float)S, (float)S, -inf, 1.5f, -6, 0, S));
      v.push_back(build(ecq::kRight, A4[i], -(float)S, (float)S, -inf, 1.5f, 0, S, S));
      v.push_back(build(ecq::kArc, A4[i], (float)S, -(float)S, -0.5f, inf, 5, 0, S));
      v.push_back(build(ecq::kLeft, A4[i], (float)S, -(float)S, -0.5f, inf, 0, S, S));
      v.push_back(build(ecq::kInside, A4[i], (float)S, -(float)S, -0.5f, inf, 0, S, S));
    }
  } else if (!std::strcmp(name, "below_the_apex")) {
    for (int i = 1; i < 4; i++) {
      v.push_back(build(ecq::kArc, A4[i], 0.5f * (float)S, 0.25f * (float)S, -1, 2, 0, 0, S));
      v.push_back(build(ecq::kArc, A4[i], 0.5f * (float)S, 0.25f * (float)S, -1, 2, 0, 0, 1e-3L * S));
    }
  } else if (!std::strcmp(name, "on_the_boundary")) {
    for (int i = 0; i < 4; i++) {
      v.push_back(build(ecq::kLeft, A4[i], 0.5f * (float)S, -0.5f * (float)S, -1, 2, 0, S, 0));
      v.push_back(build(ecq::kRight, A4[i], 0.5f * (float)S, -0.5f * (float)S, -1, 2, 0, S, 0));
      v.push_back(build(ecq::kLeft, A4[i], 0.5f * (float)S, -0.5f * (float)S, -1, 2, 0, 0, 0));
      v.push_back(build(ecq::kRight, A4[i], 0.5f * (float)S, -0.5f * (float)S, -1, 2, 0, 0, 0));
      if (A4[i] > 0) v.push_back(build(ecq::kArc, A4[i], 0.5f * (float)S, -0.5f * (float)S, -1, 2, 0.5, 0, 0));
    }
  } else if (!std::strcmp(name, "normal_through_contact")) {
    for (int i = 0; i < 4; i++) {
      v.push_back(build(ecq::kLeft, A4[i], -0.5f * (float)S, 0.5f * (float)S, -1.5f, 0.75f, 0, 0, S));
      v.push_back(build(ecq::kRight, A4[i], -0.5f * (float)S, 0.5f * (float)S, -1.5f, 0.75f, 0, 0, 3 * S));
    }
  } else if (!std::strcmp(name, "vertex_cone")) {
    const L xs[5] = {-1, -0.5, 0, 1, 2};
    for (L x : xs) v.push_back(build(ecq::kVertex, 0, 0.5f * (float)S, 0.25f * (float)S, -1, 2, x, 0, S));
  } else if (!std::strcmp(name, "high_on_the_other_side")) {
    v.push_back(build(ecq::kRight, 1, 0, 0, -2, 3, 0, 94 * S, 28.77L * S));
    v.push_back(build(ecq::kLeft, 1, 0, 0, -2, 3, 0, 96 * S, 93 * S));
    v.push_back(build(ecq::kRight, 0, 0, 0, -2, 3, 0, 100 * S, 30 * S));
    v.push_back(build(ecq::kLeft, 0, 0, 0, -2, 3, 0, 100 * S, 90 * S));
  }
  return v;
}

template <class T>
static L closed_form_error(const Case& k, T y0, T t0) {
  // the piece's own closed form in T at the true answer, against P
  T y = (T)k.P[0], t = (T)k.P[1];
  if (k.region == ecq::kLeft || k.region == ecq::kRight) {
    const T m = k.region == ecq::kLeft ? (T)k.alpha : (T)k.beta;
    const T f = ((T)k.a * m + (T)k.b) * m + (T)k.c;
    const T viol = (m * y0 - t0) - f;
    const T step = viol / (m * m + (T)1);
    y = y0 - step * m; t = t0 + step;
  } else if (k.region == ecq::kArc) {
    const T u = y - (T)k.b;
    t = ((T)1 / ((T)4 * (T)k.a)) * (u * u) - (T)k.c;
  }
  return std::fmax(std::fabs((L)y - k.P[0]), std::fabs((L)t - k.P[1]));
}

struct Tally { int cases = 0, capped = 0, failures = 0, most_steps = 0; };

template <class T>
static void run(const char* name, L S, const char* tname, int cap, Tally& tally) {
  std::mt19937_64 rng(12345);
  const std::vector<Case> cases = family(name, S, rng);
  const L eps = std::numeric_limits<T>::epsilon();
  L worst = 0;
  int steps_max = 0, bad = 0, capped_n = 0, seen[5] = {0, 0, 0, 0, 0};
  for (const Case& k : cases) {
    ecq::Piece<T> p;
    p.Set((T)k.a, (T)k.b, (T)k.c, (T)k.alpha, (T)k.beta);
    const T y0 = (T)k.z0[0], t0 = (T)k.z0[1];
    T y, t;
    int steps = 0;
    bool capped = false;
    const int region = ecq::Project<T>(p, y0, t0, cap, y, t, steps, capped);
    seen[region]++;
    const L scale = std::fmax((L)1, std::fmax(std::fabs((L)y0), std::fabs((L)t0)));
    const L e_t = closed_form_error<T>(k, y0, t0) / scale;
    const L bound = std::fmax(4 * e_t, 32 * eps) * scale;
    const L err = std::fmax(std::fabs((L)y - k.P[0]), std::fabs((L)t - k.P[1]));
    if (!(err <= bound)) {
      if (bad++ < 5)
        std::printf("FAIL %s %s: designed %d found %d a=%g b=%g c=%g alpha=%g beta=%g z0=(%.12Lg, %.12Lg) P=(%.12Lg, %.12Lg) got (%.12Lg, %.12Lg) err %.3Lg bound %.3Lg\n",
                    name, tname, k.region, region, (double)k.a, (double)k.b, (double)k.c, (double)k.alpha, (double)k.beta, k.z0[0], k.z0[1], k.P[0], k.P[1], (L)y, (L)t, err, bound);
    }
    if (capped) capped_n++;
    worst = std::fmax(worst, err / bound);
    steps_max = steps > steps_max ? steps : steps_max;
  }
  std::printf("%s scale=%Lg %s: %zu cases, regions %d/%d/%d/%d/%d, worst error / bound %.3Lf, most steps %d, capped %d: %s\n", name, S, tname, cases.size(),
              seen[0], seen[1], seen[2], seen[3], seen[4], worst, steps_max, capped_n, bad == 0 && capped_n == 0 ? "within" : "OUTSIDE");
  tally.cases += (int)cases.size(); tally.capped += capped_n; tally.failures += bad;
  tally.most_steps = steps_max > tally.most_steps ? steps_max : tally.most_steps;
}

int main(int argc, char** argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: %s <step cap>\n", argv[0]); return 2; }
  const int cap = std::atoi(argv[1]);
  if (cap != ecq::kStepCap) { std::fprintf(stderr, "the header's step cap is %d, not %d\n", ecq::kStepCap, cap); return 1; }
  const char* names[] = {"random", "alpha_eq_beta", "infinite", "below_the_apex", "on_the_boundary", "normal_through_contact", "vertex_cone", "high_on_the_other_side"};
  Tally tally;
  for (const char* name : names)
    for (L S : {(L)1, (L)1000}) {
      run<float>(name, S, "fp32", cap, tally);
      run<double>(name, S, "fp64", cap, tally);
    }
  // the cap itself: with no step allowed an arc point comes back as the feasible point straight above z0
  {
    ecq::Piece<double> p;
    p.Set(1.0, 0.0, 0.0, -std::numeric_limits<double>::infinity(), std::numeric_limits<double>::infinity());
    double y, t;
    int steps;
    bool capped;
    const int region = ecq::Project<double>(p, 3.0, -1.0, 0, y, t, steps, capped);
    const bool good = region == ecq::kArc && capped && y == 3.0 && t == 2.25 && steps == 0;
    std::printf("cap 0: %s\n", good ? "within" : "OUTSIDE");
    if (!good) tally.failures++;
  }
  std::printf("%d cases, most steps %d of %d, reached the cap %d, failures %d\n", tally.cases, tally.most_steps, cap, tally.capped, tally.failures);
  if (tally.failures || tally.capped) { std::printf("FAILED\n"); return 1; }
  std::printf("ok\n");
  return 0;
}
