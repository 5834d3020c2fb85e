// epi_polyhedral_harness.cpp -- include/prost/prox/epi_polyhedral.hpp on the host, stand-alone (plain g++, no HIP), meant to be built
// with -fsanitize=address,undefined -ffp-contract=off.  The step loop of prost_amd/csrc/kernels_prox_epi_polyhedral.hip with a serial
// scan, for fp32 and fp64 and dim 2 .. 4, on random lists (m in {1, 2, 7, 25}, points of scale 1 and 1000) and on the degenerate
// lists (a duplicated constraint, parallel constraints, the pyramids y >= |x|_inf and y >= |x|_1 with points in the polar cone and
// points that land on an edge, rows with a = 0).
// The truth is a brute force of its own in long double: the equality-constrained projection for every subset of at most dim
// constraints (Gaussian elimination with pivoting), the closest feasible candidate wins.  A case is `within` when
//   |z - truth|_inf <= max(4 e_T, 32 eps_T) max(1, |z0|_inf, |b|_inf),
// e_T being the error of the same elimination run in T on the winning subset: what a straightforward evaluation in T makes of the
// answer once the active set is known.  Prints one line per case with the largest step count; exits 1 on a FAIL or when a group
// reached the step cap.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "prost/prox/epi_polyhedral.hpp"

namespace ep = prost::epi;

// projection of z0 onto the intersection of the hyperplanes <(a_i, -1), z> = b_i, i in sub; false when the normals are dependent
template <class F>
static bool solve_subset(int dim, const std::vector<int>& sub, const std::vector<long double>& a, const std::vector<long double>& b,
                         const std::vector<long double>& z0, std::vector<F>& z) {
  const int q = (int)sub.size(), d = dim - 1;
  std::vector<F> n(q * dim), g(q * q), rhs(q);
  for (int s = 0; s < q; s++) {
    for (int j = 0; j < d; j++) n[s * dim + j] = (F)a[sub[s] * d + j];
    n[s * dim + d] = (F)-1;
  }
  for (int s = 0; s < q; s++) {
    F r = -(F)b[sub[s]];
    for (int j = 0; j < dim; j++) r += n[s * dim + j] * (F)z0[j];
    rhs[s] = r;
    for (int t = 0; t < q; t++) {
      F v = 0;
      for (int j = 0; j < dim; j++) v += n[s * dim + j] * n[t * dim + j];
      g[s * q + t] = v;
    }
  }
  for (int c = 0; c < q; c++) {
    int p = c;
    for (int r = c + 1; r < q; r++) if (std::fabs(g[r * q + c]) > std::fabs(g[p * q + c])) p = r;
    if (!(std::fabs(g[p * q + c]) > (F)1e-9 * std::fabs(g[c * q + c] + (F)1))) return false;
    if (p != c) { for (int t = 0; t < q; t++) std::swap(g[p * q + t], g[c * q + t]); std::swap(rhs[p], rhs[c]); }
    for (int r = c + 1; r < q; r++) {
      const F f = g[r * q + c] / g[c * q + c];
      for (int t = c; t < q; t++) g[r * q + t] -= f * g[c * q + t];
      rhs[r] -= f * rhs[c];
    }
  }
  std::vector<F> lam(q);
  for (int c = q - 1; c >= 0; c--) {
    F v = rhs[c];
    for (int t = c + 1; t < q; t++) v -= g[c * q + t] * lam[t];
    lam[c] = v / g[c * q + c];
  }
  z.assign(dim, 0);
  for (int j = 0; j < dim; j++) {
    F v = (F)z0[j];
    for (int s = 0; s < q; s++) v -= lam[s] * n[s * dim + j];
    z[j] = v;
  }
  return true;
}

static void brute_force(int dim, int m, const std::vector<long double>& a, const std::vector<long double>& b, const std::vector<long double>& z0,
                        long double scale, std::vector<long double>& best, std::vector<int>& best_sub) {
  const int d = dim - 1;
  long double best_dist = std::numeric_limits<long double>::infinity();
  std::vector<int> sub;
  // subsets as bit masks would overflow nothing here (m <= 25), but only those of at most dim bits are visited
  for (int q = 0; q <= std::min(dim, m); q++) {
    std::vector<int> pick(q);
    for (int i = 0; i < q; i++) pick[i] = i;
    while (true) {
      std::vector<long double> z;
      if (solve_subset<long double>(dim, pick, a, b, z0, z)) {
        bool feasible = true;
        for (int i = 0; i < m && feasible; i++) {
          long double v = -z[d] - b[i], n1 = 1;
          for (int j = 0; j < d; j++) { v += a[i * d + j] * z[j]; n1 += std::fabs(a[i * d + j]); }
          feasible = v <= 1e-15L * scale * n1;
        }
        if (feasible) {
          long double dist = 0;
          for (int j = 0; j < dim; j++) dist += (z[j] - z0[j]) * (z[j] - z0[j]);
          if (dist < best_dist) { best_dist = dist; best = z; best_sub = pick; }
        }
      }
      int i = q - 1;
      while (i >= 0 && pick[i] == m - q + i) i--;
      if (i < 0) break;
      pick[i]++;
      for (int j = i + 1; j < q; j++) pick[j] = pick[j - 1] + 1;
    }
  }
  if (best.empty()) { std::printf("brute force found no feasible candidate\n"); std::exit(1); }
}

struct Tally { int cases = 0, fails = 0, capped = 0, max_steps = 0; double worst = 0; };

// the step loop of the kernel with a serial scan; returns the steps, -1 when the cap was reached
template <class T, int DIM>
static int project(const T (&z0)[DIM], int k, const T* a, const T* b, T (&out)[DIM]) {
  constexpr int D = DIM - 1;
  ep::ActiveSet<T, DIM> st;
  st.Init(z0);
  const int cap = ep::StepCap(k, DIM);
  bool capped = false;
  while (true) {
    if (!st.pending) {
      int bi = -1;
      T bv = -std::numeric_limits<T>::infinity();
      for (int i = 0; i < k; i++) {
        T v;
        if (ep::Violation<T, DIM>(st.z, a + (size_t)i * D, b[i], v) && v > bv) { bv = v; bi = i; }
      }
      if (bi < 0) { if (st.polished || !st.Polish()) break; continue; }
      st.Begin(a + (size_t)bi * D, b[bi]);
    }
    if (st.steps >= cap || st.Step() == ep::kStuck) { capped = true; break; }
  }
  if (capped) {
    T worst = -std::numeric_limits<T>::infinity();
    for (int i = 0; i < k; i++) {
      T s = -b[i];
      for (int j = 0; j < D; j++) s += a[(size_t)i * D + j] * z0[j];
      worst = std::max(worst, s);
    }
    ep::Fallback<T, DIM>(z0, worst, out);
    return -1;
  }
  for (int j = 0; j < DIM; j++) out[j] = st.z[j];
  return st.steps;
}

template <class T, int DIM>
static void run_case(const char* name, const std::vector<double>& a_in, const std::vector<double>& b_in, const std::vector<double>& pts, Tally& total) {
  constexpr int D = DIM - 1;
  const int m = (int)b_in.size(), P = (int)(pts.size() / DIM);
  // the inputs are values of T: truth and code under test see the same numbers
  std::vector<T> a(a_in.size()), b(m);
  std::vector<long double> al(a_in.size()), bl(m);
  for (size_t i = 0; i < a_in.size(); i++) { a[i] = (T)a_in[i]; al[i] = a[i]; }
  for (int i = 0; i < m; i++) { b[i] = (T)b_in[i]; bl[i] = b[i]; }
  Tally t;
  for (int p = 0; p < P; p++) {
    T z0[DIM], z[DIM];
    std::vector<long double> z0l(DIM);
    long double scale = 1;
    for (int j = 0; j < DIM; j++) { z0[j] = (T)pts[(size_t)p * DIM + j]; z0l[j] = z0[j]; scale = std::max(scale, std::fabs(z0l[j])); }
    for (int i = 0; i < m; i++) scale = std::max(scale, std::fabs(bl[i]));
    const int steps = project<T, DIM>(z0, m, a.data(), b.data(), z);
    if (steps < 0) { t.capped++; continue; }
    t.max_steps = std::max(t.max_steps, steps);
    std::vector<long double> truth;
    std::vector<int> sub;
    brute_force(DIM, m, al, bl, z0l, scale, truth, sub);
    std::vector<T> zt;
    solve_subset<T>(DIM, sub, al, bl, z0l, zt);
    long double e_t = 0, err = 0;
    for (int j = 0; j < DIM; j++) {
      e_t = std::max(e_t, std::fabs((long double)zt[j] - truth[j]));
      err = std::max(err, std::fabs((long double)z[j] - truth[j]));
    }
    const long double bound = std::max(4 * e_t, 32 * (long double)std::numeric_limits<T>::epsilon() * scale);
    t.worst = std::max(t.worst, (double)(err / bound));
    if (!(err <= bound)) t.fails++;
    // a feasible input has to come back bit for bit
    bool inside = true;
    for (int i = 0; i < m && inside; i++) {
      long double v = -z0l[D] - bl[i];
      for (int j = 0; j < D; j++) v += al[(size_t)i * D + j] * z0l[j];
      inside = v <= 0;
    }
    if (inside) for (int j = 0; j < DIM; j++) if (z[j] != z0[j]) { t.fails++; break; }
  }
  std::printf("%s %s dim=%d m=%d: %d points, at most %d steps, error / bound %.3f, %s\n", name, sizeof(T) == 4 ? "fp32" : "fp64", DIM, m, P, t.max_steps,
              t.worst, (t.fails || t.capped) ? "FAIL" : "within");
  total.cases++; total.fails += t.fails; total.capped += t.capped; total.max_steps = std::max(total.max_steps, t.max_steps);
}

template <class T, int DIM>
static void run_all(Tally& total) {
  constexpr int D = DIM - 1;
  std::mt19937_64 gen(12345 + DIM);
  std::normal_distribution<double> nrm(0.0, 1.0);
  std::uniform_real_distribution<double> uni(-0.9, 0.9);
  auto points = [&](int n, double scale) { std::vector<double> p((size_t)n * DIM); for (auto& v : p) v = scale * nrm(gen); return p; };
  for (int m : {1, 2, 7, 25}) {
    if (DIM == 4 && m == 25) m = 12;                       // the enumeration at dim 4
    for (double scale : {1.0, 1000.0}) {
      std::vector<double> a((size_t)m * D), b(m);
      for (auto& v : a) v = nrm(gen);
      for (auto& v : b) v = nrm(gen);
      run_case<T, DIM>(scale == 1.0 ? "random" : "random1000", a, b, points(20, scale), total);
    }
  }
  std::vector<double> pts = points(6, 1.0), far = points(6, 1000.0);
  pts.insert(pts.end(), far.begin(), far.end());
  {  // a duplicated constraint: rows 0 = 1, 2 = 3
    std::vector<double> a((size_t)4 * D), b(4);
    for (int i = 0; i < 4; i += 2) { for (int j = 0; j < D; j++) a[(size_t)i * D + j] = a[(size_t)(i + 1) * D + j] = nrm(gen); b[i] = b[i + 1] = nrm(gen); }
    run_case<T, DIM>("duplicate", a, b, pts, total);
  }
  {  // parallel: the same normal with two offsets, and twice the normal
    std::vector<double> a((size_t)3 * D), b = {0.5, -0.5, 0.1};
    for (int j = 0; j < D; j++) { a[j] = nrm(gen); a[D + j] = a[j]; a[2 * D + j] = 2 * a[j]; }
    run_case<T, DIM>("parallel", a, b, pts, total);
  }
  // the pyramids; points in the polar cone (|x|_1 <= 0.9 |y|, y <= -1: the apex is the answer), points above an edge, random points
  std::vector<double> pyr;
  for (int p = 0; p < 8; p++) {
    const double depth = 1 + 25 * (uni(gen) + 1);
    for (int j = 0; j < D; j++) pyr.push_back(uni(gen) * depth / D);
    pyr.push_back(-depth);
  }
  for (double tv : {2.0, 5.0, -3.0, 40.0}) { pyr.push_back(tv); for (int j = 1; j < D; j++) pyr.push_back(0.0); pyr.push_back(tv > 4 ? -30.0 : 0.5); }
  pyr.insert(pyr.end(), pts.begin(), pts.end());
  {
    std::vector<double> a((size_t)2 * D * D, 0.0), b(2 * D, 0.0);
    for (int j = 0; j < D; j++) { a[(size_t)j * D + j] = 1; a[(size_t)(D + j) * D + j] = -1; }
    run_case<T, DIM>("linf_pyramid", a, b, pyr, total);
  }
  {
    const int m = 1 << D;
    std::vector<double> a((size_t)m * D), b(m, 0.0);
    for (int i = 0; i < m; i++) for (int j = 0; j < D; j++) a[(size_t)i * D + j] = ((i >> j) & 1) ? 1 : -1;
    run_case<T, DIM>("l1_pyramid", a, b, pyr, total);
  }
  {  // a = 0: y >= -b
    std::vector<double> a((size_t)3 * D, 0.0), b = {0.5, -2.0, 1.0};
    run_case<T, DIM>("zero_rows", a, b, pts, total);
  }
  {  // no constraints: the identity
    T z0[DIM], z[DIM];
    for (int j = 0; j < DIM; j++) z0[j] = (T)(j + 0.5);
    const int steps = project<T, DIM>(z0, 0, nullptr, nullptr, z);
    bool same = steps == 0;
    for (int j = 0; j < DIM; j++) same = same && z[j] == z0[j];
    std::printf("empty %s dim=%d: %s\n", sizeof(T) == 4 ? "fp32" : "fp64", DIM, same ? "within" : "FAIL");
    total.cases++; total.fails += same ? 0 : 1;
  }
}

int main(int argc, char** argv) {
  // the caps the library reports have to be the header's: the harness and the plan cannot drift apart unnoticed
  if (argc == 3 && (std::atoi(argv[1]) != ep::kStepCapA || std::atoi(argv[2]) != ep::kStepCapB)) {
    std::printf("step cap %d, %d expected, the header has %d, %d\n", std::atoi(argv[1]), std::atoi(argv[2]), ep::kStepCapA, ep::kStepCapB);
    return 1;
  }
  Tally total;
  run_all<float, 2>(total); run_all<float, 3>(total); run_all<float, 4>(total);
  run_all<double, 2>(total); run_all<double, 3>(total); run_all<double, 4>(total);
  std::printf("cases %d, at most %d steps, reached the cap %d, failures %d\n", total.cases, total.max_steps, total.capped, total.fails);
  if (total.fails || total.capped) return 1;
  std::printf("ok\n");
  return 0;
}
