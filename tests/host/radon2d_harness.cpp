// radon2d_harness.cpp -- include/prost/linop/radon2d.hpp on the host, as a stand-alone program (plain g++, no HIP): the per-angle
// table, the forward enumeration, the gather enumeration with its candidate window, the two marches the kernels call in every lane, and
// the sums of the host block.  Built with -fsanitize=address,undefined by tests/test_radon2d_host.py; every buffer has exactly its size.
//
//   * table values at theta = 0, pi / 4, pi / 2, pi;
//   * at the small shapes the gather enumeration and the forward enumeration give the same entry set with the same bits, and the
//     marches (plain and accumulating) on unit vectors reproduce the entries and their transpose bit for bit;
//   * on random vectors the marches stay within 1.01 (t + 1) u (|K| |x|) of the entry list summed in long double;
//   * the sums equal a brute-force sum over the entry list, empty rows and columns exactly 0;
//   * for 10^6 sampled entries at 8192 x 8192 in fp32, at spacing 0.5, 1 and 8, no entry is outside the candidate window.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "prost/linop/radon2d.hpp"

namespace r2d = prost::radon2d;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static const double kPi = 3.14159265358979323846;

template <class T> static bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

template <class T> struct Entries {
  std::map<std::pair<long, long>, T> at;      // (row, column) -> value
};

template <class T>
static Entries<T> forward_entries(const std::vector<T>& table, const r2d::Geometry& g) {
  Entries<T> e;
  for (int a = 0; a < g.na; a++)
    for (int d = 0; d < g.ndet; d++)
      r2d::ForEachInRay<T>(table.data(), g, a, d, [&](int t, int i, T v) {
        int y, x;
        r2d::PixelOf<T>(table.data(), a, t, i, y, x);
        const std::pair<long, long> key((long)a * g.ndet + d, (long)y + (long)x * g.ny);
        CHECK(e.at.find(key) == e.at.end(), "forward enumeration names entry (%ld, %ld) twice", key.first, key.second);
        e.at[key] = v;
      });
  return e;
}

template <class T>
static int small_shape(const char* name, int ny, int nx, int planes, int ndet, double spacing, double shift, const std::vector<double>& angles, double& worst) {
  const r2d::Geometry g = r2d::MakeGeometry(ny, nx, planes, ndet, (long)angles.size(), spacing, false);
  const std::vector<T> table = r2d::MakeTable<T>(ny, nx, ndet, spacing, shift, angles);
  const Entries<T> fwd = forward_entries<T>(table, g);
  // the gather enumeration: the same set, the same bits, rows ascending inside a pixel
  size_t seen = 0;
  for (int x = 0; x < nx; x++)
    for (int y = 0; y < ny; y++) {
      long last = -1;
      r2d::ForEachAtPixel<T>(table.data(), g, y, x, [&](int a, int d, T v) {
        const long row = (long)a * ndet + d;
        CHECK(row > last, "%s: pixel (%d, %d) visits row %ld after %ld", name, y, x, row, last);
        last = row;
        auto it = fwd.at.find(std::make_pair(row, (long)y + (long)x * ny));
        CHECK(it != fwd.at.end(), "%s: the gather names entry (%ld; %d, %d) the forward does not have", name, row, y, x);
        if (it != fwd.at.end()) CHECK(same_bits(it->second, v), "%s: entry (%ld; %d, %d) differs in its bits", name, row, y, x);
        seen++;
      });
    }
  CHECK(seen == fwd.at.size(), "%s: the gather found %zu of %zu entries", name, seen, fwd.at.size());
  // sums against a brute-force sum over the entry list
  const size_t m = (size_t)angles.size() * (size_t)ndet, n = (size_t)ny * (size_t)nx;
  for (double alpha : {1.0, 2.0, 0.5}) {
    std::vector<long double> rs(m, 0), cs(n, 0);
    std::vector<int> rt(m, 0), ct(n, 0);
    for (const auto& kv : fwd.at) {
      const long double v = std::pow(std::fabs((long double)kv.second), (long double)alpha);
      rs[(size_t)kv.first.first] += v; cs[(size_t)kv.first.second] += v; rt[(size_t)kv.first.first]++; ct[(size_t)kv.first.second]++;
    }
    for (size_t r = 0; r < m; r++) {
      const double got = r2d::RowSum<T>(table.data(), g, alpha, (int)(r / (size_t)ndet), (int)(r % (size_t)ndet));
      if (rt[r] == 0) CHECK(got == 0, "%s: empty row %zu sums to %g", name, r, got);
      else CHECK(std::fabs((long double)got - rs[r]) <= (rt[r] + 8) * std::numeric_limits<double>::epsilon() * rs[r], "%s: row sum %zu", name, r);
    }
    for (size_t c = 0; c < n; c++) {
      const double got = r2d::ColSum<T>(table.data(), g, alpha, (int)(c % (size_t)ny), (int)(c / (size_t)ny));
      if (ct[c] == 0) CHECK(got == 0, "%s: empty column %zu sums to %g", name, c, got);
      else CHECK(std::fabs((long double)got - cs[c]) <= (ct[c] + 8) * std::numeric_limits<double>::epsilon() * cs[c], "%s: column sum %zu", name, c);
    }
  }
  // the marches on unit vectors: entry for entry, plain and accumulating
  int runs = 0;
  if (m * n <= 40000) {
    std::vector<T> unit(n * planes, (T)0), out(m * planes), acc(m * planes);
    for (size_t c = 0; c < n; c++) {
      unit[c + (planes - 1) * n] = (T)1;
      for (size_t r = 0; r < m * planes; r++) acc[r] = (T)(0.5 + (double)r);
      r2d::Apply<T, false>(out.data(), unit.data(), g, table.data(), false);
      r2d::Apply<T, true>(acc.data(), unit.data(), g, table.data(), false);
      for (size_t r = 0; r < m * planes; r++) {
        auto it = r >= (planes - 1) * m ? fwd.at.find(std::make_pair((long)(r - (planes - 1) * m), (long)c)) : fwd.at.end();
        const T want = it == fwd.at.end() ? (T)0 : it->second;
        CHECK(out[r] == want, "%s: K e_%zu at row %zu", name, c, r);
        CHECK(same_bits(acc[r], (T)((T)(0.5 + (double)r) + out[r])), "%s: accumulating K e_%zu at row %zu", name, c, r);
      }
      unit[c + (planes - 1) * n] = (T)0;
    }
    std::vector<T> unit_t(m * planes, (T)0), out_t(n * planes), acc_t(n * planes);
    for (size_t r = 0; r < m; r++) {
      unit_t[r] = (T)1;
      for (size_t c = 0; c < n * planes; c++) acc_t[c] = (T)(0.25 - (double)c);
      r2d::Apply<T, false>(out_t.data(), unit_t.data(), g, table.data(), true);
      r2d::Apply<T, true>(acc_t.data(), unit_t.data(), g, table.data(), true);
      for (size_t c = 0; c < n * planes; c++) {
        auto it = c < n ? fwd.at.find(std::make_pair((long)r, (long)c)) : fwd.at.end();
        const T want = it == fwd.at.end() ? (T)0 : it->second;
        CHECK(out_t[c] == want, "%s: K^T e_%zu at column %zu", name, r, c);
        CHECK(same_bits(acc_t[c], (T)((T)(0.25 - (double)c) + out_t[c])), "%s: accumulating K^T e_%zu at column %zu", name, r, c);
      }
      unit_t[r] = (T)0;
    }
    runs = 1;
  }
  // random vectors against the entry list in long double
  std::mt19937_64 rng(17 + ny * 131 + nx);
  std::normal_distribution<double> normal;
  const long double u = std::numeric_limits<T>::epsilon() / 2;
  for (int transpose = 0; transpose < 2; transpose++) {
    const size_t nin = transpose ? m : n, nout = transpose ? n : m;
    std::vector<T> x(nin * planes), out(nout * planes);
    for (T& v : x) v = (T)normal(rng);
    r2d::Apply<T, false>(out.data(), x.data(), g, table.data(), transpose != 0);
    for (int c = 0; c < planes; c++) {
      std::vector<long double> exact(nout, 0), mag(nout, 0);
      std::vector<int> t(nout, 0);
      for (const auto& kv : fwd.at) {
        const size_t o = (size_t)(transpose ? kv.first.second : kv.first.first), i = (size_t)(transpose ? kv.first.first : kv.first.second);
        const long double p = (long double)kv.second * (long double)x[i + c * nin];
        exact[o] += p; mag[o] += std::fabs(p); t[o]++;
      }
      for (size_t o = 0; o < nout; o++) {
        const long double err = std::fabs((long double)out[o + c * nout] - exact[o]), bound = 1.01L * (t[o] + 1) * u * mag[o];
        CHECK(err <= bound, "%s: transpose %d component %zu: error %Lg over bound %Lg", name, transpose, o, err, bound);
        if (bound > 0 && (double)(err / bound) > worst) worst = (double)(err / bound);
      }
    }
  }
  std::printf("%s: %zu entries, worst error / bound %.3f, within\n", name, fwd.at.size(), worst);
  return runs;
}

template <class T>
static void table_values() {
  const std::vector<double> angles = {0.0, kPi / 4, kPi / 2, kPi};
  const std::vector<T> t = r2d::MakeTable<T>(5, 7, 11, 1.0, 0.0, angles);        // ny 5, nx 7: cx = 3, cy = 2, cd = 5
  const T tol = 8 * std::numeric_limits<T>::epsilon();
  const T* e = t.data();
  CHECK(e[r2d::kQ] == (T)1 && e[r2d::kP] == (T)0 && e[r2d::kR] == (T)-2 && e[r2d::kC] == (T)1 && e[r2d::kAxis] == (T)0, "table at 0");
  e = t.data() + r2d::kTableWidth;
  CHECK(std::fabs(e[r2d::kC] - (T)std::sqrt(2.0)) <= tol && std::fabs(std::fabs(e[r2d::kP]) - (T)1) <= tol && std::fabs(e[r2d::kQ] - (T)std::sqrt(2.0)) <= tol, "table at pi / 4");
  CHECK(e[r2d::kAxis] == (std::fabs(std::cos(kPi / 4)) >= std::fabs(std::sin(kPi / 4)) ? (T)0 : (T)1), "the tie at pi / 4");
  e = t.data() + 2 * r2d::kTableWidth;
  CHECK(e[r2d::kQ] == (T)1 && std::fabs(e[r2d::kP]) <= tol && std::fabs(e[r2d::kR] - (T)-3) <= 8 * tol && e[r2d::kC] == (T)1 && e[r2d::kAxis] == (T)1, "table at pi / 2");
  e = t.data() + 3 * r2d::kTableWidth;
  CHECK(e[r2d::kQ] == (T)-1 && std::fabs(e[r2d::kP]) <= tol && std::fabs(e[r2d::kR] - (T)8) <= 8 * tol && e[r2d::kC] == (T)1 && e[r2d::kAxis] == (T)0, "table at pi");
}

/// entries sampled at random rays and driving lines of a large image: each has to lie in the candidate window of its pixel
static void window_at_scale(double spacing, long samples) {
  typedef float T;
  const int n = 8192, ndet = (int)r2d::DefaultBins(n, n, spacing);
  std::mt19937_64 rng(99);
  std::uniform_real_distribution<double> any_angle(-kPi, 2 * kPi);
  std::vector<double> angles = {0.0, kPi / 4, kPi / 2, 3 * kPi / 4, kPi, -kPi / 4};
  while (angles.size() < 64) angles.push_back(any_angle(rng));
  const r2d::Geometry g = r2d::MakeGeometry(n, n, 1, ndet, (long)angles.size(), spacing, false);
  const std::vector<T> table = r2d::MakeTable<T>(n, n, ndet, spacing, 0.1, angles);
  std::uniform_int_distribution<int> pick_a(0, g.na - 1), pick_t(0, n - 1);
  std::uniform_real_distribution<double> pick_i(-1.0, (double)n);
  long checked = 0, outside = 0, widest = 0;
  while (checked < samples) {
    // a ray through a random point of a random driving line, so that every sample has an entry
    const int a = pick_a(rng), t = pick_t(rng);
    const T* e = table.data() + (size_t)a * r2d::kTableWidth;
    const double d_real = (pick_i(rng) - ((double)e[r2d::kR] + (double)e[r2d::kP] * t)) / (double)e[r2d::kQ];
    const int d = (int)std::floor(d_real);
    if (d < 0 || d >= ndet) continue;
    T w0, w1;
    const T pt = e[r2d::kP] * (T)t;
    const int i0 = r2d::Weights<T>(r2d::Position(r2d::Base(e, d), pt), n, w0, w1);
    for (int s = 0; s < 2; s++) {
      const int i = i0 + s;
      const T w = s ? w1 : w0;
      if (i0 < -1 || i < 0 || i >= n || w == (T)0) continue;
      const int first = r2d::FirstCandidate<T>(e, pt, i, g.m, ndet);
      if (d < first || d > first + 2 * g.m + 1) outside++;
      // how many bins reach this pixel on this line: the width the window has to hold
      long bins = 0;
      for (int k = -8; k <= 8; k++) {
        if (d + k < 0 || d + k >= ndet) continue;
        T v0, v1;
        const int j0 = r2d::Weights<T>(r2d::Position(r2d::Base(e, d + k), pt), n, v0, v1);
        if ((j0 == i && v0 != (T)0) || (j0 + 1 == i && v1 != (T)0)) bins++;
      }
      if (bins > widest) widest = bins;
      checked++;
    }
  }
  CHECK(outside == 0, "spacing %g: %ld of %ld sampled entries lie outside the candidate window", spacing, outside, checked);
  std::printf("8192x8192 fp32 spacing %g: %ld sampled entries, %ld outside the window, at most %ld bins per pixel and angle (window %d)\n", spacing, checked, outside, widest,
              2 * g.m + 2);
}

int main() {
  table_values<float>();
  table_values<double>();
  const std::vector<double> special = {0.0, kPi / 4, kPi / 2, 3 * kPi / 4, kPi, -kPi / 4, 2 * kPi + 0.1};
  std::vector<double> more = special;
  std::mt19937_64 rng(5);
  std::uniform_real_distribution<double> any_angle(-kPi, 2 * kPi);
  for (int k = 0; k < 12; k++) more.push_back(any_angle(rng));
  struct Shape { int ny, nx, planes, ndet; double spacing, shift; bool all; };
  const Shape shapes[] = {{1, 1, 1, 3, 1.0, 0.0, false},  {1, 1, 1, 1, 1.0, 0.3, false},   {5, 5, 1, 9, 1.0, 0.0, true},    {5, 5, 2, 63, 0.5, -0.3, false},
                          {9, 7, 1, 13, 1.0, 0.3, true},  {9, 7, 1, 3, 1.0, 0.0, false},   {7, 10, 1, 7, 2.0, 0.0, true},   {7, 10, 1, 65, 0.5, 0.3, false},
                          {11, 10, 1, 17, 1.0, -0.3, true}, {10, 11, 2, 9, 2.5, 0.3, false}, {65, 6, 1, 135, 0.5, 0.0, false}, {33, 70, 1, 64, 1.0, 0.0, true}};
  int runs = 0;
  double worst32 = 0, worst64 = 0;
  for (const Shape& s : shapes) {
    char name[128];
    std::snprintf(name, sizeof(name), "%dx%dx%d ndet %d spacing %g shift %g fp32", s.ny, s.nx, s.planes, s.ndet, s.spacing, s.shift);
    runs += small_shape<float>(name, s.ny, s.nx, s.planes, s.ndet, s.spacing, s.shift, s.all ? more : special, worst32);
    std::snprintf(name, sizeof(name), "%dx%dx%d ndet %d spacing %g shift %g fp64", s.ny, s.nx, s.planes, s.ndet, s.spacing, s.shift);
    runs += small_shape<double>(name, s.ny, s.nx, s.planes, s.ndet, s.spacing, s.shift, s.all ? more : special, worst64);
  }
  for (double spacing : {0.5, 1.0, 8.0}) window_at_scale(spacing, 1000000);
  std::printf("entry list and transpose reproduced entry for entry in %d runs\n", runs);
  std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
