// fanbeam2d_harness.cpp -- include/prost/linop/fanbeam2d.hpp on the host, as a stand-alone program (plain g++, no HIP): the three
// tables, the ray enumeration, the gather enumeration with its candidate window, the two marches the kernels call in every lane, and
// the sums of the host block.  Built with -fsanitize=address,undefined by tests/test_fanbeam2d_host.py; every buffer has exactly its size.
//
//   * table values at beta = 0, pi / 2 and the tie at pi / 4; the fit of atan against libm on the whole fan range;
//   * at the small shapes the gather enumeration and the ray enumeration give the same entry set with the same bits, and the marches
//     (plain and accumulating) on unit vectors reproduce the entries and their transpose bit for bit;
//   * on random vectors the marches stay within 1.01 (t + 1) u (|K| |x|) of the entry list summed in long double;
//   * the sums equal a brute-force sum over the entry list, empty rows and columns exactly 0;
//   * the digests (FNV-1a over the bytes) of both products of a fixed input, which tests/test_fanbeam2d_host.py compares with the NumPy
//     restatement of tests/fanbeam2d_reference.py;
//   * for 10^6 sampled entries at 8192 x 8192 in fp32, flat and curved, at the closest source the margin admits and far away, no entry
//     is outside the candidate window.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "prost/linop/fanbeam2d.hpp"

namespace f2d = prost::fanbeam2d;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static const double kPi = 3.14159265358979323846;

template <class T> static bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

template <class T> struct Entries {
  std::map<std::pair<long, long>, T> at;      // (row, column) -> value
};

template <class T>
static Entries<T> forward_entries(const std::vector<T>& table, const f2d::Geometry& g) {
  Entries<T> e;
  for (int a = 0; a < g.na; a++)
    for (int d = 0; d < g.ndet; d++)
      f2d::ForEachInRay<T>(table.data(), g, a, d, [&](int t, int i, T v) {
        int y, x;
        f2d::PixelOf<T>(table.data(), a, t, i, y, x);
        const std::pair<long, long> key((long)a * g.ndet + d, (long)y + (long)x * g.ny);
        CHECK(e.at.find(key) == e.at.end(), "ray enumeration names entry (%ld, %ld) twice", key.first, key.second);
        e.at[key] = v;
      });
  return e;
}

template <class T> static uint64_t digest(const std::vector<T>& v) {
  uint64_t h = 1469598103934665603ull;
  const unsigned char* p = reinterpret_cast<const unsigned char*>(v.data());
  for (size_t k = 0; k < v.size() * sizeof(T); k++) h = (h ^ p[k]) * 1099511628211ull;
  return h;
}
template <class T> static std::vector<T> digest_input(size_t n, uint64_t salt) {
  std::vector<T> v(n);
  for (size_t k = 0; k < n; k++) v[k] = (T)((double)(((uint64_t)k + salt) * 2654435761ull % 4294967296ull) / 4294967296.0 - 0.5);
  return v;
}

struct Shape { int ny, nx, planes, ndet; double spacing, shift, R, D; bool curved; };

template <class T>
static int small_shape(const char* name, const char* type, const Shape& sh, const std::vector<double>& angles, const std::vector<double>& digest_angles, double& worst) {
  const int ny = sh.ny, nx = sh.nx, planes = sh.planes, ndet = sh.ndet;
  const f2d::Scanner s = {ny, nx, ndet, sh.R, sh.D, sh.spacing, sh.shift, sh.curved};
  CHECK(sh.R >= f2d::HalfDiagonal(nx, ny) + 1 && f2d::MaxFanAngle(s) <= kPi / 6 && f2d::MarginOf(s) <= f2d::kMaxMargin && f2d::Slack<T>(s) <= f2d::kSlack,
        "%s: the shape is not admissible", name);
  const f2d::Geometry g = f2d::MakeGeometry(s, planes, (long)angles.size(), false);
  const std::vector<T> table = f2d::MakeTable<T>(s, angles);
  CHECK(table.size() == f2d::TableSize((long)angles.size(), ndet), "%s: table size", name);
  const Entries<T> fwd = forward_entries<T>(table, g);
  // the gather enumeration: the same set, the same bits, rows ascending inside a pixel
  size_t seen = 0;
  for (int x = 0; x < nx; x++)
    for (int y = 0; y < ny; y++) {
      long last = -1;
      f2d::ForEachAtPixel<T>(table.data(), g, y, x, [&](int a, int d, T v) {
        const long row = (long)a * ndet + d;
        CHECK(row > last, "%s: pixel (%d, %d) visits row %ld after %ld", name, y, x, row, last);
        last = row;
        auto it = fwd.at.find(std::make_pair(row, (long)y + (long)x * ny));
        CHECK(it != fwd.at.end(), "%s: the gather names entry (%ld; %d, %d) the rays do not have", name, row, y, x);
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
      const double got = f2d::RowSum<T>(table.data(), g, alpha, (int)(r / (size_t)ndet), (int)(r % (size_t)ndet));
      if (rt[r] == 0) CHECK(got == 0, "%s: empty row %zu sums to %g", name, r, got);
      else CHECK(std::fabs((long double)got - rs[r]) <= (rt[r] + 8) * std::numeric_limits<double>::epsilon() * rs[r], "%s: row sum %zu", name, r);
    }
    for (size_t c = 0; c < n; c++) {
      const double got = f2d::ColSum<T>(table.data(), g, alpha, (int)(c % (size_t)ny), (int)(c / (size_t)ny));
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
      f2d::Apply<T, false>(out.data(), unit.data(), g, table.data(), false);
      f2d::Apply<T, true>(acc.data(), unit.data(), g, table.data(), false);
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
      f2d::Apply<T, false>(out_t.data(), unit_t.data(), g, table.data(), true);
      f2d::Apply<T, true>(acc_t.data(), unit_t.data(), g, table.data(), true);
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
    f2d::Apply<T, false>(out.data(), x.data(), g, table.data(), transpose != 0);
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
  // the digests of both products of a fixed input, at the views the restatement can name
  {
    const f2d::Geometry gd = f2d::MakeGeometry(s, planes, (long)digest_angles.size(), false);
    const std::vector<T> td = f2d::MakeTable<T>(s, digest_angles);
    const size_t md = digest_angles.size() * (size_t)ndet;
    const std::vector<T> u_in = digest_input<T>(n * planes, 1), v_in = digest_input<T>(md * planes, 2);
    std::vector<T> ku(md * planes), ktv(n * planes);
    f2d::Apply<T, false>(ku.data(), u_in.data(), gd, td.data(), false);
    f2d::Apply<T, false>(ktv.data(), v_in.data(), gd, td.data(), true);
    std::printf("digest %d %d %d %d %.17g %.17g %.17g %.17g %s %s margin %d forward %016llx adjoint %016llx\n", ny, nx, planes, ndet, sh.spacing, sh.shift, sh.R, sh.D,
                sh.curved ? "curved" : "flat", type, gd.m, (unsigned long long)digest(ku), (unsigned long long)digest(ktv));
  }
  std::printf("%s: %zu entries, margin %d, worst error / bound %.3f, within\n", name, fwd.at.size(), g.m, worst);
  return runs;
}

template <class T>
static void table_values() {
  const std::vector<double> angles = {0.0, kPi / 2, kPi / 4};
  const f2d::Scanner s = {5, 7, 11, 100.0, 100.0, 1.0, 0.0, false};            // ny 5, nx 7: cx = 3, cy = 2, cd = 5
  const std::vector<T> t = f2d::MakeTable<T>(s, angles);
  const T tol = 8 * std::numeric_limits<T>::epsilon();
  const T* e = t.data();
  CHECK(e[f2d::kCos] == (T)1 && e[f2d::kSin] == (T)0 && e[f2d::kSx] == (T)3 && e[f2d::kSy] == (T)-98 && e[f2d::kAxis] == (T)0, "view at 0");
  e += f2d::kViewWidth;
  CHECK(std::fabs(e[f2d::kCos]) <= tol && e[f2d::kSin] == (T)1 && e[f2d::kSx] == (T)103 && std::fabs(e[f2d::kSy] - (T)2) <= 100 * tol && e[f2d::kAxis] == (T)1, "view at pi / 2");
  e += f2d::kViewWidth;
  CHECK(e[f2d::kAxis] == (std::fabs(std::cos(kPi / 4)) >= std::fabs(std::sin(kPi / 4)) ? (T)0 : (T)1), "the tie at pi / 4");
  e += f2d::kViewWidth;
  CHECK(e[5 * f2d::kBinWidth + f2d::kSinGamma] == (T)0 && e[5 * f2d::kBinWidth + f2d::kCosGamma] == (T)1, "the central bin");
  CHECK(std::fabs(e[10 * f2d::kBinWidth + f2d::kSinGamma] - (T)(5 / std::sqrt(10025.0))) <= tol, "the last bin: tan gamma = 5 / 100");
  e += 11 * f2d::kBinWidth;
  CHECK(e[f2d::kK0] == (T)5 && e[f2d::kK1] == (T)100 && std::fabs(e[f2d::kHi] - (T)0.05) <= tol && std::fabs(e[f2d::kLo] + (T)0.05) <= tol && e[f2d::kPoly] == (T)0, "inverse map");
  // the ray of the central bin at beta = 0 runs along column cx: p = 0, r = cx, c = 1
  const f2d::Geometry g = f2d::MakeGeometry(s, 1, 3, false);
  const f2d::Ray<T> ray = f2d::RayOf(t.data(), g, 0, 5);
  CHECK(ray.p == (T)0 && ray.r == (T)3 && ray.c == (T)1, "the central ray at 0");
}

/// the fit of atan: the largest error on the fan range against libm
static void atan_fit() {
  double worst = 0;
  const double top = std::tan(kPi / 6);
  for (int k = -200000; k <= 200000; k++) {
    const double tau = top * k / 200000.0, z = tau * tau;
    double poly = f2d::kAtan[f2d::kPolyTerms - 1];
    for (int j = f2d::kPolyTerms - 2; j >= 0; j--) poly = poly * z + f2d::kAtan[j];
    worst = std::fmax(worst, std::fabs(tau + tau * (z * poly) - std::atan(tau)));
  }
  CHECK(worst <= f2d::kAtanError, "the fit of atan is off by %g", worst);
  std::printf("atan fit: largest error %.3g on |tau| <= tan 30 degrees (kAtanError %.3g)\n", worst, f2d::kAtanError);
}

/// entries sampled at random rays and driving lines of a large image: each has to lie in the candidate window of its pixel
static void window_at_scale(double spacing, double distance, bool curved, long samples) {
  typedef float T;
  const int n = 8192;
  const double R = distance * f2d::HalfDiagonal(n, n);
  const int ndet = (int)f2d::DefaultBins(n, n, R, R, spacing, curved);
  std::mt19937_64 rng(99);
  std::uniform_real_distribution<double> any_angle(-kPi, 2 * kPi);
  std::vector<double> angles = {0.0, kPi / 4, kPi / 2, 3 * kPi / 4, kPi, -kPi / 4};
  while (angles.size() < 64) angles.push_back(any_angle(rng));
  const f2d::Scanner s = {n, n, ndet, R, R, spacing, 0.1, curved};
  CHECK(f2d::MaxFanAngle(s) <= kPi / 6 && f2d::MarginOf(s) <= f2d::kMaxMargin && f2d::Slack<T>(s) <= f2d::kSlack, "spacing %g distance %g: not admissible (slack %g)", spacing,
        distance, f2d::Slack<T>(s));
  const f2d::Geometry g = f2d::MakeGeometry(s, 1, (long)angles.size(), false);
  const std::vector<T> table = f2d::MakeTable<T>(s, angles);
  const T* inv = f2d::InverseTable(table.data(), g);
  std::uniform_int_distribution<int> pick_a(0, g.na - 1), pick_t(0, n - 1), pick_d(0, ndet - 1);
  long checked = 0, outside = 0, widest = 0;
  while (checked < samples) {
    const int a = pick_a(rng), t = pick_t(rng), d = pick_d(rng);
    const T* e = table.data() + (size_t)a * f2d::kViewWidth;
    const bool column = e[f2d::kAxis] != (T)0;
    const f2d::Ray<T> ray = f2d::RayOf(table.data(), g, a, d);
    T w0, w1;
    const int i0 = f2d::Weights<T>(f2d::Position(ray.r, ray.p * (T)t), n, w0, w1);
    for (int k = 0; k < 2; k++) {
      const int i = i0 + k;
      const T w = k ? w1 : w0;
      if (i0 < -1 || i < 0 || i >= n || w == (T)0) continue;
      const int y = column ? i : t, x = column ? t : i;
      const int first = f2d::FirstCandidate<T>(e, inv, y, x, g.m, ndet);
      if (d < first || d > first + 2 * g.m + 1) outside++;
      // how many bins reach this pixel on this line: the width the window has to hold
      long bins = 0;
      for (int j = -12; j <= 12; j++) {
        if (d + j < 0 || d + j >= ndet) continue;
        const f2d::Ray<T> other = f2d::RayOf(table.data(), g, a, d + j);
        T v0, v1;
        const int j0 = f2d::Weights<T>(f2d::Position(other.r, other.p * (T)t), n, v0, v1);
        if ((j0 == i && v0 != (T)0) || (j0 + 1 == i && v1 != (T)0)) bins++;
      }
      if (bins > widest) widest = bins;
      checked++;
    }
  }
  CHECK(outside == 0, "spacing %g distance %g: %ld of %ld sampled entries lie outside the candidate window", spacing, distance, outside, checked);
  std::printf("8192x8192 fp32 %s spacing %g R %g hd: %ld sampled entries, %ld outside the window, at most %ld bins per pixel and view (window %d)\n", curved ? "curved" : "flat",
              spacing, distance, checked, outside, widest, 2 * g.m + 2);
}

int main() {
  table_values<float>();
  table_values<double>();
  atan_fit();
  const std::vector<double> special = {0.0, kPi / 4, kPi / 2, 3 * kPi / 4, kPi, -kPi / 4, 5 * kPi / 4 + 0.1, 2 * kPi + 0.1, -2.0};
  std::vector<double> more = special;
  std::mt19937_64 rng(5);
  std::uniform_real_distribution<double> any_angle(-kPi, 2 * kPi);
  for (int k = 0; k < 12; k++) more.push_back(any_angle(rng));
  struct Run { Shape shape; bool all; };
  // { ny, nx, planes, ndet, spacing, shift, R, D, curved }
  const Run runs_[] = {{{1, 1, 1, 3, 1.0, 0.0, 4.0, 4.0, false}, false},        {{1, 1, 1, 1, 0.5, 0.25, 1.75, 1.75, true}, false},
                       {{3, 5, 1, 1, 0.5, 0.25, 4.0, 4.0, false}, true},         {{3, 5, 2, 63, 0.5, 0.0, 27.0, 27.0, false}, false},
                       {{9, 7, 1, 13, 1.0, 0.25, 12.0, 12.0, true}, true},       {{9, 7, 1, 3, 1.0, 0.0, 8.0, 12.0, false}, false},
                       {{7, 10, 1, 7, 2.0, 0.0, 14.0, 14.0, true}, true},        {{7, 10, 1, 65, 0.5, 0.25, 600.0, 40.0, false}, false},
                       {{11, 10, 1, 17, 1.0, -0.3, 16.0, 24.0, true}, true},     {{10, 11, 2, 9, 2.5, 0.3, 800.0, 800.0, false}, false},
                       {{65, 6, 1, 135, 0.5, 0.0, 70.0, 70.0, true}, false},     {{33, 70, 1, 64, 1.0, 0.0, 100.0, 100.0, false}, true}};
  int runs = 0;
  double worst32 = 0, worst64 = 0;
  for (const Run& r : runs_) {
    const Shape& s = r.shape;
    char name[160];
    std::snprintf(name, sizeof(name), "%dx%dx%d ndet %d spacing %g shift %g R %g D %g %s fp32", s.ny, s.nx, s.planes, s.ndet, s.spacing, s.shift, s.R, s.D, s.curved ? "curved" : "flat");
    runs += small_shape<float>(name, "fp32", s, r.all ? more : special, special, worst32);
    std::snprintf(name, sizeof(name), "%dx%dx%d ndet %d spacing %g shift %g R %g D %g %s fp64", s.ny, s.nx, s.planes, s.ndet, s.spacing, s.shift, s.R, s.D, s.curved ? "curved" : "flat");
    runs += small_shape<double>(name, "fp64", s, r.all ? more : special, special, worst64);
  }
  window_at_scale(0.5, 2.01, false, 1000000);
  window_at_scale(0.5, 2.01, true, 1000000);
  window_at_scale(1.0, 3.0, false, 1000000);
  window_at_scale(8.0, 3.0, true, 1000000);
  std::printf("entry list and transpose reproduced entry for entry in %d runs\n", runs);
  std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
