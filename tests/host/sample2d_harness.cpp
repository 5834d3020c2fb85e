// sample2d_harness.cpp -- include/prost/linop/sample2d.hpp on the host, as a stand-alone program (plain g++, no HIP): the entries of a
// row, the bucket tables, the gather enumeration, the two sums the kernels call in every lane, and the sums of the host block.  Built
// with -fsanitize=address,undefined by tests/test_sample2d_host.py; every buffer has exactly its size.
//
//   * bucket construction: every sample with entries appears exactly once, in its own cell, ascending inside the cell; the samples
//     without entries stand behind the last cell;
//   * the gather enumeration and the forward enumeration give the same entry set with the same bits, in the pinned order;
//   * the products (plain and accumulating) on unit vectors reproduce the entries and their transpose bit for bit;
//   * on random vectors the products stay within 1.01 (t + 1) u (|K| |x|) of the entry list summed in long double;
//   * the sums equal a brute-force sum over the entry list, empty rows and columns exactly 0;
//   * index safety of 10^6 random positions, huge, negative and non-finite ones included, at 16384 x 16384 in fp32: every offset and
//     every cell is checked by value there (the image alone would be 1 GiB), and run against exactly sized buffers at 16384 x 2 and
//     2 x 16384.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "prost/linop/sample2d.hpp"

namespace s2d = prost::sample2d;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } while (0)

static const double kPi = 3.14159265358979323846;

template <class T> static bool same_bits(T a, T b) { return std::memcmp(&a, &b, sizeof(T)) == 0; }

static std::vector<double> special_values(int n) {
  return {0.0, (double)(n - 1), -1.0, -0.5, -0.25, n - 0.5, n - 0.75, (double)n, -1.0 - 1.0 / 1024, n + 1.0 / 1024, 1e30, -1e30,
          std::fmin(0.5, n - 1.0), (n - 1) * 0.375, (n - 1) / 2.0};
}

static void positions(const std::string& kind, int ny, int nx, size_t m, unsigned seed, std::vector<double>& x, std::vector<double>& y) {
  std::mt19937_64 rng(seed);
  x.assign(m, 0); y.assign(m, 0);
  if (kind == "integers") {
    for (size_t i = 0; i < m; i++) { x[i] = (double)(i / (size_t)ny); y[i] = (double)(i % (size_t)ny); }
  } else if (kind == "flow") {
    for (size_t i = 0; i < m; i++) {
      const double px = (double)(i / (size_t)ny), py = (double)(i % (size_t)ny);
      x[i] = px + 4.5 * std::sin(2 * kPi * 1.5 * px / nx) * std::cos(2 * kPi * py / ny);
      y[i] = py + 4.5 * std::cos(2 * kPi * px / nx) * std::sin(2 * kPi * 2.0 * py / ny);
    }
  } else if (kind == "onecell") {
    std::uniform_real_distribution<double> in_cell(0.01, 0.99);
    for (size_t i = 0; i < m; i++) { x[i] = nx / 2 + in_cell(rng); y[i] = ny / 2 + in_cell(rng); }
  } else if (kind == "random") {
    std::uniform_real_distribution<double> rx(-1.5, nx + 0.5), ry(-1.5, ny + 0.5);
    for (size_t i = 0; i < m; i++) { x[i] = rx(rng); y[i] = ry(rng); }
  } else {
    const std::vector<double> sx = special_values(nx), sy = special_values(ny);
    for (size_t i = 0; i < m; i++) {
      const bool grid = i < sx.size() * sy.size();
      x[i] = sx[grid ? i % sx.size() : rng() % sx.size()];
      y[i] = sy[grid ? (i / sx.size() + i) % sy.size() : rng() % sy.size()];
    }
  }
}

template <class T> struct Entries {
  std::map<std::pair<long, long>, T> at;      // (row, column) -> value
};

template <class T>
static int small_shape(const char* name, int ny, int nx, int planes, const std::string& kind, size_t m, double& worst) {
  std::vector<double> xd, yd;
  positions(kind, ny, nx, m, (unsigned)(31 * ny + nx + m), xd, yd);
  const std::vector<T> px(xd.begin(), xd.end()), py(yd.begin(), yd.end());       // rounded once to T
  const s2d::Geometry g = s2d::MakeGeometry(ny, nx, (long)m, planes, false);
  const size_t n = (size_t)ny * (size_t)nx, cells = s2d::Cells(ny, nx);
  // the forward enumeration
  Entries<T> fwd;
  std::vector<int> has(m, 0);
  for (size_t i = 0; i < m; i++) {
    int last_slot = -1;
    s2d::ForEachInRow<T>(px.data(), py.data(), g, i, [&](int slot, int yy, int xx, T v) {
      CHECK(slot > last_slot && yy >= 0 && yy < ny && xx >= 0 && xx < nx && v != (T)0, "%s: row %zu slot %d at (%d, %d)", name, i, slot, yy, xx);
      last_slot = slot;
      const std::pair<long, long> key((long)i, (long)yy + (long)xx * ny);
      CHECK(fwd.at.find(key) == fwd.at.end(), "%s: forward enumeration names entry (%ld, %ld) twice", name, key.first, key.second);
      fwd.at[key] = v;
      has[i] = 1;
    });
  }
  // the bucket tables
  std::vector<int32_t> order, cell_start;
  s2d::MakeBuckets<T>(px.data(), py.data(), m, ny, nx, order, cell_start);
  CHECK(order.size() == m && cell_start.size() == cells + 1 && cell_start[0] == 0, "%s: table sizes", name);
  std::vector<int> times(m, 0);
  size_t with_entries = 0;
  for (size_t i = 0; i < m; i++) with_entries += (size_t)has[i];
  CHECK((size_t)cell_start[cells] == with_entries, "%s: %d bucketed samples, %zu have entries", name, (int)cell_start[cells], with_entries);
  for (size_t c = 0; c < cells; c++) {
    CHECK(cell_start[c] <= cell_start[c + 1], "%s: cell %zu has a negative count", name, c);
    for (int32_t k = cell_start[c]; k < cell_start[c + 1]; k++) {
      const int32_t s = order[(size_t)k];
      CHECK(s >= 0 && (size_t)s < m, "%s: order[%d] = %d", name, (int)k, (int)s);
      if (s < 0 || (size_t)s >= m) continue;
      times[(size_t)s]++;
      CHECK(has[(size_t)s], "%s: sample %d has no entries and is bucketed", name, (int)s);
      const long own = ((long)std::floor((double)py[(size_t)s]) + 1) + ((long)std::floor((double)px[(size_t)s]) + 1) * (ny + 1);
      CHECK(own == (long)c, "%s: sample %d of cell %ld stands in cell %zu", name, (int)s, own, c);
      if (k > cell_start[c]) CHECK(order[(size_t)k - 1] < s, "%s: cell %zu is not ascending", name, c);
    }
  }
  for (size_t k = with_entries; k < m; k++) {
    CHECK(order[k] >= 0 && (size_t)order[k] < m && !has[(size_t)order[k]], "%s: the tail of order", name);
    if (order[k] >= 0 && (size_t)order[k] < m) times[(size_t)order[k]]++;
  }
  for (size_t i = 0; i < m; i++) CHECK(times[i] == 1, "%s: sample %zu appears %d times", name, i, times[i]);
  // the gather enumeration: the same set, the same bits; inside a pixel by cell (slot 3, 2, 1, 0), inside a cell ascending
  size_t seen = 0;
  for (int xx = 0; xx < nx; xx++)
    for (int yy = 0; yy < ny; yy++) {
      long last_cell = -1, last = -1;
      s2d::ForEachAtPixel<T>(px.data(), py.data(), order.data(), cell_start.data(), g, yy, xx, [&](size_t i, T v) {
        const int i0 = (int)std::floor((double)py[i]), j0 = (int)std::floor((double)px[i]);
        const long rank = (j0 == xx ? 2 : 0) + (i0 == yy ? 1 : 0);      // (yy-1, xx-1), (yy, xx-1), (yy-1, xx), (yy, xx)
        CHECK((i0 == yy || i0 == yy - 1) && (j0 == xx || j0 == xx - 1), "%s: pixel (%d, %d) visits sample %zu of another cell", name, yy, xx, i);
        CHECK(rank > last_cell || (rank == last_cell && (long)i > last), "%s: pixel (%d, %d) visits sample %zu out of order", name, yy, xx, i);
        last_cell = rank; last = (long)i;
        auto it = fwd.at.find(std::make_pair((long)i, (long)yy + (long)xx * ny));
        CHECK(it != fwd.at.end(), "%s: the gather names entry (%zu; %d, %d) the forward does not have", name, i, yy, xx);
        if (it != fwd.at.end()) CHECK(same_bits(it->second, v), "%s: entry (%zu; %d, %d) differs in its bits", name, i, yy, xx);
        seen++;
      });
    }
  CHECK(seen == fwd.at.size(), "%s: the gather found %zu of %zu entries", name, seen, fwd.at.size());
  // sums against a brute-force sum over the entry list
  for (double alpha : {1.0, 2.0, 0.5}) {
    std::vector<long double> rs(m, 0), cs(n, 0);
    std::vector<int> rt(m, 0), ct(n, 0);
    for (const auto& kv : fwd.at) {
      const long double v = std::pow(std::fabs((long double)kv.second), (long double)alpha);
      rs[(size_t)kv.first.first] += v; cs[(size_t)kv.first.second] += v; rt[(size_t)kv.first.first]++; ct[(size_t)kv.first.second]++;
    }
    for (size_t r = 0; r < m; r++) {
      const double got = s2d::RowSum<T>(px.data(), py.data(), g, alpha, r);
      if (rt[r] == 0) CHECK(got == 0, "%s: empty row %zu sums to %g", name, r, got);
      else CHECK(std::fabs((long double)got - rs[r]) <= (rt[r] + 8) * std::numeric_limits<double>::epsilon() * rs[r], "%s: row sum %zu", name, r);
    }
    for (size_t c = 0; c < n; c++) {
      const double got = s2d::ColSum<T>(px.data(), py.data(), order.data(), cell_start.data(), g, alpha, (int)(c % (size_t)ny), (int)(c / (size_t)ny));
      if (ct[c] == 0) CHECK(got == 0, "%s: empty column %zu sums to %g", name, c, got);
      else CHECK(std::fabs((long double)got - cs[c]) <= (ct[c] + 8) * std::numeric_limits<double>::epsilon() * cs[c], "%s: column sum %zu", name, c);
    }
  }
  // the products on unit vectors: entry for entry, plain and accumulating
  int runs = 0;
  if (m * n <= 40000) {
    std::vector<T> unit(n * planes, (T)0), out(m * planes), acc(m * planes);
    for (size_t c = 0; c < n; c++) {
      unit[c + (planes - 1) * n] = (T)1;
      for (size_t r = 0; r < m * planes; r++) acc[r] = (T)(0.5 + (double)r);
      s2d::Apply<T, false>(out.data(), unit.data(), g, px.data(), py.data(), order.data(), cell_start.data(), false);
      s2d::Apply<T, true>(acc.data(), unit.data(), g, px.data(), py.data(), order.data(), cell_start.data(), false);
      for (size_t r = 0; r < m * planes; r++) {
        auto it = r >= (planes - 1) * m ? fwd.at.find(std::make_pair((long)(r - (planes - 1) * m), (long)c)) : fwd.at.end();
        const T want = it == fwd.at.end() ? (T)0 : it->second;
        CHECK(same_bits(out[r], want), "%s: K e_%zu at row %zu", name, c, r);
        CHECK(same_bits(acc[r], (T)((T)(0.5 + (double)r) + out[r])), "%s: accumulating K e_%zu at row %zu", name, c, r);
      }
      unit[c + (planes - 1) * n] = (T)0;
    }
    std::vector<T> unit_t(m * planes, (T)0), out_t(n * planes), acc_t(n * planes);
    for (size_t r = 0; r < m; r++) {
      unit_t[r] = (T)1;
      for (size_t c = 0; c < n * planes; c++) acc_t[c] = (T)(0.25 - (double)c);
      s2d::Apply<T, false>(out_t.data(), unit_t.data(), g, px.data(), py.data(), order.data(), cell_start.data(), true);
      s2d::Apply<T, true>(acc_t.data(), unit_t.data(), g, px.data(), py.data(), order.data(), cell_start.data(), true);
      for (size_t c = 0; c < n * planes; c++) {
        auto it = c < n ? fwd.at.find(std::make_pair((long)r, (long)c)) : fwd.at.end();
        const T want = it == fwd.at.end() ? (T)0 : it->second;
        CHECK(same_bits(out_t[c], want), "%s: K^T e_%zu at column %zu", name, r, c);
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
    s2d::Apply<T, false>(out.data(), x.data(), g, px.data(), py.data(), order.data(), cell_start.data(), transpose != 0);
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

/// a float of any kind: in and around the image, huge, negative, non-finite
static float any_position(std::mt19937_64& rng, int n) {
  const unsigned kind = (unsigned)(rng() % 8);
  std::uniform_real_distribution<double> near(-2.0, n + 1.0), wide(-1e6, 1e6);
  switch (kind) {
    case 0: return (float)std::floor(near(rng));
    case 1: return (float)wide(rng);
    case 2: { const float s[] = {1e30f, -1e30f, 3e38f, -3e38f, 2147483648.0f, -2147483904.0f, 4294967296.0f, 1e-45f, -1e-45f, -0.0f}; return s[rng() % 10]; }
    case 3: { const float s[] = {std::numeric_limits<float>::infinity(), -std::numeric_limits<float>::infinity(), std::numeric_limits<float>::quiet_NaN(),
                                 -1.0f, (float)n, (float)(n - 1), std::nextafter((float)n, 0.0f), std::nextafter(-1.0f, -2.0f)}; return s[rng() % 8]; }
    default: return (float)near(rng);
  }
}

static void index_safety(long samples) {
  typedef float T;
  std::mt19937_64 rng(2401);
  // by value at the largest image
  {
    const int n = s2d::kMaxSide;
    const int64_t plane = (int64_t)n * n, cells = (int64_t)s2d::Cells(n, n);
    long with_entries = 0, out_of_reach = 0;
    for (long i = 0; i < samples; i++) {
      const T fx = any_position(rng, n), fy = any_position(rng, n);
      const s2d::Row<T> r = s2d::MakeRow<T>(fx, fy, n, n);
      bool any = false;
      for (int k = 0; k < 4; k++) {
        CHECK(r.at[k] >= 0 && (int64_t)r.at[k] < plane, "offset %d of (%g, %g) is %d", k, (double)fx, (double)fy, (int)r.at[k]);
        any = any || r.has[k];
      }
      CHECK(r.cell >= -1 && (int64_t)r.cell < cells && (!any || r.cell >= 0), "cell of (%g, %g) is %d", (double)fx, (double)fy, (int)r.cell);
      (void)s2d::WeightAt<T>(fx, fy, n - 1, n - 1);
      with_entries += any; out_of_reach += r.cell < 0;
    }
    CHECK(with_entries > samples / 8 && out_of_reach > samples / 8, "the positions do not exercise both sides: %ld with entries, %ld out of reach", with_entries, out_of_reach);
    std::printf("16384x16384 fp32: %ld positions, %ld with entries, %ld out of reach, every offset and cell inside\n", samples, with_entries, out_of_reach);
  }
  // against exactly sized buffers at the longest sides
  for (int tall = 0; tall < 2; tall++) {
    const int ny = tall ? s2d::kMaxSide : 2, nx = tall ? 2 : s2d::kMaxSide;
    const size_t m = (size_t)samples / 4, n = (size_t)ny * (size_t)nx;
    std::vector<T> px(m), py(m);
    for (size_t i = 0; i < m; i++) { px[i] = any_position(rng, nx); py[i] = any_position(rng, ny); }
    const s2d::Geometry g = s2d::MakeGeometry(ny, nx, (long)m, 1, false);
    std::vector<int32_t> order, cell_start;
    s2d::MakeBuckets<T>(px.data(), py.data(), m, ny, nx, order, cell_start);
    std::vector<T> image(n, (T)1), out(m), back(n);
    s2d::Apply<T, false>(out.data(), image.data(), g, px.data(), py.data(), order.data(), cell_start.data(), false);
    s2d::Apply<T, false>(back.data(), out.data(), g, px.data(), py.data(), order.data(), cell_start.data(), true);
    long double a = 0, b = 0;
    for (size_t i = 0; i < m; i++) { CHECK(out[i] >= 0 && out[i] <= 1.000001f, "sample %zu of the constant image is %g", i, (double)out[i]); a += (long double)out[i] * out[i]; }
    for (size_t p = 0; p < n; p++) b += (long double)back[p];            // <K 1, K 1> = <1, K^T K 1>
    CHECK(std::fabs((double)(a - b)) <= 1e-4 * (double)a, "adjointness at %dx%d: %Lg against %Lg", ny, nx, a, b);
    std::printf("%dx%d fp32: %zu positions against exactly sized buffers, %d bucketed\n", ny, nx, m, (int)cell_start.back());
  }
}

int main() {
  struct Shape { int ny, nx, planes; const char* kind; size_t m; };
  const Shape shapes[] = {{1, 1, 1, "random", 1},   {1, 1, 1, "special", 65},  {1, 7, 2, "special", 63},   {7, 1, 3, "special", 64},   {5, 4, 1, "integers", 20},
                          {65, 3, 2, "integers", 195}, {64, 5, 1, "random", 257}, {65, 6, 2, "special", 257}, {9, 7, 2, "random", 257},   {7, 10, 1, "onecell", 300},
                          {33, 70, 1, "flow", 2310}, {33, 70, 3, "random", 257}, {33, 70, 1, "special", 257}};
  int runs = 0;
  double worst32 = 0, worst64 = 0;
  for (const Shape& s : shapes) {
    char name[128];
    std::snprintf(name, sizeof(name), "%dx%dx%d %s M %zu fp32", s.ny, s.nx, s.planes, s.kind, s.m);
    runs += small_shape<float>(name, s.ny, s.nx, s.planes, s.kind, s.m, worst32);
    std::snprintf(name, sizeof(name), "%dx%dx%d %s M %zu fp64", s.ny, s.nx, s.planes, s.kind, s.m);
    runs += small_shape<double>(name, s.ny, s.nx, s.planes, s.kind, s.m, worst64);
  }
  index_safety(1000000);
  std::printf("entry list and transpose reproduced entry for entry in %d runs\n", runs);
  std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
  return failures ? 1 : 0;
}
