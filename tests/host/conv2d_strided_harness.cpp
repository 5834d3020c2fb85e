// conv2d_strided_harness.cpp -- include/prost/linop/conv2d_strided.hpp on the host, stand-alone (plain g++, no HIP), meant to be built
// with -fsanitize=address,undefined -ffp-contract=off.  The entry list of the matrix is written down from the definition
//
//   K[(y, x), (v, u)] = k(i, j)  for  v = y sy + py + oy - i,  u = x sx + px + ox - j  inside the image,  0 <= y < my, 0 <= x < mx
//
// and the header's Apply -- tile by tile and lane by lane as the kernels run it -- is held against it:
//   * both directions against the entry list summed in long double: |got - exact| <= 1.01 (t + 1) u (|K| |x|) componentwise, t the
//     non-zero tap count, u the unit roundoff of T; the largest error / bound is printed;
//   * every entry of the tile table that fits gives the bits of the smallest tile;
//   * the accumulating forms are res0 + plain, bit for bit;
//   * at the small shapes unit vectors reproduce the entry list and its transpose entry for entry;
//   * the row and column sums (Sums and SumAt) within (t + 8) eps_T of the sums of the entry list in long double, empty ones exactly 0;
//   * every (T, sy, sx, ky, kx) has a tile, and every staged tile stays within 64 KiB.
// Every buffer is allocated at exactly its size, so a march that leaves its planes is an AddressSanitizer report.
// Prints one line per case and precision ending in `within`, then `ok`; exit status 1 on any failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <vector>

#include "prost/linop/conv2d_strided.hpp"

namespace c2d = prost::conv2d;
namespace c2s = prost::conv2d_strided;
typedef long double ld;

static int failures = 0, transposed = 0;

struct Case { int ny, nx, L, ky, kx, sy, sx, py, px, shape; bool zeros; };
struct Entry { size_t r, c; ld k; };

template <class T>
static void run(const char* name, const Case& c, unsigned seed) {
  static const char* shape_name[] = {"full", "same", "valid"};
  long my, mx, oy, ox;
  if (!c2s::OutputSize(c.shape, c.ny, c.nx, c.ky, c.kx, c.sy, c.sx, c.py, c.px, my, mx, oy, ox)) { std::printf("FAIL %s: the case is not legal\n", name); failures++; return; }
  std::mt19937_64 gen(seed);
  std::normal_distribution<double> normal(0.0, 1.0);
  std::vector<double> kernel((size_t)(c.ky * c.kx));
  for (double& v : kernel) v = normal(gen);
  if (c.zeros) for (size_t q = 1; q < kernel.size(); q += 3) kernel[q] = 0.0;             // dropped taps
  const size_t ncols = (size_t)c.L * c.ny * c.nx, nrows = (size_t)c.L * my * mx;
  const std::vector<T> w = c2s::Window<T>(kernel.data(), c.ky, c.kx);
  const int pick = c2s::PickTile(sizeof(T), c.sy, c.sx, c.ky, c.kx);
  bool ok = pick >= 0;
  c2s::Geometry g[2];
  std::vector<c2d::Tap<T>> taps[2];
  for (int dir = 0; dir < 2; dir++) {
    g[dir] = c2s::MakeGeometry(c.shape, c.ny, c.nx, c.ky, c.kx, c.sy, c.sx, c.py, c.px, c.L, dir == 1);
    taps[dir] = c2s::CompactTaps<T>(g[dir], w, pick);
  }
  const size_t t = taps[0].size();
  ok = ok && taps[1].size() == t && t > 0 && g[1].class_start[c2s::kClasses] == (int32_t)t && g[0].class_start[1] == (int32_t)t;
  // the entry list, from the definition
  std::vector<Entry> entries;
  for (int p = 0; p < c.L; p++)
    for (long x = 0; x < mx; x++)
      for (long y = 0; y < my; y++)
        for (int j = 0; j < c.kx; j++)
          for (int i = 0; i < c.ky; i++) {
            const long v = y * c.sy + c.py + oy - i, u = x * c.sx + c.px + ox - j;
            const ld k = (ld)w[(size_t)(i + j * c.ky)];
            if (v < 0 || v >= c.ny || u < 0 || u >= c.nx || k == 0) continue;
            entries.push_back({(size_t)p * my * mx + (size_t)y + (size_t)x * my, (size_t)p * c.ny * c.nx + (size_t)v + (size_t)u * c.ny, k});
          }
  const ld u = (ld)std::numeric_limits<T>::epsilon() / 2, fac = 1.01L * (ld)(t + 1) * u;
  ld worst = 0;
  std::vector<T> x(ncols), y(nrows), res0(nrows), res1(ncols);
  for (T& v : x) v = (T)normal(gen);
  for (T& v : y) v = (T)normal(gen);
  for (T& v : res0) v = (T)normal(gen);
  for (T& v : res1) v = (T)normal(gen);
  std::vector<T> plain(nrows, (T)77), acc(res0), plain_t(ncols, (T)77), acc_t(res1);
  c2s::Apply<T, false>(plain.data(), x.data(), g[0], taps[0].data(), (int)t, pick);
  c2s::Apply<T, true>(acc.data(), x.data(), g[0], taps[0].data(), (int)t, pick);
  c2s::Apply<T, false>(plain_t.data(), y.data(), g[1], taps[1].data(), (int)t, pick);
  c2s::Apply<T, true>(acc_t.data(), y.data(), g[1], taps[1].data(), (int)t, pick);
  // every entry of the tile table that fits: the bits of the smallest tile (the last entry)
  for (int tile = 0; tile < c2s::kTileCount; tile++) {
    if (c2s::ForwardLdsElements(c2s::kTiles[tile], c.ky, c.kx, c.sy, c.sx) * sizeof(T) > c2s::kLdsLimit || tile == pick) continue;
    c2s::Geometry gt = g[0];
    const std::vector<c2d::Tap<T>> tt = c2s::CompactTaps<T>(gt, w, tile);
    std::vector<T> other(nrows, (T)55);
    c2s::Apply<T, false>(other.data(), x.data(), gt, tt.data(), (int)tt.size(), tile);
    for (size_t r = 0; r < nrows; r++)
      if (std::memcmp(&other[r], &plain[r], sizeof(T)) != 0) { ok = false; std::printf("FAIL %s: tile %d differs from tile %d at element %zu\n", name, tile, pick, r); break; }
  }
  const double alphas[2] = {1.0, 0.5};
  std::vector<ld> val(nrows, 0), mag(nrows, 0), val_t(ncols, 0), mag_t(ncols, 0), rs_want[2], cs_want[2];
  for (int a = 0; a < 2; a++) { rs_want[a].assign(nrows, 0); cs_want[a].assign(ncols, 0); }
  for (const Entry& e : entries) {
    val[e.r] += e.k * (ld)x[e.c]; mag[e.r] += std::fabs(e.k * (ld)x[e.c]);
    val_t[e.c] += e.k * (ld)y[e.r]; mag_t[e.c] += std::fabs(e.k * (ld)y[e.r]);
    for (int a = 0; a < 2; a++) { const ld pw = std::pow(std::fabs(e.k), (ld)alphas[a]); rs_want[a][e.r] += pw; cs_want[a][e.c] += pw; }
  }
  for (size_t r = 0; r < nrows; r++) {
    const ld err = std::fabs((ld)plain[r] - val[r]), bound = fac * mag[r];
    if (!(err <= bound)) { ok = false; std::printf("FAIL %s element %zu: error %Lg, bound %Lg\n", name, r, err, bound); }
    if (bound > 0 && err / bound > worst) worst = err / bound;
    const T want = (T)(res0[r] + plain[r]);
    if (std::memcmp(&acc[r], &want, sizeof(T)) != 0) { ok = false; std::printf("FAIL %s element %zu: accumulating form\n", name, r); }
  }
  for (size_t cc = 0; cc < ncols; cc++) {
    const ld err = std::fabs((ld)plain_t[cc] - val_t[cc]), bound = fac * mag_t[cc];
    if (!(err <= bound)) { ok = false; std::printf("FAIL %s adjoint element %zu: error %Lg, bound %Lg\n", name, cc, err, bound); }
    if (bound > 0 && err / bound > worst) worst = err / bound;
    const T want = (T)(res1[cc] + plain_t[cc]);
    if (std::memcmp(&acc_t[cc], &want, sizeof(T)) != 0) { ok = false; std::printf("FAIL %s adjoint element %zu: accumulating form\n", name, cc); }
  }
  // the sums, alpha = 1 and 0.5; an empty row or column is exactly 0
  for (int a = 0; a < 2; a++) {
    const ld tol = (ld)(t + 8) * std::numeric_limits<T>::epsilon();
    std::vector<T> rs(nrows, (T)0), cs(ncols, (T)0);
    c2s::Sums<T>(g[0], w, alphas[a], false, rs.data());
    c2s::Sums<T>(g[0], w, alphas[a], true, cs.data());
    for (size_t r = 0; r < nrows; r++) {
      const size_t p = r % ((size_t)my * mx);
      const ld one = (ld)c2s::SumAt<T>(g[0], w, alphas[a], false, (int)(p % my), (int)(p / my)), want = rs_want[a][r];
      if (!(std::fabs((ld)rs[r] - want) <= tol * want) || !(std::fabs(one - want) <= tol * want)) {
        ok = false; std::printf("FAIL %s: row sum %zu, alpha %g: %Lg and %Lg, expected %Lg\n", name, r, alphas[a], (ld)rs[r], one, want);
      }
    }
    for (size_t cc = 0; cc < ncols; cc++) {
      const size_t p = cc % ((size_t)c.ny * c.nx);
      const ld one = (ld)c2s::SumAt<T>(g[0], w, alphas[a], true, (int)(p % c.ny), (int)(p / c.ny)), want = cs_want[a][cc];
      if (!(std::fabs((ld)cs[cc] - want) <= tol * want) || !(std::fabs(one - want) <= tol * want)) {
        ok = false; std::printf("FAIL %s: column sum %zu, alpha %g: %Lg and %Lg, expected %Lg\n", name, cc, alphas[a], (ld)cs[cc], one, want);
      }
    }
  }
  // unit vectors reproduce the entry list and its transpose entry for entry (small shapes)
  if (nrows * ncols <= (size_t)1 << 16 && t <= 100) {
    std::vector<T> K(nrows * ncols, (T)0), e(ncols, (T)0), f(nrows, (T)0), col(nrows), row(ncols);
    for (const Entry& en : entries) K[en.r + en.c * nrows] = (T)en.k;
    size_t bad = 0;
    for (size_t cc = 0; cc < ncols; cc++) {
      e[cc] = (T)1;
      c2s::Apply<T, false>(col.data(), e.data(), g[0], taps[0].data(), (int)t, pick);
      e[cc] = (T)0;
      for (size_t r = 0; r < nrows; r++) if (K[r + cc * nrows] != col[r]) bad++;
    }
    for (size_t r = 0; r < nrows; r++) {
      f[r] = (T)1;
      c2s::Apply<T, false>(row.data(), f.data(), g[1], taps[1].data(), (int)t, pick);
      f[r] = (T)0;
      for (size_t cc = 0; cc < ncols; cc++) if (K[r + cc * nrows] != row[cc]) bad++;
    }
    if (bad) { ok = false; std::printf("FAIL %s: %zu entries differ from the entry list\n", name, bad); }
    else transposed++;
  }
  if (!ok) failures++;
  std::printf("%dx%dx%d window %dx%d stride %dx%d phase %d,%d %s %s: %zu taps, tile %d, worst error / bound %.3Lf, %s\n", c.ny, c.nx, c.L, c.ky, c.kx, c.sy, c.sx, c.py, c.px,
              shape_name[c.shape], name, t, pick, worst, ok ? "within" : "FAIL");
}

int main() {
  // the tile table: every argument combination has an entry, and no staged tile passes 64 KiB
  size_t most_forward = 0, most_adjoint = 0;
  for (size_t bytes : {sizeof(float), sizeof(double)})
    for (int sy = 1; sy <= c2s::kMaxStride; sy++)
      for (int sx = 1; sx <= c2s::kMaxStride; sx++)
        for (int ky = 1; ky <= c2s::kMaxWindow; ky++)
          for (int kx = 1; kx <= c2s::kMaxWindow; kx++) {
            const int pick = c2s::PickTile(bytes, sy, sx, ky, kx);
            if (pick < 0) { std::printf("FAIL: no tile for %zu bytes, stride %d x %d, window %d x %d\n", bytes, sy, sx, ky, kx); return 1; }
            const size_t lds = c2s::ForwardLdsElements(c2s::kTiles[pick], ky, kx, sy, sx) * bytes;
            if (lds > most_forward) most_forward = lds;
            c2s::Geometry g = c2s::MakeGeometry(c2d::kFull, 64, 64, ky, kx, sy, sx, 0, 0, 1, true);
            for (g.py = 0; g.py < sy; g.py++)
              for (g.oy = 0; g.oy < ky; g.oy++) {
                const size_t adj = (size_t)c2s::AdjointPitch(g) * (size_t)c2s::AdjointColumnBound(g) * bytes;
                if (adj > most_adjoint) most_adjoint = adj;
              }
          }
  if (most_forward > c2s::kLdsLimit || most_adjoint > c2s::kLdsLimit) { std::printf("FAIL: a staged tile of %zu / %zu bytes\n", most_forward, most_adjoint); return 1; }
  std::printf("largest staged tile: forward %zu bytes, adjoint %zu bytes\n", most_forward, most_adjoint);
  // ny, nx, L, ky, kx, sy, sx, py, px, shape (0 full, 1 same, 2 valid), zero taps
  const Case cases[] = {
      {1, 1, 1, 1, 1, 1, 1, 0, 0, 1, false},      {1, 1, 1, 3, 3, 4, 4, 0, 0, 1, false},      {7, 5, 1, 1, 1, 2, 2, 1, 1, 1, false},      {7, 5, 1, 1, 1, 4, 4, 3, 3, 0, false},
      {7, 5, 1, 3, 3, 2, 2, 0, 0, 0, false},      {7, 5, 1, 2, 5, 3, 2, 2, 1, 1, false},      {7, 5, 1, 5, 4, 1, 3, 0, 1, 2, true},       {17, 13, 3, 3, 3, 1, 1, 0, 0, 0, false},
      {17, 13, 3, 2, 5, 2, 2, 1, 0, 2, false},    {17, 13, 3, 5, 4, 3, 2, 0, 1, 1, true},     {17, 13, 3, 9, 9, 4, 4, 3, 3, 0, false},    {17, 13, 3, 9, 9, 1, 3, 0, 0, 1, false},
      {12, 11, 2, 3, 3, 3, 2, 1, 0, 1, false},    {5, 4, 1, 5, 4, 2, 2, 0, 0, 2, true},       {9, 6, 1, 31, 31, 4, 4, 3, 3, 1, false},    {9, 6, 1, 31, 31, 1, 1, 0, 0, 0, false},
      {253, 61, 1, 3, 3, 4, 4, 0, 0, 1, false},   {257, 65, 1, 3, 3, 4, 4, 0, 0, 1, false},   {64, 16, 1, 3, 3, 1, 1, 0, 0, 1, false},    {65, 17, 1, 5, 4, 1, 1, 0, 0, 1, true},
      {129, 33, 1, 9, 9, 2, 2, 0, 0, 1, false},   {125, 13, 1, 31, 31, 4, 4, 0, 0, 1, true},  {129, 17, 1, 31, 31, 4, 4, 1, 2, 1, true},  {300, 20, 2, 5, 4, 3, 2, 1, 1, 0, true}};
  unsigned seed = 1;
  for (const Case& c : cases) {
    run<float>("fp32", c, seed++);
    run<double>("fp64", c, seed++);
  }
  if (failures) { std::printf("%d runs failed\n", failures); return 1; }
  std::printf("entry list and transpose reproduced entry for entry in %d runs\nok\n", transposed);
  return 0;
}
