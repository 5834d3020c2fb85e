// conv2d_harness.cpp -- include/prost/linop/conv2d.hpp on the host, stand-alone (plain g++, no HIP), meant to be built with
// -fsanitize=address,undefined -ffp-contract=off: the geometry, the tap compaction, the march over staged tiles (accumulating and not)
// and the row / column sums, in fp32 and fp64, against the explicit sum
//
//   out(y, x) = sum over taps (i, j) with 0 <= y + oy - i < ny, 0 <= x + ox - j < nx  of  k(i, j) in(y + oy - i, x + ox - j)
//
// in long double: |got - exact| <= 1.01 (t + 1) u (|K| |x|) componentwise, t the non-zero tap count, u the unit roundoff of T (the
// forward error bound of a t-term sum of rounded products in any order).  The adjoint, which runs from the flipped table with the
// mirrored geometry, is held against the transpose of the forward definition within the same bound at every shape, and at the small
// shapes it has to be the transpose of the forward matrix entry for entry: both matrices are read off the marches by applying them to
// unit vectors.  The sums have to be within (t + 8) eps_T of the sums of the matrix in long double.  Every buffer is allocated
// at exactly its size, so a march that leaves its planes is an AddressSanitizer report.
// Prints one line per shape and precision ending in `within`, then `ok`; exit status 1 on any failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "prost/linop/conv2d.hpp"

namespace c2d = prost::conv2d;
typedef long double ld;

static int failures = 0, transposed = 0;

struct Case { int ny, nx, L, ky, kx; bool motion; };

/// a sparse window in the manner of the motion window of examples/deblurring.py: two neighbouring anti-diagonals, everything else zero
static std::vector<double> line_window(int k) {
  std::vector<double> w((size_t)(k * k), 0.0);
  for (int i = 0; i < k; i++) { w[(size_t)(i + (k - 1 - i) * k)] = 0.04 + 0.001 * i; if (i + 1 < k) w[(size_t)(i + 1 + (k - 1 - i) * k)] = 0.013; }
  return w;
}

template <class T>
static void run(const char* name, const Case& c, int shape, unsigned seed) {
  static const char* shape_name[] = {"full", "same", "valid"};
  long my, mx, oy, ox;
  if (!c2d::OutputSize(shape, c.ny, c.nx, c.ky, c.kx, my, mx, oy, ox)) return;      // "valid" with a window larger than the image
  std::mt19937_64 gen(seed);
  std::normal_distribution<double> normal(0.0, 1.0);
  std::vector<double> kernel = c.motion ? line_window(c.ky) : std::vector<double>((size_t)(c.ky * c.kx));
  if (!c.motion) for (double& v : kernel) v = normal(gen);
  if (!c.motion && c.ky * c.kx > 4) kernel[1] = 0.0;                                // a dropped tap
  const size_t ncols = (size_t)c.L * c.ny * c.nx, nrows = (size_t)c.L * my * mx;
  c2d::Geometry g[2];
  std::vector<T> w[2];
  std::vector<c2d::Tap<T>> taps[2];
  for (int dir = 0; dir < 2; dir++) {
    g[dir] = c2d::MakeGeometry(shape, c.ny, c.nx, c.ky, c.kx, c.L, dir == 1);
    w[dir] = c2d::Window<T>(kernel.data(), c.ky, c.kx, dir == 1);
    taps[dir] = c2d::CompactTaps<T>(w[dir], c.ky, c.kx);
  }
  const size_t t = taps[0].size();
  bool ok = taps[1].size() == t && t > 0;
  for (int dir = 0; dir < 2; dir++)
    for (size_t q = 1; q < taps[dir].size(); q++)
      if (!(taps[dir][q - 1].offset < taps[dir][q].offset)) { ok = false; std::printf("FAIL %s: the taps are not in ascending order\n", name); }
  const ld u = (ld)std::numeric_limits<T>::epsilon() / 2, fac = 1.01L * (ld)(t + 1) * u;
  ld worst = 0;
  // both directions against the explicit sum in long double: the forward product row by row, the adjoint as the transpose of the
  // SAME entries (scattered), so the flipped table and the mirrored geometry are held against the forward definition
  std::vector<T> x(ncols), y(nrows), res0(nrows), res1(ncols);
  for (T& v : x) v = (T)normal(gen);
  for (T& v : y) v = (T)normal(gen);
  for (T& v : res0) v = (T)normal(gen);
  for (T& v : res1) v = (T)normal(gen);
  std::vector<T> plain(nrows, (T)77), acc(res0), plain_t(ncols, (T)77), acc_t(res1);
  c2d::Apply<T, false>(plain.data(), x.data(), g[0], taps[0].data(), (int)t);
  c2d::Apply<T, true>(acc.data(), x.data(), g[0], taps[0].data(), (int)t);
  c2d::Apply<T, false>(plain_t.data(), y.data(), g[1], taps[1].data(), (int)t);
  c2d::Apply<T, true>(acc_t.data(), y.data(), g[1], taps[1].data(), (int)t);
  const double alphas[2] = {1.0, 0.5};
  std::vector<ld> val(nrows, 0), mag(nrows, 0), val_t(ncols, 0), mag_t(ncols, 0), rs_want[2], cs_want[2];
  for (int a = 0; a < 2; a++) { rs_want[a].assign(nrows, 0); cs_want[a].assign(ncols, 0); }
  for (int p = 0; p < c.L; p++)
    for (long xx = 0; xx < mx; xx++)
      for (long yy = 0; yy < my; yy++) {
        const size_t r = (size_t)p * my * mx + (size_t)yy + (size_t)xx * my;
        for (int j = 0; j < c.kx; j++)
          for (int i = 0; i < c.ky; i++) {
            const long sy = yy + oy - i, sx = xx + ox - j;
            const ld k = (ld)w[0][(size_t)(i + j * c.ky)];
            if (sy < 0 || sy >= c.ny || sx < 0 || sx >= c.nx || k == 0) continue;
            const size_t cc = (size_t)p * c.ny * c.nx + (size_t)sy + (size_t)sx * c.ny;
            val[r] += k * (ld)x[cc]; mag[r] += std::fabs(k * (ld)x[cc]);
            val_t[cc] += k * (ld)y[r]; mag_t[cc] += std::fabs(k * (ld)y[r]);
            for (int a = 0; a < 2; a++) { const ld pw = std::pow(std::fabs(k), (ld)alphas[a]); rs_want[a][r] += pw; cs_want[a][cc] += pw; }
          }
      }
  for (size_t r = 0; r < nrows; r++) {
    const ld err = std::fabs((ld)plain[r] - val[r]), bound = fac * mag[r];
    if (!(err <= bound)) { ok = false; std::printf("FAIL %s element %zu: error %Lg, bound %Lg\n", name, r, err, bound); }
    if (bound > 0 && err / bound > worst) worst = err / bound;
    if (acc[r] != (T)(res0[r] + plain[r])) { ok = false; std::printf("FAIL %s element %zu: accumulating form\n", name, r); }
  }
  for (size_t cc = 0; cc < ncols; cc++) {
    const ld err = std::fabs((ld)plain_t[cc] - val_t[cc]), bound = fac * mag_t[cc];
    if (!(err <= bound)) { ok = false; std::printf("FAIL %s adjoint element %zu: error %Lg, bound %Lg\n", name, cc, err, bound); }
    if (bound > 0 && err / bound > worst) worst = err / bound;
    if (acc_t[cc] != (T)(res1[cc] + plain_t[cc])) { ok = false; std::printf("FAIL %s adjoint element %zu: accumulating form\n", name, cc); }
  }
  // the sums, alpha = 1 and 0.5, against the sums of the matrix in long double; the single-row forms add the same terms in another order
  for (int a = 0; a < 2; a++) {
    const ld tol = (ld)(t + 8) * std::numeric_limits<T>::epsilon();
    std::vector<T> rs(nrows, (T)0), cs(ncols, (T)0);
    c2d::RowSums<T>(g[0], w[0], alphas[a], rs.data());
    c2d::RowSums<T>(g[1], w[1], alphas[a], cs.data());
    for (size_t r = 0; r < nrows; r++) {
      const size_t p = r % ((size_t)my * mx);
      const ld one = (ld)c2d::SumAt<T>(g[0], w[0], alphas[a], (int)(p % my), (int)(p / my)), want = rs_want[a][r];
      if (!(std::fabs((ld)rs[r] - want) <= tol * want) || !(std::fabs(one - want) <= tol * want)) {
        ok = false; std::printf("FAIL %s: row sum %zu, alpha %g: %Lg and %Lg, expected %Lg\n", name, r, alphas[a], (ld)rs[r], one, want);
      }
    }
    for (size_t cc = 0; cc < ncols; cc++) {
      const size_t p = cc % ((size_t)c.ny * c.nx);
      const ld one = (ld)c2d::SumAt<T>(g[1], w[1], alphas[a], (int)(p % c.ny), (int)(p / c.ny)), want = cs_want[a][cc];
      if (!(std::fabs((ld)cs[cc] - want) <= tol * want) || !(std::fabs(one - want) <= tol * want)) {
        ok = false; std::printf("FAIL %s: column sum %zu, alpha %g: %Lg and %Lg, expected %Lg\n", name, cc, alphas[a], (ld)cs[cc], one, want);
      }
    }
  }
  // the adjoint is the transpose entry for entry, read off the marches with unit vectors (small shapes)
  if (nrows * ncols <= (size_t)1 << 19 && t <= 32) {
    std::vector<T> K(nrows * ncols), e(ncols, (T)0), f(nrows, (T)0), col(nrows), row(ncols);
    for (size_t cc = 0; cc < ncols; cc++) {
      e[cc] = (T)1;
      c2d::Apply<T, false>(col.data(), e.data(), g[0], taps[0].data(), (int)t);
      e[cc] = (T)0;
      for (size_t r = 0; r < nrows; r++) K[r + cc * nrows] = col[r];
    }
    size_t bad = 0;
    for (size_t r = 0; r < nrows; r++) {
      f[r] = (T)1;
      c2d::Apply<T, false>(row.data(), f.data(), g[1], taps[1].data(), (int)t);
      f[r] = (T)0;
      for (size_t cc = 0; cc < ncols; cc++) if (K[r + cc * nrows] != row[cc]) bad++;
    }
    if (bad) { ok = false; std::printf("FAIL %s: %zu entries of the adjoint differ from the transpose\n", name, bad); }
    else transposed++;
  }
  if (!ok) failures++;
  std::printf("%dx%dx%d window %dx%d%s %s %s: %zu taps, worst error / bound %.3Lf, %s\n", c.ny, c.nx, c.L, c.ky, c.kx, c.motion ? " (line)" : "", shape_name[shape], name, t, worst,
              ok ? "within" : "FAIL");
}

int main() {
  // the shape list of tests/test_gpu_conv2d.py: 1 x 1, single rows and columns, a window larger than the image, an even window on odd
  // planes, one tile of 64 x 16 and one past it in both axes, three planes with a sparse 15 x 15 window, a dense 31 x 31
  const Case cases[] = {{1, 1, 1, 1, 1, false}, {1, 7, 1, 1, 3, false}, {5, 1, 1, 3, 1, false}, {3, 3, 1, 5, 5, false}, {17, 13, 3, 2, 2, false}, {17, 13, 3, 4, 5, false},
                        {64, 16, 1, 3, 3, false}, {65, 17, 1, 3, 3, false}, {130, 35, 3, 15, 15, true}, {40, 33, 1, 31, 31, false}};
  unsigned seed = 1;
  for (const Case& c : cases)
    for (int shape = 0; shape < 3; shape++) {
      run<float>("fp32", c, shape, seed++);
      run<double>("fp64", c, shape, seed++);
    }
  if (failures) { std::printf("%d runs failed\n", failures); return 1; }
  std::printf("adjoint equal to the transpose entry for entry in %d runs\nok\n", transposed);
  return 0;
}
