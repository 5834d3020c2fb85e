// sym_gradient2d_harness.cpp -- include/prost/linop/sym_gradient2d.hpp on the host, stand-alone (plain g++, no HIP), meant to be built
// with -fsanitize=address,undefined -ffp-contract=off: the forward and the adjoint march for W = 1, 2 and 4 rows per lane
// (accumulating and not), and the closed-form row / column sums, in fp32 and fp64, against the explicit matrix
//
//   E = [ kron(I, Bx)  0 ; 0  kron(I, By) ; w kron(I, By)  w kron(I, Bx) ],   (Bx v)(y, x) = [x < nx-1] v(y, x) - [x > 0] v(y, x-1),
//                                                                             (By v)(y, x) = [y < ny-1] v(y, x) - [y > 0] v(y-1, x)
//
// written here entry by entry and summed in long double: |got - exact| <= 1.01 (t + 1) u (|E| |x|) componentwise, t = 4, u the unit
// roundoff of T (the forward error bound of a t-term sum of rounded products).  The adjoint march is held against the transpose of
// the SAME entries, and at the small shapes both marches are applied to unit vectors: the adjoint has to be the transpose of the
// forward matrix entry for entry, and the forward matrix has to be the entry list.  The marches of every W and of narrow strips and
// forced chunk widths give the bits of W = 1.  The sums have to be within (t + 8) eps_T of the sums of the entries in long double
// (w = 0.5, alpha = 1: equal).  Every buffer is allocated at exactly its size, so a march that leaves its planes is an
// AddressSanitizer report.  Prints one line per shape, weight and precision ending in `within`, then `ok`; exit status 1 on any failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "prost/linop/sym_gradient2d.hpp"

namespace sg2 = prost::sym_gradient2d;
typedef long double ld;

static int failures = 0, transposed = 0;

struct Case { size_t ny, nx, L; };
struct Entry { size_t r, c; int sign; bool weighted; };

/// the entries of E, row by row in ascending column order
static std::vector<Entry> entries(const Case& k) {
  std::vector<Entry> e;
  const size_t N = k.nx * k.ny, L = k.L;
  for (size_t c = 0; c < L; c++)
    for (size_t x = 0; x < k.nx; x++)
      for (size_t y = 0; y < k.ny; y++) {
        const size_t p = y + x * k.ny;
        const bool ax = x + 1 < k.nx, bx = x > 0, ay = y + 1 < k.ny, by = y > 0;
        if (bx) e.push_back({c * N + p, c * N + p - k.ny, -1, false});
        if (ax) e.push_back({c * N + p, c * N + p, +1, false});
        if (by) e.push_back({(L + c) * N + p, (L + c) * N + p - 1, -1, false});
        if (ay) e.push_back({(L + c) * N + p, (L + c) * N + p, +1, false});
        if (by) e.push_back({(2 * L + c) * N + p, c * N + p - 1, -1, true});
        if (ay) e.push_back({(2 * L + c) * N + p, c * N + p, +1, true});
        if (bx) e.push_back({(2 * L + c) * N + p, (L + c) * N + p - k.ny, -1, true});
        if (ax) e.push_back({(2 * L + c) * N + p, (L + c) * N + p, +1, true});
      }
  return e;
}

template <class T, int W>
static void product(std::vector<T>& out, const std::vector<T>& in, const Case& k, double w, bool transpose, bool acc, int lanes = 256, int force_cols = 0) {
  if (acc) sg2::Apply<T, W, true>(out.data(), in.data(), k.nx, k.ny, k.L, w, transpose, lanes, force_cols);
  else sg2::Apply<T, W, false>(out.data(), in.data(), k.nx, k.ny, k.L, w, transpose, lanes, force_cols);
}

template <class T>
static void run(const char* name, const Case& k, double w, unsigned seed) {
  std::mt19937_64 gen(seed);
  std::normal_distribution<double> normal(0.0, 1.0);
  const size_t N = k.nx * k.ny, nrows = 3 * k.L * N, ncols = 2 * k.L * N;
  const std::vector<Entry> E = entries(k);
  const T wt = sg2::RoundWeight<T>(w);
  const ld u = (ld)std::numeric_limits<T>::epsilon() / 2, fac = 1.01L * (ld)(sg2::kTerms + 1) * u;
  bool ok = true;
  ld worst = 0;
  std::vector<T> x(ncols), y(nrows), res0(nrows), res1(ncols);
  for (T& v : x) v = (T)normal(gen);
  for (T& v : y) v = (T)normal(gen);
  for (T& v : res0) v = (T)normal(gen);
  for (T& v : res1) v = (T)normal(gen);
  std::vector<T> plain(nrows, (T)77), acc(res0), plain_t(ncols, (T)77), acc_t(res1);
  product<T, 1>(plain, x, k, w, false, false);
  product<T, 1>(acc, x, k, w, false, true);
  product<T, 1>(plain_t, y, k, w, true, false);
  product<T, 1>(acc_t, y, k, w, true, true);
  std::vector<ld> val(nrows, 0), mag(nrows, 0), val_t(ncols, 0), mag_t(ncols, 0);
  for (const Entry& e : E) {
    const ld a = (ld)e.sign * (e.weighted ? (ld)wt : 1.0L);
    val[e.r] += a * (ld)x[e.c]; mag[e.r] += std::fabs(a * (ld)x[e.c]);
    val_t[e.c] += a * (ld)y[e.r]; mag_t[e.c] += std::fabs(a * (ld)y[e.r]);
  }
  for (size_t r = 0; r < nrows; r++) {
    const ld err = std::fabs((ld)plain[r] - val[r]), bound = fac * mag[r];
    if (!(err <= bound)) { ok = false; std::printf("FAIL %s element %zu: error %Lg, bound %Lg\n", name, r, err, bound); }
    if (bound > 0 && err / bound > worst) worst = err / bound;
    if (acc[r] != (T)(res0[r] + plain[r])) { ok = false; std::printf("FAIL %s element %zu: accumulating form\n", name, r); }
  }
  for (size_t c = 0; c < ncols; c++) {
    const ld err = std::fabs((ld)plain_t[c] - val_t[c]), bound = fac * mag_t[c];
    if (!(err <= bound)) { ok = false; std::printf("FAIL %s adjoint element %zu: error %Lg, bound %Lg\n", name, c, err, bound); }
    if (bound > 0 && err / bound > worst) worst = err / bound;
    if (acc_t[c] != (T)(res1[c] + plain_t[c])) { ok = false; std::printf("FAIL %s adjoint element %zu: accumulating form\n", name, c); }
  }
  // the vector widths, narrow strips (4 lanes: several strips and the edge-lane reads at small heights) and forced chunk widths (the
  // halo column kept from the neighbouring step): the bits of W = 1
  const int lanes[3] = {256, 4, 1}, widths[3] = {0, 3, 2};
  for (int v = 0; v < (N <= 20000 ? 3 : 1); v++) {
    std::vector<T> a2(nrows, (T)5), a4(nrows, (T)5), b2(ncols, (T)5), b4(ncols, (T)5), c4(res0), d4(res1);
    product<T, 2>(a2, x, k, w, false, false, lanes[v], widths[v]);
    product<T, 4>(a4, x, k, w, false, false, lanes[v], widths[v]);
    product<T, 2>(b2, y, k, w, true, false, lanes[v], widths[v]);
    product<T, 4>(b4, y, k, w, true, false, lanes[v], widths[v]);
    product<T, 4>(c4, x, k, w, false, true, lanes[v], widths[v]);
    product<T, 4>(d4, y, k, w, true, true, lanes[v], widths[v]);
    if (a2 != plain || a4 != plain || b2 != plain_t || b4 != plain_t || c4 != acc || d4 != acc_t) {
      ok = false; std::printf("FAIL %s: W = 2 / 4 with %d lanes and chunk width %d differ from W = 1\n", name, lanes[v], widths[v]);
    }
  }
  // the sums, alpha = 1 and 0.5, against the sums of the entries in long double
  const double alphas[2] = {1.0, 0.5};
  for (int a = 0; a < 2; a++) {
    const ld tol = (ld)(sg2::kTerms + 8) * std::numeric_limits<T>::epsilon();
    const double wa = sg2::WeightPower((double)wt, alphas[a]);
    std::vector<ld> rs(nrows, 0), cs(ncols, 0);
    for (const Entry& e : E) { const ld pw = e.weighted ? std::pow(std::fabs((ld)wt), (ld)alphas[a]) : 1.0L; rs[e.r] += pw; cs[e.c] += pw; }
    const bool exact = w == 0.5 && alphas[a] == 1.0;
    std::vector<T> bulk_r(nrows, (T)0), bulk_c(ncols, (T)0);                     // the bulk forms give the single-row forms
    sg2::RowSums<T>(bulk_r.data(), k.nx, k.ny, k.L, wa);
    sg2::ColSums<T>(bulk_c.data(), k.nx, k.ny, k.L, wa);
    for (size_t r = 0; r < nrows; r++) if (bulk_r[r] != (T)sg2::RowSum(r, k.nx, k.ny, k.L, wa)) { ok = false; std::printf("FAIL %s: bulk row sum %zu\n", name, r); }
    for (size_t c = 0; c < ncols; c++) if (bulk_c[c] != (T)sg2::ColSum(c, k.nx, k.ny, k.L, wa)) { ok = false; std::printf("FAIL %s: bulk column sum %zu\n", name, c); }
    for (size_t r = 0; r < nrows; r++) {
      const ld got = (ld)(T)sg2::RowSum(r, k.nx, k.ny, k.L, wa);
      if (!(std::fabs(got - rs[r]) <= tol * rs[r]) || (exact && got != rs[r])) { ok = false; std::printf("FAIL %s: row sum %zu, alpha %g: %Lg, expected %Lg\n", name, r, alphas[a], got, rs[r]); }
    }
    for (size_t c = 0; c < ncols; c++) {
      const ld got = (ld)(T)sg2::ColSum(c, k.nx, k.ny, k.L, wa);
      if (!(std::fabs(got - cs[c]) <= tol * cs[c]) || (exact && got != cs[c])) { ok = false; std::printf("FAIL %s: column sum %zu, alpha %g: %Lg, expected %Lg\n", name, c, alphas[a], got, cs[c]); }
    }
  }
  // unit vectors: the forward march is the entry list, the adjoint march its transpose, entry for entry
  if (nrows * ncols <= (size_t)1 << 19) {
    std::vector<T> K(nrows * ncols), want(nrows * ncols, (T)0), e(ncols, (T)0), f(nrows, (T)0), col(nrows), row(ncols);
    for (const Entry& q : E) want[q.r + q.c * nrows] = (T)q.sign * (q.weighted ? wt : (T)1);
    for (size_t c = 0; c < ncols; c++) {
      e[c] = (T)1;
      product<T, 4>(col, e, k, w, false, false, 4, 2);
      e[c] = (T)0;
      for (size_t r = 0; r < nrows; r++) K[r + c * nrows] = col[r];
    }
    size_t bad = 0;
    for (size_t i = 0; i < K.size(); i++) if (K[i] != want[i]) bad++;
    for (size_t r = 0; r < nrows; r++) {
      f[r] = (T)1;
      product<T, 4>(row, f, k, w, true, false, 4, 2);
      f[r] = (T)0;
      for (size_t c = 0; c < ncols; c++) if (K[r + c * nrows] != row[c]) bad++;
    }
    if (bad) { ok = false; std::printf("FAIL %s: %zu entries of the marches differ from the matrix or its transpose\n", name, bad); }
    else transposed++;
  }
  if (!ok) failures++;
  std::printf("%zux%zux%zu w %.3f %s: %zu entries, worst error / bound %.3Lf, %s\n", k.ny, k.nx, k.L, w, name, E.size(), worst, ok ? "within" : "FAIL");
}

int main() {
  // the shape list of tests/test_gpu_sym_gradient2d.py (tests/sym_gradient2d_reference.py): 1 x 1, single rows and columns, small
  // grids, a height that is no multiple of the vector width, one strip of the vector path and one row / one vector more in both
  // precisions, every chunk width with all chunks full and with one column more
  const Case cases[] = {{1, 1, 1}, {1, 7, 1}, {5, 1, 1}, {2, 2, 1}, {3, 3, 2}, {17, 13, 3}, {66, 5, 1},
                        {512, 3, 1}, {513, 3, 1}, {514, 3, 1}, {1024, 3, 1}, {1025, 3, 1}, {1028, 2, 2},
                        {4, 6144, 1}, {4, 6145, 1}, {4, 12288, 1}, {4, 12289, 1}, {4, 24576, 1}, {4, 24577, 1}, {8, 4097, 3}};
  unsigned seed = 1;
  for (const Case& c : cases)
    for (double w : {0.5, std::sqrt(0.5)}) {
      run<float>("fp32", c, w, seed++);
      run<double>("fp64", c, w, seed++);
    }
  if (failures) { std::printf("%d runs failed\n", failures); return 1; }
  std::printf("marches equal to the matrix and its transpose entry for entry in %d runs\nok\n", transposed);
  return 0;
}
