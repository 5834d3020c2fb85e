// dataterm_sublabel_harness.cpp -- include/prost/linop/dataterm_sublabel.hpp on the host, stand-alone (plain g++, no HIP), meant to be
// built with -fsanitize=address,undefined -ffp-contract=off: the two marches (element access and a two-pixel access, accumulating and
// not) and the four sum formulas, in fp32 and fp64, against a long-double evaluation of the matrix
//
//   r_i = delta u_i + gamma_i w_i - delta sum_{j > i} w_j,   s_i = -w_i          (rows)
//   u_i = delta r_i,   w_i = gamma_i r_i - s_i - delta sum_{j < i} r_j          (columns)
//
// within |got - exact| <= 1.01 (k + 2) u (|K| |x|) componentwise, u the unit roundoff of T (the forward error bound of a sum of k + 1
// terms in any order), and <K x, y> = <x, K^T y> within the same bound carried through the inner products.  Every buffer is allocated
// at exactly its size, so a march that leaves its planes is an AddressSanitizer report.
// Prints one line per shape and precision ending in `within`, then `ok`; exit status 1 on any failure.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "prost/linop/dataterm_sublabel.hpp"

namespace dts = prost::dataterm_sublabel;
typedef long double ld;

struct PairAccess {
  template <class T> static void Load(const T* p, T (&v)[2]) { v[0] = p[0]; v[1] = p[1]; }
  template <class T> static void Store(T* p, const T (&v)[2]) { p[0] = v[0]; p[1] = v[1]; }
};

static int failures = 0;

template <class T, bool ACC>
static void apply(bool transpose, bool pairs, T* res, const T* rhs, size_t N, size_t k, T delta, const T* gamma) {
  if (pairs) {
    for (size_t p = 0; p < N; p += 2) {
      if (transpose) dts::Adjoint<T, 2, ACC, PairAccess>(res, rhs, N, k, p, delta, gamma);
      else dts::Forward<T, 2, ACC, PairAccess>(res, rhs, N, k, p, delta, gamma);
    }
  } else {
    for (size_t p = 0; p < N; p++) {
      if (transpose) dts::Adjoint<T, 1, ACC, dts::ElementAccess>(res, rhs, N, k, p, delta, gamma);
      else dts::Forward<T, 1, ACC, dts::ElementAccess>(res, rhs, N, k, p, delta, gamma);
    }
  }
}

/// exact product and |K| |x| in long double, from the T-rounded delta and gamma
template <class T>
static void exact(bool transpose, const std::vector<T>& x, size_t N, size_t k, T delta, const std::vector<T>& gamma, std::vector<ld>& val, std::vector<ld>& mag) {
  val.assign(2 * N * k, 0);
  mag.assign(2 * N * k, 0);
  const ld d = delta;
  for (size_t p = 0; p < N; p++)
    for (size_t i = 0; i < k; i++) {
      const size_t a = i * N + p, b = N * k + i * N + p;
      const ld g = gamma[i];
      if (!transpose) {
        ld v = d * (ld)x[a] + g * (ld)x[b], m = std::fabs(d * (ld)x[a]) + std::fabs(g * (ld)x[b]);
        for (size_t j = i + 1; j < k; j++) { v -= d * (ld)x[N * k + j * N + p]; m += std::fabs(d * (ld)x[N * k + j * N + p]); }
        val[a] = v; mag[a] = m;
        val[b] = -(ld)x[b]; mag[b] = std::fabs((ld)x[b]);
      } else {
        val[a] = d * (ld)x[a]; mag[a] = std::fabs(d * (ld)x[a]);
        ld v = g * (ld)x[a] - (ld)x[b], m = std::fabs(g * (ld)x[a]) + std::fabs((ld)x[b]);
        for (size_t j = 0; j < i; j++) { v -= d * (ld)x[j * N + p]; m += std::fabs(d * (ld)x[j * N + p]); }
        val[b] = v; mag[b] = m;
      }
    }
}

template <class T>
static void run_shape(const char* name, size_t N, size_t L, double left, double right, unsigned seed) {
  const size_t k = L - 1, n = 2 * N * k;
  const ld u = (ld)std::numeric_limits<T>::epsilon() / 2, fac = 1.01L * (ld)(k + 2) * u;
  std::mt19937_64 gen(seed);
  std::normal_distribution<double> normal(0.0, 1.0);
  T delta;
  std::vector<T> gamma(k);
  dts::Labels<T>(L, left, right, delta, gamma.data());
  bool ok = true;
  ld worst = 0;
  std::vector<T> x(n), y(n), res0(n);
  for (size_t i = 0; i < n; i++) { x[i] = (T)normal(gen); y[i] = (T)normal(gen); res0[i] = (T)normal(gen); }
  std::vector<ld> kx, kx_mag, kty, kty_mag;
  for (int transpose = 0; transpose < 2; transpose++) {
    const std::vector<T>& in = transpose ? y : x;
    std::vector<ld>& val = transpose ? kty : kx;
    std::vector<ld>& mag = transpose ? kty_mag : kx_mag;
    exact<T>(transpose != 0, in, N, k, delta, gamma, val, mag);
    std::vector<T> plain(n, (T)77);
    apply<T, false>(transpose != 0, false, plain.data(), in.data(), N, k, delta, gamma.data());
    for (size_t i = 0; i < n; i++) {
      const ld err = std::fabs((ld)plain[i] - val[i]), bound = fac * mag[i];
      if (!(err <= bound)) { ok = false; std::printf("FAIL %s transpose=%d element %zu: error %Lg, bound %Lg\n", name, transpose, i, err, bound); }
      if (bound > 0 && err / bound > worst) worst = err / bound;
    }
    // the accumulating form stores res0 + value, value as above
    std::vector<T> acc(res0);
    apply<T, true>(transpose != 0, false, acc.data(), in.data(), N, k, delta, gamma.data());
    for (size_t i = 0; i < n; i++)
      if (acc[i] != (T)(res0[i] + plain[i])) { ok = false; std::printf("FAIL %s transpose=%d element %zu: accumulating form\n", name, transpose, i); }
    // in place: res == rhs
    std::vector<T> inplace(in);
    apply<T, false>(transpose != 0, false, inplace.data(), inplace.data(), N, k, delta, gamma.data());
    for (size_t i = 0; i < n; i++)
      if (inplace[i] != plain[i]) { ok = false; std::printf("FAIL %s transpose=%d element %zu: in place\n", name, transpose, i); }
    // two pixels per step give the same bits
    if (N % 2 == 0) {
      std::vector<T> two(n, (T)77), two_acc(res0);
      apply<T, false>(transpose != 0, true, two.data(), in.data(), N, k, delta, gamma.data());
      apply<T, true>(transpose != 0, true, two_acc.data(), in.data(), N, k, delta, gamma.data());
      for (size_t i = 0; i < n; i++)
        if (two[i] != plain[i] || two_acc[i] != acc[i]) { ok = false; std::printf("FAIL %s transpose=%d element %zu: two pixels per step\n", name, transpose, i); }
    }
  }
  // <K x, y> = <x, K^T y>: both from the marches' results, the bound carried through the inner products
  {
    std::vector<T> fx(n), ay(n);
    apply<T, false>(false, false, fx.data(), x.data(), N, k, delta, gamma.data());
    apply<T, false>(true, false, ay.data(), y.data(), N, k, delta, gamma.data());
    ld lhs = 0, rhs = 0, bound = 0;
    for (size_t i = 0; i < n; i++) {
      lhs += (ld)fx[i] * (ld)y[i];
      rhs += (ld)x[i] * (ld)ay[i];
      bound += fac * (kx_mag[i] * std::fabs((ld)y[i]) + kty_mag[i] * std::fabs((ld)x[i]));
    }
    if (!(std::fabs(lhs - rhs) <= bound)) { ok = false; std::printf("FAIL %s: <Kx, y> = %Lg, <x, K^T y> = %Lg, bound %Lg\n", name, lhs, rhs, bound); }
  }
  // the sum formulas against the sums of the matrix, alpha = 1 and 0.5: pow is a library call, the additions are at most k + 1
  for (double alpha : {1.0, 0.5}) {
    const ld tol = (ld)(k + 8) * std::numeric_limits<T>::epsilon();
    const ld pd = std::pow((ld)std::fabs((ld)delta), (ld)alpha);
    for (size_t i = 0; i < k; i++) {
      const ld pg = gamma[i] == 0 ? 0 : std::pow((ld)std::fabs((ld)gamma[i]), (ld)alpha);
      const ld row_r = pd + pg + (ld)(k - 1 - i) * pd, col_w = pg + 1 + (ld)i * pd;
      const ld got[4] = {(ld)dts::RowSumR<T>(i, k, delta, gamma[i], (T)alpha), (ld)dts::RowSumS<T>((T)alpha), (ld)dts::ColSumU<T>(delta, (T)alpha),
                         (ld)dts::ColSumW<T>(i, delta, gamma[i], (T)alpha)};
      const ld want[4] = {row_r, 1, pd, col_w};
      for (int q = 0; q < 4; q++)
        if (!(std::fabs(got[q] - want[q]) <= tol * want[q])) { ok = false; std::printf("FAIL %s: sum %d of plane %zu, alpha %g: %Lg, expected %Lg\n", name, q, i, alpha, got[q], want[q]); }
    }
  }
  if (!ok) failures++;
  std::printf("N=%zu L=%zu [%g, %g] %s: worst error / bound %.3Lf, %s\n", N, L, left, right, name, worst, ok ? "within" : "FAIL");
}

int main() {
  struct Shape { size_t N, L; double left, right; };
  // k = 1 and N = 1 included; left = 0: gamma_0 = 0 is an absent entry; an odd N (no two-pixel pass) and even ones
  const Shape shapes[] = {{1, 2, 0.0, 1.0}, {1, 3, -0.3, 1.1}, {1, 9, 0.25, 2.25}, {2, 2, -1.0, 0.5}, {5, 4, 0.0, 1.0}, {7, 2, 0.1, 0.7},
                          {38, 9, -0.3, 1.1}, {4, 33, 0.0, 255.0}, {64, 5, 1.0, 3.0}};
  unsigned seed = 1;
  for (const Shape& s : shapes) {
    run_shape<float>("fp32", s.N, s.L, s.left, s.right, seed++);
    run_shape<double>("fp64", s.N, s.L, s.left, s.right, seed++);
  }
  if (failures) { std::printf("%d shapes failed\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
