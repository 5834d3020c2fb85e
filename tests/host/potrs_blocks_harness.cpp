// potrs_blocks_harness.cpp -- the per-block arithmetic of the ProxIndRange solve (include/prost/prox/potrs_blocks.hpp) ON THE HOST.
// The loops below stand where prost_amd/csrc/kernels_prox_range.hip has lanes and barriers: "for every row" is a lane, the end of such
// a loop is a barrier.  Built with plain g++ (-fsanitize=address,undefined in tests/test_range_host.py); no HIP header, no device.
//
//   potrs_blocks_harness <NB of prost_hip_range_potrs_plan>
// For T = float and double and n in {1, 2, NB - 1, NB, NB + 1, 2 NB + 1}:
//   exact family      AA = L L' with L = I + N (N strictly lower, entries +-1 in rows >= n / 2 and columns < n / 2, so N N = 0): the
//                     blocked factor must equal L, the inverted diagonal blocks must equal those of I - N, and the solve of AA x0 for an
//                     integer x0 must return x0 -- all bit for bit
//   tolerance family  AA = I + S'S (S sparse standard normal): the blocked solve in T against an unblocked Cholesky solve in long double; the
//                     yardstick e_T is the error of the same unblocked loop run in T; bound max(4 e_T, 32 eps_T).  Printed for the
//                     factorisation in fp64 (what the library does) and, for T = float, in T (the alternative).
// Prints one line per case and "ok" at the end; any failure prints FAIL and the exit code is 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "prost/prox/potrs_blocks.hpp"

namespace pb = prost::potrs;
static const int NB = pb::kNB;
static int g_fail = 0;

struct Rng {
  uint64_t s;
  explicit Rng(uint64_t seed) : s(seed * 6364136223846793005ull + 1442695040888963407ull) {}
  uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 33); }
  double uniform() { return (next() + 0.5) / 2147483648.0; }
  double normal() { return std::sqrt(-2.0 * std::log(uniform())) * std::cos(6.283185307179586 * uniform()); }
};

// ---- the factorisation as potrf_diag / panel / trailing / finish run it; F = the arithmetic, T = what the solve reads ----
template <class F, class T>
static int factor(std::vector<F>& W, size_t n, std::vector<T>& L, std::vector<T>& U, std::vector<T>& dinv) {
  const size_t nblk = pb::NumBlocks(n);
  const int LD = NB + 1;
  dinv.assign(nblk * 2 * NB * NB, (T)0);
  std::vector<F> D((size_t)NB * LD), col(NB), dinv_f((size_t)NB * NB);
  for (size_t k = 0; k < nblk; k++) {
    const size_t c0 = k * NB;
    const int nb = n - c0 < (size_t)NB ? (int)(n - c0) : NB;
    for (int r = 0; r < NB; r++)
      for (int c = 0; c < NB; c++) D[r + (size_t)c * LD] = (r < nb && c <= r) ? W[(c0 + r) + (c0 + c) * n] : (F)0;
    for (int j = 0; j < nb; j++) {
      if (!pb::CholPivot(D.data(), LD, j)) return (int)(c0 + j);
      for (int r = j + 1; r < nb; r++) pb::CholScaleRow(D.data(), LD, j, r);
      for (int r = j + 1; r < nb; r++) pb::CholUpdateRow(D.data(), LD, j, r);
    }
    for (int r = 0; r < nb; r++)
      for (int c = 0; c <= r; c++) W[(c0 + r) + (c0 + c) * n] = D[r + (size_t)c * LD];
    for (int j = nb - 1; j >= 0; j--) {
      for (int r = j + 1; r < nb; r++) col[r] = pb::TrtiRow(D.data(), LD, j, r);      // every row reads ...
      const F d = pb::TrtiDiag(D.data(), LD, j);
      for (int r = j + 1; r < nb; r++) D[r + (size_t)j * LD] = col[r];               // ... before any row writes
      D[j + (size_t)j * LD] = d;
    }
    T* dk = dinv.data() + k * 2 * NB * NB;
    for (int r = 0; r < NB; r++)
      for (int c = 0; c < NB; c++) {
        dinv_f[r + (size_t)c * NB] = D[r + (size_t)c * LD];
        dk[r + (size_t)c * NB] = (T)D[r + (size_t)c * LD];
        dk[NB * NB + r + (size_t)c * NB] = (T)D[c + (size_t)r * LD];
      }
    const size_t r0 = c0 + NB;
    if (r0 >= n) break;
    for (size_t row = r0; row < n; row++)
      for (int c = NB - 1; c >= 0; c--) W[row + (c0 + c) * n] = pb::PanelEntry(W.data(), n, row, c0, dinv_f.data(), NB, c);
    for (size_t row = r0; row < n; row++)
      for (size_t c = r0; c <= row; c++) W[row + c * n] -= pb::TrailingDot(W.data(), n, row, c, c0, NB);
  }
  L.assign(n * n, (T)0); U.assign(n * n, (T)0);
  for (size_t c = 0; c < n; c++)
    for (size_t i = c; i < n; i++) { L[i + c * n] = (T)W[i + c * n]; U[c + i * n] = (T)W[i + c * n]; }
  return -1;
}

// ---- one block step: z = Dk r (block_solve), then the rows [r0, r1) lose M[i, block] z (rows_update) ----
template <class T>
static void block_step(const T* Dk, const T* M, size_t n, size_t c0, int nb, size_t r0, size_t r1, const T* in, T* out, T* vec) {
  T s_in[pb::kNB], z[pb::kNB];
  for (int t = 0; t < NB; t++) s_in[t] = t < nb ? in[c0 + t] : (T)0;
  for (int r = 0; r < NB; r++) {
    T p[pb::kGroups];
    for (int g = 0; g < pb::kGroups; g++) p[g] = pb::BlockRow(Dk, (size_t)NB, (size_t)r, (size_t)0, g, NB, s_in);
    z[r] = pb::Combine4(p[0], p[1], p[2], p[3]);
  }
  for (int t = 0; t < nb; t++) out[c0 + t] = z[t];
  for (size_t i = r0; i < r1; i++) {
    T p[pb::kGroups];
    for (int g = 0; g < pb::kGroups; g++) p[g] = pb::BlockRow(M, n, i, c0, g, nb, z);
    vec[i] = vec[i] - pb::Combine4(p[0], p[1], p[2], p[3]);
  }
}
// the large tier's data flow (v -> w forward, w -> v backward); the small tier runs the same arithmetic in place
template <class T>
static void solve(std::vector<T>& v, const std::vector<T>& L, const std::vector<T>& U, const std::vector<T>& dinv, size_t n) {
  const size_t nblk = pb::NumBlocks(n);
  std::vector<T> w(n, (T)0);
  for (size_t k = 0; k < nblk; k++) {
    const size_t c0 = k * NB;
    const int nb = n - c0 < (size_t)NB ? (int)(n - c0) : NB;
    block_step<T>(dinv.data() + k * 2 * NB * NB, L.data(), n, c0, nb, c0 + NB < n ? c0 + NB : n, n, v.data(), w.data(), v.data());
  }
  for (size_t k = nblk; k-- > 0;) {
    const size_t c0 = k * NB;
    const int nb = n - c0 < (size_t)NB ? (int)(n - c0) : NB;
    block_step<T>(dinv.data() + k * 2 * NB * NB + NB * NB, U.data(), n, c0, nb, 0, c0, w.data(), v.data(), w.data());
  }
}

// ---- the unblocked reference loop ----
template <class F>
static bool reference_solve(std::vector<F> A, std::vector<F>& x, size_t n) {
  for (size_t j = 0; j < n; j++) {
    F d = A[j + j * n];
    for (size_t k = 0; k < j; k++) d -= A[j + k * n] * A[j + k * n];
    if (!(d > 0)) return false;
    d = std::sqrt(d);
    A[j + j * n] = d;
    for (size_t i = j + 1; i < n; i++) {
      F s = A[i + j * n];
      for (size_t k = 0; k < j; k++) s -= A[i + k * n] * A[j + k * n];
      A[i + j * n] = s / d;
    }
  }
  for (size_t i = 0; i < n; i++) {
    F s = x[i];
    for (size_t k = 0; k < i; k++) s -= A[i + k * n] * x[k];
    x[i] = s / A[i + i * n];
  }
  for (size_t i = n; i-- > 0;) {
    F s = x[i];
    for (size_t k = i + 1; k < n; k++) s -= A[k + i * n] * x[k];
    x[i] = s / A[i + i * n];
  }
  return true;
}

template <class T>
static void exact_case(size_t n, const char* tname) {
  Rng rng(1000 + n);
  const size_t h = n / 2, cap = h * (n - h), want = 3 * n < cap ? 3 * n : cap;
  std::vector<double> Lt(n * n, 0.0);
  for (size_t i = 0; i < n; i++) Lt[i + i * n] = 1.0;
  for (size_t placed = 0; placed < want;) {
    const size_t i = h + rng.next() % (n - h), c = rng.next() % h;
    if (Lt[i + c * n] != 0.0) continue;
    Lt[i + c * n] = (rng.next() & 1) ? 1.0 : -1.0;
    placed++;
  }
  std::vector<double> AA(n * n, 0.0);
  for (size_t i = 0; i < n; i++)
    for (size_t j = 0; j < n; j++) {
      double s = 0;
      for (size_t k = 0; k < n; k++) s += Lt[i + k * n] * Lt[j + k * n];
      AA[i + j * n] = s;
    }
  std::vector<double> W(AA);
  std::vector<T> L, U, dinv;
  const int info = factor<double, T>(W, n, L, U, dinv);
  bool ok = info == -1;
  for (size_t e = 0; ok && e < n * n; e++) ok = (double)L[e] == Lt[e] && (double)U[(e % n) * n + e / n] == Lt[e];
  // the inverse of a diagonal block of I + N is that block of I - N (the blocks of N that lie on the diagonal are zero or square to zero)
  for (size_t k = 0; ok && k < pb::NumBlocks(n); k++)
    for (int r = 0; ok && r < NB; r++)
      for (int c = 0; ok && c < NB; c++) {
        const size_t i = k * NB + r, j = k * NB + c;
        const double wantv = (i < n && j < n) ? (i == j ? 1.0 : -Lt[i + j * n]) : 0.0;
        ok = (double)dinv[k * 2 * NB * NB + r + (size_t)c * NB] == wantv && (double)dinv[k * 2 * NB * NB + NB * NB + c + (size_t)r * NB] == wantv;
      }
  std::vector<T> x0(n), v(n);
  for (size_t i = 0; i < n; i++) x0[i] = (T)((int)(rng.next() % 17) - 8);
  for (size_t i = 0; i < n; i++) {
    double s = 0;
    for (size_t j = 0; j < n; j++) s += AA[i + j * n] * (double)x0[j];
    v[i] = (T)s;
  }
  if (ok) solve<T>(v, L, U, dinv, n);
  for (size_t i = 0; ok && i < n; i++) ok = v[i] == x0[i];
  std::printf("exact %s n=%zu: %s\n", tname, n, ok ? "equal" : "FAIL");
  if (!ok) g_fail = 1;
}

template <class T, class F>
static double blocked_error(const std::vector<double>& AA, const std::vector<double>& rhs, const std::vector<double>& truth, size_t n) {
  std::vector<F> W(n * n);
  for (size_t e = 0; e < n * n; e++) W[e] = (F)(T)AA[e];
  std::vector<T> L, U, dinv, v(n);
  if (factor<F, T>(W, n, L, U, dinv) != -1) return std::numeric_limits<double>::infinity();
  for (size_t i = 0; i < n; i++) v[i] = (T)rhs[i];
  solve<T>(v, L, U, dinv, n);
  double err = 0, scale = 0;
  for (size_t i = 0; i < n; i++) { err = std::fmax(err, std::fabs((double)v[i] - truth[i])); scale = std::fmax(scale, std::fabs(truth[i])); }
  return err / scale;
}

template <class T>
static void tolerance_case(size_t n, const char* tname) {
  Rng rng(2000 + n);
  const size_t rows = n + n / 4 + 3;
  std::vector<double> S(rows * n, 0.0), AA(n * n, 0.0), rhs(n);
  for (size_t e = 0; e < rows * n; e++)
    if (rng.uniform() < 0.2) S[e] = rng.normal();
  for (size_t i = 0; i < n; i++)
    for (size_t j = 0; j < n; j++) {
      double s = i == j ? 1.0 : 0.0;
      for (size_t k = 0; k < rows; k++) s += S[k + i * rows] * S[k + j * rows];
      AA[i + j * n] = (double)(T)s;                  // the matrix every run sees is the one rounded to T
    }
  for (size_t i = 0; i < n; i++) rhs[i] = (double)(T)rng.normal();
  std::vector<long double> truth_l(rhs.begin(), rhs.end());     // the truth: the same loop in long double (64-bit mantissa on x86-64)
  bool ok = reference_solve<long double>(std::vector<long double>(AA.begin(), AA.end()), truth_l, n);
  std::vector<double> truth(truth_l.begin(), truth_l.end());
  std::vector<T> At(AA.begin(), AA.end()), xt(rhs.begin(), rhs.end());
  ok = ok && reference_solve<T>(At, xt, n);
  double e_t = 0, scale = 0;
  for (size_t i = 0; i < n; i++) { e_t = std::fmax(e_t, std::fabs((double)xt[i] - truth[i])); scale = std::fmax(scale, std::fabs(truth[i])); }
  e_t /= scale;
  const double eps = (double)std::numeric_limits<T>::epsilon(), bound = std::fmax(4 * e_t, 32 * eps);
  const double err64 = blocked_error<T, double>(AA, rhs, truth, n), errT = blocked_error<T, T>(AA, rhs, truth, n);
  ok = ok && err64 <= bound;
  std::printf("tolerance %s n=%zu: e_T %.3g, blocked with the factorisation in fp64 %.3g, in T %.3g, bound %.3g: %s\n", tname, n, e_t, err64, errT, bound,
              ok ? "within" : "FAIL");
  if (!ok) g_fail = 1;
}

int main(int argc, char** argv) {
  if (argc < 2 || std::atoi(argv[1]) != NB) { std::printf("FAIL: the plan's NB (%s) is not the header's (%d)\n", argc > 1 ? argv[1] : "missing", NB); return 1; }
  const size_t sizes[] = {1, 2, (size_t)NB - 1, (size_t)NB, (size_t)NB + 1, 2 * (size_t)NB + 1};
  for (size_t n : sizes) {
    exact_case<float>(n, "fp32"); exact_case<double>(n, "fp64");
    tolerance_case<float>(n, "fp32"); tolerance_case<double>(n, "fp64");
  }
  {   // an indefinite matrix stops at its pivot
    std::vector<double> W = {4, 2, 0, 2, 1, 0, 0, 0, 1};            // leading 2 x 2 minor is singular: pivot 1 is 0
    std::vector<double> L, U, dinv;
    const int info = factor<double, double>(W, 3, L, U, dinv);
    std::printf("indefinite: pivot %d\n", info);
    if (info != 1) g_fail = 1;
  }
  std::printf(g_fail ? "FAIL\n" : "ok\n");
  return g_fail;
}
