// hessian2d_harness.cpp -- include/prost/linop/hessian2d.hpp on the host, stand-alone (plain g++, no HIP), meant to be built with
// -fsanitize=address,undefined -ffp-contract=off.  usage: hessian2d_harness <runs.txt> <sums.bin>, both written by
// tests/test_hessian2d_host.py from tests/hessian2d_reference.py.
//
// runs.txt, one product per line: ny nx L components transpose is_double w(%a) seed_x seed_res digest_plain digest_acc.  The input is
// Values(seed_x), the accumulating form starts from Values(seed_res) -- a generator written the same way in the test -- and the
// digests are Digest() of the bits of the NumPy restatement (b), plain and accumulating.  Per line:
//   * hessian2d::Apply (W = 1), plain and accumulating, has the digests of (b): equal bit for bit;
//   * it has the bits of the chain, written here from the two existing definitions: a plain forward difference (what gradient2d
//     stores) followed by sym_gradient2d::Apply, and sym_gradient2d::Apply transposed followed by the plain adjoint difference
//     res = 0 - (divx + divy) (accumulating: res - (divx + divy)) of grad_adj_kernel; components = 4 stores the mixed plane twice and
//     adds the two mixed planes first;
//   * W = 2 and 4, and at grids of up to 20000 pixels strips of 4 lanes and of 1 lane and forced chunk widths of 3 and 2 columns
//     (the halo columns and the edge-lane reads at small heights), give the bits of W = 1.
// sums.bin, doubles: records ny nx L components is_double w alpha, then the components L N row sums and the L N column sums of
// |entry|^alpha of the explicit matrix (c).  RowSum / ColSum have to be within (7 + 8) eps_T of them, relative (7 the longest row), and
// equal for w = 0.5 and alpha = 1.  Every buffer is allocated at exactly its size, so a march that leaves its planes is an
// AddressSanitizer report.  Prints one line per product and per record of sums ending in `equal`, then `ok`; exit status 1 on any
// failure.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "prost/linop/hessian2d.hpp"

namespace h2 = prost::hessian2d;
namespace sg2 = prost::sym_gradient2d;

static int failures = 0;

static uint64_t Mix(uint64_t z) {
  z *= 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
/// n values in [-2, 2), each a multiple of 2^-51, rounded to T
template <class T> static std::vector<T> Values(uint64_t seed, size_t n) {
  std::vector<T> v(n);
  for (size_t i = 0; i < n; i++) v[i] = (T)((((double)(Mix(seed + i) >> 11)) * 0x1p-53 - 0.5) * 4.0);
  return v;
}
/// sum of bits[i] * ((Mix(i) | 1)) modulo 2^64
template <class T> static uint64_t Digest(const std::vector<T>& v) {
  uint64_t h = 0;
  for (size_t i = 0; i < v.size(); i++) {
    typename std::conditional<sizeof(T) == 4, uint32_t, uint64_t>::type bits;
    std::memcpy(&bits, &v[i], sizeof(T));
    h += (uint64_t)bits * (Mix(i) | 1ull);
  }
  return h;
}
template <class T> static bool SameBits(const std::vector<T>& a, const std::vector<T>& b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

struct Case { size_t ny, nx, L; int components; double w; };

template <class T, int W>
static void product(std::vector<T>& out, const std::vector<T>& in, const Case& k, bool transpose, bool acc, int lanes = 256, int force_cols = 0) {
  if (acc) h2::Apply<T, W, true>(out.data(), in.data(), k.nx, k.ny, k.L, k.w, k.components, transpose, lanes, force_cols);
  else h2::Apply<T, W, false>(out.data(), in.data(), k.nx, k.ny, k.L, k.w, k.components, transpose, lanes, force_cols);
}

/// the two existing blocks one after the other, with the intermediate field
template <class T>
static std::vector<T> chain(const std::vector<T>& in, const std::vector<T>& res0, const Case& k, bool transpose, bool acc) {
  const size_t N = k.nx * k.ny, L = k.L, ny = k.ny, nx = k.nx;
  const size_t order3[3] = {0, 1, 2}, order4[4] = {0, 2, 2, 1};          // E's planes (exx, eyy, exy) in the order of the range
  const size_t* order = k.components == 4 ? order4 : order3;
  if (!transpose) {
    std::vector<T> g(2 * L * N), e(3 * L * N), out(res0);
    for (size_t c = 0; c < L; c++)
      for (size_t x = 0; x < nx; x++)
        for (size_t y = 0; y < ny; y++) {                                   // grad_fwd_kernel
          const size_t p = c * N + x * ny + y;
          const T val = in[p];
          T gx = 0, gy = 0;
          if (y < ny - 1) gy = in[p + 1] - val;
          if (x < nx - 1) gx = in[p + ny] - val;
          g[p] = gx; g[p + L * N] = gy;
        }
    sg2::Apply<T, 1, false>(e.data(), g.data(), nx, ny, L, k.w, false);
    for (size_t q = 0; q < (size_t)k.components; q++)
      for (size_t i = 0; i < L * N; i++) out[q * L * N + i] = acc ? (T)(res0[q * L * N + i] + e[order[q] * L * N + i]) : e[order[q] * L * N + i];
    return out;
  }
  std::vector<T> e(3 * L * N), v(2 * L * N), out(res0);
  for (size_t i = 0; i < L * N; i++) {
    e[i] = in[i];
    e[L * N + i] = in[(k.components == 4 ? 3 : 1) * L * N + i];
    e[2 * L * N + i] = k.components == 4 ? (T)(in[L * N + i] + in[2 * L * N + i]) : in[2 * L * N + i];
  }
  sg2::Apply<T, 1, false>(v.data(), e.data(), nx, ny, L, k.w, true);
  for (size_t c = 0; c < L; c++)
    for (size_t x = 0; x < nx; x++)
      for (size_t y = 0; y < ny; y++) {                                     // grad_adj_kernel
        const size_t p = c * N + x * ny + y;
        T divx, divy;
        if (y < ny - 1) divy = v[p + L * N]; else divy = 0;
        if (y > 0) divy -= v[p + L * N - 1];
        if (x < nx - 1) divx = v[p]; else divx = 0;
        if (x > 0) divx -= v[p - ny];
        const T s = divx + divy;
        out[p] = acc ? (T)(res0[p] - s) : (T)((T)0 - s);
      }
  return out;
}

template <class T>
static void run(const char* name, const Case& k, bool transpose, uint64_t seed_x, uint64_t seed_r, uint64_t want_plain, uint64_t want_acc) {
  const size_t N = k.nx * k.ny, big = (size_t)k.components * k.L * N, small = k.L * N, nin = transpose ? big : small, nout = transpose ? small : big;
  const std::vector<T> x = Values<T>(seed_x, nin), res0 = Values<T>(seed_r, nout);
  bool ok = true;
  std::vector<T> plain(nout, (T)77), acc(res0);
  product<T, 1>(plain, x, k, transpose, false);
  product<T, 1>(acc, x, k, transpose, true);
  if (Digest(plain) != want_plain) { ok = false; std::printf("FAIL %s: the plain product differs from the restatement\n", name); }
  if (Digest(acc) != want_acc) { ok = false; std::printf("FAIL %s: the accumulating product differs from the restatement\n", name); }
  if (!SameBits(plain, chain<T>(x, std::vector<T>(nout, (T)77), k, transpose, false))) { ok = false; std::printf("FAIL %s: the plain product differs from the chain\n", name); }
  if (!SameBits(acc, chain<T>(x, res0, k, transpose, true))) { ok = false; std::printf("FAIL %s: the accumulating product differs from the chain\n", name); }
  const int lanes[3] = {256, 4, 1}, widths[3] = {0, 3, 2};
  for (int v = 0; v < (N <= 20000 ? 3 : 1); v++) {
    std::vector<T> a1(nout, (T)77), a2(nout, (T)77), a4(nout, (T)77), c2(res0), c4(res0);
    product<T, 1>(a1, x, k, transpose, false, lanes[v], widths[v]);
    product<T, 2>(a2, x, k, transpose, false, lanes[v], widths[v]);
    product<T, 4>(a4, x, k, transpose, false, lanes[v], widths[v]);
    product<T, 2>(c2, x, k, transpose, true, lanes[v], widths[v]);
    product<T, 4>(c4, x, k, transpose, true, lanes[v], widths[v]);
    if (!SameBits(a1, plain) || !SameBits(a2, plain) || !SameBits(a4, plain) || !SameBits(c2, acc) || !SameBits(c4, acc)) {
      ok = false; std::printf("FAIL %s: W = 1 / 2 / 4 with %d lanes and chunk width %d differ from W = 1 in one strip\n", name, lanes[v], widths[v]);
    }
  }
  if (!ok) failures++;
  std::printf("%zux%zux%zu c%d w %.3f %s %s: restatement, chain and every W %s\n", k.ny, k.nx, k.L, k.components, k.w, name, transpose ? "adjoint" : "forward", ok ? "equal" : "FAIL");
}

template <class T>
static void sums(const char* name, const Case& k, double alpha, const double* rows, const double* cols) {
  const size_t N = k.nx * k.ny;
  const double wt = (double)h2::RoundWeight<T>(k.w), wa = h2::WeightPower(wt, alpha), two_a = h2::TwoPower(alpha);
  const double tol = (7 + 8) * (double)std::numeric_limits<T>::epsilon();
  const bool exact = k.w == 0.5 && alpha == 1.0;
  bool ok = true;
  for (size_t r = 0; r < (size_t)k.components * k.L * N; r++) {
    const double got = (double)(T)h2::RowSum(r, k.nx, k.ny, k.L, k.components, wa, two_a);
    if (!(std::fabs(got - rows[r]) <= tol * rows[r]) || (exact && got != rows[r])) { ok = false; std::printf("FAIL %s: row sum %zu, alpha %g: %.17g, expected %.17g\n", name, r, alpha, got, rows[r]); }
  }
  for (size_t q = 0; q < k.L * N; q++) {
    const double got = (double)(T)h2::ColSum(q, k.nx, k.ny, k.components, wa, two_a);
    if (!(std::fabs(got - cols[q]) <= tol * cols[q]) || (exact && got != cols[q])) { ok = false; std::printf("FAIL %s: column sum %zu, alpha %g: %.17g, expected %.17g\n", name, q, alpha, got, cols[q]); }
  }
  if (!ok) failures++;
  std::printf("%zux%zux%zu c%d w %.3f %s sums alpha %.1f: %s\n", k.ny, k.nx, k.L, k.components, k.w, name, alpha, ok ? "equal" : "FAIL");
}

int main(int argc, char** argv) {
  if (argc != 3) { std::printf("usage: hessian2d_harness <runs.txt> <sums.bin>\n"); return 2; }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
  size_t ny, nx, L;
  int components, transpose, is_double, products = 0, records = 0;
  double w;
  unsigned long long seed_x, seed_r, plain, acc;
  while (std::fscanf(f, "%zu %zu %zu %d %d %d %la %llu %llu %llu %llu", &ny, &nx, &L, &components, &transpose, &is_double, &w, &seed_x, &seed_r, &plain, &acc) == 11) {
    const Case k = {ny, nx, L, components, w};
    if (is_double) run<double>("fp64", k, transpose != 0, seed_x, seed_r, plain, acc);
    else run<float>("fp32", k, transpose != 0, seed_x, seed_r, plain, acc);
    products++;
  }
  std::fclose(f);
  f = std::fopen(argv[2], "rb");
  if (!f) { std::printf("cannot read %s\n", argv[2]); return 2; }
  double head[7];
  while (std::fread(head, sizeof(double), 7, f) == 7) {
    const Case k = {(size_t)head[0], (size_t)head[1], (size_t)head[2], (int)head[3], head[5]};
    const size_t N = k.nx * k.ny, nrows = (size_t)k.components * k.L * N, ncols = k.L * N;
    std::vector<double> rows(nrows), cols(ncols);
    if (std::fread(rows.data(), sizeof(double), nrows, f) != nrows || std::fread(cols.data(), sizeof(double), ncols, f) != ncols) { std::printf("FAIL: %s is truncated\n", argv[2]); return 1; }
    if (head[4] != 0) sums<double>("fp64", k, head[6], rows.data(), cols.data());
    else sums<float>("fp32", k, head[6], rows.data(), cols.data());
    records++;
  }
  std::fclose(f);
  if (failures) { std::printf("%d runs failed\n", failures); return 1; }
  std::printf("%d products and %d records of sums\nok\n", products, records);
  return products > 0 && records > 0 ? 0 : 1;
}
