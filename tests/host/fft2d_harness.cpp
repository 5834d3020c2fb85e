// fft2d_harness.cpp -- include/prost/linop/fft2d.hpp on the host, a stand-alone program (plain g++, no HIP) meant to run under
// AddressSanitizer and UndefinedBehaviorSanitizer.  usage: fft2d_harness <directory>.  For every case of the list below and both
// precisions it reads <directory>/<nx>x<ny>x<L>_<fp32|fp64>_rhs.bin and .._res0.bin (2 L nx ny values of T each, written by
// tests/test_fft2d_host.py), runs fft2d::Apply forward and transposed, plain and accumulating, against exactly sized heap buffers, and
// writes .._fwd.bin, .._fwd_acc.bin, .._inv.bin, .._inv_acc.bin; the test compares them bit for bit with its NumPy restatement.  It
// also checks what needs no reference: the table's exact entries and symmetry, the period classes, the sum table against a brute-force
// sum over the table, and that the input is left alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "prost/linop/fft2d.hpp"

namespace f2d = prost::fft2d;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
  } while (0)

struct Case { int nx, ny, L; };
static const Case kCases[] = {{1, 1, 1},   {1, 2, 1},   {2, 1, 1},    {2, 2, 1},    {4, 8, 1},    {8, 4, 1},    {1, 64, 1},   {64, 1, 1},   {64, 32, 1},
                              {32, 64, 1}, {256, 64, 1}, {64, 256, 1}, {256, 32, 1}, {2048, 2, 1}, {2, 2048, 1}, {2048, 8, 1}, {8, 2048, 1}, {32, 32, 3}};

template <class T> static std::unique_ptr<T[]> read_exact(const std::string& path, size_t n) {
  std::unique_ptr<T[]> buf(new T[n]);
  std::FILE* f = std::fopen(path.c_str(), "rb");
  if (!f) { std::printf("FAIL cannot open %s\n", path.c_str()); std::exit(2); }
  const size_t got = std::fread(buf.get(), sizeof(T), n, f);
  const int more = std::fgetc(f);
  std::fclose(f);
  if (got != n || more != EOF) { std::printf("FAIL %s does not hold %zu values\n", path.c_str(), n); std::exit(2); }
  return buf;
}
template <class T> static void write_all(const std::string& path, const T* v, size_t n) {
  std::FILE* f = std::fopen(path.c_str(), "wb");
  if (!f || std::fwrite(v, sizeof(T), n, f) != n) { std::printf("FAIL cannot write %s\n", path.c_str()); std::exit(2); }
  std::fclose(f);
}

template <class T> static void check_table(int n) {
  const std::vector<T> w = f2d::MakeTable<T>(n);
  CHECK(w.size() == 2 * (size_t)n, "table size");
  CHECK(w[0] == (T)1 && w[1] == (T)0, "w[0]");
  if (n >= 2) CHECK(w[2 * (n / 2)] == (T)-1 && w[2 * (n / 2) + 1] == (T)0, "w[n/2]");
  if (n >= 4) CHECK(w[2 * (n / 4)] == (T)0 && w[2 * (n / 4) + 1] == (T)-1, "w[n/4]");
  if (n >= 8) CHECK(w[2 * (n / 8)] == (T)std::sqrt(0.5) && w[2 * (n / 8) + 1] == (T)(-std::sqrt(0.5)), "w[n/8]");
  for (int j = 1; j < n; j++) {                                        // w[n - j] = conj(w[j]); w[j + n/2] = -w[j]; w[n/4 - j] swaps the parts
    CHECK(w[2 * (n - j)] == w[2 * j] && w[2 * (n - j) + 1] == -w[2 * j + 1], "conjugate symmetry at %d of %d", j, n);
    if (j < n / 2) CHECK(w[2 * (j + n / 2)] == -w[2 * j] && w[2 * (j + n / 2) + 1] == -w[2 * j + 1], "half turn at %d of %d", j, n);
    if (j < n / 4) CHECK(w[2 * (n / 4 - j)] == -w[2 * j + 1] && w[2 * (n / 4 - j) + 1] == -w[2 * j], "octant mirror at %d of %d", j, n);
  }
}

static void check_sums(int ny, int nx) {
  for (double alpha : {0.5, 1.0, 1.5, 2.0}) {
    double sums[f2d::kMaxLog2 + 1];
    f2d::SumTable(ny, nx, alpha, sums);
    const double N = (double)ny * nx, s = 1.0 / std::sqrt(N);
    // brute force over rows of every period class of the y axis, crossed with four of the x axis
    std::vector<int> kys = {0, 3 % ny}, kxs = {0, 1 % nx, nx / 2, 3 % nx};
    for (int v = ny / 2; v >= 1; v /= 2) kys.push_back(v);
    for (int ky : kys)
      for (int kx : kxs) {
        if (N > 4096) continue;
        const int l = f2d::PeriodLog2(ky, kx, ny, nx);
        long double acc = 0;
        for (int y = 0; y < ny; y++)
          for (int x = 0; x < nx; x++) {
            // the angle index over the common period n = max(ny, nx): (ky y / ny + kx x / nx) n, an integer
            const int n = f2d::TableSize(ny, nx);
            const long idx = ((long)ky * y % ny) * (n / ny) + ((long)kx * x % nx) * (n / nx);
            double c, sn;
            f2d::Angle((int)(idx % n), n, c, sn);
            if (c != 0) acc += f2d::PowAbs(s * c, alpha);
            if (sn != 0) acc += f2d::PowAbs(s * sn, alpha);
          }
        const double want = (double)acc;
        CHECK(std::fabs(sums[l] - want) <= ((1 << l) + 8) * 2.3e-16 * want, "sum alpha %g at (%d, %d) of %d x %d: %.17g against %.17g", alpha, ky, kx, ny, nx, sums[l], want);
      }
    if (alpha == 2.0)                                                  // a unitary matrix: every row has the squared norm 1
      for (int l = 0; l <= f2d::Log2(f2d::TableSize(ny, nx)); l++) CHECK(std::fabs(sums[l] - 1.0) <= 1e-13, "squared row norm of class %d: %.17g", l, sums[l]);
  }
}

template <class T> static void run_case(const std::string& dir, const Case& c, const char* tname) {
  const size_t n = 2 * (size_t)c.L * (size_t)c.nx * (size_t)c.ny;
  const std::string stem = dir + "/" + std::to_string(c.nx) + "x" + std::to_string(c.ny) + "x" + std::to_string(c.L) + "_" + tname;
  const std::unique_ptr<T[]> rhs = read_exact<T>(stem + "_rhs.bin", n), res0 = read_exact<T>(stem + "_res0.bin", n);
  std::unique_ptr<T[]> keep(new T[n]);
  std::memcpy(keep.get(), rhs.get(), n * sizeof(T));
  const std::vector<T> table = f2d::MakeTable<T>(f2d::TableSize(c.ny, c.nx));
  const f2d::Geometry g = f2d::MakeGeometry(c.ny, c.nx, c.L, false);
  for (int transpose = 0; transpose < 2; transpose++) {
    std::unique_ptr<T[]> plain(new T[n]), acc(new T[n]);
    std::memcpy(acc.get(), res0.get(), n * sizeof(T));
    f2d::Apply<T, false>(plain.get(), rhs.get(), g, table.data(), transpose != 0);
    f2d::Apply<T, true>(acc.get(), rhs.get(), g, table.data(), transpose != 0);
    write_all(stem + (transpose ? "_inv.bin" : "_fwd.bin"), plain.get(), n);
    write_all(stem + (transpose ? "_inv_acc.bin" : "_fwd_acc.bin"), acc.get(), n);
    if (c.nx == 1 && c.ny == 1) CHECK(std::memcmp(plain.get(), rhs.get(), n * sizeof(T)) == 0, "1 x 1 is the identity, bit for bit");
  }
  CHECK(std::memcmp(keep.get(), rhs.get(), n * sizeof(T)) == 0, "the input is left alone");
  std::printf("%dx%dx%d %s: %zu values, forward and transposed, plain and accumulating\n", c.nx, c.ny, c.L, tname, n);
}

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: fft2d_harness <directory>\n"); return 2; }
  for (int n = 1; n <= f2d::kMaxSide; n *= 2) { check_table<float>(n); check_table<double>(n); }
  std::printf("tables of 1 .. %d entries: exact entries and symmetries hold\n", f2d::kMaxSide);
  CHECK(f2d::IsSide(1) && f2d::IsSide(2048) && !f2d::IsSide(0) && !f2d::IsSide(3) && !f2d::IsSide(4096) && !f2d::IsSide(-2), "IsSide");
  CHECK(f2d::PeriodLog2(0, 0, 8, 4) == 0 && f2d::PeriodLog2(4, 0, 8, 4) == 1 && f2d::PeriodLog2(1, 0, 8, 4) == 3 && f2d::PeriodLog2(0, 1, 8, 4) == 2 &&
            f2d::PeriodLog2(2, 3, 8, 4) == 2 && f2d::PeriodLog2(0, 0, 1, 1) == 0,
        "PeriodLog2");
  for (const Case& c : kCases) {
    check_sums(c.ny, c.nx);
    run_case<float>(argv[1], c, "fp32");
    run_case<double>(argv[1], c, "fp64");
  }
  if (failures) { std::printf("FAIL: %d checks\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
