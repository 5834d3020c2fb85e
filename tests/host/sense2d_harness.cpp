// sense2d_harness.cpp -- include/prost/linop/sense2d.hpp on the host, a stand-alone program (plain g++, no HIP) meant to run under
// AddressSanitizer and UndefinedBehaviorSanitizer.  usage: sense2d_harness <directory>.  For every case of the list below and both
// precisions it reads <directory>/<nx>x<ny>x<L>x<C>_<fp32|fp64>_maps.bin (2 C N values of T, real planes first), .._x.bin and .._resx.bin
// (2 L N values) and .._y.bin and .._resy.bin (2 L C N values), written by tests/test_sense2d_host.py, runs sense2d::Apply forward and
// transposed, plain and accumulating, against exactly sized heap buffers, and prints one digest per result:
//
//   <case> <fp32|fp64> <fwd|fwd_acc|inv|inv_acc> <count> <digest>,   digest = sum_i (bits_i + 0x9E3779B97F4A7C15) (2 i + 1) mod 2^64
//
// over the bit patterns of the values (fp32 zero-extended), a zero of either sign taken as +0.  The test computes the same digest from
// its NumPy restatement.  The harness also checks what needs no reference: that the inputs are left alone, that 1 x 1 with sigma = 1 is the
// identity, and the bound sums at e = 2 against a plain sum of squares.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "prost/linop/sense2d.hpp"

namespace f2d = prost::fft2d;
namespace s2d = prost::sense2d;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
  } while (0)

struct Case { int nx, ny, L, C; };
static const Case kCases[] = {{1, 1, 1, 1},   {1, 1, 2, 3},  {1, 2, 1, 2},   {2, 1, 1, 2},   {2, 2, 1, 3},   {4, 8, 1, 2},  {8, 4, 2, 3},   {1, 64, 1, 2},  {64, 1, 1, 2},
                              {64, 32, 1, 4}, {32, 64, 2, 3}, {256, 64, 1, 2}, {64, 256, 1, 2}, {2048, 2, 1, 2}, {2, 2048, 1, 2}, {32, 32, 3, 5}, {16, 16, 1, 64}, {1, 2, 1100, 64}};

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

static uint64_t bits_of(float v) { uint32_t b; std::memcpy(&b, &v, sizeof(b)); return b; }
static uint64_t bits_of(double v) { uint64_t b; std::memcpy(&b, &v, sizeof(b)); return b; }
template <class T> static uint64_t digest(const T* v, size_t n) {
  uint64_t d = 0;
  for (size_t i = 0; i < n; i++) d += (bits_of(v[i] == (T)0 ? (T)0 : v[i]) + 0x9E3779B97F4A7C15ull) * (2 * (uint64_t)i + 1);
  return d;
}

template <class T> static void run_case(const std::string& dir, const Case& c, const char* tname) {
  const size_t N = (size_t)c.nx * (size_t)c.ny, cols = 2 * (size_t)c.L * N, rows = cols * (size_t)c.C, nmaps = 2 * (size_t)c.C * N;
  const std::string id = std::to_string(c.nx) + "x" + std::to_string(c.ny) + "x" + std::to_string(c.L) + "x" + std::to_string(c.C);
  const std::string stem = dir + "/" + id + "_" + tname;
  const std::unique_ptr<T[]> maps = read_exact<T>(stem + "_maps.bin", nmaps), x = read_exact<T>(stem + "_x.bin", cols), resx = read_exact<T>(stem + "_resx.bin", cols);
  const std::unique_ptr<T[]> y = read_exact<T>(stem + "_y.bin", rows), resy = read_exact<T>(stem + "_resy.bin", rows);
  std::unique_ptr<T[]> keep_x(new T[cols]), keep_y(new T[rows]), keep_maps(new T[nmaps]);
  std::memcpy(keep_x.get(), x.get(), cols * sizeof(T));
  std::memcpy(keep_y.get(), y.get(), rows * sizeof(T));
  std::memcpy(keep_maps.get(), maps.get(), nmaps * sizeof(T));
  const std::vector<T> table = f2d::MakeTable<T>(f2d::TableSize(c.ny, c.nx));
  const s2d::Geometry g = s2d::MakeGeometry(c.ny, c.nx, c.L, c.C, false);
  {
    std::unique_ptr<T[]> plain(new T[rows]), acc(new T[rows]);
    std::memcpy(acc.get(), resy.get(), rows * sizeof(T));
    s2d::Apply<T, false>(plain.get(), x.get(), g, table.data(), maps.get(), false);
    s2d::Apply<T, true>(acc.get(), x.get(), g, table.data(), maps.get(), false);
    std::printf("%s %s fwd %zu %llu\n", id.c_str(), tname, rows, (unsigned long long)digest(plain.get(), rows));
    std::printf("%s %s fwd_acc %zu %llu\n", id.c_str(), tname, rows, (unsigned long long)digest(acc.get(), rows));
  }
  {
    std::unique_ptr<T[]> plain(new T[cols]), acc(new T[cols]);
    std::memcpy(acc.get(), resx.get(), cols * sizeof(T));
    s2d::Apply<T, false>(plain.get(), y.get(), g, table.data(), maps.get(), true);
    s2d::Apply<T, true>(acc.get(), y.get(), g, table.data(), maps.get(), true);
    std::printf("%s %s inv %zu %llu\n", id.c_str(), tname, cols, (unsigned long long)digest(plain.get(), cols));
    std::printf("%s %s inv_acc %zu %llu\n", id.c_str(), tname, cols, (unsigned long long)digest(acc.get(), cols));
  }
  CHECK(std::memcmp(keep_x.get(), x.get(), cols * sizeof(T)) == 0 && std::memcmp(keep_y.get(), y.get(), rows * sizeof(T)) == 0 &&
            std::memcmp(keep_maps.get(), maps.get(), nmaps * sizeof(T)) == 0,
        "the inputs are left alone");
  // e = 2: the bounds are the matrix's sums, s^2 sum_p |sigma_c|^2 and sum_c |sigma_c(p)|^2
  for (int coil = 0; coil < c.C; coil++) {
    long double want = 0;
    for (size_t p = 0; p < N; p++) want += (long double)maps[coil * N + p] * maps[coil * N + p] + (long double)maps[(c.C + coil) * N + p] * maps[(c.C + coil) * N + p];
    want /= (long double)N;
    const double got = s2d::RowBound<T>(maps.get(), g, 2.0, coil);
    CHECK(std::fabs(got - (double)want) <= 8 * 2.3e-16 * (double)want, "row bound of coil %d at e = 2: %.17g against %.17g", coil, got, (double)want);
  }
  for (size_t p = 0; p < N; p += (N + 6) / 7) {
    long double want = 0;
    for (int coil = 0; coil < c.C; coil++) want += (long double)maps[coil * N + p] * maps[coil * N + p] + (long double)maps[(c.C + coil) * N + p] * maps[(c.C + coil) * N + p];
    const double got = s2d::ColBound<T>(maps.get(), g, 2.0, p);
    CHECK(std::fabs(got - (double)want) <= 8 * 2.3e-16 * (double)want, "column bound of pixel %zu at e = 2: %.17g against %.17g", p, got, (double)want);
  }
}

template <class T> static void check_identity() {
  const s2d::Geometry g = s2d::MakeGeometry(1, 1, 3, 1, false);
  const std::vector<T> table = f2d::MakeTable<T>(1);
  const T maps[2] = {(T)1, (T)0}, x[6] = {(T)0.5, (T)-2, (T)3, (T)7, (T)-0.25, (T)1e-3};
  T out[6];
  for (int transpose = 0; transpose < 2; transpose++) {
    s2d::Apply<T, false>(out, x, g, table.data(), maps, transpose != 0);
    CHECK(std::memcmp(out, x, sizeof(x)) == 0, "1 x 1 with sigma = 1 is the identity on non-zero values");
  }
}

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: sense2d_harness <directory>\n"); return 2; }
  check_identity<float>();
  check_identity<double>();
  for (const Case& c : kCases) {
    run_case<float>(argv[1], c, "fp32");
    run_case<double>(argv[1], c, "fp64");
  }
  if (failures) { std::printf("FAIL: %d checks\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
