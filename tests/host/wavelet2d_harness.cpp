// wavelet2d_harness.cpp -- include/prost/linop/wavelet2d.hpp on the host, a stand-alone program (plain g++, no HIP) meant to run under
// AddressSanitizer and UndefinedBehaviorSanitizer.  usage: wavelet2d_harness <directory>.  <directory>/cases.txt, written by
// tests/test_wavelet2d_host.py, holds one case per line: <id> <nx> <ny> <L> <levels> <T> <sums>.  For every case it reads <id>_taps.bin
// (T float64 values) and, for both precisions, <id>_<fp32|fp64>_rhs.bin and .._res0.bin (L nx ny values of T each), runs
// wavelet2d::Apply forward and transposed, plain and accumulating, against exactly sized heap buffers, and writes .._fwd.bin,
// .._fwd_acc.bin, .._inv.bin, .._inv_acc.bin; with <sums> = 1 it also writes <id>_rowsum_<a>.bin and <id>_colsum_<a>.bin (N float64
// values each) for alpha = 0.5, 1, 1.5 (a = 0, 1, 2).  It writes named_<name>.bin, the named taps, and checks what needs no
// reference: the taps' orthonormality, the limits, the work buffer's size, the tail's start and that the input is left alone.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "prost/linop/wavelet2d.hpp"

namespace w2d = prost::wavelet2d;

static int failures = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) { failures++; std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } \
  } while (0)

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

struct Case { std::string id; int nx, ny, L, levels, ntaps, sums; };

template <class T> static void run_case(const std::string& dir, const Case& c, const double* h, const char* tname) {
  const size_t n = (size_t)c.L * (size_t)c.nx * (size_t)c.ny;
  const std::string stem = dir + "/" + c.id + "_" + tname;
  const std::unique_ptr<T[]> rhs = read_exact<T>(stem + "_rhs.bin", n), res0 = read_exact<T>(stem + "_res0.bin", n);
  std::unique_ptr<T[]> keep(new T[n]);
  std::memcpy(keep.get(), rhs.get(), n * sizeof(T));
  const w2d::Taps<T> w = w2d::MakeTaps<T>(h, c.ntaps);
  const w2d::Geometry g = w2d::MakeGeometry(c.ny, c.nx, c.L, c.levels, c.ntaps, false);
  for (int transpose = 0; transpose < 2; transpose++) {
    std::unique_ptr<T[]> plain(new T[n]), acc(new T[n]);
    std::memcpy(acc.get(), res0.get(), n * sizeof(T));
    w2d::Apply<T, false>(plain.get(), rhs.get(), g, w, transpose != 0);
    w2d::Apply<T, true>(acc.get(), rhs.get(), g, w, transpose != 0);
    write_all(stem + (transpose ? "_inv.bin" : "_fwd.bin"), plain.get(), n);
    write_all(stem + (transpose ? "_inv_acc.bin" : "_fwd_acc.bin"), acc.get(), n);
  }
  CHECK(std::memcmp(keep.get(), rhs.get(), n * sizeof(T)) == 0, "the input is left alone");
  std::printf("%s %s: %zu values, forward and transposed, plain and accumulating\n", c.id.c_str(), tname, n);
}

static void write_sums(const std::string& dir, const Case& c, const double* h) {
  const w2d::Geometry g = w2d::MakeGeometry(c.ny, c.nx, c.L, c.levels, c.ntaps, false);
  const double alphas[3] = {0.5, 1.0, 1.5};
  const size_t N = (size_t)c.nx * (size_t)c.ny;
  for (int a = 0; a < 3; a++) {
    const w2d::AxisSums sy = w2d::AxisTables(c.ny, c.levels, h, c.ntaps, alphas[a]), sx = w2d::AxisTables(c.nx, c.levels, h, c.ntaps, alphas[a]);
    std::unique_ptr<double[]> rows(new double[N]), cols(new double[N]);
    for (size_t p = 0; p < N; p++) {
      rows[p] = w2d::RowSum(g, sy, sx, (int)(p % (size_t)c.ny), (int)(p / (size_t)c.ny));
      cols[p] = w2d::ColSum(g, sy, sx, (int)(p % (size_t)c.ny), (int)(p / (size_t)c.ny));
    }
    write_all(dir + "/" + c.id + "_rowsum_" + std::to_string(a) + ".bin", rows.get(), N);
    write_all(dir + "/" + c.id + "_colsum_" + std::to_string(a) + ".bin", cols.get(), N);
  }
  std::printf("%s: sums of %zu rows and columns at three exponents\n", c.id.c_str(), N);
}

static void check_limits() {
  CHECK(!w2d::CheckShape(2, 2, 1, 1, 2) && !w2d::CheckShape(1, 8, 1, 1, 4) && !w2d::CheckShape(8, 1, 1, 1, 4) && !w2d::CheckShape(8, 8, 1, 2, 4), "accepted shapes");
  CHECK(!w2d::CheckShape(20, 12, 1, 2, 6) && !w2d::CheckShape(32, 32, 3, 5, 2) && !w2d::CheckShape(128, 128, 1, 4, 16), "accepted shapes");
  CHECK(w2d::CheckShape(1, 1, 1, 1, 2) && w2d::CheckShape(8, 8, 0, 1, 2) && w2d::CheckShape(8, 8, 1, 0, 2) && w2d::CheckShape(8, 8, 1, 1, 3), "refused shapes");
  CHECK(w2d::CheckShape(8, 8, 1, 1, 18) && w2d::CheckShape(8, 8, 1, 1, 0) && w2d::CheckShape(8, 8, 1, 3, 4) && w2d::CheckShape(12, 8, 1, 3, 2), "refused shapes");
  CHECK(w2d::CheckShape(8, 8, 1, 31, 2) && w2d::CheckShape(8.5, 8, 1, 1, 2) && w2d::CheckShape(8, -8, 1, 1, 2) && w2d::CheckShape(32768, 32768, 2, 1, 2), "refused shapes");
  CHECK(!w2d::CheckShape(32768, 32768, 1, 1, 2) && w2d::CheckShape(2, 1024, 1, 2, 4), "the limit of 2^31 and a thin side");
  w2d::Geometry g = w2d::MakeGeometry(64, 32, 3, 2, 2, false);
  CHECK(w2d::WorkSize(g) == 3 * (32 * 16 + 16 * 8) && w2d::WorkSlot0(g) == 3 * 32 * 16, "work buffer of 64 x 32 x 3");
  g = w2d::MakeGeometry(1, 64, 1, 2, 2, false);
  CHECK(w2d::WorkSize(g) == 32 + 16, "work buffer of a line");
  g = w2d::MakeGeometry(256, 128, 1, 7, 2, false);
  CHECK(w2d::TailStart(g) == 2, "256 x 128: the corner of level 2 holds 64 x 32 values");
  g.no_tail = 1;
  CHECK(w2d::TailStart(g) == 7, "no tail");
  g = w2d::MakeGeometry(64, 64, 1, 4, 4, false);
  CHECK(w2d::TailStart(g) == 0, "64 x 64 is all tail");
  g = w2d::MakeGeometry(96, 160, 1, 1, 6, false);
  CHECK(w2d::TailStart(g) == 1, "one level above the threshold: no tail");
}

int main(int argc, char** argv) {
  if (argc != 2) { std::printf("usage: wavelet2d_harness <directory>\n"); return 2; }
  const std::string dir = argv[1];
  for (const char* name : {"haar", "db2", "db3"}) {
    std::vector<double> h;
    CHECK(w2d::NamedTaps(name, h), "named taps %s", name);
    CHECK(w2d::OrthoDefect(h.data(), (int)h.size()) <= 1e-15 * (double)h.size(), "%s: defect %.3g", name, w2d::OrthoDefect(h.data(), (int)h.size()));
    double sum = 0;
    for (double v : h) sum += v;
    CHECK(std::fabs(sum - std::sqrt(2.0)) <= 4e-15, "%s: the taps sum to sqrt(2)", name);
    write_all(dir + "/named_" + name + ".bin", h.data(), h.size());
    std::vector<double> cut = h;
    for (double& v : cut) v = std::round(v * 1e10) / 1e10;
    if (h.size() > 2) CHECK(!(w2d::OrthoDefect(cut.data(), (int)cut.size()) <= w2d::kOrthoTolerance), "%s truncated to ten digits is refused", name);
  }
  std::vector<double> none;
  CHECK(!w2d::NamedTaps("db4", none) && none.empty(), "an unknown name");
  std::printf("named taps: orthonormal, written\n");
  check_limits();
  std::FILE* f = std::fopen((dir + "/cases.txt").c_str(), "r");
  if (!f) { std::printf("FAIL cannot open cases.txt\n"); return 2; }
  std::vector<Case> cases;
  char id[128];
  Case c;
  while (std::fscanf(f, "%127s %d %d %d %d %d %d", id, &c.nx, &c.ny, &c.L, &c.levels, &c.ntaps, &c.sums) == 7) { c.id = id; cases.push_back(c); }
  std::fclose(f);
  for (const Case& k : cases) {
    if (w2d::CheckShape(k.ny, k.nx, k.L, k.levels, k.ntaps)) { std::printf("FAIL %s: %s\n", k.id.c_str(), w2d::CheckShape(k.ny, k.nx, k.L, k.levels, k.ntaps)); return 2; }
    const std::unique_ptr<double[]> h = read_exact<double>(dir + "/" + k.id + "_taps.bin", (size_t)k.ntaps);
    CHECK(w2d::OrthoDefect(h.get(), k.ntaps) <= w2d::kOrthoTolerance, "%s: the taps are orthonormal", k.id.c_str());
    run_case<float>(dir, k, h.get(), "fp32");
    run_case<double>(dir, k, h.get(), "fp64");
    if (k.sums) write_sums(dir, k, h.get());
  }
  std::printf("%zu cases\n", cases.size());
  if (failures) { std::printf("FAIL: %d checks\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
