// nonlocal_gradient2d_harness.cpp -- include/prost/linop/nonlocal_gradient2d.hpp on the host, stand-alone (plain g++, no HIP), meant to be
// built with -fsanitize=address,undefined -ffp-contract=off.  argv[1] is a directory with cases.txt, one line `id nx ny L M with_sums` per
// case, <id>_offsets.bin (M pairs dy, dx of int8) and for every precision P in {fp32, fp64} the inputs as raw arrays of T:
//   <id>_<P>_weights.bin (M N)   <id>_<P>_rhs.bin (L N)   <id>_<P>_rhst.bin (M L N)   <id>_<P>_res0.bin (M L N)   <id>_<P>_res0t.bin (L N)
// It runs the forward and the adjoint product, plain and accumulating, in the geometry of the kernels -- tiles of 64 x 16 pixels, 256 lanes
// of VEC = 16 / sizeof(T) rows where the height is a multiple of VEC and of one row otherwise, the channels of a pass from the tile table
// -- and writes <id>_<P>_{fwd,fwd_acc,adj,adj_acc}.bin for tests/test_nonlocal_gradient2d_host.py to compare with the NumPy restatement bit
// for bit.  Every other geometry -- W = 1, 2, 4, small tiles that are no divisor of anything, few lanes, 1, 2 and 4 channels per pass --
// has to give the same bits here.  With with_sums, the single and the bulk forms of the row and column sums have to agree, and the sums
// for alpha = 1 and 2 are written as float64: <id>_<P>_{rowsum,colsum}_<0|1>.bin.  Every buffer, the staged tile included, is allocated
// at exactly its size, so a walk that leaves its planes is an AddressSanitizer report.  First it checks the tile table: for every reach
// from 0 to 15 and both precisions the staged tiles of a pass stay within 64 KiB.  Prints one line per case and precision, then `ok`;
// exit status 1 on any failure.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "prost/linop/nonlocal_gradient2d.hpp"

namespace nl = prost::nonlocal_gradient2d;

static int failures = 0;

template <class T>
static std::vector<T> read(const std::string& path, size_t n) {
  std::vector<T> v(n);
  std::ifstream f(path, std::ios::binary);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(n * sizeof(T)));
  if (!f || f.peek() != EOF) { std::printf("FAIL cannot read %zu values from %s\n", n, path.c_str()); std::exit(1); }
  return v;
}
template <class T>
static void write(const std::string& path, const std::vector<T>& v) {
  std::ofstream f(path, std::ios::binary);
  f.write(reinterpret_cast<const char*>(v.data()), (std::streamsize)(v.size() * sizeof(T)));
  if (!f) { std::printf("FAIL cannot write %s\n", path.c_str()); std::exit(1); }
}

struct Geometry { int tile_y, tile_x, threads, pass; };

template <class T, int W>
static std::vector<T> product(const std::vector<T>& in, const std::vector<T>& res0, const std::vector<T>& weights, const nl::Offsets& o, int M, size_t nx, size_t ny, size_t L,
                              bool transpose, bool acc, const Geometry& g) {
  std::vector<T> out(res0);
  if (!acc) for (T& v : out) v = (T)77;
  if (acc) nl::Apply<T, W, true>(out.data(), in.data(), weights.data(), o, M, nx, ny, L, transpose, g.tile_y, g.tile_x, g.threads, g.pass);
  else nl::Apply<T, W, false>(out.data(), in.data(), weights.data(), o, M, nx, ny, L, transpose, g.tile_y, g.tile_x, g.threads, g.pass);
  return out;
}
template <class T>
static std::vector<T> product_w(int W, const std::vector<T>& in, const std::vector<T>& res0, const std::vector<T>& weights, const nl::Offsets& o, int M, size_t nx, size_t ny,
                                size_t L, bool transpose, bool acc, const Geometry& g) {
  if (W == 1) return product<T, 1>(in, res0, weights, o, M, nx, ny, L, transpose, acc, g);
  if (W == 2) return product<T, 2>(in, res0, weights, o, M, nx, ny, L, transpose, acc, g);
  return product<T, 4>(in, res0, weights, o, M, nx, ny, L, transpose, acc, g);
}

template <class T>
static void run(const std::string& dir, const std::string& id, const char* prec, const nl::Offsets& o, int M, size_t nx, size_t ny, size_t L, bool with_sums) {
  const size_t N = nx * ny;
  const std::string stem = dir + "/" + id + "_" + prec;
  const std::vector<T> weights = read<T>(stem + "_weights.bin", (size_t)M * N);
  const std::vector<T> rhs = read<T>(stem + "_rhs.bin", L * N), rhst = read<T>(stem + "_rhst.bin", (size_t)M * L * N);
  const std::vector<T> res0 = read<T>(stem + "_res0.bin", (size_t)M * L * N), res0t = read<T>(stem + "_res0t.bin", L * N);
  constexpr int V = 16 / (int)sizeof(T);
  const int W = ny % V == 0 ? V : 1;
  const Geometry kernels = {nl::kTileY, nl::kTileX, nl::kThreads, 0};
  // tile_y is a multiple of 4 (every W divides it) and threads >= tile_y / W
  const Geometry others[5] = {{nl::kTileY, nl::kTileX, nl::kThreads, 1}, {8, 4, 16, 1}, {4, 3, 4, 2}, {16, 5, 64, 4}, {12, 7, 12, 3}};
  bool ok = true;
  for (int transpose = 0; transpose < 2; transpose++)
    for (int acc = 0; acc < 2; acc++) {
      const std::vector<T>& in = transpose ? rhst : rhs;
      const std::vector<T>& r0 = transpose ? res0t : res0;
      const std::vector<T> main = product_w<T>(W, in, r0, weights, o, M, nx, ny, L, transpose, acc, kernels);
      write(stem + (transpose ? "_adj" : "_fwd") + (acc ? "_acc" : "") + ".bin", main);
      for (const Geometry& g : others)
        for (int w : {1, 2, 4})
          if (product_w<T>(w, in, r0, weights, o, M, nx, ny, L, transpose, acc, g) != main) {
            ok = false;
            std::printf("FAIL %s %s transpose=%d acc=%d: W = %d with tiles of %d x %d, %d lanes and %d channels per pass differs\n", id.c_str(), prec, transpose, acc, w,
                        g.tile_y, g.tile_x, g.threads, g.pass);
          }
    }
  if (with_sums) {
    const double alphas[2] = {1.0, 2.0};
    for (int a = 0; a < 2; a++) {
      std::vector<double> rows((size_t)M * L * N), cols(L * N);
      for (size_t r = 0; r < rows.size(); r++) {
        rows[r] = (double)(T)nl::RowSum(r, weights.data(), o, nx, ny, L, alphas[a]);
        if (rows[r] != (double)(T)nl::PixelRowSum(weights.data(), o, (int)(r / (L * N)), nx, ny, r % N, alphas[a])) { ok = false; std::printf("FAIL %s %s: row sum %zu\n", id.c_str(), prec, r); }
      }
      for (size_t c = 0; c < cols.size(); c++) {
        cols[c] = (double)(T)nl::ColSum(c, weights.data(), o, M, nx, ny, alphas[a]);
        if (cols[c] != (double)(T)nl::PixelColSum(weights.data(), o, M, nx, ny, c % N, alphas[a])) { ok = false; std::printf("FAIL %s %s: column sum %zu\n", id.c_str(), prec, c); }
      }
      write(stem + "_rowsum_" + std::to_string(a) + ".bin", rows);
      write(stem + "_colsum_" + std::to_string(a) + ".bin", cols);
    }
  }
  if (!ok) failures++;
  int ry, rx;
  nl::Reach(o, M, ry, rx);
  std::printf("%s %s: %zu values, W = %d, reach %d x %d, %d channels per pass, forward and adjoint, plain and accumulating, %s\n", id.c_str(), prec, (size_t)M * L * N, W, ry, rx,
              nl::PassChannels(ry > rx ? ry : rx, sizeof(T)), ok ? "every geometry the same bits" : "FAIL");
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: nonlocal_gradient2d_harness <directory>\n"); return 1; }
  for (int reach = 0; reach <= nl::kMaxReach; reach++)
    for (size_t bytes : {sizeof(float), sizeof(double)}) {
      const int c = nl::PassChannels(reach, bytes);
      const size_t lds = (size_t)c * nl::TileValues(nl::kTileY, nl::kTileX, reach, reach) * bytes;
      std::printf("table reach %d bytes %zu channels %d lds %zu\n", reach, bytes, c, lds);
      if (c < 1 || c > nl::kMaxPassChannels || lds > nl::kLdsLimit) { std::printf("FAIL the tile table leaves 64 KiB\n"); failures++; }
    }
  const std::string dir = argv[1];
  std::ifstream cases(dir + "/cases.txt");
  std::string line;
  int n = 0;
  while (std::getline(cases, line)) {
    std::istringstream ss(line);
    std::string id;
    size_t nx, ny, L;
    int M, with_sums;
    if (!(ss >> id >> nx >> ny >> L >> M >> with_sums)) continue;
    if (M < 1 || M > nl::kMaxOffsets) { std::printf("FAIL %s: M = %d\n", id.c_str(), M); return 1; }
    const std::vector<signed char> pairs = read<signed char>(dir + "/" + id + "_offsets.bin", 2 * (size_t)M);
    nl::Offsets o = {};
    for (int m = 0; m < M; m++) { o.dy[m] = pairs[2 * m]; o.dx[m] = pairs[2 * m + 1]; }
    run<float>(dir, id, "fp32", o, M, nx, ny, L, with_sums != 0);
    run<double>(dir, id, "fp64", o, M, nx, ny, L, with_sums != 0);
    n++;
  }
  std::printf("%d cases\n", n);
  if (failures || n == 0) { std::printf("%d runs failed\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
