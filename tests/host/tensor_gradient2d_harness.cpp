// tensor_gradient2d_harness.cpp -- include/prost/linop/tensor_gradient2d.hpp on the host, stand-alone (plain g++, no HIP), meant to be
// built with -fsanitize=address,undefined -ffp-contract=off.  argv[1] is a directory with cases.txt, one line `id nx ny L with_sums` per
// case, and for every case, precision P in {fp32, fp64} and mode k in {1, 2, 3} the inputs as raw arrays of T:
//   <id>_<P>_k<k>_tensor.bin (k N)   <id>_<P>_rhs.bin (L N)   <id>_<P>_rhst.bin (2 L N)   <id>_<P>_res0.bin (2 L N)   <id>_<P>_res0t.bin (L N)
// It runs the forward and the adjoint march, plain and accumulating, in the geometry of the kernels -- lanes of VEC = 16 / sizeof(T)
// rows where the height is a multiple of VEC and of one row otherwise, strips of 256 lanes, chunks of PickColumns columns -- and
// writes <id>_<P>_k<k>_{fwd,fwd_acc,adj,adj_acc}.bin for tests/test_tensor_gradient2d_host.py to compare with the NumPy restatement bit
// for bit.  Every other geometry -- W = 1, 2, 4, strips of 4 lanes and of one lane (the edge reads and the recomputed fluxes at small
// heights), chunk widths forced to 3 and 2 (the halo column's flux) -- has to give the same bits here.  With with_sums, the single and
// the bulk forms of the row and column sums have to agree, and the bulk sums for alpha = 1 and 0.5 are written as float64:
// <id>_<P>_k<k>_{rowsum,colsum}_<0|1>.bin.  Every buffer is allocated at exactly its size, so a march that leaves its planes is an
// AddressSanitizer report.  Prints one line per case, precision and mode, then `ok`; exit status 1 on any failure.
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "prost/linop/tensor_gradient2d.hpp"

namespace tg2 = prost::tensor_gradient2d;

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

template <class T, int W>
static std::vector<T> product(const std::vector<T>& in, const std::vector<T>& res0, const std::vector<T>& tensor, size_t nx, size_t ny, size_t L, int mode,
                              bool transpose, bool acc, int lanes, int force_cols) {
  std::vector<T> out(res0);
  if (!acc) for (T& v : out) v = (T)77;
  if (acc) tg2::Apply<T, W, true>(out.data(), in.data(), tensor.data(), nx, ny, L, mode, transpose, lanes, force_cols);
  else tg2::Apply<T, W, false>(out.data(), in.data(), tensor.data(), nx, ny, L, mode, transpose, lanes, force_cols);
  return out;
}
template <class T>
static std::vector<T> product_w(int W, const std::vector<T>& in, const std::vector<T>& res0, const std::vector<T>& tensor, size_t nx, size_t ny, size_t L, int mode,
                                bool transpose, bool acc, int lanes, int force_cols) {
  if (W == 1) return product<T, 1>(in, res0, tensor, nx, ny, L, mode, transpose, acc, lanes, force_cols);
  if (W == 2) return product<T, 2>(in, res0, tensor, nx, ny, L, mode, transpose, acc, lanes, force_cols);
  return product<T, 4>(in, res0, tensor, nx, ny, L, mode, transpose, acc, lanes, force_cols);
}

template <class T>
static void run(const std::string& dir, const std::string& id, const char* prec, size_t nx, size_t ny, size_t L, bool with_sums) {
  const size_t N = nx * ny;
  const std::string stem = dir + "/" + id + "_" + prec;
  const std::vector<T> rhs = read<T>(stem + "_rhs.bin", L * N), rhst = read<T>(stem + "_rhst.bin", 2 * L * N);
  const std::vector<T> res0 = read<T>(stem + "_res0.bin", 2 * L * N), res0t = read<T>(stem + "_res0t.bin", L * N);
  constexpr int V = 16 / (int)sizeof(T);
  const int W = ny % V == 0 ? V : 1;
  for (int mode = 1; mode <= 3; mode++) {
    bool ok = true;
    const std::string out = stem + "_k" + std::to_string(mode);
    const std::vector<T> tensor = read<T>(out + "_tensor.bin", (size_t)mode * N);
    for (int transpose = 0; transpose < 2; transpose++)
      for (int acc = 0; acc < 2; acc++) {
        const std::vector<T>& in = transpose ? rhst : rhs;
        const std::vector<T>& r0 = transpose ? res0t : res0;
        const std::vector<T> main = product_w<T>(W, in, r0, tensor, nx, ny, L, mode, transpose, acc, 256, 0);
        write(out + (transpose ? "_adj" : "_fwd") + (acc ? "_acc" : "") + ".bin", main);
        const int lanes[4] = {256, 4, 1, 64}, widths[4] = {0, 3, 2, 1};
        for (int v = 0; v < (N <= 30000 ? 4 : 1); v++)
          for (int w : {1, 2, 4})
            if (product_w<T>(w, in, r0, tensor, nx, ny, L, mode, transpose, acc, lanes[v], widths[v]) != main) {
              ok = false; std::printf("FAIL %s %s k=%d transpose=%d acc=%d: W = %d with %d lanes and chunk width %d differs\n", id.c_str(), prec, mode, transpose, acc, w, lanes[v], widths[v]);
            }
      }
    if (with_sums) {
      const double alphas[2] = {1.0, 0.5};
      for (int a = 0; a < 2; a++) {
        std::vector<T> rows(2 * L * N, (T)0), cols(L * N, (T)0);
        tg2::RowSums<T>(rows.data(), tensor.data(), nx, ny, L, mode, alphas[a]);
        tg2::ColSums<T>(cols.data(), tensor.data(), nx, ny, L, mode, alphas[a]);
        for (size_t r = 0; r < rows.size(); r++) if (rows[r] != (T)tg2::RowSum(r, tensor.data(), nx, ny, L, mode, alphas[a])) { ok = false; std::printf("FAIL %s %s k=%d: bulk row sum %zu\n", id.c_str(), prec, mode, r); }
        for (size_t c = 0; c < cols.size(); c++) if (cols[c] != (T)tg2::ColSum(c, tensor.data(), nx, ny, L, mode, alphas[a])) { ok = false; std::printf("FAIL %s %s k=%d: bulk column sum %zu\n", id.c_str(), prec, mode, c); }
        write(out + "_rowsum_" + std::to_string(a) + ".bin", std::vector<double>(rows.begin(), rows.end()));
        write(out + "_colsum_" + std::to_string(a) + ".bin", std::vector<double>(cols.begin(), cols.end()));
      }
    }
    if (!ok) failures++;
    std::printf("%s %s k=%d: %zu values, W = %d, forward and adjoint, plain and accumulating, %s\n", id.c_str(), prec, mode, 2 * L * N, W, ok ? "every geometry the same bits" : "FAIL");
  }
}

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("usage: tensor_gradient2d_harness <directory>\n"); return 1; }
  const std::string dir = argv[1];
  std::ifstream cases(dir + "/cases.txt");
  std::string line;
  int n = 0;
  while (std::getline(cases, line)) {
    std::istringstream ss(line);
    std::string id;
    size_t nx, ny, L;
    int with_sums;
    if (!(ss >> id >> nx >> ny >> L >> with_sums)) continue;
    run<float>(dir, id, "fp32", nx, ny, L, with_sums != 0);
    run<double>(dir, id, "fp64", nx, ny, L, with_sums != 0);
    n++;
  }
  std::printf("%d cases\n", n);
  if (failures || n == 0) { std::printf("%d runs failed\n", failures); return 1; }
  std::printf("ok\n");
  return 0;
}
