// spectral_functor_harness.cpp -- runs the public spectral functors (prost/prox/elemop/elem_operation_singular_nx2.hpp,
// _eigen_2x2.hpp, _eigen_3x3.hpp composed with function_1d.hpp / function_2d.hpp) ON THE HOST, group by group over Vector
// views, the way a plugin's kernel would on the device.  They are __host__ __device__ templates, and the library's own
// kernel calls the same functions, so tests/test_spectral_frontend.py can check the arithmetic against NumPy without a GPU.
// Compiled with hipcc (-x hip); no HIP runtime call is made.
//
//   spectral_functor_harness <in> <out>
//   <in>:  int64 family (0 singular_nx2, 1 eigen_2x2, 2 eigen_3x3), fn (0..13 as FUNCTIONS_1D; 100 ind_l1_ball, 101 moreau:ind_l1_ball),
//          single (0 / 1), dim, count, interleaved, invert_tau;  then doubles: tau, arg[count * dim], tau_diag[count * dim],
//          7 x coefficient[count]
//   <out>: doubles res[count * dim]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "prost/prox/elemop/elem_operation_eigen_2x2.hpp"
#include "prost/prox/elemop/elem_operation_eigen_3x3.hpp"
#include "prost/prox/elemop/elem_operation_singular_nx2.hpp"

using namespace prost;

struct Job {
  int64_t family, fn, single, dim, count, interleaved, invert_tau;
  double tau;
  std::vector<double> arg, tau_diag, coeffs[7], res;
};

template <typename T, class OP>
static void run_op(Job& j) {
  const size_t count = (size_t)j.count, dim = (size_t)j.dim;
  std::vector<T> arg(j.arg.begin(), j.arg.end()), td(j.tau_diag.begin(), j.tau_diag.end()), res(count * dim, (T)0);
  for (size_t g = 0; g < count; g++) {
    T c[7];
    for (int k = 0; k < 7; k++) c[k] = (T)j.coeffs[k][g];
    Vector<T> r(count, dim, j.interleaved != 0, g, res.data());
    const Vector<const T> a(count, dim, j.interleaved != 0, g, arg.data());
    const Vector<const T> t(count, dim, j.interleaved != 0, g, td.data());
    typedef SharedMem<typename OP::SharedMemType, typename OP::GetSharedMemCount> Lds;      // device-only type; the spectral operations never touch it
    alignas(Lds) unsigned char lds_storage[sizeof(Lds)] = {0};
    OP op(c, dim, *reinterpret_cast<Lds*>(lds_storage));
    op(r, a, t, (T)j.tau, j.invert_tau != 0);
  }
  j.res.assign(res.begin(), res.end());
}

template <typename T, template <typename, class> class OPT>
static bool run_1d(Job& j) {
  switch (j.fn) {
    case 0: run_op<T, OPT<T, Function1DZero<T>>>(j); return true;
    case 1: run_op<T, OPT<T, Function1DAbs<T>>>(j); return true;
    case 2: run_op<T, OPT<T, Function1DSquare<T>>>(j); return true;
    case 3: run_op<T, OPT<T, Function1DIndLeq0<T>>>(j); return true;
    case 4: run_op<T, OPT<T, Function1DIndGeq0<T>>>(j); return true;
    case 5: run_op<T, OPT<T, Function1DIndEq0<T>>>(j); return true;
    case 6: run_op<T, OPT<T, Function1DIndBox01<T>>>(j); return true;
    case 7: run_op<T, OPT<T, Function1DMaxPos0<T>>>(j); return true;
    case 8: run_op<T, OPT<T, Function1DL0<T>>>(j); return true;
    case 9: run_op<T, OPT<T, Function1DHuber<T>>>(j); return true;
    case 10: run_op<T, OPT<T, Function1DLq<T>>>(j); return true;
    case 11: run_op<T, OPT<T, Function1DLqPlusEps<T>>>(j); return true;
    case 12: run_op<T, OPT<T, Function1DTruncLinear<T>>>(j); return true;
    case 13: run_op<T, OPT<T, Function1DTruncQuad<T>>>(j); return true;
  }
  return false;
}

template <typename T, class FUN_1D> using Nx2Sum1D = ElemOperationSingularNx2<T, Function2DSum1D<T, FUN_1D>>;

template <typename T>
static bool run(Job& j) {
  if (j.family == 1) return run_1d<T, ElemOperationEigen2x2>(j);
  if (j.family == 2) return run_1d<T, ElemOperationEigen3x3>(j);
  if (j.family != 0) return false;
  if (j.fn == 100) { run_op<T, ElemOperationSingularNx2<T, Function2DIndL1Ball<T>>>(j); return true; }
  if (j.fn == 101) { run_op<T, ElemOperationSingularNx2<T, Function2DMoreau<T, Function2DIndL1Ball<T>>>>(j); return true; }
  return run_1d<T, Nx2Sum1D>(j);
}

static bool read_doubles(FILE* f, std::vector<double>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(double), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc != 3) { std::fprintf(stderr, "usage: %s <in> <out>\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  Job j;
  int64_t head[7];
  bool ok = std::fread(head, sizeof(int64_t), 7, f) == 7;
  j.family = head[0]; j.fn = head[1]; j.single = head[2]; j.dim = head[3]; j.count = head[4]; j.interleaved = head[5]; j.invert_tau = head[6];
  ok = ok && j.dim > 0 && j.count >= 0 && std::fread(&j.tau, sizeof(double), 1, f) == 1;
  const size_t n = ok ? (size_t)j.count * (size_t)j.dim : 0;
  ok = ok && read_doubles(f, j.arg, n) && read_doubles(f, j.tau_diag, n);
  for (int k = 0; k < 7 && ok; k++) ok = read_doubles(f, j.coeffs[k], (size_t)j.count);
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "short or malformed input\n"); return 2; }
  if (!(j.single ? run<float>(j) : run<double>(j))) { std::fprintf(stderr, "unknown family / function\n"); return 2; }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::perror(argv[2]); return 2; }
  const bool wrote = std::fwrite(j.res.data(), sizeof(double), j.res.size(), o) == j.res.size();
  std::fclose(o);
  return wrote ? 0 : 2;
}
