// eigen_mass_functor_harness.cpp -- runs the public functors of prost/prox/elemop/elem_operation_eigen_nxn.hpp and
// elem_operation_mass_norm.hpp ON THE HOST, group by group over Vector views, the way a plugin's kernel would on the device, and the
// compile-time form EigenNApply<T, N> the library's register kernels call.  They are __host__ __device__ templates, so
// tests/test_eigen_mass_frontend.py can check the arithmetic against NumPy without a GPU.  Compiled with hipcc (-x hip); no HIP
// runtime call is made.
//
//   eigen_mass_functor_harness pairs
//       prints "m round slot p q" for every slot of RoundRobinPair, m = 2, 4, .., 32
//   eigen_mass_functor_harness <in> <out>
//   <in>:  int64 family, fn (0..13 as FUNCTIONS_1D; ignored by the mass families), single (0 / 1), dim, count, interleaved, invert_tau,
//          want_sweeps;  then doubles: tau, arg[count * dim], tau_diag[count * dim], 7 x coefficient[count]
//          family 0: ElemOperationEigenNxN (run-time n, round-robin order)   1: ElemOperationMass4<T, false>   2: ElemOperationMass4<T, true>
//                 3: ElemOperationMass5<T, false>  4: ElemOperationMass5<T, true>  (coefficient 0 is the cost; Mass5 takes none: it has to be 1)
//                 5: EigenNApply<T, N>, N = 1, 4, 5 (compile-time n, cyclic order)
//   <out>: doubles res[count * dim], then -- with want_sweeps, families 0 and 5 -- doubles sweeps[count]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "prost/prox/elemop/elem_operation_eigen_nxn.hpp"
#include "prost/prox/elemop/elem_operation_mass_norm.hpp"

using namespace prost;

struct Job {
  int64_t family, fn, single, dim, count, interleaved, invert_tau, want_sweeps;
  double tau;
  std::vector<double> arg, tau_diag, coeffs[7], res, sweeps;
};

template <typename T, class OP, bool WITH_COEFFS>
static void run_op(Job& j) {
  const size_t count = (size_t)j.count, dim = (size_t)j.dim;
  std::vector<T> arg(j.arg.begin(), j.arg.end()), td(j.tau_diag.begin(), j.tau_diag.end()), res(count * dim, (T)0);
  for (size_t g = 0; g < count; g++) {
    T c[7];
    for (int k = 0; k < 7; k++) c[k] = (T)j.coeffs[k][g];
    Vector<T> r(count, dim, j.interleaved != 0, g, res.data());
    const Vector<const T> a(count, dim, j.interleaved != 0, g, arg.data());
    const Vector<const T> t(count, dim, j.interleaved != 0, g, td.data());
    typedef SharedMem<typename OP::SharedMemType, typename OP::GetSharedMemCount> Lds;      // device-only type; these operations never touch it
    alignas(Lds) unsigned char lds_storage[sizeof(Lds)] = {0};
    if constexpr (WITH_COEFFS) {
      OP op(c, dim, *reinterpret_cast<Lds*>(lds_storage));
      op(r, a, t, (T)j.tau, j.invert_tau != 0);
    } else {
      OP op(dim, *reinterpret_cast<Lds*>(lds_storage));
      op(r, a, t, (T)j.tau, j.invert_tau != 0);
    }
  }
  j.res.assign(res.begin(), res.end());
}

// the sweeps the decomposition of each group takes (the result is computed again and dropped)
template <typename T, class FUN, int N>
static void run_direct(Job& j, bool store) {
  const size_t count = (size_t)j.count, dim = (size_t)j.dim;
  std::vector<T> arg(j.arg.begin(), j.arg.end()), td(j.tau_diag.begin(), j.tau_diag.end()), res(count * dim, (T)0);
  j.sweeps.assign(count, 0.);
  for (size_t g = 0; g < count; g++) {
    T c[7];
    for (int k = 0; k < 7; k++) c[k] = (T)j.coeffs[k][g];
    Vector<T> r(count, dim, j.interleaved != 0, g, res.data());
    const Vector<const T> a(count, dim, j.interleaved != 0, g, arg.data());
    const Vector<const T> t(count, dim, j.interleaved != 0, g, td.data());
    const double step = elemop::SpectralStep((T)j.tau, t[0], j.invert_tau != 0);
    if constexpr (N == 0) {
      int sweeps = 0;
      elemop::EigenNxNApply<T>(r, a, elemop::EigenNxNSide(dim), step, c, FUN(), &sweeps);
      j.sweeps[g] = sweeps;
    } else {
      elemop::EigenNApply<T, N>(r, a, step, c, FUN());
      double s[N][N], v[N][N];
      for (int i = 0; i < N; i++)
        for (int k = i; k < N; k++) s[i][k] = ((double)a[i * N + k] + (double)a[k * N + i]) / 2.;
      j.sweeps[g] = elemop::SymEigN<N>(s, v);
    }
  }
  if (store) j.res.assign(res.begin(), res.end());
}

template <typename T, class FUN>
static bool run_fun(Job& j) {
  if (j.family == 0) {
    run_op<T, ElemOperationEigenNxN<T, FUN>, true>(j);
    if (j.want_sweeps) run_direct<T, FUN, 0>(j, false);
    return true;
  }
  if (j.dim == 1) { run_direct<T, FUN, 1>(j, true); return true; }
  if (j.dim == 16) { run_direct<T, FUN, 4>(j, true); return true; }
  if (j.dim == 25) { run_direct<T, FUN, 5>(j, true); return true; }
  return false;
}

template <typename T>
static bool run(Job& j) {
  switch (j.family) {
    case 1: run_op<T, ElemOperationMass4<T, false>, true>(j); return true;
    case 2: run_op<T, ElemOperationMass4<T, true>, true>(j); return true;
    case 3: run_op<T, ElemOperationMass5<T, false>, false>(j); return true;
    case 4: run_op<T, ElemOperationMass5<T, true>, false>(j); return true;
    case 0: case 5: break;
    default: return false;
  }
  switch (j.fn) {
    case 0: return run_fun<T, Function1DZero<T>>(j);
    case 1: return run_fun<T, Function1DAbs<T>>(j);
    case 2: return run_fun<T, Function1DSquare<T>>(j);
    case 3: return run_fun<T, Function1DIndLeq0<T>>(j);
    case 4: return run_fun<T, Function1DIndGeq0<T>>(j);
    case 5: return run_fun<T, Function1DIndEq0<T>>(j);
    case 6: return run_fun<T, Function1DIndBox01<T>>(j);
    case 7: return run_fun<T, Function1DMaxPos0<T>>(j);
    case 8: return run_fun<T, Function1DL0<T>>(j);
    case 9: return run_fun<T, Function1DHuber<T>>(j);
    case 10: return run_fun<T, Function1DLq<T>>(j);
    case 11: return run_fun<T, Function1DLqPlusEps<T>>(j);
    case 12: return run_fun<T, Function1DTruncLinear<T>>(j);
    case 13: return run_fun<T, Function1DTruncQuad<T>>(j);
  }
  return false;
}

static bool read_doubles(FILE* f, std::vector<double>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(double), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc == 2 && std::strcmp(argv[1], "pairs") == 0) {
    for (int m = 2; m <= 32; m += 2)
      for (int round = 0; round < m - 1; round++)
        for (int slot = 0; slot < m / 2; slot++) {
          int p = -1, q = -1;
          elemop::RoundRobinPair(m, round, slot, p, q);
          std::printf("%d %d %d %d %d\n", m, round, slot, p, q);
        }
    return 0;
  }
  if (argc != 3) { std::fprintf(stderr, "usage: %s pairs | <in> <out>\n", argv[0]); return 2; }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::perror(argv[1]); return 2; }
  Job j;
  int64_t head[8];
  bool ok = std::fread(head, sizeof(int64_t), 8, f) == 8;
  j.family = head[0]; j.fn = head[1]; j.single = head[2]; j.dim = head[3]; j.count = head[4]; j.interleaved = head[5]; j.invert_tau = head[6];
  j.want_sweeps = head[7];
  ok = ok && j.dim > 0 && j.dim <= 1024 && j.count >= 0 && std::fread(&j.tau, sizeof(double), 1, f) == 1;
  const size_t n = ok ? (size_t)j.count * (size_t)j.dim : 0;
  ok = ok && read_doubles(f, j.arg, n) && read_doubles(f, j.tau_diag, n);
  for (int k = 0; k < 7 && ok; k++) ok = read_doubles(f, j.coeffs[k], (size_t)j.count);
  std::fclose(f);
  if (!ok) { std::fprintf(stderr, "short or malformed input\n"); return 2; }
  if (j.family == 0 && elemop::EigenNxNSide((size_t)j.dim) == 0) { std::fprintf(stderr, "dim is no perfect square\n"); return 2; }
  if (!(j.single ? run<float>(j) : run<double>(j))) { std::fprintf(stderr, "unknown family / function / dim\n"); return 2; }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) { std::perror(argv[2]); return 2; }
  bool wrote = std::fwrite(j.res.data(), sizeof(double), j.res.size(), o) == j.res.size();
  if (j.want_sweeps && (j.family == 0 || j.family == 5)) wrote = wrote && std::fwrite(j.sweeps.data(), sizeof(double), j.sweeps.size(), o) == j.sweeps.size();
  std::fclose(o);
  return wrote ? 0 : 2;
}
