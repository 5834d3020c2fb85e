// prost/prox/elemop/elem_operation_eigen_3x3.hpp -- prox of a function of the eigenvalues of a symmetric 3x3 matrix.
//
// Plugin contract of the reference's include/prost/prox/elemop/elem_operation_eigen_3x3.hpp:
// ElemOperationEigen3x3<T, FUN_1D> : ElemOperation<9, 7>.  A group is a column-major 3x3 matrix M; it is symmetrised as
// (M + M^T) / 2 = V diag(l) V^T, and the result is V diag(p) V^T written as a full symmetric matrix, p = the prox of
// c f(a t - b) + d t + (e/2) t^2  at each eigenvalue (spectral_common.hpp; FUN_1D one of function_1d.hpp).  The step is
// tau_scal * tau_diag[0].  The decomposition is cyclic Jacobi in fp64 (SymEig3x3), not the reference's Cardano formula with
// cross-product eigenvectors: same result where that is accurate, full accuracy for close and repeated eigenvalues too.
#ifndef PROST_PROX_ELEMOP_ELEM_OPERATION_EIGEN_3X3_HPP_
#define PROST_PROX_ELEMOP_ELEM_OPERATION_EIGEN_3X3_HPP_
#include "prost/prox/elemop/spectral_common.hpp"

namespace prost {
namespace elemop {

template <class T, class RES, class ARG, class FUN_1D>
__host__ __device__ __forceinline__ void Eigen3x3Apply(RES& res, const ARG& arg, double tau, const T* coeffs, const FUN_1D& fun) {
  double l[3], v[3][3];
  SymEig3x3((double)arg[0], ((double)arg[1] + (double)arg[3]) / 2., ((double)arg[2] + (double)arg[6]) / 2., (double)arg[4],
            ((double)arg[5] + (double)arg[7]) / 2., (double)arg[8], l, v);
  SpectralProx1D(l, tau, SpectralCoeffs<T>(coeffs), fun);
  const double t00 = v[0][0] * v[0][0] * l[0] + v[0][1] * v[0][1] * l[1] + v[0][2] * v[0][2] * l[2];
  const double t01 = v[0][0] * v[1][0] * l[0] + v[0][1] * v[1][1] * l[1] + v[0][2] * v[1][2] * l[2];
  const double t02 = v[0][0] * v[2][0] * l[0] + v[0][1] * v[2][1] * l[1] + v[0][2] * v[2][2] * l[2];
  const double t11 = v[1][0] * v[1][0] * l[0] + v[1][1] * v[1][1] * l[1] + v[1][2] * v[1][2] * l[2];
  const double t12 = v[1][0] * v[2][0] * l[0] + v[1][1] * v[2][1] * l[1] + v[1][2] * v[2][2] * l[2];
  const double t22 = v[2][0] * v[2][0] * l[0] + v[2][1] * v[2][1] * l[1] + v[2][2] * v[2][2] * l[2];
  res[0] = (T)t00; res[1] = (T)t01; res[2] = (T)t02;
  res[3] = (T)t01; res[4] = (T)t11; res[5] = (T)t12;
  res[6] = (T)t02; res[7] = (T)t12; res[8] = (T)t22;
}

}  // namespace elemop

template <typename T, class FUN_1D>
struct ElemOperationEigen3x3 : public ElemOperation<9, 7> {
  static const bool kWritesAllComponents = true;
  __host__ __device__ ElemOperationEigen3x3(T* coeffs, size_t /*dim*/, SharedMem<SharedMemType, GetSharedMemCount>& /*shared_mem*/) : coeffs_(coeffs) {}

  __host__ __device__ __forceinline__ void operator()(Vector<T>& res, const Vector<const T>& arg, const Vector<const T>& tau_diag, T tau_scal,
                                                      bool invert_tau) {
    elemop::Eigen3x3Apply<T>(res, arg, elemop::SpectralStep(tau_scal, tau_diag[0], invert_tau), coeffs_, FUN_1D());
  }

 private:
  T* coeffs_;
};

}  // namespace prost
#endif
