// prost/prox/elemop/elem_operation_eigen_2x2.hpp -- prox of a function of the eigenvalues of a symmetric 2x2 matrix.
//
// Plugin contract of the reference's include/prost/prox/elemop/elem_operation_eigen_2x2.hpp:
// ElemOperationEigen2x2<T, FUN_1D> : ElemOperation<4, 7>.  A group is a column-major 2x2 matrix M; it is symmetrised as
// (M + M^T) / 2 = V diag(l1, l2) V^T, and the result is V diag(p1, p2) V^T written as a full symmetric matrix, p = the prox of
// c f(a t - b) + d t + (e/2) t^2  at l (spectral_common.hpp; FUN_1D one of function_1d.hpp).  The step is
// tau_scal * tau_diag[0].  One Jacobi rotation is the exact decomposition of a 2x2 matrix.
#ifndef PROST_PROX_ELEMOP_ELEM_OPERATION_EIGEN_2X2_HPP_
#define PROST_PROX_ELEMOP_ELEM_OPERATION_EIGEN_2X2_HPP_
#include "prost/prox/elemop/spectral_common.hpp"

namespace prost {
namespace elemop {

template <class T, class RES, class ARG, class FUN_1D>
__host__ __device__ __forceinline__ void Eigen2x2Apply(RES& res, const ARG& arg, double tau, const T* coeffs, const FUN_1D& fun) {
  double l[2], c, s;
  SymEig2x2((double)arg[0], ((double)arg[1] + (double)arg[2]) / 2., (double)arg[3], l[0], l[1], c, s);
  SpectralProx1D(l, tau, SpectralCoeffs<T>(coeffs), fun);
  // V = [c s; -s c]
  const double t12 = (l[1] - l[0]) * c * s;
  res[0] = (T)(l[0] * c * c + l[1] * s * s);
  res[1] = (T)t12;
  res[2] = (T)t12;
  res[3] = (T)(l[0] * s * s + l[1] * c * c);
}

}  // namespace elemop

template <typename T, class FUN_1D>
struct ElemOperationEigen2x2 : public ElemOperation<4, 7> {
  static const bool kWritesAllComponents = true;
  __host__ __device__ ElemOperationEigen2x2(T* coeffs, size_t /*dim*/, SharedMem<SharedMemType, GetSharedMemCount>& /*shared_mem*/) : coeffs_(coeffs) {}

  __host__ __device__ __forceinline__ void operator()(Vector<T>& res, const Vector<const T>& arg, const Vector<const T>& tau_diag, T tau_scal,
                                                      bool invert_tau) {
    elemop::Eigen2x2Apply<T>(res, arg, elemop::SpectralStep(tau_scal, tau_diag[0], invert_tau), coeffs_, FUN_1D());
  }

 private:
  T* coeffs_;
};

}  // namespace prost
#endif
