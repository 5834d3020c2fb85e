// prost/prox/elemop/elem_operation_mass_norm.hpp -- prox of the mass norm of a 2-vector in R^4 / R^5, and the projection onto the
// unit ball of its dual, the comass norm.
//
// Plugin contract of the reference's include/prost/prox/elemop/elem_operation_mass_norm.hpp:
// ElemOperationMass4<T, conjugate> : ElemOperation<6, 1> (the coefficient is the cost, a weight on the norm) and
// ElemOperationMass5<T, conjugate> : ElemOperation<10, 0>.  A group holds the upper triangle of a skew-symmetric n x n matrix A row by
// row -- (1,2), (1,3), (1,4), (2,3), (2,4), (3,4) for n = 4, the ten entries likewise for n = 5.  With A = U S V^T the mass norm is
// the sum of the (pairwise equal) singular values, and the result is the same triangle of U f(S) V^T:
//   conjugate = false   f(s) = max(s - step, 0),  step = tau_scal * cost * tau_diag[0]  (the product in T; its reciprocal under invert_tau)
//   conjugate = true    f(s) = min(s, 1), whatever the step: the projection onto the comass ball
//
// Computed as  A g(-A^2)  with  g(s) = f(sqrt s) / sqrt s, g(0) = 0:  -A^2 = A^T A = V S^2 V^T is symmetric positive semidefinite, its
// eigendecomposition is the Jacobi of spectral_common.hpp (SymEigN, in registers), and A V g(S^2) V^T = U f(S) V^T.  There is no
// reduction to a 2x2 block and no case distinction for equal singular values; a zero group gives zeros.
#ifndef PROST_PROX_ELEMOP_ELEM_OPERATION_MASS_NORM_HPP_
#define PROST_PROX_ELEMOP_ELEM_OPERATION_MASS_NORM_HPP_
#include "prost/prox/elemop/spectral_common.hpp"

namespace prost {
namespace elemop {

/// N = 4 (6 components) or 5 (10 components)
template <class T, int N, bool CONJUGATE, class RES, class ARG>
__host__ __device__ __forceinline__ void MassNormApply(RES& res, const ARG& arg, double step) {
  double A[N][N], S[N][N], V[N][N], g[N];
  {
    int idx = 0;
#pragma unroll
    for (int i = 0; i < N; i++) {
      A[i][i] = 0.;
#pragma unroll
      for (int j = i + 1; j < N; j++, idx++) {
        A[i][j] = (double)arg[idx];
        A[j][i] = -A[i][j];
      }
    }
  }
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = i; j < N; j++) {
      double t = 0.;
#pragma unroll
      for (int k = 0; k < N; k++) t += A[k][i] * A[k][j];
      S[i][j] = t;
    }
  SymEigN<N>(S, V);
#pragma unroll
  for (int k = 0; k < N; k++) {
    const double sig = S[k][k] > 0. ? t_sqrt(S[k][k]) : 0.;
    const double f = CONJUGATE ? (sig < 1. ? sig : 1.) : (sig - step > 0. ? sig - step : 0.);
    g[k] = sig > 0. ? f / sig : 0.;
  }
  // G = V diag(g) V^T (symmetric); the result is the upper triangle of A G
  double G[N][N];
#pragma unroll
  for (int i = 0; i < N; i++)
#pragma unroll
    for (int j = i; j < N; j++) {
      double t = 0.;
#pragma unroll
      for (int k = 0; k < N; k++) t += V[i][k] * V[j][k] * g[k];
      G[i][j] = t;
      G[j][i] = t;
    }
  {
    int idx = 0;
#pragma unroll
    for (int i = 0; i < N; i++)
#pragma unroll
      for (int j = i + 1; j < N; j++, idx++) {
        double t = 0.;
#pragma unroll
        for (int k = 0; k < N; k++) t += A[i][k] * G[k][j];
        res[idx] = (T)t;
      }
  }
}

}  // namespace elemop

template <typename T, bool conjugate>
struct ElemOperationMass4 : public ElemOperation<6, 1> {
  static const bool kWritesAllComponents = true;
  __host__ __device__ ElemOperationMass4(T* coeffs, size_t /*dim*/, SharedMem<SharedMemType, GetSharedMemCount>& /*shared_mem*/) : coeffs_(coeffs) {}

  __host__ __device__ __forceinline__ void operator()(Vector<T>& res, const Vector<const T>& arg, const Vector<const T>& tau_diag, T tau_scal,
                                                      bool invert_tau) {
    tau_scal *= coeffs_[0];          // the weighted mass norm
    elemop::MassNormApply<T, 4, conjugate>(res, arg, elemop::SpectralStep(tau_scal, tau_diag[0], invert_tau));
  }

 private:
  T* coeffs_;
};

template <typename T, bool conjugate>
struct ElemOperationMass5 : public ElemOperation<10, 0> {
  static const bool kWritesAllComponents = true;
  __host__ __device__ ElemOperationMass5(size_t /*dim*/, SharedMem<SharedMemType, GetSharedMemCount>& /*shared_mem*/) {}

  __host__ __device__ __forceinline__ void operator()(Vector<T>& res, const Vector<const T>& arg, const Vector<const T>& tau_diag, T tau_scal,
                                                      bool invert_tau) {
    elemop::MassNormApply<T, 5, conjugate>(res, arg, elemop::SpectralStep(tau_scal, tau_diag[0], invert_tau));
  }
};

}  // namespace prost
#endif
