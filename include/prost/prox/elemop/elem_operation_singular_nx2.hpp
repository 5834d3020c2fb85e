// prost/prox/elemop/elem_operation_singular_nx2.hpp -- prox of a function of the two singular values of an n x 2 matrix.
//
// Plugin contract of the reference's include/prost/prox/elemop/elem_operation_singular_nx2.hpp:
// ElemOperationSingularNx2<T, FUN_2D> : ElemOperation<0, 7>, dim = 2 n a run-time argument, coefficients
// (a, b, c, d, e, alpha, beta), FUN_2D one of function_2d.hpp.  Components 0..n-1 of a group are the first column of
// the matrix M, components n..2n-1 the second.  With the thin SVD M = U diag(s1, s2) V^T the result is
// U diag(p1, p2) V^T, (p1, p2) = the prox of  c f(a t - b) + d t + (e/2) t^2  at (s1, s2) (spectral_common.hpp).
//
// How it is computed: D = M^T M (2x2, accumulated in fp64), one Jacobi rotation gives D = V diag(l) V^T, s = sqrt(l), and
//     U diag(p) V^T = M V diag(p / s) V^T = M T,    T a symmetric 2x2 matrix
// so the group is read twice (for D, for the product) and U is never formed.  Conventions kept from the reference:
//   * the part that belongs to a zero singular value is dropped (p / s := 0).  A singular value counts as zero when its
//     square is below 8 ulp of the larger eigenvalue of D: that is the rounding noise of D itself.
//   * the zero matrix gives res[0] = p1, res[n + 1] = p2 and zero elsewhere (for n = 1 there is no component n + 1: the
//     reference writes past the group there, this operation writes res[0] only).
// The step is tau_scal * tau_diag[0] (its reciprocal under invert_tau): diagsteps = false keeps the preconditioner
// constant over a group.
#ifndef PROST_PROX_ELEMOP_ELEM_OPERATION_SINGULAR_NX2_HPP_
#define PROST_PROX_ELEMOP_ELEM_OPERATION_SINGULAR_NX2_HPP_
#include "prost/prox/elemop/function_2d.hpp"
#include "prost/prox/elemop/spectral_common.hpp"

namespace prost {
namespace elemop {

/// res = prox at arg; RES / ARG are anything indexable (Vector views, register arrays); TF = the type FUN_2D computes in
template <class T, class TF, class RES, class ARG, class FUN_2D>
__host__ __device__ __forceinline__ void SingularNx2Apply(RES& res, const ARG& arg, size_t n, double tau, const T* coeffs, const FUN_2D& fun) {
  double d11 = 0., d12 = 0., d22 = 0.;
  for (size_t i = 0; i < n; i++) {
    const double x = (double)arg[i], y = (double)arg[n + i];
    d11 += x * x; d12 += x * y; d22 += y * y;
  }
  double l1, l2, c, s;
  SymEig2x2(d11, d12, d22, l1, l2, c, s);
  double v1x = c, v1y = -s, v2x = s, v2y = c;        // right singular vectors of l1 and l2
  if (l2 > l1) {
    const double l = l1; l1 = l2; l2 = l;
    v1x = s; v1y = c; v2x = c; v2y = -s;
  }
  const double sig1 = l1 > 0. ? t_sqrt(l1) : 0.;
  const double sig2 = l2 > 1.7763568394002505e-15 * l1 ? t_sqrt(l2) : 0.;      // 8 ulp
  double p[2] = {sig1, sig2};
  const SpectralCoeffs<T> k(coeffs);
  const double den = 1. + tau * k.e;
  if (k.a == 0 || k.c == 0) {
    p[0] = (p[0] - tau * k.d) / den;
    p[1] = (p[1] - tau * k.d) / den;
  } else {
    const TF step = (TF)(k.c * k.a * k.a * tau / den);
    TF x1, x2;
    fun((TF)(k.a * (p[0] - k.d * tau) / den - k.b), (TF)(k.a * (p[1] - k.d * tau) / den - k.b), x1, x2, step, (TF)k.alpha, (TF)k.beta);
    p[0] = ((double)x1 + k.b) / k.a;
    p[1] = ((double)x2 + k.b) / k.a;
  }
  if (sig1 > 0.) {
    const double g1 = p[0] / sig1, g2 = sig2 > 0. ? p[1] / sig2 : 0.;
    const double t11 = g1 * v1x * v1x + g2 * v2x * v2x, t12 = g1 * v1x * v1y + g2 * v2x * v2y, t22 = g1 * v1y * v1y + g2 * v2y * v2y;
    for (size_t i = 0; i < n; i++) {
      const double x = (double)arg[i], y = (double)arg[n + i];
      res[i] = (T)(x * t11 + y * t12);
      res[n + i] = (T)(x * t12 + y * t22);
    }
  } else {
    for (size_t i = 0; i < 2 * n; i++) res[i] = (T)0;
    res[0] = (T)p[0];
    if (n > 1) res[n + 1] = (T)p[1];
  }
}

}  // namespace elemop

template <typename T, class FUN_2D>
struct ElemOperationSingularNx2 : public ElemOperation<0, 7> {
  static const bool kWritesAllComponents = true;
  __host__ __device__ ElemOperationSingularNx2(T* coeffs, size_t dim, SharedMem<SharedMemType, GetSharedMemCount>& /*shared_mem*/)
      : coeffs_(coeffs), dim_(dim) {}

  __host__ __device__ __forceinline__ void operator()(Vector<T>& res, const Vector<const T>& arg, const Vector<const T>& tau_diag, T tau_scal,
                                                      bool invert_tau) {
    elemop::SingularNx2Apply<T, T>(res, arg, dim_ / 2, elemop::SpectralStep(tau_scal, tau_diag[0], invert_tau), coeffs_, FUN_2D());
  }

 private:
  T* coeffs_;
  size_t dim_;
};

}  // namespace prost
#endif
