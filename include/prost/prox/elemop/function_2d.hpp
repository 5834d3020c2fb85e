// prost/prox/elemop/function_2d.hpp -- proximal maps of functions of TWO values (the singular values of an n x 2 matrix).
//
// Plugin contract of the reference's include/prost/prox/elemop/function_2d.hpp: a Function2D*<T> has
//   void operator()(T y1, T y2, T& x1, T& x2, T tau, T alpha, T beta) const
// with (x1, x2) = argmin  tau f(x1, x2) + |x - y|^2 / 2.  ElemOperationSingularNx2 (elem_operation_singular_nx2.hpp)
// composes with any of them, or with a user's own struct of that signature.
//   Function2DSum1D<T, FUN_1D>      f(x1, x2) = g(x1) + g(x2), g a Function1D* of function_1d.hpp
//   Function2DIndL1Ball<T>          indicator of |x1| + |x2| <= alpha
//   Function2DMoreau<T, OTHER>      the conjugate of OTHER through Moreau's identity
#ifndef PROST_PROX_ELEMOP_FUNCTION_2D_HPP_
#define PROST_PROX_ELEMOP_FUNCTION_2D_HPP_
#include "prost/prox/elemop/function_1d.hpp"

namespace prost {

template <typename T, class FUN_1D>
struct Function2DSum1D {
  __host__ __device__ __forceinline__ void operator()(T y1, T y2, T& x1, T& x2, T tau, T alpha, T beta) const {
    FUN_1D fun;
    x1 = fun(y1, tau, alpha, beta);
    x2 = fun(y2, tau, alpha, beta);
  }
};

/// Euclidean projection of (y1, y2) onto the l1 ball of radius alpha.  Outside the ball both magnitudes shrink by the same
/// theta and are clipped at zero: theta = (|y1| + |y2| - alpha) / 2 while the smaller magnitude survives that, otherwise the
/// smaller one goes to zero and the larger one lands on alpha.
template <typename T>
struct Function2DIndL1Ball {
  __host__ __device__ __forceinline__ void operator()(T y1, T y2, T& x1, T& x2, T /*tau*/, T alpha, T /*beta*/) const {
    const T m1 = elemop::t_abs(y1), m2 = elemop::t_abs(y2);
    if (m1 + m2 <= alpha) { x1 = y1; x2 = y2; return; }
    const T hi = m1 > m2 ? m1 : m2, lo = m1 > m2 ? m2 : m1;
    const T both = (hi + lo - alpha) / 2;
    const T theta = lo > both ? both : hi - alpha;
    const T r1 = m1 - theta, r2 = m2 - theta;
    x1 = r1 > 0 ? (y1 < 0 ? -r1 : r1) : (T)0;
    x2 = r2 > 0 ? (y2 < 0 ? -r2 : r2) : (T)0;
  }
};

/// prox of the conjugate: x = y - tau prox_{f / tau}(y / tau)
template <typename T, class OTHER_FUN_2D>
struct Function2DMoreau {
  __host__ __device__ __forceinline__ void operator()(T y1, T y2, T& x1, T& x2, T tau, T alpha, T beta) const {
    OTHER_FUN_2D other;
    T r1, r2;
    other(y1 / tau, y2 / tau, r1, r2, 1 / tau, alpha, beta);
    x1 = y1 - tau * r1;
    x2 = y2 - tau * r2;
  }
};

}  // namespace prost
#endif
