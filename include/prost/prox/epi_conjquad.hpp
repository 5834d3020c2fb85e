// prost/prox/epi_conjquad.hpp -- the arithmetic of ProxIndEpiConjQuad1D: the projection of z0 = (y0, t0) onto the epigraph
// { (y, t) : t >= phi*(y) } of the conjugate of one quadratic piece, phi(x) = a x^2 + b x + c on [alpha, beta] (+inf elsewhere),
// a >= 0, alpha <= beta.  Host and device templates: prost_amd/csrc/kernels_prox_epi_conjquad.hip runs them with one group per lane,
// tests/host/epi_conjquad_harness.cpp in a plain loop under the sanitizers, tests/epi_conjquad_reference.py restates them operation
// for operation.  Nothing here allocates or knows about lanes; the caller owns the Newton loop (Projector::Begin, then Step while
// `pending`, under its own cap), so that a wave can run it in lockstep.
//
// With y_a = 2 a alpha + b and y_b = 2 a beta + b the conjugate has three pieces and is C^1 for a > 0:
//   phi*(y) = alpha y - phi(alpha)      y <= y_a          left ray, slope alpha
//           = (y - b)^2 / (4 a) - c     y_a < y < y_b     arc
//           = beta y - phi(beta)        y >= y_b          right ray, slope beta
// (a = 0 or alpha = beta: y_a = y_b, no arc; alpha = -inf / beta = +inf with a > 0: that ray is absent).  Regions of z0, with
// P_a = (y_a, phi*(y_a)), P_b = (y_b, phi*(y_b)):
//   inside   t0 >= phi*(y0): z0 comes back bit for bit
//   left     t0 < alpha y0 - phi(alpha)  and  (y0 - y_a) + alpha (t0 - P_a.t) <= 0: onto the halfspace alpha y - t <= phi(alpha)
//   right    t0 < beta y0 - phi(beta)    and  (y0 - y_b) + beta (t0 - P_b.t) >= 0: onto the halfspace beta y - t <= phi(beta)
//   vertex   a == 0 and none of the above: (b, -c)
//   arc      otherwise: onto the epigraph of the full parabola
// The "below its own line" halves matter: the tangential test alone also holds on the inward extension of a ray's normal, which for
// alpha < 0 < beta leaves the epigraph through the other ray; a point far up on the right would land on the left ray.
//
// Arc: u = y - b, s = t + c, q = 1 / (4 a).  The nearest point of s = q u^2 to (u0, s0) has |u| = the only positive root of
//   g(u) = 2 q^2 u^3 + k u - |u0|,  k = 1 - 2 q s0,
// the sign of u0, and s = q u^2 (u0 == 0: the apex).  g is convex on u >= 0 with g(0) < 0 < g(|u0|) for a point outside, so Newton
// from any point right of the root descends monotonically to it; it stops when the iterate no longer decreases.  The start is the
// smallest of a few cheap upper bounds of the root (ArcStart): from |u0| alone Newton contracts only by 2/3 per step while the cubic
// term dominates.  No libm call beyond sqrt, cbrt and fabs-like selects; compiles under -ffp-contract=off like the rest.
#ifndef PROST_PROX_EPI_CONJQUAD_HPP_
#define PROST_PROX_EPI_CONJQUAD_HPP_
#include <cmath>
#include <cstddef>
#include <limits>

#if defined(__HIPCC__)
#define PROST_ECQ_HD __host__ __device__ __forceinline__
#else
#define PROST_ECQ_HD inline
#endif

namespace prost {
namespace epi_conjquad {

/// the Newton loop of one group stops after kStepCap steps (the most any test input needs is in docs/rounds/r15.md); a group that
/// gets there writes the feasible point (y0, max(t0, phi*(y0))) and is counted
constexpr int kStepCap = 32;

enum Region { kInside = 0, kLeft = 1, kRight = 2, kVertex = 3, kArc = 4 };

template <class T> PROST_ECQ_HD T Abs(T v) { return v < (T)0 ? -v : v; }
template <class T> PROST_ECQ_HD T Min(T x, T y) { return y < x ? y : x; }
template <class T> PROST_ECQ_HD T Max(T x, T y) { return y > x ? y : x; }

/// one group's coefficients and what the regions need of them
template <class T>
struct Piece {
  T a, b, c, alpha, beta;
  bool has_left, has_right;      ///< the bound is finite: the ray exists
  T ya, yb;                      ///< 2 a alpha + b, 2 a beta + b (the infinite bound itself where the ray is absent)
  T fa, fb;                      ///< phi(alpha), phi(beta) (0 where the ray is absent)

  PROST_ECQ_HD void Set(T a_, T b_, T c_, T alpha_, T beta_) {
    const T inf = std::numeric_limits<T>::infinity();
    a = a_; b = b_; c = c_; alpha = alpha_; beta = beta_;
    has_left = alpha > -inf; has_right = beta < inf;
    const T al = has_left ? alpha : (T)0, be = has_right ? beta : (T)0;
    ya = has_left ? ((T)2 * a) * al + b : -inf;
    yb = has_right ? ((T)2 * a) * be + b : inf;
    fa = (a * al + b) * al + c;
    fb = (a * be + b) * be + c;
  }
  /// phi*(y)
  PROST_ECQ_HD T Conj(T y) const {
    if (y <= ya) return alpha * y - fa;
    if (y >= yb) return beta * y - fb;
    const T u = y - b;
    return (u * u) / ((T)4 * a) - c;       // y_a < y < y_b: a > 0
  }
};

/// an upper bound of the positive root of 2 q^2 u^3 + k u - w (w = |u0| > 0), never above w
template <class T>
PROST_ECQ_HD T ArcStart(T q, T k, T w) {
  const T q2 = q * q;
  if (k >= (T)0) {
    // both terms are non-negative right of 0: each alone bounds the root
    T s = Min(w, (T)std::cbrt(w / ((T)2 * q2)));
    if (k > (T)1) s = Min(s, w / k);
    return s;
  }
  // 2 q^2 r^3 = w + |k| r <= 2 max(w, |k| r)
  return Min(w, Max((T)std::cbrt(w / q2), (T)std::sqrt(-k) / q));
}

template <class T>
struct Projector {
  T y, t;              ///< the answer (complete once pending is false)
  T q, k, w, u;        ///< arc: 1 / (4 a), 1 - 2 q s0, |u0|, the Newton iterate
  bool neg;            ///< arc: u0 < 0
  bool pending;        ///< arc: the Newton loop has not finished
  int region, steps;

  /// classifies z0 and finishes every region but the arc, whose Newton loop the caller runs
  PROST_ECQ_HD void Begin(const Piece<T>& p, T y0, T t0) {
    y = y0; t = t0; q = 0; k = 0; w = 0; u = 0; neg = false; pending = false; steps = 0;
    if (t0 >= p.Conj(y0)) { region = kInside; return; }
    if (p.has_left) {
      const T viol = (p.alpha * y0 - t0) - p.fa;
      const T pat = p.alpha * p.ya - p.fa;
      if (viol > (T)0 && (y0 - p.ya) + p.alpha * (t0 - pat) <= (T)0) {
        const T m = viol / (p.alpha * p.alpha + (T)1);
        y = y0 - m * p.alpha; t = t0 + m; region = kLeft;
        return;
      }
    }
    if (p.has_right) {
      const T viol = (p.beta * y0 - t0) - p.fb;
      const T pbt = p.beta * p.yb - p.fb;
      if (viol > (T)0 && (y0 - p.yb) + p.beta * (t0 - pbt) >= (T)0) {
        const T m = viol / (p.beta * p.beta + (T)1);
        y = y0 - m * p.beta; t = t0 + m; region = kRight;
        return;
      }
    }
    if (!(p.a > (T)0)) { y = p.b; t = -p.c; region = kVertex; return; }
    region = kArc;
    const T u0 = y0 - p.b, s0 = t0 + p.c;
    neg = u0 < (T)0;
    w = Abs(u0);
    if (!(w > (T)0)) { y = p.b; t = -p.c; return; }      // below the apex
    q = (T)1 / ((T)4 * p.a);
    k = (T)1 - ((T)2 * q) * s0;
    u = ArcStart(q, k, w);
    pending = true;
  }
  /// one Newton step; finishes (and writes the answer) when the iterate no longer decreases
  PROST_ECQ_HD void Step(const Piece<T>& p) {
    steps++;
    const T q2 = q * q, uu = u * u;
    const T g = (((T)2 * q2) * uu + k) * u - w;
    const T gp = ((T)6 * q2) * uu + k;
    const T next = u - g / gp;
    if (gp > (T)0 && next < u && next > (T)0) { u = next; return; }
    Finish(p);
  }
  PROST_ECQ_HD void Finish(const Piece<T>& p) {
    y = p.b + (neg ? -u : u);
    t = q * (u * u) - p.c;
    pending = false;
  }
  /// the cap was reached: the feasible point straight above z0
  PROST_ECQ_HD void Fallback(const Piece<T>& p, T y0, T t0) {
    y = y0; t = Max(t0, p.Conj(y0)); pending = false;
  }
};

/// the whole projection in a plain loop (host harness); capped: the group reached `cap` and holds the fallback point
template <class T>
inline int Project(const Piece<T>& p, T y0, T t0, int cap, T& y, T& t, int& steps, bool& capped) {
  Projector<T> st;
  st.Begin(p, y0, t0);
  capped = false;
  for (int it = 0; it < cap && st.pending; it++) st.Step(p);
  if (st.pending) { st.Fallback(p, y0, t0); capped = true; }
  y = st.y; t = st.t; steps = st.steps;
  return st.region;
}

}  // namespace epi_conjquad
}  // namespace prost
#endif
