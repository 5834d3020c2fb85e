// prost/prox/epi_polyhedral.hpp -- the arithmetic of ProxIndEpiPolyhedral: the projection of z0 = (x_1 .. x_d, y), d = DIM - 1, onto
// the epigraph { y >= max_i <a_i, x> - b_i } of a convex piecewise-linear function with k pieces.  Host and device templates:
// prost_amd/csrc/kernels_prox_epi_polyhedral.hip runs them with a few lanes per group, tests/host/epi_polyhedral_harness.cpp in a
// plain loop under the sanitizers.  Nothing here allocates, loops over the constraint list or knows about lanes: the caller owns the
// step loop and the scan for the most violated constraint, and hands the chosen constraint in.
//
// The method is a dual active-set projection (Goldfarb-Idnani with the identity as Hessian).  Constraint i reads <n_i, z> <= b_i
// with the normal n_i = (a_i, -1).  The state is the point z, at most DIM active constraints with multipliers u >= 0, and possibly
// one pending constraint p that is violated at z and on its way into the active set:
//   z = z0 - sum_s u_s n_s - u_p n_p,   <n_s, z> = b_s for every active s.
// One step (ActiveSet::Step) solves G r = N n_p for the Gram matrix G = N N' of the active normals -- from scratch, by an unrolled
// Cholesky factorisation of the DIM x DIM matrix in which an empty slot is a row of the identity -- and forms d = n_p - N' r, the
// part of n_p orthogonal to the active normals.  Raising u_p by t moves z by -t d and u by -t r.  The step ends where p becomes
// tight (t2 = violation / |d|^2: p joins the active set) or where an active multiplier reaches zero first (t1 = min u_s / r_s over
// r_s > 0: that constraint is dropped and p stays pending).  A normal that is, up to rounding, in the span of the active ones
// (|d|^2 <= (kDepFactor eps)^2 |n_p|^2, or DIM constraints active already) has no t2: it can only enter through a drop.  This is how
// duplicates, parallel facets and more than DIM facets meeting at an apex are handled; nothing divides by |d|^2 ~ 0.  The last
// components of all normals are -1, so the entries of r add up to 1 whenever d = 0, and a drop candidate exists.
//
// When no constraint is violated any more, the caller runs Polish() once: z moves onto the active hyperplanes,
// z -= N' G^-1 (N z - b).  The steps subtract large moves from a large z0 (a point at distance 1000 from an answer of size 1 loses
// three digits of it on the way), and a constraint that drifted to the feasible side is never looked at again; the residual N z - b
// is formed from the small z, so at a vertex the answer is as accurate as its own size allows.  The caller scans once more after it.
//
// A constraint counts as violated when <a_i, x> - y - b_i > kTolFactor eps (sum_j |a_ij x_j| + |y| + |b_i|): the rounding error of
// that expression stays below (d + 2) eps / 2 of the same sum, so a feasible point is recognised as feasible and returned unchanged.
//
// All loops run over compile-time bounds and are fully unrolled; the active set is edited by selects on compile-time slots, so on the
// device it stays in registers.
#ifndef PROST_PROX_EPI_POLYHEDRAL_HPP_
#define PROST_PROX_EPI_POLYHEDRAL_HPP_
#include <cmath>
#include <cstddef>
#include <limits>

#if defined(__HIPCC__)
#define PROST_EPI_HD __host__ __device__ __forceinline__
#define PROST_EPI_UNROLL _Pragma("unroll")
#else
#define PROST_EPI_HD inline
#define PROST_EPI_UNROLL
#endif

namespace prost {
namespace epi {

constexpr int kMinDim = 2, kMaxDim = 4;    ///< supported group sizes (d = 1 .. 3 coefficients per constraint)
constexpr int kTolFactor = 4;              ///< violations are judged against kTolFactor eps (sum |a_ij x_j| + |y| + |b_i|)
constexpr int kDepFactor = 64;             ///< |d| <= kDepFactor eps |n_p|: n_p counts as dependent on the active normals
constexpr int kStepCapA = 10;              ///< the step loop stops after kStepCapA (k + DIM) + kStepCapB steps
constexpr int kStepCapB = 0;
// One lane per kConstraintsPerLane constraints of the longest list.  Measured at 2^20 groups of 25 constraints (fp32, dim 2, per-group
// lists / one shared list; docs/rounds/r14.md): 1 per lane 1.04 / 1.02 ms, 2: 0.66 / 0.63, 4: 0.43 / 0.39, 8: 0.30 / 0.25, 16: 0.41 / 0.18, 32 (one
// lane per group): 1.56 / 0.15 -- every lane repeats the solve, so fewer lanes win until a lane walks a private list nearly alone and
// its loads no longer coalesce; a shared list would like one lane, private lists four.  The macro exists for that measurement.
#ifndef PROST_EPI_CONSTRAINTS_PER_LANE
#define PROST_EPI_CONSTRAINTS_PER_LANE 8
#endif
constexpr int kConstraintsPerLane = PROST_EPI_CONSTRAINTS_PER_LANE;
constexpr int kMaxLanes = 64;

/// lanes that share a group: the smallest power of two with kConstraintsPerLane lanes >= max_count, at most a wave
inline int LanesPerGroup(size_t max_count) {
  int g = 1;
  while (g < kMaxLanes && (size_t)g * kConstraintsPerLane < max_count) g *= 2;
  return g;
}
/// the hard cap on the steps of one group with k constraints
PROST_EPI_HD int StepCap(int k, int dim) { return kStepCapA * (k + dim) + kStepCapB; }

template <class T> PROST_EPI_HD T Eps() { return std::numeric_limits<T>::epsilon(); }
template <class T> PROST_EPI_HD T Abs(T v) { return v < (T)0 ? -v : v; }

/// <a, x> - y - b and whether it counts as violated at z = (x, y).  a: DIM - 1 coefficients.
template <class T, int DIM>
PROST_EPI_HD bool Violation(const T (&z)[DIM], const T* a, T b, T& v) {
  T s = 0, mag = 0;
  PROST_EPI_UNROLL
  for (int j = 0; j < DIM - 1; j++) { const T p = a[j] * z[j]; s += p; mag += Abs(p); }
  v = s - z[DIM - 1] - b;
  mag += Abs(z[DIM - 1]) + Abs(b);
  return v > (T)kTolFactor * Eps<T>() * mag;
}

enum StepResult { kAdded = 0, kDropped = 1, kStuck = 2 };

template <class T, int DIM>
struct ActiveSet {
  static constexpr int D = DIM - 1;
  T z[DIM];              ///< the current point
  T a[DIM][D];           ///< slot s: the coefficients of its constraint (the normal is (a, -1))
  T bs[DIM];             ///< slot s: the right-hand side of its constraint
  T u[DIM];              ///< slot s: its multiplier
  bool on[DIM];          ///< slot s holds an active constraint
  T pa[D], pb, pu;       ///< the pending constraint and the multiplier it has gathered
  bool pending;
  bool polished;         ///< Polish() has run
  int steps;

  PROST_EPI_HD void Init(const T (&z0)[DIM]) {
    PROST_EPI_UNROLL
    for (int j = 0; j < DIM; j++) z[j] = z0[j];
    PROST_EPI_UNROLL
    for (int s = 0; s < DIM; s++) {
      on[s] = false; u[s] = 0; bs[s] = 0;
      PROST_EPI_UNROLL
      for (int j = 0; j < D; j++) a[s][j] = 0;
    }
    PROST_EPI_UNROLL
    for (int j = 0; j < D; j++) pa[j] = 0;
    pb = 0; pu = 0; pending = false; polished = false; steps = 0;
  }

  /// the most violated constraint, found by the caller, becomes the pending one
  PROST_EPI_HD void Begin(const T* an, T bn) {
    PROST_EPI_UNROLL
    for (int j = 0; j < D; j++) pa[j] = an[j];
    pb = bn; pu = 0; pending = true;
  }

  /// r := G^-1 r for the Gram matrix G of the active normals, an empty slot being a row of the identity (r is 0 there): an
  /// unrolled Cholesky factorisation from scratch and the two substitutions
  PROST_EPI_HD void SolveGram(T (&r)[DIM]) const {
    const T eps = Eps<T>();
    T L[DIM][DIM], inv[DIM];
    PROST_EPI_UNROLL
    for (int s = 0; s < DIM; s++) {
      PROST_EPI_UNROLL
      for (int t = 0; t <= s; t++) {
        T g = 1;
        PROST_EPI_UNROLL
        for (int j = 0; j < D; j++) g += a[s][j] * a[t][j];
        L[s][t] = (on[s] && on[t]) ? g : (s == t ? (T)1 : (T)0);
      }
    }
    PROST_EPI_UNROLL
    for (int j = 0; j < DIM; j++) {
      T p = L[j][j];
      PROST_EPI_UNROLL
      for (int k = 0; k < j; k++) p -= L[j][k] * L[j][k];
      p = p > eps * eps ? p : eps * eps;               // active normals are independent by construction; this only keeps a NaN out
      const T root = std::sqrt(p);
      inv[j] = (T)1 / root;
      L[j][j] = root;
      PROST_EPI_UNROLL
      for (int i = j + 1; i < DIM; i++) {
        T s = L[i][j];
        PROST_EPI_UNROLL
        for (int k = 0; k < j; k++) s -= L[i][k] * L[j][k];
        L[i][j] = s * inv[j];
      }
    }
    PROST_EPI_UNROLL
    for (int j = 0; j < DIM; j++) {
      T s = r[j];
      PROST_EPI_UNROLL
      for (int k = 0; k < j; k++) s -= L[j][k] * r[k];
      r[j] = s * inv[j];
    }
    PROST_EPI_UNROLL
    for (int j = DIM - 1; j >= 0; j--) {
      T s = r[j];
      PROST_EPI_UNROLL
      for (int k = j + 1; k < DIM; k++) s -= L[k][j] * r[k];
      r[j] = s * inv[j];
    }
  }

  /// once, when nothing is violated any more: z onto the active hyperplanes.  false (z untouched) without active constraints.
  PROST_EPI_HD bool Polish() {
    polished = true;
    T r[DIM];
    bool any = false;
    PROST_EPI_UNROLL
    for (int s = 0; s < DIM; s++) {
      T v = -z[D] - bs[s];
      PROST_EPI_UNROLL
      for (int j = 0; j < D; j++) v += a[s][j] * z[j];
      r[s] = on[s] ? v : (T)0;
      any = any || on[s];
    }
    if (!any) return false;
    SolveGram(r);
    PROST_EPI_UNROLL
    for (int s = 0; s < DIM; s++) {
      PROST_EPI_UNROLL
      for (int j = 0; j < D; j++) z[j] -= r[s] * a[s][j];
      z[D] += r[s];
    }
    return true;
  }

  /// one step with the pending constraint: kAdded (it is active now), kDropped (an active constraint left, p stays pending) or
  /// kStuck (neither step length exists: only non-finite data gets here)
  PROST_EPI_HD StepResult Step() {
    const T eps = Eps<T>();
    steps++;
    // right-hand side N n_p
    T r[DIM];
    int q = 0;
    PROST_EPI_UNROLL
    for (int s = 0; s < DIM; s++) {
      q += on[s] ? 1 : 0;
      T g = 1;
      PROST_EPI_UNROLL
      for (int j = 0; j < D; j++) g += a[s][j] * pa[j];
      r[s] = on[s] ? g : (T)0;
    }
    SolveGram(r);
    // d = n_p - N' r
    T d[DIM], nn = 1, dd = 0, rmax = 0;
    PROST_EPI_UNROLL
    for (int j = 0; j < D; j++) { d[j] = pa[j]; nn += pa[j] * pa[j]; }
    d[D] = -1;
    PROST_EPI_UNROLL
    for (int s = 0; s < DIM; s++) {
      PROST_EPI_UNROLL
      for (int j = 0; j < D; j++) d[j] -= r[s] * a[s][j];
      d[D] += r[s];
      rmax = Abs(r[s]) > rmax ? Abs(r[s]) : rmax;
    }
    PROST_EPI_UNROLL
    for (int j = 0; j < DIM; j++) dd += d[j] * d[j];
    const T dep = (T)kDepFactor * eps;
    const bool independent = q < DIM && dd > dep * dep * nn;
    // step lengths
    T v;
    Violation<T, DIM>(z, pa, pb, v);
    v = v > (T)0 ? v : (T)0;
    const T t2 = v / (independent ? dd : (T)1);
    T t1 = 0;
    int drop = -1;
    PROST_EPI_UNROLL
    for (int s = 0; s < DIM; s++) {
      if (on[s] && r[s] > dep * rmax) {
        const T ratio = u[s] / r[s];
        if (drop < 0 || ratio < t1) { t1 = ratio; drop = s; }
      }
    }
    if (!independent && drop < 0) return kStuck;
    const bool full = independent && (drop < 0 || t2 <= t1);
    const T t = full ? t2 : t1;
    if (independent) {
      PROST_EPI_UNROLL
      for (int j = 0; j < DIM; j++) z[j] -= t * d[j];
    }
    PROST_EPI_UNROLL
    for (int s = 0; s < DIM; s++) {
      const T un = u[s] - t * r[s];
      u[s] = (on[s] && un > (T)0) ? un : (T)0;
    }
    pu += t;
    if (full) {
      bool placed = false;
      PROST_EPI_UNROLL
      for (int s = 0; s < DIM; s++) {
        const bool here = !placed && !on[s];
        PROST_EPI_UNROLL
        for (int j = 0; j < D; j++) a[s][j] = here ? pa[j] : a[s][j];
        bs[s] = here ? pb : bs[s];
        u[s] = here ? pu : u[s];
        on[s] = on[s] || here;
        placed = placed || here;
      }
      pending = false;
      return kAdded;
    }
    PROST_EPI_UNROLL
    for (int s = 0; s < DIM; s++) {
      const bool here = s == drop;
      on[s] = on[s] && !here;
      u[s] = here ? (T)0 : u[s];
    }
    return kDropped;
  }
};

/// what a group that reached the cap writes: (x0, max(y0, worst)) with worst = max_i <a_i, x0> - b_i, found by the caller
template <class T, int DIM>
PROST_EPI_HD void Fallback(const T (&z0)[DIM], T worst, T (&z)[DIM]) {
  PROST_EPI_UNROLL
  for (int j = 0; j < DIM - 1; j++) z[j] = z0[j];
  z[DIM - 1] = z0[DIM - 1] > worst ? z0[DIM - 1] : worst;
}

}  // namespace epi
}  // namespace prost
#endif
