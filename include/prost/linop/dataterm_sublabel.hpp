// prost/linop/dataterm_sublabel.hpp -- the arithmetic of BlockDatatermSublabel: the coupling between the lifted labelling and the
// epigraph variables of the sublabel-accurate relaxation of a data term (Moellenhoff, Laude, Moeller, Lellmann, Cremers: Sublabel-
// accurate relaxation of nonconvex energies, CVPR 2016).  The reference ships no source for it (its cmake/CustomSources.cmake.example
// names block_dataterm_sublabel as a user add-on); this is written from the definition.
//
// L >= 2 equidistant labels on [left, right]; k = L - 1 intervals per pixel, delta = (right - left) / (L - 1), gamma_i = left + i delta
// (both formed in double on the host, then rounded to T).  N pixels; every part is k planes of N pixels, element (p, i) at i N + p.
// Domain [u ; w] (2 N k), range [r ; s] (2 N k).  With m_i = gamma_i w_i + delta (u_i - sum_{j > i} w_j) the lifted data term is
// sum_i sup_{(r_i, s_i) in epi phi_i*} (m_i r_i - w_i s_i), which is <K [u ; w], [r ; s]> for
//
//   forward  (per pixel):   S_{k-1} = 0,  S_i = S_{i+1} + w_{i+1}        r_i = (delta u_i + gamma_i w_i) - delta S_i      s_i = -w_i
//   adjoint  (per pixel):   P_0 = 0,      P_i = P_{i-1} + r_{i-1}        u_i = delta r_i      w_i = (gamma_i r_i - s_i) - delta P_i
//
// Every operation is one rounding in T in exactly this order (build without contraction); the accumulating forms store res + value.
// This header is the one place that order is written down: the kernels (prost_amd/csrc/kernels_linop_dataterm_sublabel.hip) and the
// host harness (tests/host/dataterm_sublabel_harness.cpp) instantiate the marches below with their own way of moving W neighbouring
// pixels of a plane, tests/dataterm_sublabel_reference.py restates them in NumPy.
//
// A march reads plane i of rhs (and of res, when accumulating) before it writes plane i of res and never returns to a plane, so
// res == rhs (the same pointer) is allowed; any other overlap is not.
#ifndef PROST_LINOP_DATATERM_SUBLABEL_HPP_
#define PROST_LINOP_DATATERM_SUBLABEL_HPP_
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PROST_DTS_HD __host__ __device__ __forceinline__
#else
#define PROST_DTS_HD inline
#endif

namespace prost {
namespace dataterm_sublabel {

/// element access: one pixel per step of the march (any pointer, any N)
struct ElementAccess {
  template <class T> static PROST_DTS_HD void Load(const T* p, T (&v)[1]) { v[0] = p[0]; }
  template <class T> static PROST_DTS_HD void Store(T* p, const T (&v)[1]) { p[0] = v[0]; }
};

template <class T> PROST_DTS_HD T RowR(T delta, T gamma_i, T u, T w, T S) { return (delta * u + gamma_i * w) - delta * S; }
template <class T> PROST_DTS_HD T RowS(T w) { return -w; }
template <class T> PROST_DTS_HD T ColU(T delta, T r) { return delta * r; }
template <class T> PROST_DTS_HD T ColW(T delta, T gamma_i, T r, T s, T P) { return (gamma_i * r - s) - delta * P; }

/// [r ; s] (+)= K [u ; w] for the W pixels p .. p + W - 1: i runs from k - 1 down to 0 with the suffix sum of w in S.  The planes of
/// step i - 1 are requested before step i is computed and stored (one step of look-ahead; the arithmetic does not see it).
template <class T, int W, bool ACC, class A>
PROST_DTS_HD void Forward(T* res, const T* rhs, size_t N, size_t k, size_t p, T delta, const T* __restrict__ gamma) {
  const T* u = rhs + p;
  const T* w = rhs + N * k + p;
  T* r = res + p;
  T* s = res + N * k + p;
  T S[W], un[W], wn[W];
  for (int j = 0; j < W; j++) S[j] = (T)0;
  A::Load(u + (k - 1) * N, un);
  A::Load(w + (k - 1) * N, wn);
  for (size_t i = k; i-- > 0;) {
    T uc[W], wc[W], rv[W], sv[W];
    for (int j = 0; j < W; j++) { uc[j] = un[j]; wc[j] = wn[j]; }
    if (i > 0) { A::Load(u + (i - 1) * N, un); A::Load(w + (i - 1) * N, wn); }
    const T g = gamma[i];
    for (int j = 0; j < W; j++) {
      rv[j] = RowR(delta, g, uc[j], wc[j], S[j]);
      sv[j] = RowS(wc[j]);
      S[j] = S[j] + wc[j];
    }
    if (ACC) {
      T a[W], b[W];
      A::Load(r + i * N, a);
      A::Load(s + i * N, b);
      for (int j = 0; j < W; j++) { rv[j] = a[j] + rv[j]; sv[j] = b[j] + sv[j]; }
    }
    A::Store(r + i * N, rv);
    A::Store(s + i * N, sv);
  }
}

/// [u ; w] (+)= K^T [r ; s] for the W pixels p .. p + W - 1: i runs from 0 up to k - 1 with the prefix sum of r in P
template <class T, int W, bool ACC, class A>
PROST_DTS_HD void Adjoint(T* res, const T* rhs, size_t N, size_t k, size_t p, T delta, const T* __restrict__ gamma) {
  const T* r = rhs + p;
  const T* s = rhs + N * k + p;
  T* u = res + p;
  T* w = res + N * k + p;
  T P[W], rn[W], sn[W];
  for (int j = 0; j < W; j++) P[j] = (T)0;
  A::Load(r, rn);
  A::Load(s, sn);
  for (size_t i = 0; i < k; i++) {
    T rc[W], sc[W], uv[W], wv[W];
    for (int j = 0; j < W; j++) { rc[j] = rn[j]; sc[j] = sn[j]; }
    if (i + 1 < k) { A::Load(r + (i + 1) * N, rn); A::Load(s + (i + 1) * N, sn); }
    const T g = gamma[i];
    for (int j = 0; j < W; j++) {
      uv[j] = ColU(delta, rc[j]);
      wv[j] = ColW(delta, g, rc[j], sc[j], P[j]);
      P[j] = P[j] + rc[j];
    }
    if (ACC) {
      T a[W], b[W];
      A::Load(u + i * N, a);
      A::Load(w + i * N, b);
      for (int j = 0; j < W; j++) { uv[j] = a[j] + uv[j]; wv[j] = b[j] + wv[j]; }
    }
    A::Store(u + i * N, uv);
    A::Store(w + i * N, wv);
  }
}

// sum_j |entry|^alpha of a row / column of plane i (host; pow is a library call).  An entry gamma_i = 0 is absent, as in a sparse matrix.
template <class T> inline T PowAbs(T v, T alpha) { return v == (T)0 ? (T)0 : std::pow(std::abs(v), alpha); }
/// row of r_i: delta (u_i), gamma_i (w_i), -delta (w_j, j > i)
template <class T> inline T RowSumR(size_t i, size_t k, T delta, T gamma_i, T alpha) {
  const T pd = PowAbs(delta, alpha);
  return (pd + PowAbs(gamma_i, alpha)) + (T)(k - 1 - i) * pd;
}
/// row of s_i: -1 (w_i)
template <class T> inline T RowSumS(T /*alpha*/) { return (T)1; }
/// column of u_i: delta (r_i)
template <class T> inline T ColSumU(T delta, T alpha) { return PowAbs(delta, alpha); }
/// column of w_i: gamma_i (r_i), -1 (s_i), -delta (r_j, j < i)
template <class T> inline T ColSumW(size_t i, T delta, T gamma_i, T alpha) {
  return (PowAbs(gamma_i, alpha) + (T)1) + (T)i * PowAbs(delta, alpha);
}

/// delta and the k values gamma_i for L labels on [left, right]: formed in double, then rounded to T
template <class T> inline void Labels(size_t L, double left, double right, T& delta, T* gamma) {
  const double d = (right - left) / (double)(L - 1);
  delta = (T)d;
  for (size_t i = 0; i + 1 < L; i++) gamma[i] = (T)(left + (double)i * d);
}

}  // namespace dataterm_sublabel
}  // namespace prost
#endif
