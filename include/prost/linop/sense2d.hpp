// prost/linop/sense2d.hpp -- the arithmetic of BlockSense2D: the multi-coil Fourier operator of SENSE-type parallel MRI,
//
//   K u = [ F (sigma_1 . u) ; .. ; F (sigma_C . u) ],      K^T y = sum_c conj(sigma_c) . F^H y_c,
//
// with F the unitary 2-D transform of fft2d.hpp, "." the pointwise complex product and one complex sensitivity map sigma_c per coil,
// without a matrix, without an intermediate field of C images and without a separate pointwise pass.  The reference has no such block;
// this is written from the definition.
//
// Sizes: N = nx ny, p = y + x ny; nx and ny are powers of two from 1 to 2048 (fft2d.hpp); C = 1 .. 64 coils; L >= 1 complex images (the
// frames of a dynamic series, several contrasts) share the maps.  Maps: C complex planes, stored as 2 C N values of T, real planes first
// (re sigma_c[p] at c N + p, im sigma_c[p] at (C + c) N + p), each rounded once to T; the operator is DEFINED with the rounded maps.
// Non-finite map values are refused at creation; a map that is zero everywhere is legal.
//
// Domain: that of fft2d(nx, ny, L): re_l[p] at l N + p, im_l[p] at (L + l) N + p.  Range: that of fft2d(nx, ny, L C): image j = l C + c
// holds coil c of image l, re_j[q] at j N + q, im_j[q] at (L C + j) N + q.  2 L C N < 2^31.
//
// Forward.  z = sigma_c u_l per pixel:
//
//   z.re = u.re s.re - u.im s.im,    z.im = u.re s.im + u.im s.re       (Product)
//
// every product and every sum one rounding in T, no contraction.  Then fft2d's product on z: the y pass, the x pass, the scaling by s
// = 1 / sqrt(N).  The forward bits are those of fft2d(nx, ny, L C) on the premultiplied planes.
//
// Transpose.  v_{l,c} = fft2d's transposed product of range image j = l C + c, scaling included.  The term of coil c is
//
//   t.re = v.re s.re + v.im s.im,    t.im = v.im s.re - v.re s.im       (ConjProduct)
//
// and the terms are summed in ascending c starting FROM THE TERM OF COIL 0 (not from zero): sum = t_0, sum = sum + t_1, ..  The plain
// form stores the sum, the accumulating form res + sum.  res, rhs, the maps and the work buffer must not overlap.
//
// A side of 1 has one pass; nx = ny = 1 has none and is the pointwise product (s = 1 exactly).
//
// Signs of zeros.  With C = 1 and sigma = 1 + 0 i every finite value equals that of fft2d(nx, ny, L), but the products with the zero
// imaginary part are not skipped: z.re = u.re - u.im 0 turns u.re = -0 into +0 when u.im 0 = -0 (u.im < 0 or -0), and z.im = u.re 0 +
// u.im turns u.im = -0 into +0 when u.re 0 = +0; likewise in the transposed term.  A non-finite u makes both parts of z NaN, where
// fft2d alone keeps the other part.  A non-finite value of image l reaches the C coil images of l and no other image; a non-finite
// value of coil image (l, c) reaches image l of the transpose only.
//
// Error bound.  u is the unit roundoff, gamma_k = k u / (1 - k u), B the bound of fft2d.hpp (|fl(F x) - F x|_2 <= B |x|_2 per image,
// B = 2 u without a pass).  The computed complex product is fl(a b) = a b (1 + d), |d| <= sqrt(2) gamma_2 (Higham, Accuracy and Stability
// of Numerical Algorithms, 2nd ed., Lemma 3.5), so the premultiplied image is off by at most sqrt(2) gamma_2 |sigma_c . u_l|_2, and F is
// unitary:
//
//   forward, per coil image:   |fl(K u)_{l,c} - (K u)_{l,c}|_2 <= Bf |sigma_c . u_l|_2 <= Bf m_c |u_l|_2,
//                              Bf = B + sqrt(2) gamma_2 (1 + B),   m_c = max_p |sigma_c[p]|.
//
// Transposed, the computed v_{l,c} is within B |y_{l,c}|_2 of the exact one and has at most (1 + B) |y_{l,c}|_2; its term is off by the
// product's sqrt(2) gamma_2 |sigma_c| |v|; the C - 1 additions of the coil sum add gamma_{C-1} sum_c |t_c| per component (Higham, (4.4)):
//
//   transposed, per image:     |fl(K^T y)_l - (K^T y)_l|_2 <= Bt sum_c m_c |y_{l,c}|_2,   Bt = Bf + gamma_{C-1} (1 + Bf).
//
// Sums for the preconditioners.  These are NOT the sums of the explicit matrix.  Row (l, c, q) of the real matrix holds, over the
// pixels p, the entries s |sigma_c(p)| |cos psi| and s |sigma_c(p)| |sin psi| with psi = theta_q(p) - arg sigma_c(p): the phase of the
// map shifts every angle by a different amount, fft2d's period classes are gone, and a closed form for sum |K|^e exists only at e = 2
// (cos^2 + sin^2 = 1); an enumeration costs O(N^2).  The block therefore returns upper BOUNDS, from 1 <= |cos|^e + |sin|^e <=
// 2^(1 - e/2) for e <= 2 and 2^(1 - e/2) <= |cos|^e + |sin|^e <= 1 for e >= 2:
//
//   row sum, the same for every row of coil c:   Rbar_c(e)   = f(e) s^e   sum_p |sigma_c(p)|^e
//   column sum of pixel p:                       Cbar(p, e)  = f(e) s^e N sum_c |sigma_c(p)|^e,       f(e) = max(1, 2^(1 - e/2)),
//
// an exactly zero |sigma| absent from the sum.  At e = 2 they are the matrix's sums, s^2 sum_p |sigma_c|^2 and sum_c |sigma_c(p)|^2;
// elsewhere S <= Sbar <= 2^|1 - e/2| S, at most a factor sqrt(2) at e = 1.  An upper bound on both sums only shrinks the diagonal steps:
// the proof of |Sigma^(1/2) K T^(1/2)| <= 1 (Pock & Chambolle, ICCV 2011, Lemma 2) bounds each entry's share by the sums from above and
// goes through unchanged with 1 / Sbar in place of 1 / S.  |sigma|^e is evaluated in float64 as (re^2 + im^2)^(e/2) on the rounded maps,
// and the sums over p and over c are compensated (Neumaier), so that they do not depend on N beyond a few ulps.
#ifndef PROST_LINOP_SENSE2D_HPP_
#define PROST_LINOP_SENSE2D_HPP_
#include "prost/linop/fft2d.hpp"

namespace prost {
namespace sense2d {

constexpr int kMaxCoils = 64;

/// the operator (the layout of prost_hip_sense2d_geometry in prost_hip.h)
struct Geometry {
  int32_t ny, nx;         ///< image plane, each a power of two from 1 to 2048
  int32_t planes;         ///< L complex images
  int32_t coils;          ///< C sensitivity maps, 1 .. 64
  int32_t transpose;      ///< 0: res = K rhs, else res = K^T rhs
  int32_t slab;           ///< tile of the coil-summing pass on the device: 0 the kernel file's choice, 1 the small tile, 2 fft2d's; no bit depends on it
};

inline Geometry MakeGeometry(long ny, long nx, long planes, long coils, bool transpose) {
  Geometry g;
  g.ny = (int32_t)ny; g.nx = (int32_t)nx; g.planes = (int32_t)planes; g.coils = (int32_t)coils; g.transpose = transpose ? 1 : 0; g.slab = 0;
  return g;
}
/// fft2d's geometry on the L C range images
PROST_FFT_HD fft2d::Geometry RangeGeometry(const Geometry& g, bool transpose) {
  fft2d::Geometry f;
  f.ny = g.ny; f.nx = g.nx; f.planes = g.planes * g.coils; f.transpose = transpose ? 1 : 0;
  return f;
}

/// z = sigma u
template <class T> PROST_FFT_HD fft2d::Cx<T> Product(fft2d::Cx<T> u, T sr, T si) {
  const T p0 = u.re * sr, p1 = u.im * si, p2 = u.re * si, p3 = u.im * sr;
  fft2d::Cx<T> z;
  z.re = p0 - p1; z.im = p2 + p3;
  return z;
}
/// t = conj(sigma) v
template <class T> PROST_FFT_HD fft2d::Cx<T> ConjProduct(fft2d::Cx<T> v, T sr, T si) {
  const T p0 = v.re * sr, p1 = v.im * si, p2 = v.im * sr, p3 = v.re * si;
  fft2d::Cx<T> t;
  t.re = p0 + p1; t.im = p2 - p3;
  return t;
}

#if !defined(__HIP_DEVICE_COMPILE__)
/// the product on the host: res (+)= K rhs (2 L C N values from 2 L N) or K^T rhs (2 L N values from 2 L C N); table from
/// fft2d::MakeTable<T>(TableSize(ny, nx)); maps: 2 C N values of T, real planes first
template <class T, bool ACC> inline void Apply(T* res, const T* rhs, const Geometry& g, const T* table, const T* maps, bool transpose) {
  const size_t N = (size_t)g.ny * (size_t)g.nx, L = (size_t)g.planes, C = (size_t)g.coils, J = L * C;
  const fft2d::Geometry f = RangeGeometry(g, transpose);
  std::vector<T> work(2 * J * N);
  if (!transpose) {
    for (size_t l = 0; l < L; l++)
      for (size_t c = 0; c < C; c++)
        for (size_t p = 0; p < N; p++) {
          const fft2d::Cx<T> u = {rhs[l * N + p], rhs[(L + l) * N + p]};
          const fft2d::Cx<T> z = Product<T>(u, maps[c * N + p], maps[(C + c) * N + p]);
          work[(l * C + c) * N + p] = z.re; work[(J + l * C + c) * N + p] = z.im;
        }
    fft2d::Apply<T, ACC>(res, work.data(), f, table, false);
    return;
  }
  fft2d::Apply<T, false>(work.data(), rhs, f, table, true);
  for (size_t l = 0; l < L; l++)
    for (size_t p = 0; p < N; p++) {
      fft2d::Cx<T> sum = {(T)0, (T)0};
      for (size_t c = 0; c < C; c++) {
        const fft2d::Cx<T> v = {work[(l * C + c) * N + p], work[(J + l * C + c) * N + p]};
        const fft2d::Cx<T> t = ConjProduct<T>(v, maps[c * N + p], maps[(C + c) * N + p]);
        if (c == 0) sum = t;
        else { sum.re = sum.re + t.re; sum.im = sum.im + t.im; }
      }
      T *orr = res + l * N + p, *oi = res + (L + l) * N + p;
      *orr = ACC ? *orr + sum.re : sum.re;
      *oi = ACC ? *oi + sum.im : sum.im;
    }
}

/// a compensated sum (Neumaier): the result is within a few ulps of the exact sum of non-negative terms, whatever their number
struct Compensated {
  double sum = 0, comp = 0;
  void Add(double v) {
    const double t = sum + v;
    comp += std::fabs(sum) >= std::fabs(v) ? (sum - t) + v : (v - t) + sum;
    sum = t;
  }
  double Value() const { return sum + comp; }
};

/// |sigma|^e of the rounded map value, in float64; 0 for an exactly zero value
template <class T> inline double AbsPow(T re, T im, double e) {
  const double q = (double)re * (double)re + (double)im * (double)im;
  return q == 0 ? 0.0 : (e == 2 ? q : std::pow(q, 0.5 * e));
}
/// f(e) s^e
inline double SumFactor(int ny, int nx, double e) {
  const double s = 1.0 / std::sqrt((double)ny * (double)nx);
  return std::fmax(1.0, std::pow(2.0, 1.0 - 0.5 * e)) * (e == 2 ? s * s : std::pow(s, e));
}
/// Rbar_c(e), the bound on the sum of |K|^e over every row of coil c
template <class T> inline double RowBound(const T* maps, const Geometry& g, double e, int c) {
  const size_t N = (size_t)g.ny * (size_t)g.nx, C = (size_t)g.coils;
  Compensated acc;
  for (size_t p = 0; p < N; p++) acc.Add(AbsPow<T>(maps[(size_t)c * N + p], maps[(C + (size_t)c) * N + p], e));
  return SumFactor(g.ny, g.nx, e) * acc.Value();
}
/// Cbar(p, e), the bound on the sum of |K|^e over the two columns of pixel p
template <class T> inline double ColBound(const T* maps, const Geometry& g, double e, size_t p) {
  const size_t N = (size_t)g.ny * (size_t)g.nx, C = (size_t)g.coils;
  Compensated acc;
  for (size_t c = 0; c < C; c++) acc.Add(AbsPow<T>(maps[c * N + p], maps[(C + c) * N + p], e));
  return SumFactor(g.ny, g.nx, e) * (double)N * acc.Value();
}
#endif

}  // namespace sense2d
}  // namespace prost
#endif
