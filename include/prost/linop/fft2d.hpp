// prost/linop/fft2d.hpp -- the arithmetic of BlockFFT2D: the unitary 2-D discrete Fourier transform of L complex images and its
// transpose (the unitary inverse transform), without a matrix.  The reference has no such block; this is written from the definition.
//
// Domain: L complex images of ny x nx as 2 L real planes, real parts first: re_c[p] at c N + p, im_c[p] at (L + c) N + p, N = nx ny,
// p = y + x ny (the domain layout of gradient2d(nx, ny, 2 L)).  Range: the same layout over frequencies q = ky + kx ny, DC at q = 0.
//
//   Y[ky, kx] = s sum_{y, x} X[y, x] exp(-+ 2 pi i (ky y / ny + kx x / nx)),   s = 1 / sqrt(nx ny),   - forward (K), + transpose (K^T)
//
// nx and ny are powers of two from 1 to 2048.  This header is the one place the arithmetic and its order are written down; kernels,
// host library and harness build without contraction, and every operation is one rounding in T.
//
// Twiddle table (MakeTable): n = max(nx, ny) entries of (cos(2 pi j / n), -sin(2 pi j / n)), computed in float64 and rounded once to T,
// stored interleaved.  Only the first octant calls cos and sin (on 2.0 * pi * j / n, evaluated in that order); the rest follows by
// symmetry, so that w[0] = (1, 0), w[n/4] = (0, -1), w[n/8] = (sqrt(1/2), -sqrt(1/2)) hold exactly and the table is symmetric.  A
// line of m <= n points reads it with the stride n / m; the transpose negates the second component on the fly.
//
// A line of m = 2^t points (LineTransform) is the radix-2 decimation-in-time tree:
//
//   F_m(a)[k]       = E[k] + w_m^k O[k]
//   F_m(a)[k + m/2] = E[k] - w_m^k O[k],   k < m / 2,   E = F_{m/2}(a[0], a[2], ..), O = F_{m/2}(a[1], a[3], ..),   F_1(a) = a
//
// evaluated breadth first without a permutation (Stockham): stage h = 1, 2, 4, .., m / 2 takes butterfly j = k + h r (k < h), reads
// a = Y[j] and b = Y[j + m/2] and writes Y'[k + 2 h r] = a + t, Y'[k + h + 2 h r] = a - t, with t = w b and w = table[k (n / 2 h)]:
//
//   k == 0:            t = b                                            (w = 1)
//   k == h / 2, h > 1: t = (b.im, -b.re) forward, (-b.im, b.re) transposed    (w = -+ i)
//   otherwise:         t = (b.re w.re - b.im w.im, b.re w.im + b.im w.re), each product and each sum rounded once
//
// The two skipped multiplications change no finite value (the products with 0 and 1 are exact), only the sign of a zero and what a
// non-finite input turns into.  A kernel may hold a stage in registers or LDS or merge stages; each output keeps this tree.
//
// The product: every column (the y pass, lines of ny contiguous points) first, then every row (the x pass, lines of nx points with
// stride ny); a side of 1 has no pass.  Then every value is multiplied once by s rounded to T (s = 1 exactly for nx = ny = 1: the
// identity, bit for bit), and the accumulating form stores res + value.  res, rhs and the work buffer must not overlap.  A plane pair
// (re_c, im_c) is transformed on its own: a non-finite value spreads over its own pair only.
//
// Error bound (Higham, Accuracy and Stability of Numerical Algorithms, 2nd ed., Thm 24.2, applied to this tree).  Stage h is a
// product with a matrix A_h whose rows hold two entries, 1 and +-w, so |A_h|_2 = sqrt(2).  The computed stage is A_h + dA_h: the
// stored twiddle is off by mu <= u relative (first-octant values are correctly rounded up to the libm's error, taken as <= u), the
// complex product (two products, one sum per component) by gamma_2 sqrt(2) relative, the complex sum by another u; together
// |dA_h| <= eta |A_h| componentwise with eta = mu + gamma_4 (sqrt(2) + mu), gamma_4 = 4 u / (1 - 4 u).  t = log2 nx + log2 ny stages give
// |fl(F x) - F x|_2 <= (t eta / (1 - t eta)) |F|_2 |x|_2 with |F|_2 = sqrt(nx ny) before scaling; the scaling by s (rounded: u; the
// product: u) makes the operator unitary and adds 2 u:
//
//   |fl(K x) - K x|_2 <= B |x|_2 per plane pair,   B = t eta / (1 - t eta) + 2 u.
//
// Sums for the preconditioners (closed form): |K| has the entries s |cos(theta)| and s |sin(theta)| with theta = 2 pi (ky y / ny +
// kx x / nx).  Over a row the angles are uniform over the multiples of 2 pi / g, g = max(ny / gcd(ky, ny), nx / gcd(kx, nx)),
// gcd(0, n) = n, each taken N / g times:  sum |K|^alpha = s^alpha (N / g) sum_{j < g} (|cos(2 pi j / g)|^alpha + |sin(2 pi j / g)|^alpha),
// an exactly zero term absent.  The matrix is symmetric in (frequency, pixel), so the column of pixel (y, x) has the same sum.
#ifndef PROST_LINOP_FFT2D_HPP_
#define PROST_LINOP_FFT2D_HPP_
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PROST_FFT_HD __host__ __device__ __forceinline__
#else
#define PROST_FFT_HD inline
#endif

namespace prost {
namespace fft2d {

constexpr int kMaxSide = 2048;           ///< nx, ny: powers of two up to it
constexpr int kMaxLog2 = 11;
constexpr double kPi = 3.14159265358979323846;

/// the operator (the layout of prost_hip_fft2d_geometry in prost_hip.h)
struct Geometry {
  int32_t ny, nx;         ///< image plane, each a power of two from 1 to 2048
  int32_t planes;         ///< L complex images: 2 L real planes
  int32_t transpose;      ///< 0: res = K rhs, else res = K^T rhs
};

inline Geometry MakeGeometry(long ny, long nx, long planes, bool transpose) {
  Geometry g;
  g.ny = (int32_t)ny; g.nx = (int32_t)nx; g.planes = (int32_t)planes; g.transpose = transpose ? 1 : 0;
  return g;
}
PROST_FFT_HD bool IsSide(long v) { return v >= 1 && v <= kMaxSide && (v & (v - 1)) == 0; }
PROST_FFT_HD int Log2(int v) { int t = 0; while ((1 << t) < v) t++; return t; }
PROST_FFT_HD int TableSize(int ny, int nx) { return ny > nx ? ny : nx; }

template <class T> struct Cx { T re, im; };

/// t = w b of butterfly k at stage h; (wr, wi) is the table entry k (n / 2 h), read by the caller
template <class T, bool INV> PROST_FFT_HD Cx<T> Twiddled(Cx<T> b, int k, int h, T wr, T wi) {
  Cx<T> t;
  if (k == 0) {
    t = b;
  } else if (2 * k == h) {
    if (INV) { t.re = -b.im; t.im = b.re; } else { t.re = b.im; t.im = -b.re; }
  } else {
    const T vi = INV ? -wi : wi;
    const T p0 = b.re * wr, p1 = b.im * vi, p2 = b.re * vi, p3 = b.im * wr;
    t.re = p0 - p1; t.im = p2 + p3;
  }
  return t;
}

/// s = 1 / sqrt(nx ny), computed in float64 and rounded once to T (a host value; kernels take it as an argument)
template <class T> inline T Scale(int ny, int nx) { return (T)(1.0 / std::sqrt((double)ny * (double)nx)); }

#if !defined(__HIP_DEVICE_COMPILE__)
/// (cos, sin)(2 pi j / n) in float64 for j < n, n a power of two: cos and sin are called in the first octant only
inline void Angle(int j, int n, double& c, double& s) {
  if (n >= 2 && j >= n / 2) { Angle(j - n / 2, n, c, s); c = -c; s = -s; return; }
  if (n >= 4 && j >= n / 4) { double c0, s0; Angle(j - n / 4, n, c0, s0); c = -s0; s = c0; return; }
  if (j == 0) { c = 1.0; s = 0.0; return; }
  if (8 * j == n) { c = s = std::sqrt(0.5); return; }
  if (8 * j > n) { double c0, s0; Angle(n / 4 - j, n, c0, s0); c = s0; s = c0; return; }
  const double a = 2.0 * kPi * (double)j / (double)n;
  c = std::cos(a); s = std::sin(a);
}

/// the twiddle table: n entries (cos, -sin)(2 pi j / n), interleaved, rounded once to T
template <class T> inline std::vector<T> MakeTable(int n) {
  std::vector<T> w(2 * (size_t)n);
  for (int j = 0; j < n; j++) {
    double c, s;
    Angle(j, n, c, s);
    w[2 * (size_t)j] = (T)c; w[2 * (size_t)j + 1] = (T)(-s);
  }
  return w;
}

/// one line of m points in place; re and im have the element stride `stride`; tmp holds 4 m values
template <class T, bool INV> inline void LineTransform(T* re, T* im, size_t stride, int m, const T* table, int ntable, T* tmp) {
  T *ar = tmp, *ai = tmp + m, *br = tmp + 2 * (size_t)m, *bi = tmp + 3 * (size_t)m;
  for (int e = 0; e < m; e++) { ar[e] = re[(size_t)e * stride]; ai[e] = im[(size_t)e * stride]; }
  for (int h = 1; h < m; h *= 2) {
    const int step = ntable / (2 * h);
    for (int j = 0; j < m / 2; j++) {
      const int k = j % h, r = j / h;
      const Cx<T> a = {ar[j], ai[j]}, b = {ar[j + m / 2], ai[j + m / 2]};
      const Cx<T> t = Twiddled<T, INV>(b, k, h, table[2 * (size_t)(k * step)], table[2 * (size_t)(k * step) + 1]);
      br[k + 2 * h * r] = a.re + t.re; bi[k + 2 * h * r] = a.im + t.im;
      br[k + h + 2 * h * r] = a.re - t.re; bi[k + h + 2 * h * r] = a.im - t.im;
    }
    T* sw = ar; ar = br; br = sw;
    sw = ai; ai = bi; bi = sw;
  }
  for (int e = 0; e < m; e++) { re[(size_t)e * stride] = ar[e]; im[(size_t)e * stride] = ai[e]; }
}

/// the product on the host: res (+)= K rhs or K^T rhs; table from MakeTable<T>(TableSize(ny, nx)); res and rhs hold 2 L N values
template <class T, bool ACC> inline void Apply(T* res, const T* rhs, const Geometry& g, const T* table, bool transpose) {
  const size_t ny = (size_t)g.ny, nx = (size_t)g.nx, N = ny * nx, L = (size_t)g.planes;
  const int ntable = TableSize(g.ny, g.nx);
  const T s = Scale<T>(g.ny, g.nx);
  std::vector<T> re(N), im(N), tmp(4 * (size_t)ntable);
  for (size_t c = 0; c < L; c++) {
    for (size_t p = 0; p < N; p++) { re[p] = rhs[c * N + p]; im[p] = rhs[(L + c) * N + p]; }
    if (g.ny > 1)
      for (size_t x = 0; x < nx; x++) {
        if (transpose) LineTransform<T, true>(re.data() + x * ny, im.data() + x * ny, 1, g.ny, table, ntable, tmp.data());
        else LineTransform<T, false>(re.data() + x * ny, im.data() + x * ny, 1, g.ny, table, ntable, tmp.data());
      }
    if (g.nx > 1)
      for (size_t y = 0; y < ny; y++) {
        if (transpose) LineTransform<T, true>(re.data() + y, im.data() + y, ny, g.nx, table, ntable, tmp.data());
        else LineTransform<T, false>(re.data() + y, im.data() + y, ny, g.nx, table, ntable, tmp.data());
      }
    for (size_t p = 0; p < N; p++) {
      const T vr = re[p] * s, vi = im[p] * s;
      T *orr = res + c * N + p, *oi = res + (L + c) * N + p;
      *orr = ACC ? *orr + vr : vr;
      *oi = ACC ? *oi + vi : vi;
    }
  }
}

inline double PowAbs(double v, double alpha) { return alpha == 1 ? std::fabs(v) : (alpha == 2 ? v * v : (v == 0 ? 0.0 : std::pow(std::fabs(v), alpha))); }

/// the period class of frequency (or pixel) index (iy, ix): log2 of g = max(ny / gcd(iy, ny), nx / gcd(ix, nx)), gcd(0, n) = n
PROST_FFT_HD int PeriodLog2(int iy, int ix, int ny, int nx) {
  int gy = 0, gx = 0;
  if (iy != 0) { int v = iy, z = 0; while (!(v & 1)) { v >>= 1; z++; } gy = Log2(ny) - z; }
  if (ix != 0) { int v = ix, z = 0; while (!(v & 1)) { v >>= 1; z++; } gx = Log2(nx) - z; }
  return gy > gx ? gy : gx;
}

/// the sum of |K|^alpha over a row (or column) of period class l, g = 2^l <= max(ny, nx)
inline double ClassSum(int ny, int nx, double alpha, int l) {
  const double N = (double)ny * (double)nx, sa = PowAbs(1.0 / std::sqrt(N), alpha);
  const int g = 1 << l;
  double acc = 0;
  for (int j = 0; j < g; j++) {
    double c, s;
    Angle(j, g, c, s);
    if (c != 0) acc += PowAbs(c, alpha);
    if (s != 0) acc += PowAbs(s, alpha);
  }
  return sa * (N / (double)g) * acc;
}

/// sums[l] = s^alpha (N / g) sum_{j < g} (|cos(2 pi j / g)|^alpha + |sin(2 pi j / g)|^alpha), g = 2^l, for l = 0 .. kMaxLog2: the row sum
/// of |K|^alpha for every row of period class l, and the column sum likewise.  At most 12 values; in double.
inline void SumTable(int ny, int nx, double alpha, double sums[kMaxLog2 + 1]) {
  const int top = Log2(TableSize(ny, nx));
  for (int l = 0; l <= kMaxLog2; l++) sums[l] = l > top ? 0.0 : ClassSum(ny, nx, alpha, l);
}
#endif

}  // namespace fft2d
}  // namespace prost
#endif
