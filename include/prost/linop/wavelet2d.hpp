// prost/linop/wavelet2d.hpp -- the arithmetic of BlockWavelet2D: the orthogonal, periodised, separable multi-level discrete wavelet
// transform (Mallat's pyramid) of L real planes and its transpose, the inverse transform, without a matrix.  The reference has no such
// block; this is written from the definition.
//
// Domain and range: L planes of ny x nx, N = nx ny, pixel (y, x) of plane c at c N + y + x ny.  K is L N x L N and K^T K = I.
//
// Taps.  h is a low-pass filter of even length T, 2 <= T <= 16, given in float64; the high-pass filter is g[t] = (-1)^t h[T-1-t].
// Named filters are evaluated in float64 from closed forms, in exactly this order of operations (NamedTaps):
//   haar:  h = (1, 1) / sqrt(2)
//   db2:   s = sqrt(3);  h = (1+s, 3+s, 3-s, 1-s) / (4 sqrt(2))
//   db3:   a = sqrt(10), b = sqrt(5 + 2a);  h = (1+a+b, 5+a+3b, 10-2a+2b, 10-2a-2b, 5+a-3b, 1+a-b) / (16 sqrt(2))
// each numerator summed left to right, the denominator formed first (4.0 * sqrt(2.0), 16.0 * sqrt(2.0)), then one division.  Any other
// filter is accepted if |sum_k h[k] h[k+2l] - delta_l| <= 1e-12 for every l (OrthoDefect).  h and g are rounded once to T (MakeTaps).
//
// One level on a line x of even length m >= T (Analysis), for k < m / 2:
//   lo[k] = sum_t h[t] x[(2k + t) mod m],   hi[k] = sum_t g[t] x[(2k + t) mod m]
// each sum from +0, t ascending, every product and every sum rounded once in T (no contraction).  Lows at 0 .. m/2-1, highs at
// m/2 .. m-1.  Its transpose (Synthesis): output n is the sum, from +0, over the taps t = n mod 2, n mod 2 + 2, .. < T ascending of
// h[t] lo[k] and then g[t] hi[k], k = ((n - t) / 2) mod (m / 2): two additions per tap, the low one first.
//
// The product.  Level l = 0 .. levels-1 acts on the corner my x mx, my = ny >> l, mx = nx >> l (a side of 1 stays 1 and has no pass):
// the y pass over all mx columns, then the x pass over all my rows, the intermediate rounded to T; the next level acts on the low-low
// corner.  The result is the in-place quadrant layout, the approximation at the top left.  The transpose runs the levels in reverse
// and, in a level, the x pass before the y pass.  The accumulating form stores res + value; every element of res is stored once.
// Limits (CheckShape): planes >= 1, levels >= 1, 2 <= T <= 16 even, a side > 1 divisible by 2^levels with side / 2^(levels-1) >= T
// (no level folds its taps), not 1 x 1, planes N < 2^31.  Sides need not be powers of two.
//
// Work buffer (WorkSize).  The low-low corner after level l + 1 lives in slot l mod 2 of a work buffer, packed (column height = its own
// height, plane after plane).  Slot 0 holds planes C(1) values, slot 1 planes C(2), C(j) = the size of the corner after j levels: 5/16 of
// planes N in 2-D, 3/4 with a side of 1.  A one-level transform does not touch it.
//
// Error bound.  One 1-D pass is a product with an orthogonal matrix W1 whose rows hold the T taps; |W1| has row and column sums
// S = sum |h_t|, so | |W1| |_2 <= S.  A computed row is a T-term dot product with taps rounded to T: (1 + u) for the tap, (1 + u) for
// the product, T additions (the first one onto +0 is exact): componentwise |fl(W1 x) - W1 x| <= gamma_(T+1) |W1| |x|, gamma_n =
// n u / (1 - n u), so |fl(W1 x) - W1 x|_2 <= eta |x|_2 with eta = gamma_(T+1) S.  A level is two passes and the exact passes keep the
// 2-norm, so after 2 levels passes, by induction |fl(K x) - K x|_2 <= ((1 + eta)^(2 levels) - 1) |x|_2 = B |x|_2 per plane; the same
// for K^T (the transpose pass is a T-term sum over the same entries).
//
// Sums for the preconditioners.  Every basis function is a tensor product of two 1-D level-j functions, so a row of level j and type
// (ty, tx) in {lo, hi}^2 has sum |K|^alpha = R_y(j, ty) R_x(j, tx), R(j, t) the sum over one periodised 1-D level-j cascade function.
// The column of pixel (y, x) sums C_y(j, lo, y) C_x(j, hi, x) + C_y(j, hi, y) C_x(j, lo, x) + C_y(j, hi, y) C_x(j, hi, x) over the
// levels j plus C_y(levels, lo, y) C_x(levels, lo, x), with C(j, t, y) = the sum over the level-j functions of type t at position y,
// which depends on y mod 2^j only.  AxisTables builds R and C in double by applying the 1-D synthesis to one unit coefficient per level
// and type (the others are its shifts by 2^j); an axis of length 1 has R(lo) = C(lo) = 1 and no highs.
#ifndef PROST_LINOP_WAVELET2D_HPP_
#define PROST_LINOP_WAVELET2D_HPP_
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PROST_WV_HD __host__ __device__ __forceinline__
#else
#define PROST_WV_HD inline
#endif

namespace prost {
namespace wavelet2d {

constexpr int kMaxTaps = 16;
constexpr int kMaxLevels = 30;
constexpr double kOrthoTolerance = 1e-12;
constexpr int kTailValues = 4096;        ///< a corner of at most this many values per plane is finished by one workgroup (the kernels' tail)

/// the operator (the layout of prost_hip_wavelet2d_geometry in prost_hip.h)
struct Geometry {
  int32_t ny, nx;         ///< image plane
  int32_t planes;         ///< L
  int32_t levels;
  int32_t ntaps;          ///< T
  int32_t transpose;      ///< 0: res = K rhs, else res = K^T rhs
  int32_t no_tail;        ///< 0; else one launch per level all the way down (for measurements; the bits are the same)
  int32_t reserved;       ///< 0
};

inline Geometry MakeGeometry(long ny, long nx, long planes, long levels, long ntaps, bool transpose) {
  Geometry g;
  g.ny = (int32_t)ny; g.nx = (int32_t)nx; g.planes = (int32_t)planes; g.levels = (int32_t)levels; g.ntaps = (int32_t)ntaps;
  g.transpose = transpose ? 1 : 0; g.no_tail = 0; g.reserved = 0;
  return g;
}

/// h and g rounded once to T; passed to the kernels by value (scalar loads)
template <class T> struct Taps { T h[kMaxTaps], g[kMaxTaps]; };

template <class T> inline Taps<T> MakeTaps(const double* h, int ntaps) {
  Taps<T> w;
  for (int t = 0; t < kMaxTaps; t++) { w.h[t] = (T)0; w.g[t] = (T)0; }
  for (int t = 0; t < ntaps; t++) {
    w.h[t] = (T)h[t];
    const T m = (T)h[ntaps - 1 - t];
    w.g[t] = (t & 1) ? -m : m;
  }
  return w;
}

/// the side of the corner level l acts on (l = 0: the image)
PROST_WV_HD int CornerSide(int side, int l) { return side > 1 ? side >> l : 1; }
/// values of a plane's corner after j levels
PROST_WV_HD size_t CornerSize(int ny, int nx, int j) { return (size_t)CornerSide(ny, j) * (size_t)CornerSide(nx, j); }
/// values of the work buffer: slot 0 (corners after 1, 3, .. levels), then slot 1 (after 2, 4, ..)
PROST_WV_HD size_t WorkSlot0(const Geometry& g) { return (size_t)g.planes * CornerSize(g.ny, g.nx, 1); }
PROST_WV_HD size_t WorkSize(const Geometry& g) { return WorkSlot0(g) + (size_t)g.planes * CornerSize(g.ny, g.nx, 2); }
/// the first level whose corner one workgroup finishes; levels: none
PROST_WV_HD int TailStart(const Geometry& g) {
  if (g.no_tail) return g.levels;
  for (int l = 0; l < g.levels; l++)
    if (CornerSize(g.ny, g.nx, l) <= (size_t)kTailValues) return l;
  return g.levels;
}

/// nullptr if the shape is supported, else what is wrong with it
inline const char* CheckShape(double ny, double nx, double planes, double levels, double ntaps) {
  if (!(nx >= 1) || nx != std::floor(nx) || nx >= 2147483648.0) return "nx has to be a positive integer below 2^31";
  if (!(ny >= 1) || ny != std::floor(ny) || ny >= 2147483648.0) return "ny has to be a positive integer below 2^31";
  if (!(planes >= 1) || planes != std::floor(planes) || planes >= 2147483648.0) return "L has to be a positive integer below 2^31";
  if (!(levels >= 1) || levels != std::floor(levels)) return "levels has to be a positive integer";
  if (!(ntaps >= 2) || ntaps > kMaxTaps || ntaps != std::floor(ntaps) || std::fmod(ntaps, 2.0) != 0) return "the filter has to have an even number of taps from 2 to 16";
  if (nx == 1 && ny == 1) return "a plane of 1 x 1 has nothing to transform";
  if (levels > kMaxLevels) return "a side greater than 1 has to be divisible by 2^levels";
  const double p = std::ldexp(1.0, (int)levels);
  for (double side : {ny, nx}) {
    if (side == 1) continue;
    if (std::fmod(side, p) != 0) return "a side greater than 1 has to be divisible by 2^levels";
    if (side / (p / 2) < ntaps) return "the coarsest line, side / 2^(levels-1), has to hold the filter's taps";
  }
  if (planes * ny * nx >= 2147483648.0) return "L nx ny has to stay below 2^31";
  return nullptr;
}

/// lo and hi of one output pair: x(t) is the line at (2 k + t) mod m
template <class T, class F> PROST_WV_HD void Analysis(const Taps<T>& w, int ntaps, F x, T& lo, T& hi) {
  T a = (T)0, b = (T)0;
  for (int t = 0; t < ntaps; t++) {
    const T v = x(t);
    const T p = w.h[t] * v, q = w.g[t] * v;
    a = a + p; b = b + q;
  }
  lo = a; hi = b;
}

/// output n of the transposed pass on a line with `half` lows and `half` highs: lo(k), hi(k) for k < half
template <class T, class FL, class FH> PROST_WV_HD T Synthesis(const Taps<T>& w, int ntaps, int n, int half, FL lo, FH hi) {
  T a = (T)0;
  for (int t = n & 1; t < ntaps; t += 2) {
    int k = (n - t) / 2;                 // n - t is even; at least -(T / 2 - 1) > -half
    if (k < 0) k += half;
    const T p = w.h[t] * lo(k), q = w.g[t] * hi(k);
    a = a + p; a = a + q;
  }
  return a;
}

// ---- host only from here on (plain functions; a device pass parses them and emits nothing) ----
/// the float64 taps of "haar", "db2", "db3"; false for any other name
inline bool NamedTaps(const char* name, std::vector<double>& h) {
  h.clear();
  if (!std::strcmp(name, "haar")) {
    const double d = std::sqrt(2.0);
    h = {1.0 / d, 1.0 / d};
  } else if (!std::strcmp(name, "db2")) {
    const double s = std::sqrt(3.0), d = 4.0 * std::sqrt(2.0);
    h = {(1.0 + s) / d, (3.0 + s) / d, (3.0 - s) / d, (1.0 - s) / d};
  } else if (!std::strcmp(name, "db3")) {
    const double a = std::sqrt(10.0), b = std::sqrt(5.0 + 2.0 * a), d = 16.0 * std::sqrt(2.0);
    h = {(1.0 + a + b) / d,           (5.0 + a + 3.0 * b) / d, (10.0 - 2.0 * a + 2.0 * b) / d,
         (10.0 - 2.0 * a - 2.0 * b) / d, (5.0 + a - 3.0 * b) / d, (1.0 + a - b) / d};
  } else {
    return false;
  }
  return true;
}

/// max_l |sum_k h[k] h[k + 2 l] - delta_l|, l = 0 .. T/2 - 1
inline double OrthoDefect(const double* h, int ntaps) {
  double worst = 0;
  for (int l = 0; 2 * l < ntaps; l++) {
    double acc = 0;
    for (int k = 0; k + 2 * l < ntaps; k++) acc += h[k] * h[k + 2 * l];
    const double d = std::fabs(acc - (l == 0 ? 1.0 : 0.0));
    if (!(d <= worst)) worst = d;      // a NaN sticks
  }
  return worst;
}

/// one analysis pass on a line of m values with the element stride `stride`, in place; tmp holds m values
template <class T> inline void LineForward(T* line, size_t stride, int m, const Taps<T>& w, int ntaps, T* tmp) {
  for (int e = 0; e < m; e++) tmp[e] = line[(size_t)e * stride];
  for (int k = 0; k < m / 2; k++) {
    T lo, hi;
    Analysis<T>(w, ntaps, [&](int t) { int e = 2 * k + t; if (e >= m) e -= m; return tmp[e]; }, lo, hi);
    line[(size_t)k * stride] = lo; line[(size_t)(m / 2 + k) * stride] = hi;
  }
}
/// one synthesis pass, in place
template <class T> inline void LineInverse(T* line, size_t stride, int m, const Taps<T>& w, int ntaps, T* tmp) {
  for (int e = 0; e < m; e++) tmp[e] = line[(size_t)e * stride];
  const int half = m / 2;
  for (int n = 0; n < m; n++)
    line[(size_t)n * stride] = Synthesis<T>(w, ntaps, n, half, [&](int k) { return tmp[k]; }, [&](int k) { return tmp[half + k]; });
}

/// the product on the host: res (+)= K rhs or K^T rhs; res and rhs hold planes N values and do not overlap
template <class T, bool ACC> inline void Apply(T* res, const T* rhs, const Geometry& g, const Taps<T>& w, bool transpose) {
  const size_t ny = (size_t)g.ny, N = ny * (size_t)g.nx;
  std::vector<T> plane(N), tmp((size_t)(g.ny > g.nx ? g.ny : g.nx));
  for (size_t c = 0; c < (size_t)g.planes; c++) {
    for (size_t p = 0; p < N; p++) plane[p] = rhs[c * N + p];
    for (int i = 0; i < g.levels; i++) {
      const int l = transpose ? g.levels - 1 - i : i;
      const int my = CornerSide(g.ny, l), mx = CornerSide(g.nx, l);
      if (!transpose) {
        if (my > 1) for (int x = 0; x < mx; x++) LineForward<T>(plane.data() + (size_t)x * ny, 1, my, w, g.ntaps, tmp.data());
        if (mx > 1) for (int y = 0; y < my; y++) LineForward<T>(plane.data() + y, ny, mx, w, g.ntaps, tmp.data());
      } else {
        if (mx > 1) for (int y = 0; y < my; y++) LineInverse<T>(plane.data() + y, ny, mx, w, g.ntaps, tmp.data());
        if (my > 1) for (int x = 0; x < mx; x++) LineInverse<T>(plane.data() + (size_t)x * ny, 1, my, w, g.ntaps, tmp.data());
      }
    }
    for (size_t p = 0; p < N; p++) res[c * N + p] = ACC ? res[c * N + p] + plane[p] : plane[p];
  }
}

inline double PowAbs(double v, double alpha) { return alpha == 1 ? std::fabs(v) : (alpha == 2 ? v * v : (v == 0 ? 0.0 : std::pow(std::fabs(v), alpha))); }

/// the 1-D tables of one axis of length m.  row[2 j + t]: R(j, t) for j = 1 .. levels, t = 0 (lo), 1 (hi).  col[2 j + t]: C(j, t, y) for
/// y < 2^j (m > 1) or one value (m = 1)
struct AxisSums {
  std::vector<double> row;
  std::vector<std::vector<double>> col;
  int m = 1;
  double Col(int j, int t, int y) const { const std::vector<double>& c = col[2 * (size_t)j + t]; return c[(size_t)y & (c.size() - 1)]; }
};
inline AxisSums AxisTables(int m, int levels, const double* h, int ntaps, double alpha) {
  AxisSums s;
  s.m = m;
  s.row.assign(2 * (size_t)(levels + 1), 0.0);
  s.col.assign(2 * (size_t)(levels + 1), std::vector<double>(1, 0.0));
  if (m == 1) {
    for (int j = 1; j <= levels; j++) { s.row[2 * (size_t)j] = 1.0; s.col[2 * (size_t)j][0] = 1.0; }
    return s;
  }
  const Taps<double> w = MakeTaps<double>(h, ntaps);
  std::vector<double> v((size_t)m), tmp((size_t)m);
  for (int j = 1; j <= levels; j++)
    for (int t = 0; t < 2; t++) {
      std::fill(v.begin(), v.end(), 0.0);
      v[t ? (size_t)(m >> j) : 0] = 1.0;
      for (int i = j; i >= 1; i--) LineInverse<double>(v.data(), 1, m >> (i - 1), w, ntaps, tmp.data());
      std::vector<double>& c = s.col[2 * (size_t)j + t];
      c.assign((size_t)1 << j, 0.0);
      double acc = 0;
      for (int n = 0; n < m; n++) { const double p = PowAbs(v[(size_t)n], alpha); acc += p; c[(size_t)n & (c.size() - 1)] += p; }
      s.row[2 * (size_t)j + t] = acc;
    }
  return s;
}

/// level (1 .. levels) and types of coefficient (iy, ix)
inline void RowClass(const Geometry& g, int iy, int ix, int& j, int& ty, int& tx) {
  for (j = 1; j <= g.levels; j++) {
    ty = g.ny > 1 && iy >= (g.ny >> j); tx = g.nx > 1 && ix >= (g.nx >> j);
    if (ty || tx) return;
  }
  j = g.levels; ty = tx = 0;
}
inline double RowSum(const Geometry& g, const AxisSums& sy, const AxisSums& sx, int iy, int ix) {
  int j, ty, tx;
  RowClass(g, iy, ix, j, ty, tx);
  return sy.row[2 * (size_t)j + ty] * sx.row[2 * (size_t)j + tx];
}
inline double ColSum(const Geometry& g, const AxisSums& sy, const AxisSums& sx, int y, int x) {
  double acc = 0;
  for (int j = 1; j <= g.levels; j++)
    acc += sy.Col(j, 0, y) * sx.Col(j, 1, x) + sy.Col(j, 1, y) * sx.Col(j, 0, x) + sy.Col(j, 1, y) * sx.Col(j, 1, x);
  return acc + sy.Col(g.levels, 0, y) * sx.Col(g.levels, 0, x);
}

}  // namespace wavelet2d
}  // namespace prost
#endif
