// prost/linop/radon2d.hpp -- the arithmetic of BlockRadon2D: the parallel-beam projector of an image (Joseph's method) and its exact
// transpose, without a matrix.  The reference has no such block; this is written from the definition.
//
// Domain: L column-major planes of ny x nx, element (y, x, c) at y + x ny + c nx ny.  Range: L sinograms, bin d of angle a of plane c at
// d + a ndet + c ndet na.  Pixel centres are at X = x - (nx - 1) / 2, Y = y - (ny - 1) / 2 (pixel size 1); a point's detector coordinate
// at angle theta is s = X cos theta + Y sin theta; bin d sits at s_d = (d - (ndet - 1) / 2) spacing + shift.
//
// Joseph's method: per angle a driving axis, chosen on the host in double.  |cos theta| >= |sin theta|: the ray is marched over rows
// t = y and interpolated linearly along x (ni = nx, "row-driven", axis 0); otherwise over columns t = x and interpolated along y
// (ni = ny, "column-driven", axis 1).  The per-angle table, formed in double and rounded once to T, with cx = (nx - 1) / 2,
// cy = (ny - 1) / 2, cd = (ndet - 1) / 2, h = spacing:
//
//   row-driven:     q = h / cos,  p = -sin / cos,  r = ((shift - cd h) + cy sin) / cos + cx,  c = 1 / |cos|
//   column-driven:  q = h / sin,  p = -cos / sin,  r = ((shift - cd h) + cx cos) / sin + cy,  c = 1 / |sin|
//
// kTableWidth values of T per angle: q, p, r, c and the axis (0 or 1).
//
// Order of operations (the one place it is written down; kernels and host library build without contraction; every operation is one
// rounding in T).  The position of ray (a, d) on driving line t is f = (r + q d) + p t with d and t converted to T;
// i0 = floor(f), w1 = f - i0, w0 = 1 - w1.  The matrix has A[(a, d), (t, i0)] = c w0 and A[(a, d), (t, i0 + 1)] = c w1; an entry is
// absent when its interpolated index is outside 0 .. ni - 1 or its weight is exactly 0 (so Inf or NaN in a pixel no ray samples stays
// out).  The device evaluates multiply, add, floor, conversion and, for the adjoint's window only, one division: no transcendental.
//
//   forward:  out(a, d) = sum of A u over t ascending, the i0 term before the i0 + 1 term; each term is (c w) u, two roundings; the
//             sum starts from its first term (the accumulator starts at -0, and -0 + p == p for every p).
//   adjoint:  pixel (t, i) collects, over angles ascending and within an angle over bins ascending, the rays whose entry at that pixel
//             is present.  The candidate bins are b - m .. b + m + 1 with b = floor((i - (r + p t)) / q) in T and m = ceil(1 / spacing);
//             each candidate's weight is recomputed with the forward's expressions: w0 if i0 == i, w1 if i0 + 1 == i, otherwise no
//             entry.  K^T is therefore exactly the transpose of the one matrix above, and no atomics are needed.
//
// The accumulating forms store res + value.  res and rhs must not overlap.
#ifndef PROST_LINOP_RADON2D_HPP_
#define PROST_LINOP_RADON2D_HPP_
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PROST_R2D_HD __host__ __device__ __forceinline__
#define PROST_R2D_UNROLL(n) _Pragma(#n)
#else
#define PROST_R2D_HD inline
#define PROST_R2D_UNROLL(n)
#endif
// keeps the compiler from moving a batched load back under the test of whether its value is used
#if defined(__HIP_DEVICE_COMPILE__)
#define PROST_R2D_PIN(v) asm volatile("" : "+v"(v))
#else
#define PROST_R2D_PIN(v) (void)(v)
#endif

namespace prost {
namespace radon2d {

constexpr int kMaxSide = 8192;          ///< nx, ny: the range in which the candidate window was checked in fp32
constexpr int kMaxAngles = 4096;
constexpr int kTableWidth = 5;          ///< q, p, r, c, axis
constexpr int kMaxMargin = 2;           ///< m = ceil(1 / spacing) for spacing >= 0.5
constexpr int kBinsPerWave = 64;        ///< forward: a wavefront owns 64 consecutive bins of one angle
constexpr int kForwardBatch = 8;        ///< forward: driving lines whose loads are in flight together
constexpr int kSlabRows = 16;           ///< forward, row-driven angles: rows of the image a wavefront stages in LDS at a time ...
constexpr int kSlabColumns = 128;       ///< ... and the most columns: 64 bins at spacing 1 span up to 64 sqrt(2) + 16 + 3 = 110
constexpr int kAdjointBatch = 4;        ///< adjoint: angles whose loads are in flight together
constexpr int32_t kMaxBins = 2147483647 - 1024;
enum Column { kQ = 0, kP = 1, kR = 2, kC = 3, kAxis = 4 };

/// the operator (the layout of prost_hip_radon2d_geometry in prost_hip.h)
struct Geometry {
  int32_t ny, nx;         ///< image plane
  int32_t ndet, na;       ///< bins per angle, angles
  int32_t planes;         ///< L
  int32_t m;              ///< the margin of the candidate window, ceil(1 / spacing): 1 or 2
  int32_t transpose;      ///< 0: res = K rhs, else res = K^T rhs
  int32_t reserved;       ///< 0
};

/// the default detector length: every pixel is seen at every angle
inline long DefaultBins(long nx, long ny, double spacing) { return 2 * (long)std::ceil(std::hypot((double)nx, (double)ny) / (2 * spacing)) + 1; }
inline int Margin(double spacing) { return (int)std::ceil(1.0 / spacing); }

inline Geometry MakeGeometry(long ny, long nx, long planes, long ndet, long na, double spacing, bool transpose) {
  Geometry g;
  g.ny = (int32_t)ny; g.nx = (int32_t)nx; g.ndet = (int32_t)ndet; g.na = (int32_t)na; g.planes = (int32_t)planes;
  g.m = Margin(spacing); g.transpose = transpose ? 1 : 0; g.reserved = 0;
  return g;
}

/// the per-angle table: every entry formed in double, rounded once to T
template <class T> inline std::vector<T> MakeTable(long ny, long nx, long ndet, double spacing, double shift, const std::vector<double>& angles) {
  std::vector<T> table(angles.size() * (size_t)kTableWidth);
  const double cx = (double)(nx - 1) / 2, cy = (double)(ny - 1) / 2, cd = (double)(ndet - 1) / 2, h = spacing;
  for (size_t a = 0; a < angles.size(); a++) {
    const double co = std::cos(angles[a]), si = std::sin(angles[a]);
    T* e = table.data() + a * (size_t)kTableWidth;
    if (std::fabs(co) >= std::fabs(si)) {
      e[kQ] = (T)(h / co); e[kP] = (T)(-si / co); e[kR] = (T)(((shift - cd * h) + cy * si) / co + cx); e[kC] = (T)(1 / std::fabs(co)); e[kAxis] = (T)0;
    } else {
      e[kQ] = (T)(h / si); e[kP] = (T)(-co / si); e[kR] = (T)(((shift - cd * h) + cx * co) / si + cy); e[kC] = (T)(1 / std::fabs(si)); e[kAxis] = (T)1;
    }
  }
  return table;
}

/// r + q d: the position of ray d on driving line 0
template <class T> PROST_R2D_HD T Base(const T* __restrict__ e, int d) { return e[kR] + e[kQ] * (T)d; }
/// the position on driving line t, pt = p * (T)t
template <class T> PROST_R2D_HD T Position(T base, T pt) { return base + pt; }
/// -> i0 = floor(f) with w1 = f - i0, w0 = 1 - w1 when an entry is possible (-1 <= i0 < ni); otherwise -2 (no index matches)
template <class T> PROST_R2D_HD int Weights(T f, int ni, T& w0, T& w1) {
  const T fl = std::floor(f);
  w1 = f - fl;
  w0 = (T)1 - w1;
  return (fl >= (T)-1 && fl < (T)ni) ? (int)fl : -2;
}
/// the first candidate bin of pixel (t, i) at an angle, b - m, as an int that can be advanced 2 m + 1 times; bins outside
/// 0 .. ndet - 1 are skipped by the caller.  b is clamped to -1 .. ndet - 1 first: a candidate that is no entry adds nothing.
template <class T> PROST_R2D_HD int FirstCandidate(const T* __restrict__ e, T pt, int i, int m, int ndet) {
  const T g = e[kR] + pt;
  T b = std::floor(((T)i - g) / e[kQ]);
  b = b > (T)-1 ? b : (T)-1;                      // (also NaN, which a finite table cannot give)
  const int bi = b < (T)(ndet - 1) ? (int)b : ndet - 1;
  return bi - m;
}

/// one ray of the forward product: bin d of the angle whose table row is e, over the plane.  The ray is marched kForwardBatch
/// driving lines at a time: the positions, weights and (clamped, always valid) indices of a batch first, then all its loads, then the
/// additions in the pinned order -- the loads do not depend on the running sum, so a lane keeps 2 kForwardBatch of them in flight.
template <class T> PROST_R2D_HD T ForwardSum(const T* __restrict__ e, const T* plane, const Geometry& g, int d) {
  const bool column = e[kAxis] != (T)0;
  const int nt = column ? g.nx : g.ny, ni = column ? g.ny : g.nx;
  const int st = column ? g.ny : 1, si = column ? 1 : g.ny;         // a plane holds fewer than 2^31 elements
  const T p = e[kP], c = e[kC], base = Base(e, d);
  T acc = -(T)0;
  for (int t0 = 0; t0 < nt; t0 += kForwardBatch) {
    T a0[kForwardBatch], a1[kForwardBatch], v0[kForwardBatch], v1[kForwardBatch];
    bool has0[kForwardBatch], has1[kForwardBatch];
    PROST_R2D_UNROLL(unroll)
    for (int k = 0; k < kForwardBatch; k++) {
      const int t = t0 + k < nt ? t0 + k : nt - 1;
      T w0, w1;
      const int i0 = Weights(Position(base, p * (T)t), ni, w0, w1);
      has0[k] = t0 + k < nt && i0 >= 0 && w0 != (T)0;
      has1[k] = t0 + k < nt && i0 >= -1 && i0 + 1 < ni && w1 != (T)0;
      a0[k] = c * w0;
      a1[k] = c * w1;
      v0[k] = plane[t * st + (has0[k] ? i0 : 0) * si];
      v1[k] = plane[t * st + (has1[k] ? i0 + 1 : 0) * si];
    }
    PROST_R2D_UNROLL(unroll)
    for (int k = 0; k < kForwardBatch; k++) { PROST_R2D_PIN(v0[k]); PROST_R2D_PIN(v1[k]); }
    PROST_R2D_UNROLL(unroll)
    for (int k = 0; k < kForwardBatch; k++) {
      if (has0[k]) acc = acc + a0[k] * v0[k];
      if (has1[k]) acc = acc + a1[k] * v1[k];
    }
  }
  return acc;
}

/// one pixel of the adjoint product, M = the margin of the candidate window.  kAdjointBatch angles at a time: the candidates' weights
/// and (clamped, always valid) bins of a batch first, then all its loads, then the additions in the pinned order.
template <class T, int M> PROST_R2D_HD T AdjointSum(const T* __restrict__ table, const T* sino, const Geometry& g, int y, int x) {
  constexpr int kCandidates = 2 * M + 2;
  T acc = -(T)0;
  for (int a0 = 0; a0 < g.na; a0 += kAdjointBatch) {
    T w[kAdjointBatch][kCandidates], v[kAdjointBatch][kCandidates];
    bool has[kAdjointBatch][kCandidates];
    PROST_R2D_UNROLL(unroll)
    for (int b = 0; b < kAdjointBatch; b++) {
      const int a = a0 + b < g.na ? a0 + b : g.na - 1;
      const T* __restrict__ e = table + (size_t)a * kTableWidth;
      const bool column = e[kAxis] != (T)0;
      const int t = column ? x : y, i = column ? y : x, ni = column ? g.ny : g.nx;
      const T pt = e[kP] * (T)t, c = e[kC];
      const int first = FirstCandidate(e, pt, i, M, g.ndet);
      const T* row = sino + (size_t)a * (size_t)g.ndet;
      PROST_R2D_UNROLL(unroll)
      for (int k = 0; k < kCandidates; k++) {
        const int d = first + k, dc = d < 0 ? 0 : (d >= g.ndet ? g.ndet - 1 : d);
        T w0, w1;
        const int i0 = Weights(Position(Base(e, dc), pt), ni, w0, w1);
        const T wk = i0 == i ? w0 : w1;
        has[b][k] = a0 + b < g.na && d == dc && (i0 == i || i0 + 1 == i) && wk != (T)0;
        w[b][k] = c * wk;
        v[b][k] = row[dc];
      }
    }
    PROST_R2D_UNROLL(unroll)
    for (int b = 0; b < kAdjointBatch; b++) {
      PROST_R2D_UNROLL(unroll)
      for (int k = 0; k < kCandidates; k++) PROST_R2D_PIN(v[b][k]);
    }
    PROST_R2D_UNROLL(unroll)
    for (int b = 0; b < kAdjointBatch; b++) {
      PROST_R2D_UNROLL(unroll)
      for (int k = 0; k < kCandidates; k++)
        if (has[b][k]) acc = acc + w[b][k] * v[b][k];
    }
  }
  return acc;
}

#if !defined(__HIP_DEVICE_COMPILE__)
/// visit(t, i, value) for every entry of row (a, d) of the matrix, in the forward's order
template <class T, class F> inline void ForEachInRay(const T* table, const Geometry& g, int a, int d, F visit) {
  const T* e = table + (size_t)a * kTableWidth;
  const bool column = e[kAxis] != (T)0;
  const int nt = column ? g.nx : g.ny, ni = column ? g.ny : g.nx;
  const T base = Base(e, d);
  for (int t = 0; t < nt; t++) {
    T w0, w1;
    const int i0 = Weights(Position(base, e[kP] * (T)t), ni, w0, w1);
    if (i0 >= 0 && w0 != (T)0) visit(t, i0, e[kC] * w0);
    if (i0 >= -1 && i0 + 1 < ni && w1 != (T)0) visit(t, i0 + 1, e[kC] * w1);
  }
}
/// visit(a, d, value) for every entry of column (y, x) of the matrix, in the adjoint's order: the gather enumeration
template <class T, class F> inline void ForEachAtPixel(const T* table, const Geometry& g, int y, int x, F visit) {
  for (int a = 0; a < g.na; a++) {
    const T* e = table + (size_t)a * kTableWidth;
    const bool column = e[kAxis] != (T)0;
    const int t = column ? x : y, i = column ? y : x, ni = column ? g.ny : g.nx;
    const T pt = e[kP] * (T)t;
    const int first = FirstCandidate(e, pt, i, g.m, g.ndet);
    for (int k = 0; k < 2 * g.m + 2; k++) {
      const int d = first + k;
      if (d < 0 || d >= g.ndet) continue;
      T w0, w1;
      const int i0 = Weights(Position(Base(e, d), pt), ni, w0, w1);
      const T w = i0 == i ? w0 : w1;
      if ((i0 == i || i0 + 1 == i) && w != (T)0) visit(a, d, e[kC] * w);
    }
  }
}
/// (y, x) of entry (t, i) of an angle
template <class T> inline void PixelOf(const T* table, int a, int t, int i, int& y, int& x) {
  if (table[(size_t)a * kTableWidth + kAxis] != (T)0) { x = t; y = i; } else { y = t; x = i; }
}

inline double PowAbs(double v, double alpha) { return alpha == 1 ? std::fabs(v) : (alpha == 2 ? v * v : (v == 0 ? 0.0 : std::pow(std::fabs(v), alpha))); }

/// sum |A|^alpha over row (a, d); a ray that misses the image gives exactly 0
template <class T> inline double RowSum(const T* table, const Geometry& g, double alpha, int a, int d) {
  double s = 0;
  ForEachInRay<T>(table, g, a, d, [&](int, int, T v) { s += PowAbs((double)v, alpha); });
  return s;
}
/// sum |A|^alpha over column (y, x); a pixel no ray samples gives exactly 0
template <class T> inline double ColSum(const T* table, const Geometry& g, double alpha, int y, int x) {
  double s = 0;
  ForEachAtPixel<T>(table, g, y, x, [&](int, int, T v) { s += PowAbs((double)v, alpha); });
  return s;
}

/// the products on the host, lane by lane as the kernels run them (tests/host/radon2d_harness.cpp)
template <class T, bool ACC> inline void Apply(T* res, const T* rhs, const Geometry& g, const T* table, bool transpose) {
  const size_t plane = (size_t)g.ny * (size_t)g.nx, sino = (size_t)g.ndet * (size_t)g.na;
  for (int c = 0; c < g.planes; c++) {
    if (!transpose) {
      for (int a = 0; a < g.na; a++)
        for (int d = 0; d < g.ndet; d++) {
          T* o = res + (size_t)c * sino + (size_t)a * (size_t)g.ndet + (size_t)d;
          const T v = ForwardSum<T>(table + (size_t)a * kTableWidth, rhs + (size_t)c * plane, g, d);
          *o = ACC ? *o + v : v;
        }
    } else {
      for (int x = 0; x < g.nx; x++)
        for (int y = 0; y < g.ny; y++) {
          T* o = res + (size_t)c * plane + (size_t)y + (size_t)x * (size_t)g.ny;
          const T v = g.m == 1 ? AdjointSum<T, 1>(table, rhs + (size_t)c * sino, g, y, x) : AdjointSum<T, 2>(table, rhs + (size_t)c * sino, g, y, x);
          *o = ACC ? *o + v : v;
        }
    }
  }
}
#endif

}  // namespace radon2d
}  // namespace prost
#endif
