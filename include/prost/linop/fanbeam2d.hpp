// prost/linop/fanbeam2d.hpp -- the arithmetic of BlockFanbeam2D: the fan-beam projector of an image (a point source, a flat or an
// equiangular detector; Joseph's method) and its exact transpose, without a matrix.  The reference has no such block; this is written
// from the definition and follows radon2d.hpp, whose parallel beams are its limit.
//
// Domain: L column-major planes of ny x nx, element (y, x, c) at y + x ny + c nx ny.  Range: L sinograms, bin d of view a of plane c at
// d + a ndet + c ndet na.  Pixel centres are at X = x - (nx - 1) / 2, Y = y - (ny - 1) / 2 (pixel size 1).  View beta: detector axis
// e = (cos beta, sin beta), central ray n = (-sin beta, cos beta), source S = -R n (R = source_distance).  A point P has depth
// l = P.n + R and lateral coordinate s = P.e.  Bin d sits at u_d = (d - (ndet - 1) / 2) spacing + shift along a detector at distance D
// from the source; its fan angle is gamma_d = atan(u_d / D) on a flat detector and u_d / D on a curved (equiangular) one.  Ray (a, d)
// leaves S in direction sin gamma_d e + cos gamma_d n.  With D = R -> infinity the flat geometry tends to radon2d(.., spacing, shift).
//
// Tables, formed in double and rounded once to T; together O(na + ndet) values, nothing per ray:
//   per view  (kViewWidth values):  cos beta, sin beta, the source in index coordinates sx = R sin beta + (nx - 1) / 2,
//             sy = -R cos beta + (ny - 1) / 2, and the driving axis: 0 (rows, t = y, interpolated along x) if |cos beta| >= |sin beta|,
//             else 1 (columns, t = x, interpolated along y).  One axis per VIEW: a ray of the fan meets its driving lines at
//             |beta - gamma| <= 45 + 30 degrees, because creation refuses max |gamma_d| > 30 degrees, so c <= 1 / cos 75 = 3.87.  An axis
//             per ray would keep c below sqrt 2 but double the candidate windows of the adjoint; it is out of scope.
//   per bin   (kBinWidth values):   sin gamma_d, cos gamma_d -- shared by all views, the same for both detector types: the marches do
//             not know which type they run.
//   inverse   (kInverseWidth values): k0 = (ndet - 1) / 2 - shift / spacing, k1 = D / spacing, lo = tan gamma_0, hi = tan gamma_(ndet-1)
//             and kPolyTerms coefficients a_1 .. of g(tau) = tau (1 + z (a_1 + z (a_2 + ..))), z = tau^2: all 0 on a flat detector
//             (g = tau), kAtan on a curved one (g = atan tau within kAtanError on |tau| <= tan 30 degrees).  The real-valued bin of a
//             point with s / l = tau is k0 + k1 g(tau).
//
// Order of operations (the one place it is written down; kernels and host library build without contraction; every operation is one
// rounding in T, divisions are IEEE divisions; the device evaluates no transcendental function).
//   prologue of ray (a, d), once per product:  dx = sg cos - cg sin,  dy = sg sin + cg cos  (sg, cg the bin's table row);
//             (dt, di) = (dy, dx) and (st, si) = (sy, sx) at a row-driven view, (dx, dy) and (sx, sy) at a column-driven one;
//             p = di / dt,  r = si - st p,  c = 1 / |dt|.
//   march:    f = r + p t with t converted to T;  i0 = floor(f), w1 = f - i0, w0 = 1 - w1.  A[(a, d), (t, i0)] = c w0 and
//             A[(a, d), (t, i0 + 1)] = c w1; an entry is absent when its index is outside 0 .. ni - 1 or its weight is exactly 0.
//   forward:  out(a, d) = sum over t ascending, the i0 term before the i0 + 1 term, each term (c w) u; the sum starts from its first
//             term (the accumulator starts at -0).
//   adjoint:  pixel (t, i) collects, over views ascending and within a view over bins ascending, the rays whose entry at that pixel is
//             present: those that cross driving line t strictly between i - 1 and i + 1, one contiguous range of bins.  It is located
//             from the pixel's own tau = s / l, with s = (x - sx) cos + (y - sy) sin and l = (y - sy) cos - (x - sx) sin: tau clamped
//             to lo .. hi, b = floor(k0 + k1 g(tau)) clamped to -1 .. ndet - 1, candidates b - m .. b + m + 1.  Each candidate's
//             weight is recomputed with the prologue and the march above: w0 if i0 == i, w1 if i0 + 1 == i, otherwise no entry.  The
//             window only has to be wide enough; K^T is exactly the transpose of the one matrix above, and no atomics are needed.
//
// The margin m.  A ray through Q on line t with |Q - P| < 1 along the interpolated axis has tau_P - tau_Q = (ds - tau_Q dl) / l_P with
// (ds, dl) a vector shorter than 1, so |tau_P - tau_ray| < sec(gamma_ray) / l_P <= 1 / (cos(gamma_max) (R - hc)), hc = hypot(nx - 1,
// ny - 1) / 2 the farthest pixel centre; atan is 1-Lipschitz, so the same bound holds for the fan angles of a curved detector.  In
// bins: W = (D / (R - hc)) / (spacing cos gamma_max), the worst magnification over the spacing.  Clamping tau to the fan keeps every
// ray of the fan within W of it.  m = ceil(W + kSlack): kSlack = 1 / 4 bin pays for the rounding of b, of the rays' own positions
// (about 16 (R + hd) eps pixels each) and for kAtanError; Slack() estimates the three in T and creation refuses a geometry that needs
// more (fp32 with a source millions of pixels away).  m is capped at kMaxMargin = 5: the default detector at R >= 2 hd (hd = hypot(nx,
// ny) / 2, the circumscribed circle), D = R and spacing >= 0.5 has D / (R - hc) < 2, gamma_max <= 30 degrees, so W < 2 * 2 / cos 30 =
// 4.62 and m <= ceil(4.87) = 5.  The source lies at least one pixel outside the circumscribed circle, R >= hd + 1, so every point within
// a pixel of the image has l >= 1 / 2 and the lines of the rays continued behind the source never reach the image.
//
// The accumulating forms store res + value.  res and rhs must not overlap.
#ifndef PROST_LINOP_FANBEAM2D_HPP_
#define PROST_LINOP_FANBEAM2D_HPP_
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PROST_F2D_HD __host__ __device__ __forceinline__
#define PROST_F2D_UNROLL(n) _Pragma(#n)
#else
#define PROST_F2D_HD inline
#define PROST_F2D_UNROLL(n)
#endif
// keeps the compiler from moving a batched load back under the test of whether its value is used
#if defined(__HIP_DEVICE_COMPILE__)
#define PROST_F2D_PIN(v) asm volatile("" : "+v"(v))
#else
#define PROST_F2D_PIN(v) (void)(v)
#endif

namespace prost {
namespace fanbeam2d {

constexpr int kMaxSide = 8192;
constexpr int kMaxViews = 4096;
constexpr int kViewWidth = 5;           ///< cos, sin, sx, sy, axis
constexpr int kBinWidth = 2;            ///< sin gamma, cos gamma
constexpr int kPolyTerms = 6;
constexpr int kInverseWidth = 4 + kPolyTerms;   ///< k0, k1, lo, hi, a_1 .. a_6
constexpr int kMaxMargin = 5;           ///< see the head of the file
constexpr double kSlack = 0.25;         ///< bins
constexpr double kMaxFanDegrees = 30;
constexpr int kBinsPerWave = 64;        ///< forward: a wavefront owns 64 consecutive bins of one view
constexpr int kForwardBatch = 8;        ///< forward: driving lines whose loads are in flight together
constexpr int kSlabRows = 16;           ///< forward, row-driven views: rows of the image a wavefront stages in LDS at a time ...
constexpr int kSlabColumns = 128;       ///< ... and the most columns; the kernel measures each slab's width and reads a wider one directly
constexpr int32_t kMaxBins = 2147483647 - 1024;
enum ViewColumn { kCos = 0, kSin = 1, kSx = 2, kSy = 3, kAxis = 4 };
enum BinColumn { kSinGamma = 0, kCosGamma = 1 };
enum InverseColumn { kK0 = 0, kK1 = 1, kLo = 2, kHi = 3, kPoly = 4 };
/// views of the adjoint whose loads are in flight together, by margin: at most 16 candidates
constexpr int AdjointBatch(int m) { return m == 1 ? 4 : (m <= 3 ? 2 : 1); }

/// atan(tau) = tau (1 + z (a_1 + z (a_2 + ..))), z = tau^2, on |tau| <= tan 30 degrees: a least-squares fit at 400 Chebyshev nodes
/// of z in 0 .. 0.335; the largest error on that range is 3.33e-9 (tests/test_fanbeam2d_frontend.py measures it against libm)
constexpr double kAtan[kPolyTerms] = {-0x1.555554068e4bfp-2, 0x1.9997596a700bdp-3, -0x1.24411bcc780e6p-3, 0x1.be972ff58fbf4p-4, -0x1.3eaccbf0ae46ap-4, 0x1.21335f33de351p-5};
constexpr double kAtanError = 3.4e-9;

/// the operator (the layout of prost_hip_fanbeam2d_geometry in prost_hip.h)
struct Geometry {
  int32_t ny, nx;         ///< image plane
  int32_t ndet, na;       ///< bins per view, views
  int32_t planes;         ///< L
  int32_t m;              ///< the margin of the candidate window, 1 .. kMaxMargin
  int32_t transpose;      ///< 0: res = K rhs, else res = K^T rhs
  int32_t reserved;       ///< 0
};

/// the scanner, in double
struct Scanner {
  long ny, nx, ndet;
  double R, D, spacing, shift;
  bool curved;
};

inline double HalfDiagonal(long nx, long ny) { return std::hypot((double)nx, (double)ny) / 2; }                   ///< hd: the circumscribed circle
inline double CentreRadius(long nx, long ny) { return std::hypot((double)(nx - 1), (double)(ny - 1)) / 2; }       ///< hc: the farthest pixel centre
/// the default detector length: the smallest odd count of bins whose outermost rays pass outside the circumscribed circle
inline double DefaultBins(long nx, long ny, double R, double D, double spacing, bool curved) {
  const double need = std::asin(HalfDiagonal(nx, ny) / R), u = curved ? D * need : D * std::tan(need);
  return 2 * std::ceil(u / spacing) + 1;
}
inline double BinAngle(const Scanner& s, long d) {
  const double u = ((double)d - (double)(s.ndet - 1) / 2) * s.spacing + s.shift;
  return s.curved ? u / s.D : std::atan2(u, s.D);
}
inline double MaxFanAngle(const Scanner& s) { return std::fmax(std::fabs(BinAngle(s, 0)), std::fabs(BinAngle(s, s.ndet - 1))); }
/// W, in bins (for max |gamma| below 90 degrees and R > hc)
inline double Window(const Scanner& s) { return s.D / (s.R - CentreRadius(s.nx, s.ny)) / (s.spacing * std::cos(MaxFanAngle(s))); }
inline double MarginOf(const Scanner& s) { return std::ceil(Window(s) + kSlack); }
/// the part of kSlack the roundings of T and the fit of atan use up, estimated
template <class T> inline double Slack(const Scanner& s) {
  const double eps = (double)std::numeric_limits<T>::epsilon(), k0 = std::fabs((double)(s.ndet - 1) / 2 - s.shift / s.spacing), k1 = s.D / s.spacing;
  return Window(s) * 16 * (s.R + HalfDiagonal(s.nx, s.ny)) * eps + 4 * eps * (k0 + 0.58 * k1) + (s.curved ? k1 * kAtanError : 0.0);
}

inline Geometry MakeGeometry(const Scanner& s, long planes, long na, bool transpose) {
  Geometry g;
  g.ny = (int32_t)s.ny; g.nx = (int32_t)s.nx; g.ndet = (int32_t)s.ndet; g.na = (int32_t)na; g.planes = (int32_t)planes;
  g.m = (int32_t)MarginOf(s); g.transpose = transpose ? 1 : 0; g.reserved = 0;
  return g;
}

inline size_t TableSize(long na, long ndet) { return (size_t)na * kViewWidth + (size_t)ndet * kBinWidth + (size_t)kInverseWidth; }
/// the three tables in one array: na view rows, ndet bin rows, the inverse map; every entry formed in double, rounded once to T
template <class T> inline std::vector<T> MakeTable(const Scanner& s, const std::vector<double>& angles) {
  std::vector<T> table(TableSize((long)angles.size(), s.ndet));
  const double cx = (double)(s.nx - 1) / 2, cy = (double)(s.ny - 1) / 2;
  T* e = table.data();
  for (size_t a = 0; a < angles.size(); a++, e += kViewWidth) {
    const double co = std::cos(angles[a]), si = std::sin(angles[a]);
    e[kCos] = (T)co; e[kSin] = (T)si; e[kSx] = (T)(s.R * si + cx); e[kSy] = (T)(-s.R * co + cy); e[kAxis] = std::fabs(co) >= std::fabs(si) ? (T)0 : (T)1;
  }
  for (long d = 0; d < s.ndet; d++, e += kBinWidth) {
    const double gamma = BinAngle(s, d);
    e[kSinGamma] = (T)std::sin(gamma); e[kCosGamma] = (T)std::cos(gamma);
  }
  e[kK0] = (T)((double)(s.ndet - 1) / 2 - s.shift / s.spacing); e[kK1] = (T)(s.D / s.spacing);
  e[kLo] = (T)std::tan(BinAngle(s, 0)); e[kHi] = (T)std::tan(BinAngle(s, s.ndet - 1));
  for (int k = 0; k < kPolyTerms; k++) e[kPoly + k] = s.curved ? (T)kAtan[k] : (T)0;
  return table;
}
template <class T> PROST_F2D_HD const T* BinTable(const T* table, const Geometry& g) { return table + (size_t)g.na * kViewWidth; }
template <class T> PROST_F2D_HD const T* InverseTable(const T* table, const Geometry& g) { return table + (size_t)g.na * kViewWidth + (size_t)g.ndet * kBinWidth; }

/// slope, intercept and weight of one ray
template <class T> struct Ray { T p, r, c; };
/// the prologue of the ray of a bin (sg, cg) at the view whose table row is e
template <class T> PROST_F2D_HD Ray<T> Prologue(const T* __restrict__ e, T sg, T cg) {
  const bool column = e[kAxis] != (T)0;
  const T dx = sg * e[kCos] - cg * e[kSin], dy = sg * e[kSin] + cg * e[kCos];
  const T dt = column ? dx : dy, di = column ? dy : dx;
  const T st = column ? e[kSx] : e[kSy], si = column ? e[kSy] : e[kSx];
  Ray<T> ray;
  ray.p = di / dt;
  ray.r = si - st * ray.p;
  ray.c = (T)1 / std::fabs(dt);
  return ray;
}
/// the position on driving line t, pt = p * (T)t
template <class T> PROST_F2D_HD T Position(T r, T pt) { return r + pt; }
/// -> i0 = floor(f) with w1 = f - i0, w0 = 1 - w1 when an entry is possible (-1 <= i0 < ni); otherwise -2 (no index matches)
template <class T> PROST_F2D_HD int Weights(T f, int ni, T& w0, T& w1) {
  const T fl = std::floor(f);
  w1 = f - fl;
  w0 = (T)1 - w1;
  return (fl >= (T)-1 && fl < (T)ni) ? (int)fl : -2;
}
/// the first candidate bin of pixel (y, x) at a view, b - m, as an int that can be advanced 2 m + 1 times; bins outside 0 .. ndet - 1
/// are skipped by the caller.  b is clamped to -1 .. ndet - 1: a candidate that is no entry adds nothing.
template <class T> PROST_F2D_HD int FirstCandidate(const T* __restrict__ e, const T* __restrict__ inv, int y, int x, int m, int ndet) {
  const T px = (T)x - e[kSx], py = (T)y - e[kSy];
  const T s = px * e[kCos] + py * e[kSin], l = py * e[kCos] - px * e[kSin];
  T tau = s / l;
  tau = tau > inv[kLo] ? tau : inv[kLo];          // (also NaN, which a pixel of the image cannot give: l >= 1)
  tau = tau < inv[kHi] ? tau : inv[kHi];
  const T z = tau * tau;
  T poly = inv[kPoly + kPolyTerms - 1];
  PROST_F2D_UNROLL(unroll)
  for (int k = kPolyTerms - 2; k >= 0; k--) poly = poly * z + inv[kPoly + k];
  const T gamma = tau + tau * (z * poly);
  T b = std::floor(inv[kK0] + inv[kK1] * gamma);
  b = b > (T)-1 ? b : (T)-1;
  const int bi = b < (T)(ndet - 1) ? (int)b : ndet - 1;
  return bi - m;
}

/// one ray of the forward product over the plane, kForwardBatch driving lines at a time: the positions, weights and (clamped, always
/// valid) indices of a batch first, then all its loads, then the additions in the pinned order
template <class T> PROST_F2D_HD T ForwardSum(const T* __restrict__ e, const Ray<T>& ray, const T* plane, const Geometry& g) {
  const bool column = e[kAxis] != (T)0;
  const int nt = column ? g.nx : g.ny, ni = column ? g.ny : g.nx;
  const int st = column ? g.ny : 1, si = column ? 1 : g.ny;         // a plane holds fewer than 2^31 elements
  const T p = ray.p, c = ray.c, r = ray.r;
  T acc = -(T)0;
  for (int t0 = 0; t0 < nt; t0 += kForwardBatch) {
    T a0[kForwardBatch], a1[kForwardBatch], v0[kForwardBatch], v1[kForwardBatch];
    bool has0[kForwardBatch], has1[kForwardBatch];
    PROST_F2D_UNROLL(unroll)
    for (int k = 0; k < kForwardBatch; k++) {
      const int t = t0 + k < nt ? t0 + k : nt - 1;
      T w0, w1;
      const int i0 = Weights(Position(r, p * (T)t), ni, w0, w1);
      has0[k] = t0 + k < nt && i0 >= 0 && w0 != (T)0;
      has1[k] = t0 + k < nt && i0 >= -1 && i0 + 1 < ni && w1 != (T)0;
      a0[k] = c * w0;
      a1[k] = c * w1;
      v0[k] = plane[t * st + (has0[k] ? i0 : 0) * si];
      v1[k] = plane[t * st + (has1[k] ? i0 + 1 : 0) * si];
    }
    PROST_F2D_UNROLL(unroll)
    for (int k = 0; k < kForwardBatch; k++) { PROST_F2D_PIN(v0[k]); PROST_F2D_PIN(v1[k]); }
    PROST_F2D_UNROLL(unroll)
    for (int k = 0; k < kForwardBatch; k++) {
      if (has0[k]) acc = acc + a0[k] * v0[k];
      if (has1[k]) acc = acc + a1[k] * v1[k];
    }
  }
  return acc;
}

/// one pixel of the adjoint product, M = the margin of the candidate window.  AdjointBatch(M) views at a time: the candidates' weights
/// and (clamped, always valid) bins of a batch first, then all its loads, then the additions in the pinned order.
template <class T, int M> PROST_F2D_HD T AdjointSum(const T* __restrict__ table, const T* sino, const Geometry& g, int y, int x) {
  constexpr int kCandidates = 2 * M + 2, kBatch = AdjointBatch(M);
  const T* __restrict__ bins = BinTable(table, g);
  const T* __restrict__ inv = InverseTable(table, g);
  T acc = -(T)0;
  for (int a0 = 0; a0 < g.na; a0 += kBatch) {
    T w[kBatch][kCandidates], v[kBatch][kCandidates];
    bool has[kBatch][kCandidates];
    PROST_F2D_UNROLL(unroll)
    for (int b = 0; b < kBatch; b++) {
      const int a = a0 + b < g.na ? a0 + b : g.na - 1;
      const T* __restrict__ e = table + (size_t)a * kViewWidth;
      const bool column = e[kAxis] != (T)0;
      const int t = column ? x : y, i = column ? y : x, ni = column ? g.ny : g.nx;
      const int first = FirstCandidate(e, inv, y, x, M, g.ndet);
      const T* row = sino + (size_t)a * (size_t)g.ndet;
      PROST_F2D_UNROLL(unroll)
      for (int k = 0; k < kCandidates; k++) {
        const int d = first + k, dc = d < 0 ? 0 : (d >= g.ndet ? g.ndet - 1 : d);
        const Ray<T> ray = Prologue(e, bins[(size_t)dc * kBinWidth + kSinGamma], bins[(size_t)dc * kBinWidth + kCosGamma]);
        T w0, w1;
        const int i0 = Weights(Position(ray.r, ray.p * (T)t), ni, w0, w1);
        const T wk = i0 == i ? w0 : w1;
        has[b][k] = a0 + b < g.na && d == dc && (i0 == i || i0 + 1 == i) && wk != (T)0;
        w[b][k] = ray.c * wk;
        v[b][k] = row[dc];
      }
    }
    PROST_F2D_UNROLL(unroll)
    for (int b = 0; b < kBatch; b++) {
      PROST_F2D_UNROLL(unroll)
      for (int k = 0; k < kCandidates; k++) PROST_F2D_PIN(v[b][k]);
    }
    PROST_F2D_UNROLL(unroll)
    for (int b = 0; b < kBatch; b++) {
      PROST_F2D_UNROLL(unroll)
      for (int k = 0; k < kCandidates; k++)
        if (has[b][k]) acc = acc + w[b][k] * v[b][k];
    }
  }
  return acc;
}
/// AdjointSum<T, g.m>
template <class T> PROST_F2D_HD T AdjointSumOf(const T* __restrict__ table, const T* sino, const Geometry& g, int y, int x) {
  switch (g.m) {
    case 1: return AdjointSum<T, 1>(table, sino, g, y, x);
    case 2: return AdjointSum<T, 2>(table, sino, g, y, x);
    case 3: return AdjointSum<T, 3>(table, sino, g, y, x);
    case 4: return AdjointSum<T, 4>(table, sino, g, y, x);
    default: return AdjointSum<T, 5>(table, sino, g, y, x);
  }
}

#if !defined(__HIP_DEVICE_COMPILE__)
template <class T> inline Ray<T> RayOf(const T* table, const Geometry& g, int a, int d) {
  const T* bin = BinTable(table, g) + (size_t)d * kBinWidth;
  return Prologue(table + (size_t)a * kViewWidth, bin[kSinGamma], bin[kCosGamma]);
}
/// visit(t, i, value) for every entry of row (a, d) of the matrix, in the forward's order
template <class T, class F> inline void ForEachInRay(const T* table, const Geometry& g, int a, int d, F visit) {
  const T* e = table + (size_t)a * kViewWidth;
  const bool column = e[kAxis] != (T)0;
  const int nt = column ? g.nx : g.ny, ni = column ? g.ny : g.nx;
  const Ray<T> ray = RayOf(table, g, a, d);
  for (int t = 0; t < nt; t++) {
    T w0, w1;
    const int i0 = Weights(Position(ray.r, ray.p * (T)t), ni, w0, w1);
    if (i0 >= 0 && w0 != (T)0) visit(t, i0, ray.c * w0);
    if (i0 >= -1 && i0 + 1 < ni && w1 != (T)0) visit(t, i0 + 1, ray.c * w1);
  }
}
/// visit(a, d, value) for every entry of column (y, x) of the matrix, in the adjoint's order: the gather enumeration
template <class T, class F> inline void ForEachAtPixel(const T* table, const Geometry& g, int y, int x, F visit) {
  const T* inv = InverseTable(table, g);
  for (int a = 0; a < g.na; a++) {
    const T* e = table + (size_t)a * kViewWidth;
    const bool column = e[kAxis] != (T)0;
    const int t = column ? x : y, i = column ? y : x, ni = column ? g.ny : g.nx;
    const int first = FirstCandidate(e, inv, y, x, g.m, g.ndet);
    for (int k = 0; k < 2 * g.m + 2; k++) {
      const int d = first + k;
      if (d < 0 || d >= g.ndet) continue;
      const Ray<T> ray = RayOf(table, g, a, d);
      T w0, w1;
      const int i0 = Weights(Position(ray.r, ray.p * (T)t), ni, w0, w1);
      const T w = i0 == i ? w0 : w1;
      if ((i0 == i || i0 + 1 == i) && w != (T)0) visit(a, d, ray.c * w);
    }
  }
}
/// (y, x) of entry (t, i) of a view
template <class T> inline void PixelOf(const T* table, int a, int t, int i, int& y, int& x) {
  if (table[(size_t)a * kViewWidth + kAxis] != (T)0) { x = t; y = i; } else { y = t; x = i; }
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

/// the products on the host, lane by lane as the kernels run them (tests/host/fanbeam2d_harness.cpp)
template <class T, bool ACC> inline void Apply(T* res, const T* rhs, const Geometry& g, const T* table, bool transpose) {
  const size_t plane = (size_t)g.ny * (size_t)g.nx, sino = (size_t)g.ndet * (size_t)g.na;
  for (int c = 0; c < g.planes; c++) {
    if (!transpose) {
      for (int a = 0; a < g.na; a++)
        for (int d = 0; d < g.ndet; d++) {
          T* o = res + (size_t)c * sino + (size_t)a * (size_t)g.ndet + (size_t)d;
          const T v = ForwardSum<T>(table + (size_t)a * kViewWidth, RayOf(table, g, a, d), rhs + (size_t)c * plane, g);
          *o = ACC ? *o + v : v;
        }
    } else {
      for (int x = 0; x < g.nx; x++)
        for (int y = 0; y < g.ny; y++) {
          T* o = res + (size_t)c * plane + (size_t)y + (size_t)x * (size_t)g.ny;
          const T v = AdjointSumOf<T>(table, rhs + (size_t)c * sino, g, y, x);
          *o = ACC ? *o + v : v;
        }
    }
  }
}
#endif

}  // namespace fanbeam2d
}  // namespace prost
#endif
