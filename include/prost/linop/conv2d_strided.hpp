// prost/linop/conv2d_strided.hpp -- the arithmetic of BlockConv2DStrided: blur, then keep every s-th pixel (K = S B, the operator of
// super-resolution), and its adjoint, the fractionally strided convolution, without a matrix.  Written from the definition; the
// conventions (layout, shapes, tap records, order of operations) are those of conv2d.hpp, which this header includes and reuses.
//
// Images are ny x nx, column-major, L planes: element (y, x, c) at y + x ny + c nx ny.  The window k is ky x kx, rounded to T.  The
// shape gives the size (cy, cx) of the un-decimated convolution and its crop offset (oy, ox) exactly as conv2d::OutputSize.  With
// stride (sy, sx), each 1 .. 4, and phase (py, px), 0 <= py < min(sy, cy), 0 <= px < min(sx, cx), the output plane is my x mx,
// my = (cy - 1 - py) / sy + 1, mx likewise, and
//
//   forward:  out(y, x) = sum_{i, j}  k(i, j) in(y sy + py + oy - i, x sx + px + ox - j)                       (zero outside the image)
//   adjoint:  in'(v, u) = sum_{i, j, y, x : y sy + py + oy - i = v, x sx + px + ox - j = u, 0 <= y < my, 0 <= x < mx}  k(i, j) out(y, x)
//
// Order of operations (kernels and host build without contraction): zero taps are dropped; the terms of one result are visited by
// ascending source index -- source column ascending, source row ascending within a column: forward j from kx - 1 down to 0 and inside
// that i from ky - 1 down to 0, adjoint j ascending and inside that i ascending, restricted to the residue class of the destination
// pixel (i = py + oy - v mod sy, j = px + ox - u mod sx); source cells outside the plane take part as zeros; the accumulator starts at
// -0; every product and every addition is one rounding in T; the accumulating form stores res + value last.  A destination pixel of
// the adjoint whose class holds no non-zero tap stores zero (the accumulating form adds that zero: res stays numerically unchanged).
// With stride (1, 1) and phase (0, 0) this is, term for term, conv2d in both directions.
//
// Forward tile: ty x tx outputs of one plane (kTiles, chosen by PickTile: the first entry whose staged tile fits kLdsLimit), lanes
// along y, `outputs` neighbouring outputs along x per lane.  Its source tile of ((ty - 1) sy + ky) x ((tx - 1) sx + kx) cells is staged
// de-interleaved by row residue: tile row r goes to sub-plane r mod sy, position r / sy, so tap (i, j) of output row t reads position
// t + (ky - 1 - i) / sy of sub-plane (ky - 1 - i) mod sy -- consecutive words for consecutive lanes.  A sub-plane has
// SubPitch = ty + (ky - 1) / sy positions, a column sy SubPitch cells.  Cell (ly, lx) of the tile of the outputs at (y0, x0) is source
// (y0 sy + py + oy - (ky - 1) + ly, x0 sx + px + ox - (kx - 1) + lx).
//
// Adjoint tile: kAdjLanes sy x kAdjColumns destination pixels; a lane owns sy consecutive rows v0 + l sy + ry of kAdjOutputs
// neighbouring columns, one accumulator each.  All residues of a lane read the staged source rows l + const of the natural layout:
// cell (ly, lx) is source (v0 / sy - lo + ly, X0 + lx), lo = (py + oy) / sy, X0 = floor((u0 - px - ox) / sx).  The taps are sorted into
// one sub-list per class (ry, rx), class_start[ry sx + rx] .. class_start[ry sx + rx + 1], each in the order above.
// res and rhs must not overlap.
#ifndef PROST_LINOP_CONV2D_STRIDED_HPP_
#define PROST_LINOP_CONV2D_STRIDED_HPP_
#include "prost/linop/conv2d.hpp"

namespace prost {
namespace conv2d_strided {

using conv2d::Tap;
using conv2d::kMaxWindow;

constexpr int kMaxStride = 4;                               ///< strides 1 .. 4 per axis
constexpr int kClasses = kMaxStride * kMaxStride;           ///< residue classes (ry, rx) of the adjoint
constexpr int kThreads = 256;                               ///< lanes of a workgroup
constexpr size_t kLdsLimit = 65536;                         ///< bytes of LDS a workgroup may have

/// a forward tile: ty x tx outputs, `outputs` of them along x per lane; ty tx / outputs <= kThreads lanes work
struct Tile { int ty, tx, outputs; };
constexpr int kTileCount = 5;
constexpr Tile kTiles[kTileCount] = {{64, 16, 4}, {64, 8, 2}, {64, 4, 1}, {32, 8, 1}, {32, 4, 1}};

constexpr int kAdjLanes = 64;                               ///< lanes along y of an adjoint tile (sy destination rows each)
constexpr int kAdjOutputs = 4;                              ///< destination columns a lane keeps in registers
constexpr int kAdjColumns = (kThreads / kAdjLanes) * kAdjOutputs;   ///< destination columns of an adjoint tile

/// the operator (the layout of prost_hip_conv2d_strided_geometry in prost_hip.h); one record per direction, they differ in
/// `transpose` and in the class table
struct Geometry {
  int32_t ny, nx;         ///< image plane
  int32_t my, mx;         ///< decimated output plane
  int32_t oy, ox;         ///< crop offset into the full convolution
  int32_t ky, kx;         ///< window
  int32_t sy, sx;         ///< stride
  int32_t py, px;         ///< phase
  int32_t planes;         ///< L
  int32_t transpose;      ///< 0: rhs is an image, res an output; 1: the adjoint
  int32_t class_start[kClasses + 1];   ///< adjoint: the sub-list of class c = ry sx + rx is [class_start[c], class_start[c + 1]); forward: { 0, ntaps, .. }
};

PROST_C2D_HD int FloorDiv(int a, int b) { const int q = a / b; return (a % b != 0 && (a < 0)) ? q - 1 : q; }
PROST_C2D_HD int Clamp(int v, int n, bool& inside) { const int c = v < 0 ? 0 : (v >= n ? n - 1 : v); inside = c == v; return c; }

/// the decimated size; false: an empty convolution, an unknown shape, or stride / phase out of range
inline bool OutputSize(int shape, long ny, long nx, long ky, long kx, long sy, long sx, long py, long px, long& my, long& mx, long& oy, long& ox) {
  long cy = 0, cx = 0;
  if (!conv2d::OutputSize(shape, ny, nx, ky, kx, cy, cx, oy, ox)) return false;
  if (sy < 1 || sx < 1 || sy > kMaxStride || sx > kMaxStride) return false;
  if (py < 0 || px < 0 || py >= (sy < cy ? sy : cy) || px >= (sx < cx ? sx : cx)) return false;
  my = (cy - 1 - py) / sy + 1;
  mx = (cx - 1 - px) / sx + 1;
  return true;
}

// ---- forward: the staged tile ----
PROST_C2D_HD int SubPitch(int ty, int ky, int sy) { return ty + (ky - 1) / sy; }
PROST_C2D_HD int ForwardRows(int ty, int ky, int sy) { return (ty - 1) * sy + ky; }
PROST_C2D_HD int ForwardColumns(int tx, int kx, int sx) { return (tx - 1) * sx + kx; }
PROST_C2D_HD size_t ForwardLdsElements(const Tile& t, int ky, int kx, int sy, int sx) {
  return (size_t)sy * (size_t)SubPitch(t.ty, ky, sy) * (size_t)ForwardColumns(t.tx, kx, sx);
}
/// the tile of a forward product: the first entry of kTiles whose staged tile fits (the last one always does)
inline int PickTile(size_t element_bytes, int sy, int sx, int ky, int kx) {
  for (int t = 0; t < kTileCount; t++)
    if (ForwardLdsElements(kTiles[t], ky, kx, sy, sx) * element_bytes <= kLdsLimit) return t;
  return -1;
}
/// where tile cell (ly, lx) lives in LDS
PROST_C2D_HD int ForwardCell(int ly, int lx, int sy, int subpitch) { return ly / sy + (ly % sy) * subpitch + lx * sy * subpitch; }
/// where it comes from: always a valid index of the plane, inside = false: the cell is zero
PROST_C2D_HD size_t ForwardSourceIndex(const Geometry& g, int y0, int x0, int ly, int lx, bool& inside) {
  bool iy, ix;
  const int cy = Clamp(y0 * g.sy + g.py + g.oy - (g.ky - 1) + ly, g.ny, iy), cx = Clamp(x0 * g.sx + g.px + g.ox - (g.kx - 1) + lx, g.nx, ix);
  inside = iy && ix;
  return (size_t)cy + (size_t)cx * (size_t)g.ny;
}

// ---- adjoint: the staged tile ----
PROST_C2D_HD int AdjointLow(const Geometry& g) { return (g.py + g.oy) / g.sy; }
PROST_C2D_HD int AdjointPitch(const Geometry& g) { return kAdjLanes + AdjointLow(g) + (g.sy + g.ky - 2 - g.py - g.oy) / g.sy; }
/// an upper bound of the staged columns of any tile, and the columns of the tile of destination columns u0 ..
PROST_C2D_HD int AdjointColumnBound(const Geometry& g) { return (kAdjColumns + g.kx - 2) / g.sx + 2; }
PROST_C2D_HD int AdjointFirstColumn(const Geometry& g, int u0) { return FloorDiv(u0 - g.px - g.ox, g.sx); }
PROST_C2D_HD int AdjointColumns(const Geometry& g, int u0) { return FloorDiv(u0 + kAdjColumns - 1 + g.kx - 1 - g.px - g.ox, g.sx) - AdjointFirstColumn(g, u0) + 1; }
PROST_C2D_HD size_t AdjointSourceIndex(const Geometry& g, int v0, int u0, int ly, int lx, bool& inside) {
  bool iy, ix;
  const int cy = Clamp(v0 / g.sy - AdjointLow(g) + ly, g.my, iy), cx = Clamp(AdjointFirstColumn(g, u0) + lx, g.mx, ix);
  inside = iy && ix;
  return (size_t)cy + (size_t)cx * (size_t)g.my;
}

// ---- tables ----
/// the operator's record for one direction, its class table still empty
inline Geometry MakeGeometry(int shape, long ny, long nx, long ky, long kx, long sy, long sx, long py, long px, long planes, bool transpose) {
  long my = 0, mx = 0, oy = 0, ox = 0;
  OutputSize(shape, ny, nx, ky, kx, sy, sx, py, px, my, mx, oy, ox);
  Geometry g;
  g.ny = (int32_t)ny; g.nx = (int32_t)nx; g.my = (int32_t)my; g.mx = (int32_t)mx; g.oy = (int32_t)oy; g.ox = (int32_t)ox;
  g.ky = (int32_t)ky; g.kx = (int32_t)kx; g.sy = (int32_t)sy; g.sx = (int32_t)sx; g.py = (int32_t)py; g.px = (int32_t)px;
  g.planes = (int32_t)planes; g.transpose = transpose ? 1 : 0;
  for (int c = 0; c <= kClasses; c++) g.class_start[c] = 0;
  return g;
}

/// the window rounded to T (column-major ky x kx, NOT flipped: both directions index it by (i, j))
template <class T> inline std::vector<T> Window(const double* k, long ky, long kx) { return conv2d::Window<T>(k, ky, kx, false); }

/// the tap table of a direction in the order the march visits it, for the forward tile `tile`; fills g.class_start
template <class T> inline std::vector<Tap<T>> CompactTaps(Geometry& g, const std::vector<T>& w, int tile) {
  std::vector<Tap<T>> taps;
  const int ky = g.ky, kx = g.kx, sy = g.sy, sx = g.sx;
  for (int c = 0; c <= kClasses; c++) g.class_start[c] = 0;
  if (!g.transpose) {
    const int sub = SubPitch(kTiles[tile].ty, ky, sy);
    for (int j = kx - 1; j >= 0; j--)
      for (int i = ky - 1; i >= 0; i--) {
        const T v = w[(size_t)(i + j * ky)];
        if (v != (T)0) { Tap<T> t; t.offset = (int32_t)ForwardCell(ky - 1 - i, kx - 1 - j, sy, sub); t.value = v; taps.push_back(t); }
      }
    for (int c = 1; c <= kClasses; c++) g.class_start[c] = (int32_t)taps.size();
    return taps;
  }
  const int cyo = g.py + g.oy, cxo = g.px + g.ox, lo = AdjointLow(g), pitch = AdjointPitch(g);
  for (int ry = 0; ry < sy; ry++)
    for (int rx = 0; rx < sx; rx++) {
      g.class_start[ry * sx + rx] = (int32_t)taps.size();
      for (int j = 0; j < kx; j++)
        for (int i = 0; i < ky; i++) {
          if ((ry + i - cyo) % sy != 0 || (rx + j - cxo) % sx != 0) continue;
          const T v = w[(size_t)(i + j * ky)];
          if (v == (T)0) continue;
          Tap<T> t; t.offset = (int32_t)((ry + i - cyo) / sy + lo + ((rx + j - cxo) / sx) * pitch); t.value = v; taps.push_back(t);
        }
    }
  for (int c = sy * sx; c <= kClasses; c++) g.class_start[c] = (int32_t)taps.size();
  return taps;
}

// ---- the marches ----
/// forward: the R outputs (ty, tx .. tx + R - 1) of a tile; `cell` points at the staged cell of output (ty, tx), xstep = sx sy SubPitch
template <class T, int R> PROST_C2D_HD void ForwardMarch(T (&acc)[R], const T* cell, int xstep, const Tap<T>* __restrict__ taps, int ntaps) {
  for (int r = 0; r < R; r++) acc[r] = -(T)0;
  for (int t = 0; t < ntaps; t++) {
    const T* c = cell + taps[t].offset;
    const T k = taps[t].value;
    for (int r = 0; r < R; r++) acc[r] = acc[r] + k * c[r * xstep];
  }
}
template <class T, int R, bool ACC> PROST_C2D_HD void ForwardStore(T* plane, const Geometry& g, int y, int x, const T (&acc)[R]) {
  if (y >= g.my) return;
  for (int r = 0; r < R; r++)
    if (x + r < g.mx) {
      T* p = plane + (size_t)y + (size_t)(x + r) * (size_t)g.my;
      *p = ACC ? *p + acc[r] : acc[r];
    }
}
/// adjoint: the SY rows of destination column u of lane l; `column` points at staged cell (l, 0); X0 the tile's first source column
template <class T, int SY> PROST_C2D_HD void AdjointMarch(T (&acc)[SY], const T* column, const Geometry& g, int u, int X0, int pitch, const Tap<T>* __restrict__ taps) {
  const int rx = u % g.sx;
  const T* cell = column + (u / g.sx - X0) * pitch;
  for (int ry = 0; ry < SY; ry++) {
    const int t0 = g.class_start[ry * g.sx + rx], t1 = g.class_start[ry * g.sx + rx + 1];
    T a = -(T)0;
    for (int t = t0; t < t1; t++) a = a + taps[t].value * cell[taps[t].offset];
    acc[ry] = (t0 == t1) ? (T)0 : a;
  }
}
/// one element at a time (the kernel moves the SY values of a lane at once where the address allows: the same bits)
template <class T, int SY, bool ACC> PROST_C2D_HD void AdjointStoreElements(T* plane, const Geometry& g, int v, int u, const T (&acc)[SY]) {
  if (u >= g.nx) return;
  T* p = plane + (size_t)v + (size_t)u * (size_t)g.ny;
  for (int ry = 0; ry < SY; ry++)
    if (v + ry < g.ny) p[ry] = ACC ? p[ry] + acc[ry] : acc[ry];
}

#if !defined(__HIP_DEVICE_COMPILE__)
/// the product of one direction on the host, tile by tile and lane by lane as the kernels run it (tests/host/conv2d_strided_harness.cpp).
/// `tile`: the forward tile the table was made for.
template <class T, bool ACC> inline void Apply(T* res, const T* rhs, const Geometry& g, const Tap<T>* taps, int ntaps, int tile) {
  if (!g.transpose) {
    const Tile tl = kTiles[tile];
    const int rows = ForwardRows(tl.ty, g.ky, g.sy), cols = ForwardColumns(tl.tx, g.kx, g.sx), sub = SubPitch(tl.ty, g.ky, g.sy);
    std::vector<T> lds(ForwardLdsElements(tl, g.ky, g.kx, g.sy, g.sx));
    for (int plane = 0; plane < g.planes; plane++) {
      const T* src = rhs + (size_t)plane * (size_t)g.ny * (size_t)g.nx;
      T* dst = res + (size_t)plane * (size_t)g.my * (size_t)g.mx;
      for (int x0 = 0; x0 < g.mx; x0 += tl.tx)
        for (int y0 = 0; y0 < g.my; y0 += tl.ty) {
          for (int lx = 0; lx < cols; lx++)
            for (int ly = 0; ly < rows; ly++) {
              bool inside;
              const T v = src[ForwardSourceIndex(g, y0, x0, ly, lx, inside)];
              lds[(size_t)ForwardCell(ly, lx, g.sy, sub)] = inside ? v : (T)0;
            }
          for (int tx = 0; tx < tl.tx; tx += tl.outputs)
            for (int ty = 0; ty < tl.ty; ty++) {
              const T* cell = lds.data() + ty + tx * g.sx * g.sy * sub;
              const int xstep = g.sx * g.sy * sub;
              if (tl.outputs == 4) { T a[4]; ForwardMarch<T, 4>(a, cell, xstep, taps, ntaps); ForwardStore<T, 4, ACC>(dst, g, y0 + ty, x0 + tx, a); }
              else if (tl.outputs == 2) { T a[2]; ForwardMarch<T, 2>(a, cell, xstep, taps, ntaps); ForwardStore<T, 2, ACC>(dst, g, y0 + ty, x0 + tx, a); }
              else { T a[1]; ForwardMarch<T, 1>(a, cell, xstep, taps, ntaps); ForwardStore<T, 1, ACC>(dst, g, y0 + ty, x0 + tx, a); }
            }
        }
    }
    return;
  }
  const int pitch = AdjointPitch(g), bound = AdjointColumnBound(g);
  std::vector<T> lds((size_t)pitch * (size_t)bound);
  for (int plane = 0; plane < g.planes; plane++) {
    const T* src = rhs + (size_t)plane * (size_t)g.my * (size_t)g.mx;
    T* dst = res + (size_t)plane * (size_t)g.ny * (size_t)g.nx;
    for (int u0 = 0; u0 < g.nx; u0 += kAdjColumns)
      for (int v0 = 0; v0 < g.ny; v0 += kAdjLanes * g.sy) {
        const int cols = AdjointColumns(g, u0), X0 = AdjointFirstColumn(g, u0);
        for (int lx = 0; lx < cols; lx++)
          for (int ly = 0; ly < pitch; ly++) {
            bool inside;
            const T v = src[AdjointSourceIndex(g, v0, u0, ly, lx, inside)];
            lds[(size_t)(ly + lx * pitch)] = inside ? v : (T)0;
          }
        for (int c = 0; c < kAdjColumns; c++)
          for (int l = 0; l < kAdjLanes; l++) {
            const int u = u0 + c, v = v0 + l * g.sy;
            if (u >= g.nx || v >= g.ny) continue;
            switch (g.sy) {
              case 1: { T a[1]; AdjointMarch<T, 1>(a, lds.data() + l, g, u, X0, pitch, taps); AdjointStoreElements<T, 1, ACC>(dst, g, v, u, a); break; }
              case 2: { T a[2]; AdjointMarch<T, 2>(a, lds.data() + l, g, u, X0, pitch, taps); AdjointStoreElements<T, 2, ACC>(dst, g, v, u, a); break; }
              case 3: { T a[3]; AdjointMarch<T, 3>(a, lds.data() + l, g, u, X0, pitch, taps); AdjointStoreElements<T, 3, ACC>(dst, g, v, u, a); break; }
              default: { T a[4]; AdjointMarch<T, 4>(a, lds.data() + l, g, u, X0, pitch, taps); AdjointStoreElements<T, 4, ACC>(dst, g, v, u, a); break; }
            }
          }
      }
  }
}

// ---- preconditioner sums ----
/// the window indices along one axis that reach a pixel: { lo, lo + step, .. <= hi }, empty if lo > hi
struct AxisClass { int lo, hi, step; };
/// row q of the output (forward matrix rows): every i with 0 <= q s + p + o - i < n
inline AxisClass ForwardAxis(int q, int s, int p, int o, int n, int k) {
  const int Y = q * s + p + o;
  AxisClass a; a.lo = Y - n + 1 < 0 ? 0 : Y - n + 1; a.hi = Y > k - 1 ? k - 1 : Y; a.step = 1;
  return a;
}
/// pixel v of the image (columns of the matrix): every i = p + o - v mod s with 0 <= (v + i - p - o) / s < m
inline AxisClass AdjointAxis(int v, int s, int p, int o, int m, int k) {
  const int d = p + o - v;
  AxisClass a; a.step = s;
  a.lo = d >= 0 ? d : ((d % s) + s) % s;
  a.hi = d + (m - 1) * s > k - 1 ? k - 1 : d + (m - 1) * s;
  if (a.lo > a.hi) { a.lo = 1; a.hi = 0; a.step = 1; }           // one name for the empty class
  return a;
}
inline AxisClass AxisOf(const Geometry& g, bool columns_of_matrix, bool along_x, int q) {
  if (!columns_of_matrix) return along_x ? ForwardAxis(q, g.sx, g.px, g.ox, g.nx, g.kx) : ForwardAxis(q, g.sy, g.py, g.oy, g.ny, g.ky);
  return along_x ? AdjointAxis(q, g.sx, g.px, g.ox, g.mx, g.kx) : AdjointAxis(q, g.sy, g.py, g.oy, g.my, g.ky);
}
/// sum |w(i, j)|^alpha over the taps of one pixel: one row sum (columns_of_matrix: one column sum) of the matrix
template <class T> inline double SumAt(const Geometry& g, const std::vector<T>& w, double alpha, bool columns_of_matrix, int y, int x) {
  const AxisClass a = AxisOf(g, columns_of_matrix, false, y), b = AxisOf(g, columns_of_matrix, true, x);
  double s = 0;
  for (int j = b.lo; j <= b.hi; j += b.step)
    for (int i = a.lo; i <= a.hi; i += a.step) s += conv2d::PowAbs((double)w[(size_t)(i + j * g.ky)], alpha);
  return s;
}
/// out[p] += the row sums (columns_of_matrix: the column sums) of |entry|^alpha, one plane after the other: per axis the table of the
/// distinct (residue, range) classes, per pair of classes one sum of non-negative terms in double, one look-up per pixel
template <class T> inline void Sums(const Geometry& g, const std::vector<T>& w, double alpha, bool columns_of_matrix, T* out) {
  const int dny = columns_of_matrix ? g.ny : g.my, dnx = columns_of_matrix ? g.nx : g.mx;
  std::vector<int> yid((size_t)dny), xid((size_t)dnx);
  std::vector<AxisClass> yc, xc;
  auto classify = [&](bool along_x, int n, std::vector<AxisClass>& cls, std::vector<int>& id) {
    for (int q = 0; q < n; q++) {
      const AxisClass a = AxisOf(g, columns_of_matrix, along_x, q);
      size_t c = cls.size();
      for (size_t e = cls.size(); e-- > 0;)                   // the neighbours' classes come first: runs and short cycles
        if (cls[e].lo == a.lo && cls[e].hi == a.hi && cls[e].step == a.step) { c = e; break; }
      if (c == cls.size()) cls.push_back(a);
      id[(size_t)q] = (int)c;
    }
  };
  classify(false, dny, yc, yid);
  classify(true, dnx, xc, xid);
  std::vector<double> table(yc.size() * xc.size()), column((size_t)g.kx);
  for (size_t a = 0; a < yc.size(); a++) {
    for (int j = 0; j < g.kx; j++) {
      double s = 0;
      for (int i = yc[a].lo; i <= yc[a].hi; i += yc[a].step) s += conv2d::PowAbs((double)w[(size_t)(i + j * g.ky)], alpha);
      column[(size_t)j] = s;
    }
    for (size_t b = 0; b < xc.size(); b++) {
      double s = 0;
      for (int j = xc[b].lo; j <= xc[b].hi; j += xc[b].step) s += column[(size_t)j];
      table[a * xc.size() + b] = s;
    }
  }
  for (int plane = 0; plane < g.planes; plane++) {
    T* o = out + (size_t)plane * (size_t)dny * (size_t)dnx;
    for (int x = 0; x < dnx; x++) {
      const double* row = table.data() + xid[(size_t)x];
      for (int y = 0; y < dny; y++) o[(size_t)y + (size_t)x * (size_t)dny] += (T)row[(size_t)yid[(size_t)y] * xc.size()];
    }
  }
}
#endif

}  // namespace conv2d_strided
}  // namespace prost
#endif
