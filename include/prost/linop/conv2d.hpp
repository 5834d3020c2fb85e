// prost/linop/conv2d.hpp -- the arithmetic of BlockConv2D: one small window applied at every pixel of L image planes, zero padding,
// without a matrix.  The reference has no such block (its deblurring example hands kron(speye(nc), convmtx2(kernel, ny, nx)) over as a
// sparse matrix); this is written from the definition.
//
// Images are ny x nx, column-major: element (y, x, c) at y + x ny + c nx ny.  The window k is ky x kx, column-major, rounded to T.
// With (oy, ox) the crop offset into the full convolution and (my, mx) the output size
//
//   out(y, x) = sum over taps (i, j) with k(i, j) != 0 and 0 <= y + oy - i < ny, 0 <= x + ox - j < nx  of  k(i, j) in(y + oy - i, x + ox - j)
//
//   "full":  (oy, ox) = (0, 0),                 (my, mx) = (ny + ky - 1, nx + kx - 1)
//   "same":  (oy, ox) = (ky / 2, kx / 2),       (my, mx) = (ny, nx)
//   "valid": (oy, ox) = (ky - 1, kx - 1),       (my, mx) = (ny - ky + 1, nx - kx + 1)
//
// The adjoint is the same formula with the window flipped in both axes, source size (my, mx), destination size (ny, nx) and offsets
// (ky - 1 - oy, kx - 1 - ox): one Geometry record and one tap table per direction, one march for both.
//
// Order of operations (the one place it is written down; kernels and host library build without contraction): zero taps are dropped;
// the others are visited by ascending source index -- source column ascending, within a column source row ascending, i.e. j from
// kx - 1 down to 0 and inside that i from ky - 1 down to 0; out-of-range source cells take part as zeros (a staged tile holds them as
// zeros); the sum starts from the first term (the accumulator starts at -0, and -0 + p == p for every p); every product and every
// addition is one rounding in T; the accumulating forms store res + value.
//
// A tile of kTileY x kTileX outputs of one plane reads a staged source tile of (kTileY + ky - 1) x (kTileX + kx - 1) cells with the
// fixed column pitch kPitch; cell (ly, lx) of the tile of outputs (y0, x0) is source (y0 + oy - (ky - 1) + ly, x0 + ox - (kx - 1) + lx).
// Tap (i, j) of the output at tile position (ty, tx) reads cell (ty + ky - 1 - i, tx + kx - 1 - j): its table entry holds the
// offset (ky - 1 - i) + (kx - 1 - j) kPitch.  res and rhs must not overlap.
#ifndef PROST_LINOP_CONV2D_HPP_
#define PROST_LINOP_CONV2D_HPP_
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PROST_C2D_HD __host__ __device__ __forceinline__
#else
#define PROST_C2D_HD inline
#endif

namespace prost {
namespace conv2d {

constexpr int kMaxWindow = 31;                    ///< windows up to 31 x 31
constexpr int kTileY = 64;                        ///< outputs of a tile along y (the contiguous axis: one lane each)
constexpr int kTileX = 16;                        ///< outputs of a tile along x
constexpr int kOutputs = 4;                       ///< outputs along x one lane keeps in registers
constexpr int kPitch = kTileY + kMaxWindow - 1;   ///< column pitch of a staged tile, in elements (the same for every window)

enum Shape { kFull = 0, kSame = 1, kValid = 2 };

/// one direction of the operator (the layout of prost_hip_conv2d_geometry in prost_hip.h)
struct Geometry {
  int32_t sny, snx;       ///< source plane
  int32_t dny, dnx;       ///< destination plane
  int32_t oy, ox;         ///< crop offset into the full convolution of the source with this direction's window
  int32_t ky, kx;         ///< window
  int32_t planes;         ///< L
};

/// one non-zero tap: the offset of its cell in a staged tile, relative to the output's own position, and its value
template <class T> struct Tap {
  int32_t offset;
  T value;
};

/// the output size of the forward direction; false: empty ("valid" with a window larger than the image) or an unknown shape
inline bool OutputSize(int shape, long ny, long nx, long ky, long kx, long& my, long& mx, long& oy, long& ox) {
  switch (shape) {
    case kFull: oy = 0; ox = 0; my = ny + ky - 1; mx = nx + kx - 1; break;
    case kSame: oy = ky / 2; ox = kx / 2; my = ny; mx = nx; break;
    case kValid: oy = ky - 1; ox = kx - 1; my = ny - ky + 1; mx = nx - kx + 1; break;
    default: return false;
  }
  return my >= 1 && mx >= 1;
}

/// the record of one direction: forward reads ny x nx and writes my x mx, the adjoint the other way round with mirrored offsets
inline Geometry MakeGeometry(int shape, long ny, long nx, long ky, long kx, long planes, bool adjoint) {
  long my = 0, mx = 0, oy = 0, ox = 0;
  OutputSize(shape, ny, nx, ky, kx, my, mx, oy, ox);
  Geometry g;
  g.ky = (int32_t)ky; g.kx = (int32_t)kx; g.planes = (int32_t)planes;
  if (!adjoint) { g.sny = (int32_t)ny; g.snx = (int32_t)nx; g.dny = (int32_t)my; g.dnx = (int32_t)mx; g.oy = (int32_t)oy; g.ox = (int32_t)ox; }
  else { g.sny = (int32_t)my; g.snx = (int32_t)mx; g.dny = (int32_t)ny; g.dnx = (int32_t)nx; g.oy = (int32_t)(ky - 1 - oy); g.ox = (int32_t)(kx - 1 - ox); }
  return g;
}

/// the window of one direction rounded to T (column-major ky x kx); the adjoint's is flipped in both axes
template <class T> inline std::vector<T> Window(const double* k, long ky, long kx, bool adjoint) {
  std::vector<T> w((size_t)(ky * kx));
  for (long j = 0; j < kx; j++)
    for (long i = 0; i < ky; i++) w[(size_t)(i + j * ky)] = (T)(adjoint ? k[(ky - 1 - i) + (kx - 1 - j) * ky] : k[i + j * ky]);
  return w;
}

/// tap compaction: the non-zero taps of a direction's window in the order the march visits them (ascending offset)
template <class T> inline std::vector<Tap<T>> CompactTaps(const std::vector<T>& w, long ky, long kx) {
  std::vector<Tap<T>> taps;
  for (long j = kx - 1; j >= 0; j--)
    for (long i = ky - 1; i >= 0; i--) {
      const T v = w[(size_t)(i + j * ky)];
      if (v != (T)0) { Tap<T> t; t.offset = (int32_t)((ky - 1 - i) + (kx - 1 - j) * kPitch); t.value = v; taps.push_back(t); }
    }
  return taps;
}

/// where cell (ly, lx) of the staged tile of the outputs at (y0, x0) comes from: the index of the source element in its plane and
/// inside = true, or the index of the nearest element of the plane and inside = false (the cell is then zero).  The index is always
/// valid, so a caller can load first and choose afterwards, with all its loads in flight at once.
PROST_C2D_HD size_t SourceIndex(const Geometry& g, int y0, int x0, int ly, int lx, bool& inside) {
  const int sy = y0 + g.oy - (g.ky - 1) + ly, sx = x0 + g.ox - (g.kx - 1) + lx;
  const int cy = sy < 0 ? 0 : (sy >= g.sny ? g.sny - 1 : sy), cx = sx < 0 ? 0 : (sx >= g.snx ? g.snx - 1 : sx);
  inside = cy == sy && cx == sx;
  return (size_t)cy + (size_t)cx * (size_t)g.sny;
}
/// the value of that cell
template <class T> PROST_C2D_HD T SourceCell(const T* plane, const Geometry& g, int y0, int x0, int ly, int lx) {
  bool inside;
  const T v = plane[SourceIndex(g, y0, x0, ly, lx, inside)];
  return inside ? v : (T)0;
}

/// the march over the tap list for the R outputs (ty, tx .. tx + R - 1) of a tile; `cell` points at staged cell (ty, tx)
template <class T, int R> PROST_C2D_HD void March(T (&acc)[R], const T* cell, const Tap<T>* __restrict__ taps, int ntaps) {
  for (int r = 0; r < R; r++) acc[r] = -(T)0;
  for (int t = 0; t < ntaps; t++) {
    const T* c = cell + taps[t].offset;
    const T k = taps[t].value;
    for (int r = 0; r < R; r++) acc[r] = acc[r] + k * c[r * kPitch];
  }
}

/// the finished sums of a lane go to the destination plane; the accumulating form adds the sum onto res last
template <class T, int R, bool ACC> PROST_C2D_HD void Store(T* plane, const Geometry& g, int y, int x, const T (&acc)[R]) {
  if (y >= g.dny) return;
  for (int r = 0; r < R; r++)
    if (x + r < g.dnx) {
      T* p = plane + (size_t)y + (size_t)(x + r) * (size_t)g.dny;
      *p = ACC ? *p + acc[r] : acc[r];
    }
}

#if !defined(__HIP_DEVICE_COMPILE__)
/// the product of one direction on the host, tile by tile and lane by lane as the kernel runs it (tests/host/conv2d_harness.cpp)
template <class T, bool ACC> inline void Apply(T* res, const T* rhs, const Geometry& g, const Tap<T>* taps, int ntaps) {
  const int rows = kTileY + g.ky - 1, cols = kTileX + g.kx - 1;
  std::vector<T> tile((size_t)kPitch * (size_t)cols);
  for (int plane = 0; plane < g.planes; plane++) {
    const T* src = rhs + (size_t)plane * (size_t)g.sny * (size_t)g.snx;
    T* dst = res + (size_t)plane * (size_t)g.dny * (size_t)g.dnx;
    for (int x0 = 0; x0 < g.dnx; x0 += kTileX)
      for (int y0 = 0; y0 < g.dny; y0 += kTileY) {
        for (int lx = 0; lx < cols; lx++)
          for (int ly = 0; ly < rows; ly++) tile[(size_t)(ly + lx * kPitch)] = SourceCell(src, g, y0, x0, ly, lx);
        for (int tx = 0; tx < kTileX; tx += kOutputs)
          for (int ty = 0; ty < kTileY; ty++) {
            T acc[kOutputs];
            March<T, kOutputs>(acc, tile.data() + ty + tx * kPitch, taps, ntaps);
            Store<T, kOutputs, ACC>(dst, g, y0 + ty, x0 + tx, acc);
          }
      }
  }
}

inline double PowAbs(double v, double alpha) { return v == 0 ? 0.0 : std::pow(std::fabs(v), alpha); }

/// the window rows that reach destination row y (columns: the same with x): i in [lo, hi], empty if lo > hi
inline void TapRange(int y, int o, int sn, int k, int& lo, int& hi) {
  lo = y + o - sn + 1; if (lo < 0) lo = 0;
  hi = y + o; if (hi > k - 1) hi = k - 1;
}

/// sum |w(i, j)|^alpha over the taps that reach destination pixel (y, x) of a direction: one row sum of its matrix, O(taps)
template <class T> inline double SumAt(const Geometry& g, const std::vector<T>& w, double alpha, int y, int x) {
  int i0, i1, j0, j1;
  TapRange(y, g.oy, g.sny, g.ky, i0, i1);
  TapRange(x, g.ox, g.snx, g.kx, j0, j1);
  double s = 0;
  for (int j = j0; j <= j1; j++)
    for (int i = i0; i <= i1; i++) s += PowAbs((double)w[(size_t)(i + j * g.ky)], alpha);
  return s;
}

/// out[p] += the sum of |entry|^alpha of row p of a direction's matrix, one plane after the other.  The taps that reach a pixel form a
/// rectangle [i0, i1] x [j0, j1] of the window; along an axis at most 2 k distinct ranges occur, in runs of neighbouring pixels.  Per
/// distinct row range the window is summed down its columns once, per distinct pair of ranges those column sums are added up: every
/// sum is a sum of non-negative terms in double (no differences of table entries, so a small rectangle keeps its relative accuracy),
/// O(ky kx (ky + kx)) work for the table and one look-up per pixel.
template <class T> inline void RowSums(const Geometry& g, const std::vector<T>& w, double alpha, T* out) {
  struct Range { int lo, hi; };
  std::vector<int> yid((size_t)g.dny), xid((size_t)g.dnx);
  std::vector<Range> yr, xr;
  for (int y = 0; y < g.dny; y++) {
    Range r; TapRange(y, g.oy, g.sny, g.ky, r.lo, r.hi);
    if (yr.empty() || yr.back().lo != r.lo || yr.back().hi != r.hi) yr.push_back(r);
    yid[(size_t)y] = (int)yr.size() - 1;
  }
  for (int x = 0; x < g.dnx; x++) {
    Range r; TapRange(x, g.ox, g.snx, g.kx, r.lo, r.hi);
    if (xr.empty() || xr.back().lo != r.lo || xr.back().hi != r.hi) xr.push_back(r);
    xid[(size_t)x] = (int)xr.size() - 1;
  }
  std::vector<double> table(yr.size() * xr.size()), column((size_t)g.kx);
  for (size_t a = 0; a < yr.size(); a++) {
    for (int j = 0; j < g.kx; j++) {
      double s = 0;
      for (int i = yr[a].lo; i <= yr[a].hi; i++) s += PowAbs((double)w[(size_t)(i + j * g.ky)], alpha);
      column[(size_t)j] = s;
    }
    for (size_t b = 0; b < xr.size(); b++) {
      double s = 0;
      for (int j = xr[b].lo; j <= xr[b].hi; j++) s += column[(size_t)j];
      table[a * xr.size() + b] = s;
    }
  }
  for (int plane = 0; plane < g.planes; plane++) {
    T* o = out + (size_t)plane * (size_t)g.dny * (size_t)g.dnx;
    for (int x = 0; x < g.dnx; x++) {
      const double* row = table.data() + xid[(size_t)x];
      for (int y = 0; y < g.dny; y++) o[(size_t)y + (size_t)x * (size_t)g.dny] += (T)row[(size_t)yid[(size_t)y] * xr.size()];
    }
  }
}
#endif

}  // namespace conv2d
}  // namespace prost
#endif
