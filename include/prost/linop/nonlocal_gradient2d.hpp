// prost/linop/nonlocal_gradient2d.hpp -- the arithmetic of BlockNonlocalGradient2D: the nonlocal gradient of L channels of an ny x nx grid,
//   (K u)_m[p] = w_m(p) (u[p + d_m] - u[p]),   m = 0 .. M-1,
// a fixed set of M displacements d_m = (dy_m, dx_m) inside a search window and one weight per displacement and pixel, without a matrix:
// the operator of nonlocal TV (Gilboa-Osher) and of the nonlocal Huber / TV-L1 regularisers of flow and depth.  The reference has no such
// block; this is written from the definition.
//
// Grid: N = nx ny, pixel (y, x) at p = y + x ny (column-major).  Domain (L N values): u_c[p] at c N + p.  Range (M L N values,
// displacement-major like the gx / gy planes of gradient2d): plane (m, c) at (m L + c) N + p.  Displacements: integers, pairwise distinct,
// not (0, 0), |dy_m|, |dx_m| <= kMaxReach = 15, 1 <= M <= kMaxOffsets = 64; they travel to the kernels by value (Offsets).  Weights: M planes
// of N values shared by all channels, w_m[p] at m N + p, each value rounded to T once, on the host; zeros and negative values are legal.
// Term m is PRESENT at p iff (y + dy_m, x + dx_m) lies in the grid; a row with no target has no entry in the explicit matrix.
//
// Order of operations (the one place it is written down; kernels and host library build without contraction):
//   forward   res[(m L + c) N + p] = present ? w_m[p] * (u_c[q] - u_c[p]) : +0,   q = p + dy_m + dx_m ny:  one subtraction, one product, each
//             rounded once.  K applied to a constant image is exactly zero.
//   adjoint   for pixel p of channel c: s = +0, then for m ascending
//               outgoing   if term m is present at p:                    s = s - w_m[p] * y_{m,c}[p]
//               incoming   if p' = (y - dy_m, x - dx_m) lies in the grid:  s = s + w_m[p'] * y_{m,c}[p']
//             every product rounded on its own, every addition rounded once.
//   The accumulating forms store res + value, added last.  The select sits on the TERM: a masked term is never formed, so a weight at a
//   position whose target is outside the grid reaches no output, whatever it holds.  With offsets ((0, +1), (+1, 0)) and all weights 1
//   the forward product is gradient2d(nx, ny, L) bit for bit, signs of zeros included (1 * d is d).
//
// The explicit matrix: row (m, c, p), where present, holds -w_m[p] at column c N + p and +w_m[p] at column c N + q; p != q always.
//
// Error bound against that matrix in exact arithmetic, componentwise: |got - exact| <= gamma_n B, gamma_n = n u / (1 - n u), u the unit
// roundoff, B from the absolute values of the UNMERGED terms:
//   forward   B = |w_m[p]| (|u[q]| + |u[p]|);  adjoint   B = sum over the present outgoing and incoming terms of |w| |y|.
//   block, forward:   the difference 1, the product 1                                                                   n = 2
//   block, adjoint:   a column of at most 2 M terms: the product 1, then 2 M additions from +0 of which the first is exact   n = 2 M
//   a CSR twin with entries rounded to T (the entries are +-w, no rounding) that adds its products one by one from 0:
//     forward, a row of 2 entries: the product 1, one addition (the first is exact)                                     n = 2
//     adjoint, a column of at most 2 M entries: the product 1, 2 M - 1 additions                                        n = 2 M
//   |block - twin| <= (gamma_block + gamma_twin) B.  Where the data and the weights are dyadic and small every operation is exact.
//
// Who computes what: a workgroup of kThreads lanes owns a tile of kTileY x kTileX pixels and the channels c0 .. c0 + C - 1 of one pass, C
// at most PassChannels(reach, sizeof(T)); more channels are walked in further passes.  A lane owns W consecutive rows (one 16-byte access
// where the height and the pointers allow, else one row) of a column; kTileY / W lanes stand side by side in a column.  Forward: the tile of
// u with a halo of the block's actual reach (max |dy|, max |dx| of the given offsets) is staged once (StageTile; cells outside the grid
// hold 0 and are never selected), then every lane walks m: its W weights are loaded once and serve all C channels.  Adjoint: a gather,
// outgoing terms as one access at p, incoming terms at p - d_m through the Mover's gather; no atomics, nothing depends on the launch order.
// A Mover says how W rows are moved:
//   void load(const T* p, T (&v)[W], int nvalid) const;   void store(T* p, const T (&v)[W], int nvalid) const;
//   void gather(const T* plane, long xq, long row0, int dy, long nx, long ny, T (&v)[W]) const;
//        v[j] = plane[xq ny + row0 - dy + j] where that position lies in the grid, anything elsewhere (it is never selected)
// res must not overlap rhs or the weights.
#ifndef PROST_LINOP_NONLOCAL_GRADIENT2D_HPP_
#define PROST_LINOP_NONLOCAL_GRADIENT2D_HPP_
#include <cmath>
#include <cstddef>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PROST_NLG2_HD __host__ __device__ __forceinline__
#define PROST_NLG2_UNROLL _Pragma("unroll")
#else
#define PROST_NLG2_HD inline
#define PROST_NLG2_UNROLL
#endif

namespace prost {
namespace nonlocal_gradient2d {

constexpr int kMaxOffsets = 64;                 ///< M
constexpr int kMaxReach = 15;                   ///< |dy|, |dx|: the reach of conv2d's 31 x 31 window
constexpr int kTileY = 64, kTileX = 16;         ///< the pixels of a workgroup
constexpr int kThreads = 256;
constexpr int kMaxPassChannels = 4;             ///< channels of one pass (the lane's registers: C W accumulators)
constexpr size_t kLdsLimit = 65536;             ///< the LDS a workgroup may ask for

/// the displacements as the kernels get them: by value, read through scalar loads
struct Offsets {
  signed char dy[kMaxOffsets];
  signed char dx[kMaxOffsets];
};

/// the staged tile of one channel: (tile_x + 2 rx) columns of (tile_y + 2 ry) values, column-major
constexpr size_t TileValues(int tile_y, int tile_x, int ry, int rx) { return (size_t)(tile_y + 2 * ry) * (size_t)(tile_x + 2 * rx); }

/// the tile table: channels staged together by reach = max(ry, rx) (0 .. kMaxReach), row 0 for 4-byte and row 1 for 8-byte values.  The
/// largest count up to kMaxPassChannels whose kTileY x kTileX tiles with a halo of `reach` on every side stay within kLdsLimit.
constexpr int kPassChannels[2][kMaxReach + 1] = {
    {4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 4, 3},
    {4, 4, 4, 4, 4, 4, 3, 3, 3, 2, 2, 2, 2, 2, 2, 1}};
constexpr int PassChannels(int reach, size_t value_bytes) { return kPassChannels[value_bytes > 4 ? 1 : 0][reach < 0 ? 0 : (reach > kMaxReach ? kMaxReach : reach)]; }
constexpr bool TableFits() {
  for (int r = 0; r <= kMaxReach; r++)
    for (int b = 0; b < 2; b++) {
      const size_t one = TileValues(kTileY, kTileX, r, r) * (b ? 8 : 4);
      const int c = kPassChannels[b][r];
      if (c < 1 || c > kMaxPassChannels || c * one > kLdsLimit) return false;
      if (c < kMaxPassChannels && (c + 1) * one <= kLdsLimit) return false;      // and no entry is smaller than it has to be
    }
  return true;
}
static_assert(TableFits(), "the tile table keeps a workgroup within 64 KiB of LDS");

/// max |dy| and max |dx| of the M offsets
inline void Reach(const Offsets& o, int M, int& ry, int& rx) {
  ry = rx = 0;
  for (int m = 0; m < M; m++) {
    const int ay = o.dy[m] < 0 ? -o.dy[m] : o.dy[m], ax = o.dx[m] < 0 ? -o.dx[m] : o.dx[m];
    if (ay > ry) ry = ay;
    if (ax > rx) rx = ax;
  }
}

/// (y + dy, x + dx) lies in the grid
PROST_NLG2_HD bool Inside(long y, long x, int dy, int dx, long ny, long nx) {
  const long ty = y + dy, tx = x + dx;
  return ty >= 0 && ty < ny && tx >= 0 && tx < nx;
}

/// the tile of a workgroup: origin, sizes, halo; `values` of one channel one after the other
struct Tile {
  long y0, x0;          ///< the first pixel of the tile
  int ty, tx;           ///< its sides
  int ry, rx;           ///< the halo
  PROST_NLG2_HD size_t pitch() const { return (size_t)(ty + 2 * ry); }
  PROST_NLG2_HD size_t values() const { return pitch() * (size_t)(tx + 2 * rx); }
  /// the index of grid position (y, x), which lies in the tile or its halo, in the staged values of channel cc of the pass
  PROST_NLG2_HD size_t at(int cc, long y, long x) const { return (size_t)cc * values() + (size_t)(x - x0 + rx) * pitch() + (size_t)(y - y0 + ry); }
};

/// lane `tid` of `threads` stages its share of channels c0 .. c0 + C - 1 of u: cells outside the grid hold 0
template <class T>
PROST_NLG2_HD void StageTile(T* staged, const Tile& t, const T* u, size_t nx, size_t ny, size_t c0, int C, int tid, int threads) {
  const int py = t.ty + 2 * t.ry, px = t.tx + 2 * t.rx;
  const int lanes = threads < 64 ? threads : 64, yl = tid % lanes, xl = tid / lanes, xstep = threads / lanes;      // y across the lanes of a wave
  if (xl >= xstep) return;                                            // threads is no multiple of 64: the rest stages nothing
  for (int cc = 0; cc < C; cc++)
    for (int xx = xl; xx < px; xx += xstep) {
      const long x = t.x0 - t.rx + xx;
      const bool xin = x >= 0 && x < (long)nx;
      for (int yy = yl; yy < py; yy += lanes) {
        const long y = t.y0 - t.ry + yy;
        T v = (T)0;
        if (xin && y >= 0 && y < (long)ny) v = u[(c0 + (size_t)cc) * nx * ny + (size_t)x * ny + (size_t)y];
        staged[(size_t)cc * t.values() + (size_t)xx * (size_t)py + (size_t)yy] = v;
      }
    }
}

template <class T, int W, bool ACC, class Mover>
PROST_NLG2_HD void Put(const Mover& mv, T* p, T (&v)[W], int nvalid) {
  if (ACC) {
    T o[W];
    mv.load(p, o, nvalid);
PROST_NLG2_UNROLL
    for (int j = 0; j < W; j++) v[j] = o[j] + v[j];
  }
  mv.store(p, v, nvalid);
}

/// res (+)= K rhs on rows row0 .. row0 + W - 1 of column x, channels c0 .. c0 + C - 1; u comes from the staged tile.  A lane with
/// row0 >= ny or x >= nx moves nothing.
template <class T, int W, bool ACC, class Mover>
PROST_NLG2_HD void ForwardCell(const Mover& mv, T* res, const T* staged, const Tile& t, const T* weights, const Offsets& o, int M, size_t nx, size_t ny, size_t L,
                               size_t c0, int C, size_t row0, size_t x) {
  if (row0 >= ny || x >= nx) return;
  const size_t N = nx * ny, at = x * ny + row0;
  const int nvalid = ny - row0 < (size_t)W ? (int)(ny - row0) : W;
  T up[kMaxPassChannels][W];
PROST_NLG2_UNROLL
  for (int cc = 0; cc < kMaxPassChannels; cc++)
PROST_NLG2_UNROLL
    for (int j = 0; j < W; j++) up[cc][j] = cc < C ? staged[t.at(cc, (long)row0 + j, (long)x)] : (T)0;
  for (int m = 0; m < M; m++) {
    const int dy = o.dy[m], dx = o.dx[m];
    T w[W];
    mv.load(weights + (size_t)m * N + at, w, nvalid);
PROST_NLG2_UNROLL
    for (int cc = 0; cc < kMaxPassChannels; cc++) {
      if (cc >= C) break;
      T v[W];
PROST_NLG2_UNROLL
      for (int j = 0; j < W; j++) {
        const bool present = j < nvalid && Inside((long)row0 + j, (long)x, dy, dx, (long)ny, (long)nx);
        const T uq = staged[t.at(cc, (long)row0 + j + dy, (long)x + dx)];       // in the halo at worst: always staged
        v[j] = present ? w[j] * (uq - up[cc][j]) : (T)0;
      }
      Put<T, W, ACC>(mv, res + ((size_t)m * L + c0 + (size_t)cc) * N + at, v, nvalid);
    }
  }
}

/// res (+)= K^T rhs on the same rows, column and channels: a gather from memory
template <class T, int W, bool ACC, class Mover>
PROST_NLG2_HD void AdjointCell(const Mover& mv, T* res, const T* rhs, const T* weights, const Offsets& o, int M, size_t nx, size_t ny, size_t L, size_t c0, int C,
                               size_t row0, size_t x) {
  if (row0 >= ny || x >= nx) return;
  const size_t N = nx * ny, at = x * ny + row0;
  const int nvalid = ny - row0 < (size_t)W ? (int)(ny - row0) : W;
  T s[kMaxPassChannels][W];
PROST_NLG2_UNROLL
  for (int cc = 0; cc < kMaxPassChannels; cc++)
PROST_NLG2_UNROLL
    for (int j = 0; j < W; j++) s[cc][j] = (T)0;
  for (int m = 0; m < M; m++) {
    const int dy = o.dy[m], dx = o.dx[m];
    bool out[W], in[W];
    T wo[W], wi[W];
    mv.load(weights + (size_t)m * N + at, wo, nvalid);
    mv.gather(weights + (size_t)m * N, (long)x - dx, (long)row0, dy, (long)nx, (long)ny, wi);
PROST_NLG2_UNROLL
    for (int j = 0; j < W; j++) {
      out[j] = j < nvalid && Inside((long)row0 + j, (long)x, dy, dx, (long)ny, (long)nx);
      in[j] = j < nvalid && Inside((long)row0 + j, (long)x, -dy, -dx, (long)ny, (long)nx);
    }
PROST_NLG2_UNROLL
    for (int cc = 0; cc < kMaxPassChannels; cc++) {
      if (cc >= C) break;
      const T* plane = rhs + ((size_t)m * L + c0 + (size_t)cc) * N;
      T yo[W], yi[W];
      mv.load(plane + at, yo, nvalid);
      mv.gather(plane, (long)x - dx, (long)row0, dy, (long)nx, (long)ny, yi);
PROST_NLG2_UNROLL
      for (int j = 0; j < W; j++) {
        if (out[j]) s[cc][j] = s[cc][j] - wo[j] * yo[j];
        if (in[j]) s[cc][j] = s[cc][j] + wi[j] * yi[j];
      }
    }
  }
PROST_NLG2_UNROLL
  for (int cc = 0; cc < kMaxPassChannels; cc++) {
    if (cc >= C) break;
    Put<T, W, ACC>(mv, res + (c0 + (size_t)cc) * N + at, s[cc], nvalid);
  }
}

/// the cell of lane `tid` at step `step` of a tile: kTileY / W lanes stand in a column, the columns of a step side by side
template <int W>
PROST_NLG2_HD bool CellOf(const Tile& t, int tid, int threads, int step, size_t& row0, size_t& x) {
  const int lanes = t.ty / W, across = threads / lanes;
  const int col = step * across + tid / lanes;
  row0 = (size_t)t.y0 + (size_t)(tid % lanes) * W;
  x = (size_t)t.x0 + (size_t)col;
  return tid / lanes < across && col < t.tx;
}
template <int W>
PROST_NLG2_HD int Steps(const Tile& t, int threads) {
  const int across = threads / (t.ty / W);
  return (t.tx + across - 1) / across;
}

// ---- the sums of |entry|^alpha over the explicit matrix: in double from the T-rounded planes ----
/// |v|^alpha, 0 for an entry of 0 (no entry); exact for alpha = 1
inline double EntryPower(double v, double alpha) { return v == 0 ? 0.0 : (alpha == 1.0 ? std::fabs(v) : std::pow(std::fabs(v), alpha)); }

/// row (m, p) of any channel: the entries -w and +w where the term is present
template <class T>
inline double PixelRowSum(const T* weights, const Offsets& o, int m, size_t nx, size_t ny, size_t p, double alpha) {
  if (!Inside((long)(p % ny), (long)(p / ny), o.dy[m], o.dx[m], (long)ny, (long)nx)) return 0.0;
  return 2.0 * EntryPower((double)weights[(size_t)m * nx * ny + p], alpha);
}
/// column p of any channel: |w_m[p]|^alpha of every outgoing and |w_m[p']|^alpha of every incoming term, m ascending
template <class T>
inline double PixelColSum(const T* weights, const Offsets& o, int M, size_t nx, size_t ny, size_t p, double alpha) {
  const long y = (long)(p % ny), x = (long)(p / ny);
  const size_t N = nx * ny;
  double s = 0.0;
  for (int m = 0; m < M; m++) {
    if (Inside(y, x, o.dy[m], o.dx[m], (long)ny, (long)nx)) s += EntryPower((double)weights[(size_t)m * N + p], alpha);
    if (Inside(y, x, -o.dy[m], -o.dx[m], (long)ny, (long)nx))
      s += EntryPower((double)weights[(size_t)m * N + (size_t)((long)p - o.dy[m] - (long)o.dx[m] * (long)ny)], alpha);
  }
  return s;
}
/// row r of K (0 <= r < M L N)
template <class T>
inline double RowSum(size_t r, const T* weights, const Offsets& o, size_t nx, size_t ny, size_t L, double alpha) {
  const size_t N = nx * ny;
  return PixelRowSum(weights, o, (int)(r / (L * N)), nx, ny, r % N, alpha);
}
/// column q of K (0 <= q < L N)
template <class T>
inline double ColSum(size_t q, const T* weights, const Offsets& o, int M, size_t nx, size_t ny, double alpha) {
  return PixelColSum(weights, o, M, nx, ny, q % (nx * ny), alpha);
}

#if !defined(__HIP_DEVICE_COMPILE__)
/// W rows moved one by one: the host form (tests/host/nonlocal_gradient2d_harness.cpp)
template <class T, int W> struct HostMover {
  void load(const T* p, T (&v)[W], int nvalid) const { for (int j = 0; j < W; j++) v[j] = j < nvalid ? p[j] : (T)0; }
  void store(T* p, const T (&v)[W], int nvalid) const { for (int j = 0; j < W; j++) if (j < nvalid) p[j] = v[j]; }
  void gather(const T* plane, long xq, long row0, int dy, long nx, long ny, T (&v)[W]) const {
    for (int j = 0; j < W; j++) {
      const long row = row0 - dy + j;
      v[j] = xq >= 0 && xq < nx && row >= 0 && row < ny ? plane[(size_t)xq * (size_t)ny + (size_t)row] : (T)0;
    }
  }
};

/// one product on the host, pass by pass, tile by tile and lane by lane as the kernels run it: tiles of tile_y x tile_x pixels (tile_y a
/// multiple of W), `threads` lanes of W rows, `pass` channels staged together (0: the tile table's count for the reach of the offsets)
template <class T, int W, bool ACC>
inline void Apply(T* res, const T* rhs, const T* weights, const Offsets& o, int M, size_t nx, size_t ny, size_t L, bool transpose, int tile_y = kTileY,
                  int tile_x = kTileX, int threads = kThreads, int pass = 0) {
  const HostMover<T, W> mv;
  int ry, rx;
  Reach(o, M, ry, rx);
  if (pass <= 0) pass = PassChannels(ry > rx ? ry : rx, sizeof(T));
  if (pass > kMaxPassChannels) pass = kMaxPassChannels;
  std::vector<T> staged;
  for (size_t c0 = 0; c0 < L; c0 += (size_t)pass) {
    const int C = L - c0 < (size_t)pass ? (int)(L - c0) : pass;
    for (size_t x0 = 0; x0 < nx; x0 += (size_t)tile_x)
      for (size_t y0 = 0; y0 < ny; y0 += (size_t)tile_y) {
        const Tile t = {(long)y0, (long)x0, tile_y, tile_x, ry, rx};
        if (!transpose) {
          staged.assign((size_t)C * t.values(), (T)77);                 // exactly the values of this pass; every one is staged below
          for (int tid = 0; tid < threads; tid++) StageTile<T>(staged.data(), t, rhs, nx, ny, c0, C, tid, threads);
        }
        for (int step = 0; step < Steps<W>(t, threads); step++)
          for (int tid = 0; tid < threads; tid++) {
            size_t row0, x;
            if (!CellOf<W>(t, tid, threads, step, row0, x)) continue;
            if (transpose) AdjointCell<T, W, ACC>(mv, res, rhs, weights, o, M, nx, ny, L, c0, C, row0, x);
            else ForwardCell<T, W, ACC>(mv, res, staged.data(), t, weights, o, M, nx, ny, L, c0, C, row0, x);
          }
      }
  }
}
#endif

}  // namespace nonlocal_gradient2d
}  // namespace prost
#endif
