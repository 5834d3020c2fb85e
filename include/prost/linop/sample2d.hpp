// prost/linop/sample2d.hpp -- the arithmetic of BlockSample2D: bilinear resampling of an image at M arbitrary positions (a warp by a
// flow field, a rotation or zoom, scattered samples) and its exact transpose, without a matrix.  The reference has no such block; this
// is written from the definition.
//
// Domain: L column-major planes of ny x nx, element (yy, xx, c) at yy + xx ny + c nx ny.  Range: L planes of M samples, sample i of
// plane c at i + c M.  Positions x[i], y[i] are pixel coordinates with the pixel centres at the integers, float64 on the host and
// rounded once to T.
//
// Entries of row i (the one place the arithmetic and its order are written down; kernels and host library build without contraction;
// every operation is one rounding in T).  With fx, fy in T:
//
//   j0 = floor(fx), ax = fx - j0, bx = 1 - ax;   i0 = floor(fy), ay = fy - i0, by = 1 - ay
//   slot 0: by bx at (i0, j0)     slot 1: ay bx at (i0 + 1, j0)     slot 2: by ax at (i0, j0 + 1)     slot 3: ay ax at (i0 + 1, j0 + 1)
//
// each product rounded once.  An entry whose pixel lies outside the image is absent (zero padding); an entry whose weight is exactly 0
// is absent (integer positions give the identity exactly; Inf or NaN in the neighbouring pixel does not leak).  A sample with
// !(fx >= -1 && fx < nx && fy >= -1 && fy < ny), tested in T before anything is converted to an integer, has no entries (this covers
// NaN and every huge value).
//
//   forward:  res[i] starts at +0 and adds its present terms in slot order (ascending column index); a term is (w) u, two roundings.
//   adjoint:  res(yy, xx) starts at +0 and adds the entries of column (yy, xx) by cell, then by ascending sample index inside the cell.
//             The cell of a sample is (i0, j0); the cells that reach pixel (yy, xx) are taken in the order (yy-1, xx-1), (yy, xx-1),
//             (yy-1, xx), (yy, xx) -- the pixel is slot 3, 2, 1, 0 of their samples.  The weight is recomputed from the position with
//             the expressions above, so K^T holds the bits of the forward matrix, and no atomics are needed.
//
// The adjoint's tables (MakeBuckets): the samples that have entries, sorted by cell with a stable counting sort over the
// (ny + 1)(nx + 1) cells, i0 = -1 .. ny - 1 and j0 = -1 .. nx - 1, cell (i0, j0) at (i0 + 1) + (j0 + 1)(ny + 1).  `order` holds the
// sorted sample indices (int32; behind them, never read, the samples without entries, so that it is a permutation of 0 .. M - 1);
// `cell_start` holds (ny + 1)(nx + 1) + 1 offsets into it.  Cells (yy-1, xx-1) and (yy, xx-1) are neighbours in that numbering, as are
// (yy-1, xx) and (yy, xx): a pixel walks two contiguous stretches of `order`.  A stretch is a finite count read from the table, so the
// walk needs no step cap; many samples in one cell serialise in one lane -- slow, but correct.
//
// The accumulating forms store res + value; an empty row and an empty column store (add) zero.  res and rhs must not overlap.
#ifndef PROST_LINOP_SAMPLE2D_HPP_
#define PROST_LINOP_SAMPLE2D_HPP_
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PROST_S2D_HD __host__ __device__ __forceinline__
#define PROST_S2D_UNROLL(n) _Pragma(#n)
#else
#define PROST_S2D_HD inline
#define PROST_S2D_UNROLL(n)
#endif
// keeps the compiler from moving a batched load back under the test of whether its value is used
#if defined(__HIP_DEVICE_COMPILE__)
#define PROST_S2D_PIN(v) asm volatile("" : "+v"(v))
#else
#define PROST_S2D_PIN(v) (void)(v)
#endif

namespace prost {
namespace sample2d {

constexpr int kMaxSide = 16384;          ///< nx, ny: every integer up to it, and every cell index, is exact in fp32
constexpr int kSamplesPerWave = 64;      ///< forward: a lane owns a sample
constexpr int kRowsPerWave = 64;         ///< adjoint: the lanes of a wave own 64 consecutive rows of one column
constexpr int kAdjointBatch = 4;         ///< adjoint: samples whose loads are in flight together

/// the operator (the layout of prost_hip_sample2d_geometry in prost_hip.h)
struct Geometry {
  int32_t ny, nx;         ///< image plane
  int32_t m;              ///< samples per plane
  int32_t planes;         ///< L
  int32_t transpose;      ///< 0: res = K rhs, else res = K^T rhs
  int32_t reserved;       ///< 0
};

inline Geometry MakeGeometry(long ny, long nx, long m, long planes, bool transpose) {
  Geometry g;
  g.ny = (int32_t)ny; g.nx = (int32_t)nx; g.m = (int32_t)m; g.planes = (int32_t)planes; g.transpose = transpose ? 1 : 0; g.reserved = 0;
  return g;
}
inline size_t Cells(int ny, int nx) { return (size_t)(ny + 1) * (size_t)(nx + 1); }

/// the four entries of a sample: weight, offset inside a plane (0 where the entry is absent: always a valid address) and presence
template <class T> struct Row {
  T w[4];
  int32_t at[4];
  bool has[4];
  int32_t cell;           ///< (i0 + 1) + (j0 + 1)(ny + 1), or -1 for a sample outside the image's reach
};

template <class T> PROST_S2D_HD bool InReach(T fx, T fy, int ny, int nx) { return fx >= (T)-1 && fx < (T)nx && fy >= (T)-1 && fy < (T)ny; }

template <class T> PROST_S2D_HD Row<T> MakeRow(T fx, T fy, int ny, int nx) {
  Row<T> r;
  const bool in = InReach(fx, fy, ny, nx);
  const T flx = std::floor(fx), fly = std::floor(fy);
  const T ax = fx - flx, bx = (T)1 - ax, ay = fy - fly, by = (T)1 - ay;
  const int j0 = in ? (int)flx : 0, i0 = in ? (int)fly : 0;          // -1 .. nx - 1, -1 .. ny - 1
  r.w[0] = by * bx; r.w[1] = ay * bx; r.w[2] = by * ax; r.w[3] = ay * ax;
  const bool y0 = i0 >= 0, y1 = i0 + 1 < ny, x0 = j0 >= 0, x1 = j0 + 1 < nx;
  r.has[0] = in && y0 && x0 && r.w[0] != (T)0;
  r.has[1] = in && y1 && x0 && r.w[1] != (T)0;
  r.has[2] = in && y0 && x1 && r.w[2] != (T)0;
  r.has[3] = in && y1 && x1 && r.w[3] != (T)0;
  r.at[0] = r.has[0] ? i0 + j0 * ny : 0;                             // a plane holds at most 2^28 elements
  r.at[1] = r.has[1] ? i0 + 1 + j0 * ny : 0;
  r.at[2] = r.has[2] ? i0 + (j0 + 1) * ny : 0;
  r.at[3] = r.has[3] ? i0 + 1 + (j0 + 1) * ny : 0;
  r.cell = in ? (i0 + 1) + (j0 + 1) * (ny + 1) : -1;
  return r;
}

/// one sample of the forward product over one plane: the four loads unconditionally, then selected, then added in slot order
template <class T> PROST_S2D_HD T ForwardSum(const Row<T>& r, const T* plane) {
  T v0 = plane[r.at[0]], v1 = plane[r.at[1]], v2 = plane[r.at[2]], v3 = plane[r.at[3]];
  PROST_S2D_PIN(v0); PROST_S2D_PIN(v1); PROST_S2D_PIN(v2); PROST_S2D_PIN(v3);
  T acc = (T)0;
  if (r.has[0]) acc = acc + r.w[0] * v0;
  if (r.has[1]) acc = acc + r.w[1] * v1;
  if (r.has[2]) acc = acc + r.w[2] * v2;
  if (r.has[3]) acc = acc + r.w[3] * v3;
  return acc;
}

/// the weight at pixel (yy, xx) of a sample whose cell reaches it, recomputed with the forward's expressions; nothing is converted
/// to an integer, so any position is accepted (one that does not reach the pixel gives a weight no entry has; the tables hold none)
template <class T> PROST_S2D_HD T WeightAt(T fx, T fy, int yy, int xx) {
  const T flx = std::floor(fx), fly = std::floor(fy);
  const T ax = fx - flx, bx = (T)1 - ax, ay = fy - fly, by = (T)1 - ay;
  return (fly == (T)yy ? by : ay) * (flx == (T)xx ? bx : ax);
}

/// one pixel of the adjoint product over one plane of samples.  The two stretches are walked as one list, kAdjointBatch samples at a
/// time: the sample indices of a batch first, then all their loads, then the additions in the pinned order -- the loads do not depend
/// on the running sum, so a lane keeps 3 kAdjointBatch of them in flight instead of waiting for two dependent loads per sample.
template <class T>
PROST_S2D_HD T AdjointSum(const T* __restrict__ px, const T* __restrict__ py, const int32_t* __restrict__ order, const int32_t* __restrict__ cell_start,
                          const T* samples, int ny, int yy, int xx) {
  const int32_t* cs = cell_start + (size_t)yy + (size_t)xx * (size_t)(ny + 1);      // cells (yy-1, xx-1), (yy, xx-1); a column on: (yy-1, xx), (yy, xx)
  const int32_t a0 = cs[0], na = cs[2] - a0, b0 = cs[ny + 1], total = na + (cs[ny + 3] - b0);
  T acc = (T)0;
  for (int32_t t0 = 0; t0 < total; t0 += kAdjointBatch) {
    int32_t s[kAdjointBatch];
    T fx[kAdjointBatch], fy[kAdjointBatch], v[kAdjointBatch];
    PROST_S2D_UNROLL(unroll)
    for (int u = 0; u < kAdjointBatch; u++) {
      const int32_t t = t0 + u < total ? t0 + u : total - 1;                          // past the end: the last one again, not added
      s[u] = order[t < na ? a0 + t : b0 + (t - na)];
    }
    PROST_S2D_UNROLL(unroll)
    for (int u = 0; u < kAdjointBatch; u++) { fx[u] = px[s[u]]; fy[u] = py[s[u]]; v[u] = samples[s[u]]; }
    PROST_S2D_UNROLL(unroll)
    for (int u = 0; u < kAdjointBatch; u++) { PROST_S2D_PIN(fx[u]); PROST_S2D_PIN(fy[u]); PROST_S2D_PIN(v[u]); }
    PROST_S2D_UNROLL(unroll)
    for (int u = 0; u < kAdjointBatch; u++) {
      const T w = WeightAt(fx[u], fy[u], yy, xx);
      if (t0 + u < total && w != (T)0) acc = acc + w * v[u];
    }
  }
  return acc;
}

#if !defined(__HIP_DEVICE_COMPILE__)
/// the bucket tables of the adjoint (see the head of this file); px, py already rounded to T
template <class T> inline void MakeBuckets(const T* px, const T* py, size_t m, int ny, int nx, std::vector<int32_t>& order, std::vector<int32_t>& cell_start) {
  const size_t cells = Cells(ny, nx);
  cell_start.assign(cells + 1, 0);
  std::vector<int32_t> cell(m);
  for (size_t i = 0; i < m; i++) {
    const Row<T> r = MakeRow(px[i], py[i], ny, nx);
    cell[i] = (r.has[0] || r.has[1] || r.has[2] || r.has[3]) ? r.cell : -1;
    if (cell[i] >= 0) cell_start[(size_t)cell[i] + 1]++;
  }
  for (size_t c = 0; c < cells; c++) cell_start[c + 1] += cell_start[c];
  order.assign(m, 0);
  std::vector<int32_t> next(cell_start.begin(), cell_start.end() - 1);
  size_t rest = (size_t)cell_start[cells];
  for (size_t i = 0; i < m; i++) {
    if (cell[i] >= 0) order[(size_t)next[(size_t)cell[i]]++] = (int32_t)i;
    else order[rest++] = (int32_t)i;
  }
}

/// visit(slot, yy, xx, value) for every entry of row i of the matrix, in the forward's order
template <class T, class F> inline void ForEachInRow(const T* px, const T* py, const Geometry& g, size_t i, F visit) {
  const Row<T> r = MakeRow(px[i], py[i], g.ny, g.nx);
  for (int k = 0; k < 4; k++)
    if (r.has[k]) visit(k, r.at[k] % g.ny, r.at[k] / g.ny, r.w[k]);
}
/// visit(i, value) for every entry of column (yy, xx) of the matrix, in the adjoint's order: the gather enumeration
template <class T, class F>
inline void ForEachAtPixel(const T* px, const T* py, const int32_t* order, const int32_t* cell_start, const Geometry& g, int yy, int xx, F visit) {
  for (int half = 0; half < 2; half++) {
    const int32_t* cs = cell_start + (size_t)yy + (size_t)(xx + half) * (size_t)(g.ny + 1);
    for (int32_t k = cs[0]; k < cs[2]; k++) {
      const int32_t s = order[k];
      const T w = WeightAt(px[s], py[s], yy, xx);
      if (w != (T)0) visit((size_t)s, w);
    }
  }
}

inline double PowAbs(double v, double alpha) { return alpha == 1 ? std::fabs(v) : (alpha == 2 ? v * v : (v == 0 ? 0.0 : std::pow(std::fabs(v), alpha))); }

/// sum |A|^alpha over row i; a sample without entries gives exactly 0
template <class T> inline double RowSum(const T* px, const T* py, const Geometry& g, double alpha, size_t i) {
  double s = 0;
  ForEachInRow<T>(px, py, g, i, [&](int, int, int, T v) { s += PowAbs((double)v, alpha); });
  return s;
}
/// sum |A|^alpha over column (yy, xx); a pixel no sample reaches gives exactly 0
template <class T> inline double ColSum(const T* px, const T* py, const int32_t* order, const int32_t* cell_start, const Geometry& g, double alpha, int yy, int xx) {
  double s = 0;
  ForEachAtPixel<T>(px, py, order, cell_start, g, yy, xx, [&](size_t, T v) { s += PowAbs((double)v, alpha); });
  return s;
}

/// the products on the host, lane by lane as the kernels run them (tests/host/sample2d_harness.cpp)
template <class T, bool ACC>
inline void Apply(T* res, const T* rhs, const Geometry& g, const T* px, const T* py, const int32_t* order, const int32_t* cell_start, bool transpose) {
  const size_t plane = (size_t)g.ny * (size_t)g.nx, m = (size_t)g.m;
  if (!transpose) {
    for (size_t i = 0; i < m; i++) {
      const Row<T> r = MakeRow(px[i], py[i], g.ny, g.nx);
      for (int c = 0; c < g.planes; c++) {
        T* o = res + (size_t)c * m + i;
        const T v = ForwardSum<T>(r, rhs + (size_t)c * plane);
        *o = ACC ? *o + v : v;
      }
    }
  } else {
    for (int c = 0; c < g.planes; c++)
      for (int xx = 0; xx < g.nx; xx++)
        for (int yy = 0; yy < g.ny; yy++) {
          T* o = res + (size_t)c * plane + (size_t)yy + (size_t)xx * (size_t)g.ny;
          const T v = AdjointSum<T>(px, py, order, cell_start, rhs + (size_t)c * m, g.ny, yy, xx);
          *o = ACC ? *o + v : v;
        }
  }
}
#endif

}  // namespace sample2d
}  // namespace prost
#endif
