// prost/linop/sym_gradient2d.hpp -- the arithmetic of BlockSymGradient2D: the symmetrised gradient E of a vector field on L channels of
// an ny x nx grid, the second-order operator of total generalised variation (TGV^2: K = [grad -I ; 0 E]), without a matrix.  The
// reference has no such block; this is written from the definition.
//
// Grid: N = nx ny, pixel (y, x) at p = y + x ny (column-major).  Domain (2 L N values, the range layout of gradient2d(nx, ny, L)):
// vx_c[p] at c N + p, vy_c[p] at (L + c) N + p.  Range (3 L N values): exx_c[p] at c N + p, eyy_c[p] at (L + c) N + p, exy_c[p] at
// (2 L + c) N + p.  With Dx, Dy the forward differences of gradient2d (zero in the last column / row), Bx = -Dx^T, By = -Dy^T:
//
//   E = [ kron(I, Bx)  0 ; 0  kron(I, By) ; w kron(I, By)  w kron(I, Bx) ]
//
// i.e. backward differences with the boundary handling of the divergence.  Masks: ax = [x < nx-1], bx = [x > 0], ay = [y < ny-1],
// by = [y > 0].  Order of operations (the one place it is written down; kernels and host library build without contraction): a sum
// starts from +0 and its present terms are added left to right, in ascending column index of the explicit matrix; a masked term is
// absent (selected away, never multiplied by zero); every product w a is one rounding in T, every addition one more; the
// accumulating forms store res + value.
//
//   forward   exx[p] = (bx) -vx[p-ny], (ax) +vx[p]
//             eyy[p] = (by) -vy[p-1],  (ay) +vy[p]
//             exy[p] = (by) -(w vx[p-1]), (ay) +(w vx[p]), (bx) -(w vy[p-ny]), (ax) +(w vy[p])
//   adjoint   vx[p]  = (ax) +exx[p], (ax) -exx[p+ny], (ay) +(w exy[p]), (ay) -(w exy[p+1])
//             vy[p]  = (ay) +eyy[p], (ay) -eyy[p+1],  (ax) +(w exy[p]), (ax) -(w exy[p+ny])
//
// A march walks the columns x0 .. x1 - 1 of one channel for W consecutive rows row0 .. row0 + W - 1: the column neighbour (x - 1
// forward, x + 1 adjoint) is the group loaded for the neighbouring step and kept, the row neighbour (y - 1 forward, y + 1 adjoint) is
// one scalar the Mover supplies (on the device the adjacent lane's edge element).  A Mover says how W rows are moved:
//   void load(const T* p, T (&v)[W], int nvalid) const;   void store(T* p, const T (&v)[W], int nvalid) const;
//   T above(const T (&v)[W], const T* column, size_t row0, bool active) const;             // column[row0 - 1], anything if row0 == 0
//   T below(const T (&v)[W], const T* column, size_t row0, size_t ny, bool active) const;  // column[row0 + W], anything if past ny
// res and rhs must not overlap.
#ifndef PROST_LINOP_SYM_GRADIENT2D_HPP_
#define PROST_LINOP_SYM_GRADIENT2D_HPP_
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PROST_SG2_HD __host__ __device__ __forceinline__
#define PROST_SG2_UNROLL _Pragma("unroll")
#else
#define PROST_SG2_HD inline
#define PROST_SG2_UNROLL
#endif

namespace prost {
namespace sym_gradient2d {

constexpr int kTerms = 4;                 ///< the longest sum (the t of the error bound (t + 1) u)
constexpr int kColumnChoices[3] = {12, 6, 3};   ///< columns of a chunk, the largest that still leaves kFillBlocks workgroups; else 1
constexpr size_t kFillBlocks = 2048;

/// the weight: formed in double, rounded to T once
template <class T> PROST_SG2_HD T RoundWeight(double w) { return (T)w; }

/// columns per chunk for a grid of `strips` row strips and L channels (the rule of the gradient2d vector kernels)
inline int PickColumns(size_t nx, size_t strips, size_t L) {
  for (int c : kColumnChoices)
    if (strips * ((nx + (size_t)c - 1) / (size_t)c) * L >= kFillBlocks) return c;
  return 1;
}

// ---- the terms ----
/// (m0) -a, (m1) +b: exx from (vx[p-ny], vx[p]) with (bx, ax), eyy from (vy[p-1], vy[p]) with (by, ay)
template <class T> PROST_SG2_HD T Difference(bool m0, T a, bool m1, T b) {
  T s = (T)0;
  if (m0) s = s - a;
  if (m1) s = s + b;
  return s;
}
/// exy[p]
template <class T> PROST_SG2_HD T ForwardXY(T w, bool by, T vx_n, bool ay, T vx_c, bool bx, T vy_w, bool ax, T vy_c) {
  T s = (T)0;
  if (by) s = s - w * vx_n;
  if (ay) s = s + w * vx_c;
  if (bx) s = s - w * vy_w;
  if (ax) s = s + w * vy_c;
  return s;
}
/// vx[p] from (exx[p], exx[p+ny], exy[p], exy[p+1]) with (ax, ay); vy[p] from (eyy[p], eyy[p+1], exy[p], exy[p+ny]) with (ay, ax)
template <class T> PROST_SG2_HD T Adjoint(T w, bool m, T d_c, T d_n, bool mw, T xy_c, T xy_n) {
  T s = (T)0;
  if (m) { s = s + d_c; s = s - d_n; }
  if (mw) { s = s + w * xy_c; s = s - w * xy_n; }
  return s;
}

// ---- the marches ----
template <class T, int W, bool ACC, class Mover>
PROST_SG2_HD void Put(const Mover& m, T* p, T (&v)[W], int nvalid) {
  if (ACC) {
    T o[W];
    m.load(p, o, nvalid);
PROST_SG2_UNROLL
    for (int j = 0; j < W; j++) v[j] = o[j] + v[j];
  }
  m.store(p, v, nvalid);
}

/// res (+)= E rhs on rows row0 .. row0 + W - 1, columns x0 .. x1 - 1 of channel c.  Every lane of a wave walks the same columns (the
/// Mover may exchange values between lanes); a lane with row0 >= ny moves nothing.
template <class T, int W, bool ACC, class Mover>
PROST_SG2_HD void ForwardMarch(const Mover& m, T* res, const T* rhs, size_t nx, size_t ny, size_t L, size_t c, size_t row0, size_t x0, size_t x1, T w) {
  const size_t N = nx * ny;
  const bool active = row0 < ny;
  const int nvalid = active ? (ny - row0 < (size_t)W ? (int)(ny - row0) : W) : 0;
  const T* vx = rhs + c * N;
  const T* vy = rhs + (L + c) * N;
  T vx_w[W], vy_w[W], vx_c[W], vy_c[W];
PROST_SG2_UNROLL
  for (int j = 0; j < W; j++) { vx_w[j] = (T)0; vy_w[j] = (T)0; }
  if (active && x0 > 0) { m.load(vx + (x0 - 1) * ny + row0, vx_w, nvalid); m.load(vy + (x0 - 1) * ny + row0, vy_w, nvalid); }
  for (size_t x = x0; x < x1; x++) {
    const size_t at = x * ny + row0;
PROST_SG2_UNROLL
    for (int j = 0; j < W; j++) { vx_c[j] = (T)0; vy_c[j] = (T)0; }
    if (active) { m.load(vx + at, vx_c, nvalid); m.load(vy + at, vy_c, nvalid); }
    const T vx_above = m.above(vx_c, vx + x * ny, row0, active), vy_above = m.above(vy_c, vy + x * ny, row0, active);
    const bool bx = x > 0, ax = x + 1 < nx;
    T exx[W], eyy[W], exy[W];
PROST_SG2_UNROLL
    for (int j = 0; j < W; j++) {
      const bool by = row0 + j > 0, ay = row0 + j + 1 < ny;
      const T vx_n = j > 0 ? vx_c[j > 0 ? j - 1 : 0] : vx_above, vy_n = j > 0 ? vy_c[j > 0 ? j - 1 : 0] : vy_above;
      exx[j] = Difference<T>(bx, vx_w[j], ax, vx_c[j]);
      eyy[j] = Difference<T>(by, vy_n, ay, vy_c[j]);
      exy[j] = ForwardXY<T>(w, by, vx_n, ay, vx_c[j], bx, vy_w[j], ax, vy_c[j]);
    }
    if (active) {
      Put<T, W, ACC>(m, res + c * N + at, exx, nvalid);
      Put<T, W, ACC>(m, res + (L + c) * N + at, eyy, nvalid);
      Put<T, W, ACC>(m, res + (2 * L + c) * N + at, exy, nvalid);
    }
PROST_SG2_UNROLL
    for (int j = 0; j < W; j++) { vx_w[j] = vx_c[j]; vy_w[j] = vy_c[j]; }
  }
}

/// res (+)= E^T rhs, the same walk: exx and exy of column x + 1 are the groups loaded for the next step
template <class T, int W, bool ACC, class Mover>
PROST_SG2_HD void AdjointMarch(const Mover& m, T* res, const T* rhs, size_t nx, size_t ny, size_t L, size_t c, size_t row0, size_t x0, size_t x1, T w) {
  const size_t N = nx * ny;
  const bool active = row0 < ny;
  const int nvalid = active ? (ny - row0 < (size_t)W ? (int)(ny - row0) : W) : 0;
  const T* exx = rhs + c * N;
  const T* eyy = rhs + (L + c) * N;
  const T* exy = rhs + (2 * L + c) * N;
  T xx_c[W], xy_c[W], xx_e[W], xy_e[W], yy_c[W];
PROST_SG2_UNROLL
  for (int j = 0; j < W; j++) { xx_c[j] = (T)0; xy_c[j] = (T)0; }
  if (active && x0 < x1) { m.load(exx + x0 * ny + row0, xx_c, nvalid); m.load(exy + x0 * ny + row0, xy_c, nvalid); }
  for (size_t x = x0; x < x1; x++) {
    const size_t at = x * ny + row0;
    const bool ax = x + 1 < nx;
PROST_SG2_UNROLL
    for (int j = 0; j < W; j++) { xx_e[j] = (T)0; xy_e[j] = (T)0; yy_c[j] = (T)0; }
    if (active) {
      m.load(eyy + at, yy_c, nvalid);
      if (ax) { m.load(exx + at + ny, xx_e, nvalid); m.load(exy + at + ny, xy_e, nvalid); }
    }
    const T yy_below = m.below(yy_c, eyy + x * ny, row0, ny, active), xy_below = m.below(xy_c, exy + x * ny, row0, ny, active);
    T vx[W], vy[W];
PROST_SG2_UNROLL
    for (int j = 0; j < W; j++) {
      const bool ay = row0 + j + 1 < ny;
      const T yy_s = j + 1 < W ? yy_c[j + 1 < W ? j + 1 : 0] : yy_below, xy_s = j + 1 < W ? xy_c[j + 1 < W ? j + 1 : 0] : xy_below;
      vx[j] = Adjoint<T>(w, ax, xx_c[j], xx_e[j], ay, xy_c[j], xy_s);
      vy[j] = Adjoint<T>(w, ay, yy_c[j], yy_s, ax, xy_c[j], xy_e[j]);
    }
    if (active) {
      Put<T, W, ACC>(m, res + c * N + at, vx, nvalid);
      Put<T, W, ACC>(m, res + (L + c) * N + at, vy, nvalid);
    }
PROST_SG2_UNROLL
    for (int j = 0; j < W; j++) { xx_c[j] = xx_e[j]; xy_c[j] = xy_e[j]; }
  }
}

// ---- the sums of |entry|^alpha: closed forms ----
/// |w|^alpha in double, w already rounded to T; exact for alpha = 1
inline double WeightPower(double w, double alpha) { return alpha == 1.0 ? std::fabs(w) : std::pow(std::fabs(w), alpha); }

/// row r of E (0 <= r < 3 L N); wa = WeightPower(w, alpha)
inline double RowSum(size_t r, size_t nx, size_t ny, size_t L, double wa) {
  const size_t N = nx * ny, plane = r / N, p = r % N, y = p % ny, x = p / ny;
  const double ax = x + 1 < nx, bx = x > 0, ay = y + 1 < ny, by = y > 0;
  if (plane < L) return ax + bx;
  if (plane < 2 * L) return ay + by;
  return wa * (ax + bx + ay + by);
}
/// column q of E (0 <= q < 2 L N)
inline double ColSum(size_t q, size_t nx, size_t ny, size_t L, double wa) {
  const size_t N = nx * ny, plane = q / N, p = q % N, y = p % ny, x = p / ny;
  const double ax = x + 1 < nx, ay = y + 1 < ny;
  return plane < L ? 2 * ax + 2 * wa * ay : 2 * ay + 2 * wa * ax;
}

/// out[r] += RowSum(r) for every row, plane by plane and column by column (no division per element)
template <class T> inline void RowSums(T* out, size_t nx, size_t ny, size_t L, double wa) {
  for (size_t plane = 0; plane < 3 * L; plane++)
    for (size_t x = 0; x < nx; x++) {
      T* o = out + (plane * nx + x) * ny;
      const double sx = (x + 1 < nx) + (x > 0);
      for (size_t y = 0; y < ny; y++) {
        const double sy = (y + 1 < ny) + (y > 0);
        o[y] += (T)(plane < L ? sx : (plane < 2 * L ? sy : wa * (sx + sy)));
      }
    }
}
/// out[q] += ColSum(q) for every column
template <class T> inline void ColSums(T* out, size_t nx, size_t ny, size_t L, double wa) {
  for (size_t plane = 0; plane < 2 * L; plane++)
    for (size_t x = 0; x < nx; x++) {
      T* o = out + (plane * nx + x) * ny;
      const double ax = x + 1 < nx;
      for (size_t y = 0; y < ny; y++) {
        const double ay = y + 1 < ny;
        o[y] += (T)(plane < L ? 2 * ax + 2 * wa * ay : 2 * ay + 2 * wa * ax);
      }
    }
}

#if !defined(__HIP_DEVICE_COMPILE__)
/// W rows moved one by one, neighbours read from the column: the host form (tests/host/sym_gradient2d_harness.cpp)
template <class T, int W> struct HostMover {
  void load(const T* p, T (&v)[W], int nvalid) const { for (int j = 0; j < W; j++) v[j] = j < nvalid ? p[j] : (T)0; }
  void store(T* p, const T (&v)[W], int nvalid) const { for (int j = 0; j < W; j++) if (j < nvalid) p[j] = v[j]; }
  T above(const T (&)[W], const T* column, size_t row0, bool active) const { return active && row0 > 0 ? column[row0 - 1] : (T)0; }
  T below(const T (&)[W], const T* column, size_t row0, size_t ny, bool active) const { return active && row0 + W < ny ? column[row0 + W] : (T)0; }
};

/// one product on the host, strip by strip and chunk by chunk as the kernels run it: lanes of W rows, strips of `lanes` lanes,
/// chunks of PickColumns columns (force_cols > 0: of that many)
template <class T, int W, bool ACC> inline void Apply(T* res, const T* rhs, size_t nx, size_t ny, size_t L, double w, bool transpose, int lanes = 256, int force_cols = 0) {
  const HostMover<T, W> m;
  const T wt = RoundWeight<T>(w);
  const size_t strip_rows = (size_t)lanes * W, strips = (ny + strip_rows - 1) / strip_rows;
  const size_t cols = force_cols > 0 ? (size_t)force_cols : (size_t)PickColumns(nx, strips, L);
  for (size_t c = 0; c < L; c++)
    for (size_t x0 = 0; x0 < nx; x0 += cols)
      for (size_t row0 = 0; row0 < ny; row0 += W) {              // the lanes past the last row move nothing
        const size_t x1 = x0 + cols < nx ? x0 + cols : nx;
        if (transpose) AdjointMarch<T, W, ACC>(m, res, rhs, nx, ny, L, c, row0, x0, x1, wt);
        else ForwardMarch<T, W, ACC>(m, res, rhs, nx, ny, L, c, row0, x0, x1, wt);
      }
}
#endif

}  // namespace sym_gradient2d
}  // namespace prost
#endif
