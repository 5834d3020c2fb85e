// prost/linop/hessian2d.hpp -- the arithmetic of BlockHessian2D: the second-order differences (u_xx, u_yy, u_xy) of L channels of an
// ny x nx grid, the operator of second-order total variation (TV^2, bounded Hessian), of the TV + TV^2 infimal convolution and of the
// Hessian-Schatten-norm regularisers, without a matrix and without an intermediate field.  The reference has no such block; this is
// written from the definition.
//
// Operator: H = E grad exactly, grad = gradient2d(nx, ny, L) and E = sym_gradient2d(nx, ny, L, w); w is formed in double and rounded
// to T once.  Grid: N = nx ny, pixel (y, x) at p = y + x ny (column-major).  Domain (L N values): u_c[p] at c N + p.  Range,
// components = 3 (3 L N values, the range layout of sym_gradient2d): hxx_c[p] at c N + p, hyy_c[p] at (L + c) N + p, hxy_c[p] at
// (2 L + c) N + p; w = sqrt(1/2) makes the 2-norm of the three the Frobenius norm of the Hessian.  components = 4 (4 L N values): the
// planes (hxx, hxy, hxy, hyy) at (k L + c) N + p, the column-major symmetric 2 x 2 matrix; w = 0.5 gives the true Hessian.  The
// default of w is sqrt(1/2) for both.
//
// Masks: ax = [x < nx-1], bx = [x > 0], ay = [y < ny-1], by = [y > 0].  Order of operations: that of the two blocks chained (kernels and
// host library build without contraction), so that the result has the bits of the chain, signed zeros included.
//
//   inner     gx[p] = (ax) u[p+ny] - u[p], else +0;   gy[p] = (ay) u[p+1] - u[p], else +0        one rounding each: what gradient2d stores
//   forward   hxx[p] = (bx) -gx[p-ny], (ax) +gx[p]                                               the sums of sym_gradient2d.hpp: from +0,
//             hyy[p] = (by) -gy[p-1],  (ay) +gy[p]                                               present terms left to right, a masked
//             hxy[p] = (by) -(w gx[p-1]), (ay) +(w gx[p]), (bx) -(w gy[p-ny]), (ax) +(w gy[p])   term absent, every product rounded
//   adjoint   vx[p]  = (ax) +exx[p], (ax) -exx[p+ny], (ay) +(w exy[p]), (ay) -(w exy[p+1])       E^T e, the adjoint of sym_gradient2d
//             vy[p]  = (ay) +eyy[p], (ay) -eyy[p+1],  (ax) +(w exy[p]), (ax) -(w exy[p+ny])
//             divx   = (ax) vx[p], else +0;  (bx) divx = divx - vx[p-ny]                         grad^T as prost_hip_grad2d_adj forms it
//             divy   = (ay) vy[p], else +0;  (by) divy = divy - vy[p-1]                          (grad_adj_kernel, kernels_linop.hip):
//             res[p] = 0 - (divx + divy)            accumulating: res[p] - (divx + divy)         minus the divergence
//   components = 4: forward stores hxy twice; the adjoint forms m = e_xy + e_yx (planes 1 and 2, one rounding) and uses it as exy.
//   The accumulating forward form stores res + value.
//
// Present +0 terms.  A masked inner difference is a value (+0), and the outer sum that reads it keeps the term: hxy in the last
// column adds w gx = w (+0) where ay or by hold, and in the last row w gy.  A sum that starts from +0 never becomes -0 (x + y is -0
// only if both are), so in the forward product these terms change no bit; they are formed all the same, as the chain forms them.  In
// the adjoint the zeros decide bits: res = 0 - s, not -s (s = +0 gives +0); the accumulating form is res - s, not res + (0 - s)
// (res = -0, s = +0 gives -0); and divx, divy start from a present +0 where ax, ay mask the first term, so that in the last column
// divx = +0 - vx[p-ny] is +0 for vx[p-ny] = +0 where a negation would hand -0 to the accumulating form.  vx in the last column and vy
// in the last row are not zero (E^T e has entries there); they are selected away, never multiplied by zero.
//
// The explicit matrix (E kron(I, D), merged entries; 13 per interior pixel and channel) and its sums.  Every block is symmetric:
//   hxx row p: u[p-ny]: bx, u[p]: -(ax + bx), u[p+ny]: ax                      interior (1, -2, 1); nx = 1: empty
//   hyy row p: u[p-1]: by,  u[p]: -(ay + by), u[p+1]: ay
//   hxy row p: w times  u[p-1]: by ax, u[p-1+ny]: -by ax, u[p-ny]: bx ay, u[p-ny+1]: -bx ay, u[p]: -2 ax ay, u[p+1]: ax ay, u[p+ny]: ax ay
// No two terms of a merged entry have opposite signs, so |H| = |E| |kron(I, D)|.  Sums of |entry|^alpha, with sx = ax + bx,
// sy = ay + by, c(s) = s^alpha for s > 0 and 0 for s = 0, wa = |w|^alpha (w rounded to T):
//   Sxx = sx + c(sx),  Syy = sy + c(sy),  Sxy = wa (2 by ax + 2 bx ay + (2 + 2^alpha) ax ay)
// row sums: Sxx, Syy, Sxy by plane; column sums (the blocks are symmetric): Sxx + Syy + Sxy, with components = 4 Sxx + Syy + 2 Sxy.
//
// Error bound against the exact product with the matrix above, u the unit roundoff of T, componentwise.  Forward: a path from u to
// an output crosses the inner difference (1 rounding), the product with w (1) and at most kTerms = 4 additions, the first onto +0
// included: |got - H x| <= 1.01 kRoundingsForward u (|H| |x|), kRoundingsForward = 6.  Adjoint: the sum of E^T e (product and 4
// additions, 5), divx or divy (1) and divx + divy (1); 0 - s is exact: kRoundingsAdjoint = 7, and one more for components = 4, where
// m = e_xy + e_yx is rounded first.  1.01 covers the terms of higher order.  The accumulating forms add one rounding of the stored sum.
//
// A march walks the columns x0 .. x1 - 1 of one channel for W consecutive rows row0 .. row0 + W - 1, with the Mover of
// sym_gradient2d.hpp (load / store of W rows, the element above and below from the adjacent lane or from the column).  Forward keeps
// the u columns x and x + 1 (with their elements above and below) and gx, gy of column x - 1: one column of u is loaded per step and
// three (four) are stored.  The adjoint keeps exx and the mixed column of x and x + 1, carries vx of column x - 1 and forms vy of the
// row above the lane from the elements above, in the same call of the same function: one pass, three (four) loads and one store per
// step.  res and rhs must not overlap.
#ifndef PROST_LINOP_HESSIAN2D_HPP_
#define PROST_LINOP_HESSIAN2D_HPP_
#include <cmath>
#include <cstddef>

#include "prost/linop/sym_gradient2d.hpp"

namespace prost {
namespace hessian2d {

namespace sg2 = sym_gradient2d;

constexpr int kRoundingsForward = 6;      ///< the bound 1.01 k u (|H| |x|): inner difference, product, four additions
constexpr int kRoundingsAdjoint = 7;      ///< product and four additions, divx or divy, divx + divy; one more with components = 4
using sg2::PickColumns;                   ///< the chunk rule of the gradient2d vector kernels
using sg2::RoundWeight;
using sg2::WeightPower;

/// the planes of the range: hxx, hyy, the mixed plane and (components = 4) its second copy, in units of L N
constexpr size_t PlaneXX(bool) { return 0; }
constexpr size_t PlaneYY(bool c4) { return c4 ? 3 : 1; }
constexpr size_t PlaneXY(bool c4) { return c4 ? 1 : 2; }
constexpr size_t PlaneYX(bool) { return 2; }

// ---- the terms ----
/// what gradient2d stores: (m) b - a, else +0
template <class T> PROST_SG2_HD T Inner(bool m, T b, T a) { return m ? b - a : (T)0; }
/// grad^T at one pixel: divx + divy of prost_hip_grad2d_adj
template <class T> PROST_SG2_HD T Divergence(bool ax, T vx_c, bool bx, T vx_w, bool ay, T vy_c, bool by, T vy_n) {
  T divx = ax ? vx_c : (T)0, divy = ay ? vy_c : (T)0;
  if (bx) divx = divx - vx_w;
  if (by) divy = divy - vy_n;
  return divx + divy;
}

// ---- the marches ----
template <class T, int W> PROST_SG2_HD void Zero(T (&v)[W]) {
PROST_SG2_UNROLL
  for (int j = 0; j < W; j++) v[j] = (T)0;
}
template <class T, int W> PROST_SG2_HD void Copy(T (&to)[W], const T (&from)[W]) {
PROST_SG2_UNROLL
  for (int j = 0; j < W; j++) to[j] = from[j];
}
/// p (+)= v; v is kept (the mixed plane is stored twice), unlike sym_gradient2d::Put, which a Mover of that namespace would also find
template <class T, int W, bool ACC, class Mover>
PROST_SG2_HD void Store(const Mover& m, T* p, const T (&v)[W], int nvalid) {
  T s[W];
  Copy<T, W>(s, v);
  if (ACC) {
    T o[W];
    m.load(p, o, nvalid);
PROST_SG2_UNROLL
    for (int j = 0; j < W; j++) s[j] = o[j] + v[j];
  }
  m.store(p, s, nvalid);
}
/// W rows of column `column` (zeros unless on) with the elements above and below them
template <class T, int W, class Mover>
PROST_SG2_HD void LoadColumn(const Mover& m, const T* column, size_t row0, size_t ny, bool on, int nvalid, T (&v)[W], T& above, T& below) {
  Zero<T, W>(v);
  if (on) m.load(column + row0, v, nvalid);
  above = m.above(v, column, row0, on);
  below = m.below(v, column, row0, ny, on);
}
/// the mixed column of the adjoint: exy, or exy + eyx rounded once (components = 4)
template <class T, int W, bool C4, class Mover>
PROST_SG2_HD void LoadMixed(const Mover& m, const T* exy, const T* eyx, size_t row0, size_t ny, bool on, int nvalid, T (&v)[W], T& above, T& below) {
  LoadColumn<T, W>(m, exy, row0, ny, on, nvalid, v, above, below);
  if (C4) {
    T v2[W], above2, below2;
    LoadColumn<T, W>(m, eyx, row0, ny, on, nvalid, v2, above2, below2);
PROST_SG2_UNROLL
    for (int j = 0; j < W; j++) v[j] = v[j] + v2[j];
    above = above + above2;
    below = below + below2;
  }
}

/// res (+)= H rhs on rows row0 .. row0 + W - 1, columns x0 .. x1 - 1 (x0 < x1 <= nx) of channel c.  Every lane of a wave walks the
/// same columns (the Mover may exchange values between lanes); a lane with row0 >= ny moves nothing.
template <class T, int W, bool C4, bool ACC, class Mover>
PROST_SG2_HD void ForwardMarch(const Mover& m, T* res, const T* rhs, size_t nx, size_t ny, size_t L, size_t c, size_t row0, size_t x0, size_t x1, T w) {
  const size_t N = nx * ny;
  const bool active = row0 < ny;
  const int nvalid = active ? (ny - row0 < (size_t)W ? (int)(ny - row0) : W) : 0;
  const T* u = rhs + c * N;
  T gx_w[W], gy_w[W], u_c[W], u_e[W], c_above, c_below, e_above, e_below;
  Zero<T, W>(gx_w);
  Zero<T, W>(gy_w);
  LoadColumn<T, W>(m, u + x0 * ny, row0, ny, active, nvalid, u_c, c_above, c_below);
  if (x0 > 0) {                                       // gx, gy of column x0 - 1, where ax holds
    T u_w[W], w_above, w_below;
    LoadColumn<T, W>(m, u + (x0 - 1) * ny, row0, ny, active, nvalid, u_w, w_above, w_below);
PROST_SG2_UNROLL
    for (int j = 0; j < W; j++) {
      gx_w[j] = Inner<T>(true, u_c[j], u_w[j]);
      gy_w[j] = Inner<T>(row0 + j + 1 < ny, j + 1 < W ? u_w[j + 1 < W ? j + 1 : 0] : w_below, u_w[j]);
    }
  }
  for (size_t x = x0; x < x1; x++) {
    const size_t at = x * ny + row0;
    const bool bx = x > 0, ax = x + 1 < nx;
    LoadColumn<T, W>(m, u + (x + 1) * ny, row0, ny, active && ax, nvalid, u_e, e_above, e_below);
    T gx_c[W], gy_c[W];
    const T gx_n = Inner<T>(ax, e_above, c_above), gy_n = Inner<T>(true, u_c[0], c_above);        // row row0 - 1, read where by holds
PROST_SG2_UNROLL
    for (int j = 0; j < W; j++) {
      gx_c[j] = Inner<T>(ax, u_e[j], u_c[j]);
      gy_c[j] = Inner<T>(row0 + j + 1 < ny, j + 1 < W ? u_c[j + 1 < W ? j + 1 : 0] : c_below, u_c[j]);
    }
    T hxx[W], hyy[W], hxy[W];
PROST_SG2_UNROLL
    for (int j = 0; j < W; j++) {
      const bool by = row0 + j > 0, ay = row0 + j + 1 < ny;
      const T gx_s = j > 0 ? gx_c[j > 0 ? j - 1 : 0] : gx_n, gy_s = j > 0 ? gy_c[j > 0 ? j - 1 : 0] : gy_n;
      hxx[j] = sg2::Difference<T>(bx, gx_w[j], ax, gx_c[j]);
      hyy[j] = sg2::Difference<T>(by, gy_s, ay, gy_c[j]);
      hxy[j] = sg2::ForwardXY<T>(w, by, gx_s, ay, gx_c[j], bx, gy_w[j], ax, gy_c[j]);
    }
    if (active) {
      Store<T, W, ACC>(m, res + (PlaneXX(C4) * L + c) * N + at, hxx, nvalid);
      Store<T, W, ACC>(m, res + (PlaneXY(C4) * L + c) * N + at, hxy, nvalid);
      if (C4) Store<T, W, ACC>(m, res + (PlaneYX(C4) * L + c) * N + at, hxy, nvalid);
      Store<T, W, ACC>(m, res + (PlaneYY(C4) * L + c) * N + at, hyy, nvalid);
    }
    Copy<T, W>(gx_w, gx_c);
    Copy<T, W>(gy_w, gy_c);
    Copy<T, W>(u_c, u_e);
    c_above = e_above;
    c_below = e_below;
  }
}

/// res (+)= H^T rhs, the same walk
template <class T, int W, bool C4, bool ACC, class Mover>
PROST_SG2_HD void AdjointMarch(const Mover& m, T* res, const T* rhs, size_t nx, size_t ny, size_t L, size_t c, size_t row0, size_t x0, size_t x1, T w) {
  const size_t N = nx * ny;
  const bool active = row0 < ny;
  const int nvalid = active ? (ny - row0 < (size_t)W ? (int)(ny - row0) : W) : 0;
  const T* exx = rhs + (PlaneXX(C4) * L + c) * N;
  const T* eyy = rhs + (PlaneYY(C4) * L + c) * N;
  const T* exy = rhs + (PlaneXY(C4) * L + c) * N;
  const T* eyx = rhs + (PlaneYX(C4) * L + c) * N;     // components = 4 only
  T vx_w[W], xx_c[W], xy_c[W], xx_e[W], xy_e[W], yy_c[W], xy_c_above, xy_c_below, xy_e_above, xy_e_below, yy_above, yy_below;
  Zero<T, W>(vx_w);
  Zero<T, W>(xx_c);
  if (active) m.load(exx + x0 * ny + row0, xx_c, nvalid);
  LoadMixed<T, W, C4>(m, exy + x0 * ny, eyx + x0 * ny, row0, ny, active, nvalid, xy_c, xy_c_above, xy_c_below);
  if (x0 > 0) {                                       // vx of column x0 - 1, where ax holds
    T xx_w[W], xy_w[W], xy_w_above, xy_w_below;
    Zero<T, W>(xx_w);
    if (active) m.load(exx + (x0 - 1) * ny + row0, xx_w, nvalid);
    LoadMixed<T, W, C4>(m, exy + (x0 - 1) * ny, eyx + (x0 - 1) * ny, row0, ny, active, nvalid, xy_w, xy_w_above, xy_w_below);
PROST_SG2_UNROLL
    for (int j = 0; j < W; j++)
      vx_w[j] = sg2::Adjoint<T>(w, true, xx_w[j], xx_c[j], row0 + j + 1 < ny, xy_w[j], j + 1 < W ? xy_w[j + 1 < W ? j + 1 : 0] : xy_w_below);
  }
  for (size_t x = x0; x < x1; x++) {
    const size_t at = x * ny + row0;
    const bool bx = x > 0, ax = x + 1 < nx;
    Zero<T, W>(xx_e);
    if (active && ax) m.load(exx + at + ny, xx_e, nvalid);
    LoadMixed<T, W, C4>(m, exy + (x + 1) * ny, eyx + (x + 1) * ny, row0, ny, active && ax, nvalid, xy_e, xy_e_above, xy_e_below);
    LoadColumn<T, W>(m, eyy + x * ny, row0, ny, active, nvalid, yy_c, yy_above, yy_below);
    T vx[W], vy[W], s[W];
    const T vy_n = sg2::Adjoint<T>(w, true, yy_above, yy_c[0], ax, xy_c_above, xy_e_above);       // row row0 - 1, read where by holds
PROST_SG2_UNROLL
    for (int j = 0; j < W; j++) {
      const bool ay = row0 + j + 1 < ny;
      const T yy_s = j + 1 < W ? yy_c[j + 1 < W ? j + 1 : 0] : yy_below, xy_s = j + 1 < W ? xy_c[j + 1 < W ? j + 1 : 0] : xy_c_below;
      vx[j] = sg2::Adjoint<T>(w, ax, xx_c[j], xx_e[j], ay, xy_c[j], xy_s);
      vy[j] = sg2::Adjoint<T>(w, ay, yy_c[j], yy_s, ax, xy_c[j], xy_e[j]);
    }
PROST_SG2_UNROLL
    for (int j = 0; j < W; j++) {
      const bool by = row0 + j > 0, ay = row0 + j + 1 < ny;
      s[j] = Divergence<T>(ax, vx[j], bx, vx_w[j], ay, vy[j], by, j > 0 ? vy[j > 0 ? j - 1 : 0] : vy_n);
    }
    if (active) {
      T o[W];
      Zero<T, W>(o);
      if (ACC) m.load(res + c * N + at, o, nvalid);
PROST_SG2_UNROLL
      for (int j = 0; j < W; j++) s[j] = o[j] - s[j];
      m.store(res + c * N + at, s, nvalid);
    }
    Copy<T, W>(vx_w, vx);
    Copy<T, W>(xx_c, xx_e);
    Copy<T, W>(xy_c, xy_e);
    xy_c_above = xy_e_above;
    xy_c_below = xy_e_below;
  }
}

// ---- the sums of |entry|^alpha: closed forms ----
/// 2^alpha; exact for alpha = 1
inline double TwoPower(double alpha) { return alpha == 1.0 ? 2.0 : std::pow(2.0, alpha); }
/// s + s^alpha for s = 0, 1, 2 off-centre entries of magnitude 1 and the centre of magnitude s
inline double SecondDifferenceSum(int s, double two_a) { return s == 2 ? 2.0 + two_a : (s == 1 ? 2.0 : 0.0); }
/// the three sums of pixel (y, x): wa = WeightPower(w, alpha), two_a = TwoPower(alpha)
inline void PixelSums(size_t y, size_t x, size_t nx, size_t ny, double wa, double two_a, double& sxx, double& syy, double& sxy) {
  const int ax = x + 1 < nx, bx = x > 0, ay = y + 1 < ny, by = y > 0;
  sxx = SecondDifferenceSum(ax + bx, two_a);
  syy = SecondDifferenceSum(ay + by, two_a);
  sxy = wa * (2.0 * (by * ax) + 2.0 * (bx * ay) + (2.0 + two_a) * (ax * ay));
}
/// row r of H (0 <= r < components L N)
inline double RowSum(size_t r, size_t nx, size_t ny, size_t L, int components, double wa, double two_a) {
  const size_t N = nx * ny, k = r / N / L, p = r % N;
  const bool c4 = components == 4;
  double sxx, syy, sxy;
  PixelSums(p % ny, p / ny, nx, ny, wa, two_a, sxx, syy, sxy);
  return k == PlaneXX(c4) ? sxx : (k == PlaneYY(c4) ? syy : sxy);
}
/// column q of H (0 <= q < L N)
inline double ColSum(size_t q, size_t nx, size_t ny, int components, double wa, double two_a) {
  const size_t p = q % (nx * ny);
  double sxx, syy, sxy;
  PixelSums(p % ny, p / ny, nx, ny, wa, two_a, sxx, syy, sxy);
  return sxx + syy + (components == 4 ? 2.0 : 1.0) * sxy;
}

#if !defined(__HIP_DEVICE_COMPILE__)
/// one product on the host, strip by strip and chunk by chunk as the kernels run it (sym_gradient2d::Apply): lanes of W rows, strips
/// of `lanes` lanes, chunks of PickColumns columns (force_cols > 0: of that many)
template <class T, int W, bool ACC> inline void Apply(T* res, const T* rhs, size_t nx, size_t ny, size_t L, double w, int components, bool transpose, int lanes = 256, int force_cols = 0) {
  const sg2::HostMover<T, W> m;
  const T wt = RoundWeight<T>(w);
  const size_t strip_rows = (size_t)lanes * W, strips = (ny + strip_rows - 1) / strip_rows;
  const size_t cols = force_cols > 0 ? (size_t)force_cols : (size_t)PickColumns(nx, strips, L);
  for (size_t c = 0; c < L; c++)
    for (size_t x0 = 0; x0 < nx; x0 += cols)
      for (size_t row0 = 0; row0 < ny; row0 += W) {              // the lanes past the last row move nothing
        const size_t x1 = x0 + cols < nx ? x0 + cols : nx;
        if (components == 4) {
          if (transpose) AdjointMarch<T, W, true, ACC>(m, res, rhs, nx, ny, L, c, row0, x0, x1, wt);
          else ForwardMarch<T, W, true, ACC>(m, res, rhs, nx, ny, L, c, row0, x0, x1, wt);
        } else {
          if (transpose) AdjointMarch<T, W, false, ACC>(m, res, rhs, nx, ny, L, c, row0, x0, x1, wt);
          else ForwardMarch<T, W, false, ACC>(m, res, rhs, nx, ny, L, c, row0, x0, x1, wt);
        }
      }
}
#endif

}  // namespace hessian2d
}  // namespace prost
#endif
