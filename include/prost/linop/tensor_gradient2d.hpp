// prost/linop/tensor_gradient2d.hpp -- the arithmetic of BlockTensorGradient2D: K = T grad on L channels of an ny x nx grid, a gradient
// weighted per pixel by a scalar (edge-weighted TV), by one weight per axis, or by a symmetric 2 x 2 tensor (the image-driven diffusion
// tensor D^(1/2) of anisotropic Huber-L1 and anisotropic TGV), without a matrix.  The reference has no such block; this is written from
// the definition.
//
// Grid: N = nx ny, pixel (y, x) at p = y + x ny (column-major).  Domain (L N values): u_c[p] at c N + p.  Range (2 L N values, the range
// layout of gradient2d(nx, ny, L)): gx_c[p] at c N + p, gy_c[p] at (L + c) N + p.  Masks: ax = [x < nx-1], bx = [x > 0], ay = [y < ny-1],
// by = [y > 0].  The tensor is one field of k planes of N values shared by all channels, each value rounded to T once, on the host:
//
//   k = 1   g         T(p) = g I                     (a = c = g, b absent)
//   k = 2   a, c      T(p) = diag(a, c)              (b absent)
//   k = 3   a, b, c   T(p) = [[a, b], [b, c]]
//
// Order of operations (the one place it is written down; kernels and host library build without contraction): every difference, every
// product and every addition is one rounding in T.  A term that the mode does not have is never formed, and a term whose entry of the
// explicit matrix is masked away is selected away, never multiplied by zero: the select sits on the PRODUCT, so a tensor value whose
// matrix entries are all masked (a in the last column, c in the last row) never reaches an output, whatever it holds.  For finite
// tensors this is `dx = ax ? u[p+ny] - u[p] : +0, gx = a dx` up to the sign of a zero.
//
//   forward   dx = u[p+ny] - u[p], dy = u[p+1] - u[p]   (each formed only where its mask holds)
//             k = 1:  gx = (ax) g dx                       gy = (ay) g dy
//             k = 2:  gx = (ax) a dx                       gy = (ay) c dy
//             k = 3:  gx = (ax) a dx  +  (ay) b dy         gy = (ax) b dx  +  (ay) c dy
//             a sum of two present terms is one addition; one present term is that term; none is +0.
//   adjoint   the fluxes  k = 1: qx = g gx, qy = g gy;  k = 2: qx = a gx, qy = c gy;  k = 3: qx = a gx + b gy, qy = b gx + c gy
//             (tensor, gx, gy all at p), then exactly as grad_adj_kernel:
//             divx = (ax) qx[p] else 0;  if (bx) divx -= qx[p-ny];   divy = (ay) qy[p] else 0;  if (by) divy -= qy[p-1];
//             s = divx + divy;   res = 0 - s, accumulating res - s.
//   The accumulating forward form stores res + value.  With k = 1 and g = 1 both directions are gradient2d bit for bit.
//
// The explicit matrix (rows gx[p], gy[p]; the two terms that meet in column p of one row are ONE merged entry):
//   row gx[p]:  -(ax a + ay b) at p,  ax a at p + ny,  ay b at p + 1;       row gy[p]: the same with (b, c) in place of (a, b).
//
// Error bound against that matrix in exact arithmetic, componentwise, with B = |T| (|grad| |x|) forward and |grad|^T (|T| |y|) for the
// adjoint -- the UNMERGED absolute values: a and b may have opposite signs, so |K| |x| with the merged diagonal is too small.  Each
// input reaches the output through a chain of roundings, so |got - exact| <= gamma_n B, gamma_n = n u / (1 - n u), u the unit roundoff:
//   block, forward:   difference 1, product 1, the addition of the two terms 1 (k = 3 only)                      n = 2, 2, 3
//   block, adjoint:   product 1, the addition inside the flux 1 (k = 3 only), divx / divy 1, s 1; 0 - s is exact    n = 3, 3, 4
//   a CSR twin with entries rounded to T that adds its products one by one from 0 (the first addition is exact):
//     forward, a row of 3 entries: the merged diagonal -(a + b) is rounded 1 (k = 3 only), product 1, 2 additions    n = 3, 3, 4
//     adjoint, a column of 6 entries (k = 3; 4 otherwise): diagonal 1 (k = 3 only), product 1, 5 (3) additions       n = 4, 4, 7
//   |block - twin| <= (gamma_block + gamma_twin) B.
//
// A march walks the columns x0 .. x1 - 1 of one channel for W consecutive rows row0 .. row0 + W - 1.  Forward looks ahead: u of column
// x + 1 is the group loaded for the next step and kept, u of row y + 1 is one scalar the Mover supplies (on the device the adjacent
// lane's first element).  The adjoint looks back at COMPUTED values: qx of column x - 1 is carried, and recomputed from gx, gy and the
// tensor of the halo column at the first column of a chunk; qy of row row0 - 1 is the adjacent lane's last flux, and where the Mover
// says so (the first lane of a wave, every lane on the host) it is recomputed from gx, gy and the tensor at row0 - 1 in memory.  The
// recomputation is the same expression, so it gives the same bits.  A Mover says how W rows are moved:
//   void load(const T* p, T (&v)[W], int nvalid) const;   void store(T* p, const T (&v)[W], int nvalid) const;
//   T below(const T (&v)[W], const T* column, size_t row0, size_t ny, bool active) const;   // column[row0 + W], anything if past ny
//   T up(T last) const;                                   // the `last` of the lane that owns the rows above, anything if there is none
//   bool reads_above(size_t row0, bool active) const;     // true: `up` does not hold row row0 - 1, recompute it from memory
// res must not overlap rhs or the tensor.
#ifndef PROST_LINOP_TENSOR_GRADIENT2D_HPP_
#define PROST_LINOP_TENSOR_GRADIENT2D_HPP_
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PROST_TG2_HD __host__ __device__ __forceinline__
#define PROST_TG2_UNROLL _Pragma("unroll")
#else
#define PROST_TG2_HD inline
#define PROST_TG2_UNROLL
#endif

namespace prost {
namespace tensor_gradient2d {

constexpr int kColumnChoices[3] = {12, 6, 3};   ///< columns of a chunk, the largest that still leaves kFillBlocks workgroups; else 1
constexpr size_t kFillBlocks = 2048;
constexpr int kMaxMode = 3;

/// the roundings n of the bound gamma_n B above, by mode k = 1, 2, 3
constexpr int kRoundingsForward[3] = {2, 2, 3};
constexpr int kRoundingsAdjoint[3] = {3, 3, 4};
constexpr int kTwinRoundingsForward[3] = {3, 3, 4};
constexpr int kTwinRoundingsAdjoint[3] = {4, 4, 7};
constexpr int kTerms = 6;                       ///< the longest sum of |entry|^alpha (a column at k = 3): the t of (t + 8) eps_T

/// columns per chunk for a grid of `strips` row strips and L channels (the rule of the gradient2d vector kernels)
inline int PickColumns(size_t nx, size_t strips, size_t L) {
  for (int c : kColumnChoices)
    if (strips * ((nx + (size_t)c - 1) / (size_t)c) * L >= kFillBlocks) return c;
  return 1;
}

// ---- the terms ----
/// (m0) t0 + (m1) t1: absent terms are not added
template <class T> PROST_TG2_HD T Combine(bool m0, T t0, bool m1, T t1) {
  if (m0) return m1 ? t0 + t1 : t0;
  return m1 ? t1 : (T)0;
}
/// (T(p) (vx, vy)) with the vx terms present where mx holds and the vy terms where my holds: forward (dx, dy) with (ax, ay), the adjoint's
/// fluxes (gx, gy) with (true, true).  ta, tb, tc: plane 0, 1, 2 of the tensor at p; a plane the mode does not have is not looked at.
template <class T, int K> PROST_TG2_HD void Flux(T ta, T tb, T tc, T vx, T vy, bool mx, bool my, T& qx, T& qy) {
  if (K == 1) { qx = mx ? ta * vx : (T)0; qy = my ? ta * vy : (T)0; }
  else if (K == 2) { qx = mx ? ta * vx : (T)0; qy = my ? tb * vy : (T)0; }
  else { qx = Combine<T>(mx, ta * vx, my, tb * vy); qy = Combine<T>(mx, tb * vx, my, tc * vy); }
}
/// only qy of Flux<T, K>(.., true, true, ..): the row neighbour's flux recomputed from memory
template <class T, int K> PROST_TG2_HD T FluxY(T ta, T tb, T tc, T vx, T vy) {
  if (K == 1) return ta * vy;
  if (K == 2) return tb * vy;
  return tb * vx + tc * vy;
}

// ---- the marches ----
template <class T, int W, bool ACC, class Mover>
PROST_TG2_HD void Put(const Mover& m, T* p, T (&v)[W], int nvalid) {
  if (ACC) {
    T o[W];
    m.load(p, o, nvalid);
PROST_TG2_UNROLL
    for (int j = 0; j < W; j++) v[j] = o[j] + v[j];
  }
  m.store(p, v, nvalid);
}
/// the planes of the mode at `at`; the others stay 0
template <class T, int W, int K, class Mover>
PROST_TG2_HD void LoadTensor(const Mover& m, const T* tensor, size_t N, size_t at, T (&ta)[W], T (&tb)[W], T (&tc)[W], bool active, int nvalid) {
PROST_TG2_UNROLL
  for (int j = 0; j < W; j++) { ta[j] = (T)0; tb[j] = (T)0; tc[j] = (T)0; }
  if (!active) return;
  m.load(tensor + at, ta, nvalid);
  if (K >= 2) m.load(tensor + N + at, tb, nvalid);
  if (K == 3) m.load(tensor + 2 * N + at, tc, nvalid);
}

/// res (+)= K rhs on rows row0 .. row0 + W - 1, columns x0 .. x1 - 1 of channel c.  Every lane of a wave walks the same columns (the
/// Mover may exchange values between lanes); a lane with row0 >= ny moves nothing.
template <class T, int W, int K, bool ACC, class Mover>
PROST_TG2_HD void ForwardMarch(const Mover& m, T* res, const T* rhs, const T* tensor, size_t nx, size_t ny, size_t L, size_t c, size_t row0, size_t x0, size_t x1) {
  const size_t N = nx * ny;
  const bool active = row0 < ny;
  const int nvalid = active ? (ny - row0 < (size_t)W ? (int)(ny - row0) : W) : 0;
  const T* u = rhs + c * N;
  T cur[W], nxt[W], ta[W], tb[W], tc[W];
PROST_TG2_UNROLL
  for (int j = 0; j < W; j++) cur[j] = (T)0;
  if (active && x0 < x1) m.load(u + x0 * ny + row0, cur, nvalid);
  for (size_t x = x0; x < x1; x++) {
    const size_t at = x * ny + row0;
    const bool ax = x + 1 < nx;
PROST_TG2_UNROLL
    for (int j = 0; j < W; j++) nxt[j] = (T)0;
    if (active && ax) m.load(u + at + ny, nxt, nvalid);
    LoadTensor<T, W, K>(m, tensor, N, at, ta, tb, tc, active, nvalid);
    const T below = m.below(cur, u + x * ny, row0, ny, active);
    T gx[W], gy[W];
PROST_TG2_UNROLL
    for (int j = 0; j < W; j++) {
      const bool ay = row0 + j + 1 < ny;
      const T val = cur[j], dn = j + 1 < W ? cur[j + 1 < W ? j + 1 : 0] : below;
      const T dy = ay ? dn - val : (T)0, dx = ax ? nxt[j] - val : (T)0;
      Flux<T, K>(ta[j], tb[j], tc[j], dx, dy, ax, ay, gx[j], gy[j]);
    }
    if (active) {
      Put<T, W, ACC>(m, res + c * N + at, gx, nvalid);
      Put<T, W, ACC>(m, res + (L + c) * N + at, gy, nvalid);
    }
PROST_TG2_UNROLL
    for (int j = 0; j < W; j++) cur[j] = nxt[j];
  }
}

/// res (+)= K^T rhs, the same walk
template <class T, int W, int K, bool ACC, class Mover>
PROST_TG2_HD void AdjointMarch(const Mover& m, T* res, const T* rhs, const T* tensor, size_t nx, size_t ny, size_t L, size_t c, size_t row0, size_t x0, size_t x1) {
  const size_t N = nx * ny;
  const bool active = row0 < ny;
  const int nvalid = active ? (ny - row0 < (size_t)W ? (int)(ny - row0) : W) : 0;
  const T* gxp = rhs + c * N;
  const T* gyp = rhs + (L + c) * N;
  const T* tb_plane = tensor + (K >= 2 ? N : 0);            // the plane FluxY's tb comes from (k = 1: unused)
  const T* tc_plane = tensor + (K == 3 ? 2 * N : 0);
  T prev[W], gx[W], gy[W], ta[W], tb[W], tc[W], qx[W], qy[W];
PROST_TG2_UNROLL
  for (int j = 0; j < W; j++) prev[j] = (T)0;
  if (active && x0 > 0 && x0 < x1) {                         // the halo column: its flux is computed here, nobody hands it over
    const size_t at = (x0 - 1) * ny + row0;
    m.load(gxp + at, gx, nvalid);
    m.load(gyp + at, gy, nvalid);
    LoadTensor<T, W, K>(m, tensor, N, at, ta, tb, tc, active, nvalid);
PROST_TG2_UNROLL
    for (int j = 0; j < W; j++) { T unused; Flux<T, K>(ta[j], tb[j], tc[j], gx[j], gy[j], true, true, prev[j], unused); }
  }
  for (size_t x = x0; x < x1; x++) {
    const size_t at = x * ny + row0;
    const bool ax = x + 1 < nx, bx = x > 0;
PROST_TG2_UNROLL
    for (int j = 0; j < W; j++) { gx[j] = (T)0; gy[j] = (T)0; }
    if (active) { m.load(gxp + at, gx, nvalid); m.load(gyp + at, gy, nvalid); }
    LoadTensor<T, W, K>(m, tensor, N, at, ta, tb, tc, active, nvalid);
PROST_TG2_UNROLL
    for (int j = 0; j < W; j++) Flux<T, K>(ta[j], tb[j], tc[j], gx[j], gy[j], true, true, qx[j], qy[j]);
    T above = m.up(qy[W - 1]);
    if (m.reads_above(row0, active)) above = FluxY<T, K>(tensor[at - 1], tb_plane[at - 1], tc_plane[at - 1], gxp[at - 1], gyp[at - 1]);
    T o[W];
PROST_TG2_UNROLL
    for (int j = 0; j < W; j++) {
      T divx, divy;
      if (row0 + j + 1 < ny) divy = qy[j]; else divy = (T)0;
      if (row0 + j > 0) divy -= j > 0 ? qy[j > 0 ? j - 1 : 0] : above;
      if (ax) divx = qx[j]; else divx = (T)0;
      if (bx) divx -= prev[j];
      o[j] = divx + divy;
    }
    if (active) {
      if (ACC) {
        T r[W];
        m.load(res + c * N + at, r, nvalid);
PROST_TG2_UNROLL
        for (int j = 0; j < W; j++) o[j] = r[j] - o[j];
      } else {
PROST_TG2_UNROLL
        for (int j = 0; j < W; j++) o[j] = (T)0 - o[j];
      }
      m.store(res + c * N + at, o, nvalid);
    }
PROST_TG2_UNROLL
    for (int j = 0; j < W; j++) prev[j] = qx[j];
  }
}

// ---- the sums of |entry|^alpha over the explicit matrix with its merged diagonal: in double from the T-rounded planes ----
/// |v|^alpha, 0 for an entry of 0 (no entry); exact for alpha = 1
inline double EntryPower(double v, double alpha) { return v == 0 ? 0.0 : (alpha == 1.0 ? std::fabs(v) : std::pow(std::fabs(v), alpha)); }

/// (a, b, c) of pixel p as doubles; the planes a mode does not have: a = c = g, b = 0 (k = 1), b = 0 (k = 2)
template <class T> inline void TensorAt(const T* tensor, size_t N, int mode, size_t p, double& a, double& b, double& c) {
  a = (double)tensor[p];
  b = mode == 3 ? (double)tensor[N + p] : 0.0;
  c = mode == 1 ? a : (double)tensor[(mode == 3 ? 2 : 1) * N + p];
}
/// the two row sums of pixel (y, x): rows gx[p] and gy[p]
template <class T> inline void PixelRowSums(const T* tensor, size_t nx, size_t ny, int mode, size_t x, size_t y, double alpha, double& sx, double& sy) {
  const double ax = x + 1 < nx, ay = y + 1 < ny;
  double a, b, c;
  TensorAt(tensor, nx * ny, mode, y + x * ny, a, b, c);
  sx = EntryPower(ax * a + ay * b, alpha) + ax * EntryPower(a, alpha) + ay * EntryPower(b, alpha);
  sy = EntryPower(ax * b + ay * c, alpha) + ax * EntryPower(b, alpha) + ay * EntryPower(c, alpha);
}
/// the column sum of pixel (y, x): the two diagonals, (a, b) of p - ny, (b, c) of p - 1
template <class T> inline double PixelColSum(const T* tensor, size_t nx, size_t ny, int mode, size_t x, size_t y, double alpha) {
  const size_t N = nx * ny, p = y + x * ny;
  const double ax = x + 1 < nx, ay = y + 1 < ny;
  double a, b, c;
  TensorAt(tensor, N, mode, p, a, b, c);
  double s = EntryPower(ax * a + ay * b, alpha) + EntryPower(ax * b + ay * c, alpha);
  if (x > 0) { TensorAt(tensor, N, mode, p - ny, a, b, c); s += EntryPower(a, alpha) + EntryPower(b, alpha); }
  if (y > 0) { TensorAt(tensor, N, mode, p - 1, a, b, c); s += EntryPower(b, alpha) + EntryPower(c, alpha); }
  return s;
}
/// row r of K (0 <= r < 2 L N)
template <class T> inline double RowSum(size_t r, const T* tensor, size_t nx, size_t ny, size_t L, int mode, double alpha) {
  const size_t N = nx * ny, plane = r / N, p = r % N;
  double sx, sy;
  PixelRowSums(tensor, nx, ny, mode, p / ny, p % ny, alpha, sx, sy);
  return plane < L ? sx : sy;
}
/// column q of K (0 <= q < L N)
template <class T> inline double ColSum(size_t q, const T* tensor, size_t nx, size_t ny, size_t, int mode, double alpha) {
  const size_t p = q % (nx * ny);
  return PixelColSum(tensor, nx, ny, mode, p / ny, p % ny, alpha);
}
/// out[r] += RowSum(r) for every row: one pass over the pixels, cast once
template <class T> inline void RowSums(T* out, const T* tensor, size_t nx, size_t ny, size_t L, int mode, double alpha) {
  const size_t N = nx * ny;
  for (size_t x = 0; x < nx; x++)
    for (size_t y = 0; y < ny; y++) {
      double sx, sy;
      PixelRowSums(tensor, nx, ny, mode, x, y, alpha, sx, sy);
      const T tx = (T)sx, ty = (T)sy;
      for (size_t c = 0; c < L; c++) { out[c * N + y + x * ny] += tx; out[(L + c) * N + y + x * ny] += ty; }
    }
}
/// out[q] += ColSum(q) for every column
template <class T> inline void ColSums(T* out, const T* tensor, size_t nx, size_t ny, size_t L, int mode, double alpha) {
  const size_t N = nx * ny;
  for (size_t x = 0; x < nx; x++)
    for (size_t y = 0; y < ny; y++) {
      const T s = (T)PixelColSum(tensor, nx, ny, mode, x, y, alpha);
      for (size_t c = 0; c < L; c++) out[c * N + y + x * ny] += s;
    }
}

#if !defined(__HIP_DEVICE_COMPILE__)
/// W rows moved one by one, neighbours read (and recomputed) from memory: the host form (tests/host/tensor_gradient2d_harness.cpp)
template <class T, int W> struct HostMover {
  void load(const T* p, T (&v)[W], int nvalid) const { for (int j = 0; j < W; j++) v[j] = j < nvalid ? p[j] : (T)0; }
  void store(T* p, const T (&v)[W], int nvalid) const { for (int j = 0; j < W; j++) if (j < nvalid) p[j] = v[j]; }
  T below(const T (&)[W], const T* column, size_t row0, size_t ny, bool active) const { return active && row0 + W < ny ? column[row0 + W] : (T)0; }
  T up(T) const { return (T)0; }
  bool reads_above(size_t row0, bool active) const { return active && row0 > 0; }
};

template <class T, int W, int K, bool ACC> inline void ApplyMode(T* res, const T* rhs, const T* tensor, size_t nx, size_t ny, size_t L, bool transpose, int lanes, int force_cols) {
  const HostMover<T, W> m;
  const size_t strip_rows = (size_t)lanes * W, strips = (ny + strip_rows - 1) / strip_rows;
  const size_t cols = force_cols > 0 ? (size_t)force_cols : (size_t)PickColumns(nx, strips, L);
  for (size_t c = 0; c < L; c++)
    for (size_t x0 = 0; x0 < nx; x0 += cols)
      for (size_t row0 = 0; row0 < ny; row0 += W) {              // the lanes past the last row move nothing
        const size_t x1 = x0 + cols < nx ? x0 + cols : nx;
        if (transpose) AdjointMarch<T, W, K, ACC>(m, res, rhs, tensor, nx, ny, L, c, row0, x0, x1);
        else ForwardMarch<T, W, K, ACC>(m, res, rhs, tensor, nx, ny, L, c, row0, x0, x1);
      }
}
/// one product on the host, strip by strip and chunk by chunk as the kernels run it: lanes of W rows, strips of `lanes` lanes,
/// chunks of PickColumns columns (force_cols > 0: of that many); mode 1, 2 or 3
template <class T, int W, bool ACC> inline void Apply(T* res, const T* rhs, const T* tensor, size_t nx, size_t ny, size_t L, int mode, bool transpose, int lanes = 256, int force_cols = 0) {
  if (mode == 1) ApplyMode<T, W, 1, ACC>(res, rhs, tensor, nx, ny, L, transpose, lanes, force_cols);
  else if (mode == 2) ApplyMode<T, W, 2, ACC>(res, rhs, tensor, nx, ny, L, transpose, lanes, force_cols);
  else ApplyMode<T, W, 3, ACC>(res, rhs, tensor, nx, ny, L, transpose, lanes, force_cols);
}
#endif

}  // namespace tensor_gradient2d
}  // namespace prost
#endif
