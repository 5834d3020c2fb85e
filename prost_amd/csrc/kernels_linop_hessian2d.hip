// kernels_linop_hessian2d.hip -- BlockHessian2D: res (+)= H rhs and res (+)= H^T rhs for the second-order differences (u_xx, u_yy,
// u_xy) of L channels of an ny x nx grid (TV^2, Hessian-Schatten norms), without a matrix and without the intermediate gradient field.
// H = sym_gradient2d o gradient2d with the bits of the two kernels chained.  The arithmetic, its order and the marches are
// include/prost/linop/hessian2d.hpp, which also runs on the host (tests/host/hessian2d_harness.cpp).  This file decides who reads what.
//
// Vector kernels: the planar column march of grad_fwd_vec_kernel / grad_adj_vec_kernel (kernels_linop.hip), as in
// kernels_linop_sym_gradient2d.hip.  A lane owns VEC consecutive rows (16 bytes), a workgroup of 256 a strip of 256 VEC rows and a
// chunk of 12 / 6 / 3 / 1 columns of one channel.  Forward keeps the u vectors of columns x and x + 1 and the differences of column
// x - 1 in registers; the rows above and below a lane come from the adjacent lanes by a DPP wave shift, and only the edge lanes of a
// wave read one extra scalar each: u is fetched once per workgroup, plus two halo columns per chunk.  The adjoint keeps exx and the
// mixed vector of columns x and x + 1, carries the x component of E^T e of column x - 1 and forms the y component of the row above the
// lane from the shifted elements in the same pass.  Element kernels (one row per lane, neighbours read from memory) take the heights
// that are no multiple of VEC and the pointers that are not 16-byte aligned.  No LDS, no scratch, no atomics: a repeated call repeats
// its bits.  Resource table: docs/rounds/r32.md.
#include <cmath>

#include "elementwise.hpp"
#include "fused_op.hpp"
#include "prost/linop/hessian2d.hpp"

namespace prost_hip {

namespace h2 = prost::hessian2d;

// the Movers of kernels_linop_sym_gradient2d.hip
/// VEC rows as one 16-byte access; the row neighbour from the adjacent lane
template <class T, int VEC> struct HessianVecMover {
  __device__ __forceinline__ void load(const T* p, T (&v)[VEC], int) const { ldv<T, VEC>(p, v); }
  __device__ __forceinline__ void store(T* p, const T (&v)[VEC], int) const { stv<T, VEC>(p, v); }
  __device__ __forceinline__ T above(const T (&v)[VEC], const T* column, size_t row0, bool active) const { return row_above<T, VEC>(v, column, row0, active); }
  __device__ __forceinline__ T below(const T (&v)[VEC], const T* column, size_t row0, size_t ny, bool active) const { return row_below<T, VEC>(v, column, row0, ny, active); }
};
/// one row per lane, any alignment; the row neighbour from memory
template <class T> struct HessianElemMover {
  __device__ __forceinline__ void load(const T* p, T (&v)[1], int) const { v[0] = p[0]; }
  __device__ __forceinline__ void store(T* p, const T (&v)[1], int) const { p[0] = v[0]; }
  __device__ __forceinline__ T above(const T (&)[1], const T* column, size_t row0, bool active) const { return active && row0 > 0 ? column[row0 - 1] : (T)0; }
  __device__ __forceinline__ T below(const T (&)[1], const T* column, size_t row0, size_t ny, bool active) const { return active && row0 + 1 < ny ? column[row0 + 1] : (T)0; }
};

// res and rhs are not __restrict__ here: the marches read res in the accumulating forms through the same Mover
template <class T, int VEC, bool C4, bool ADJ, bool ACC>
__global__ void __launch_bounds__(kBlock) hessian2d_kernel(T* res, const T* rhs, size_t nx, size_t ny, size_t L, T w, unsigned strips, unsigned chunks, int cols) {
  const unsigned strip = blockIdx.x % strips, chunk = (blockIdx.x / strips) % chunks;
  const size_t c = blockIdx.x / (strips * chunks);
  const size_t row0 = ((size_t)strip * kBlock + threadIdx.x) * VEC;
  const size_t x0 = (size_t)chunk * cols, x1 = x0 + cols < nx ? x0 + cols : nx;
  typedef typename std::conditional<VEC == 1, HessianElemMover<T>, HessianVecMover<T, VEC>>::type Mover;
  const Mover m;
  if (ADJ) h2::AdjointMarch<T, VEC, C4, ACC>(m, res, rhs, nx, ny, L, c, row0, x0, x1, w);
  else h2::ForwardMarch<T, VEC, C4, ACC>(m, res, rhs, nx, ny, L, c, row0, x0, x1, w);
}

template <class T, int VEC, bool C4>
static int launch_hessian2d_as(T* res, const T* rhs, size_t nx, size_t ny, size_t L, T w, int transpose, int accumulate, hipStream_t s) {
  const size_t strips = (ny + (size_t)kBlock * VEC - 1) / ((size_t)kBlock * VEC);
  const int cols = h2::PickColumns(nx, strips, L);
  const size_t chunks = (nx + cols - 1) / cols, blocks = strips * chunks * L;
  if (blocks >= (1ull << 31)) { set_error("hessian2d: more than 2^31 - 1 workgroups"); return 1; }
#define GO(ADJv, ACCv) PH_LAUNCH((hessian2d_kernel<T, VEC, C4, ADJv, ACCv>), dim3((unsigned)blocks), dim3(kBlock), 0, s, res, rhs, nx, ny, L, w, (unsigned)strips, (unsigned)chunks, cols)
  if (!transpose) { if (accumulate) GO(false, true); else GO(false, false); }
  else { if (accumulate) GO(true, true); else GO(true, false); }
#undef GO
  PH_LAUNCH_END("hessian2d kernel");
}

template <class T>
static int launch_hessian2d(T* res, const T* rhs, size_t nx, size_t ny, size_t L, double w, int components, int transpose, int accumulate, void* stream) {
  if (nx == 0 || ny == 0 || L == 0) { set_error("hessian2d: nx, ny and L have to be at least 1"); return 1; }
  if (!std::isfinite(w)) { set_error("hessian2d: w has to be finite"); return 1; }
  if (components != 3 && components != 4) { set_error("hessian2d: components has to be 3 or 4"); return 1; }
  const T wt = h2::RoundWeight<T>(w);
  if (wt == (T)0 || !std::isfinite((double)wt)) { set_error("hessian2d: w is zero or not finite after rounding to the precision"); return 1; }
  if (!res || !rhs) { set_error("hessian2d: null pointer"); return 1; }
  if ((long double)components * (long double)nx * (long double)ny * (long double)L > 9007199254740992.0L) { set_error("hessian2d: components L nx ny has to stay within 2^53"); return 1; }
  constexpr int V = VecOf<T>::N;
  hipStream_t s = as_stream(stream);
  const bool vec = ny % V == 0 && aligned16(res) && aligned16(rhs);
  if (components == 4) {
    if (vec) return launch_hessian2d_as<T, V, true>(res, rhs, nx, ny, L, wt, transpose, accumulate, s);
    return launch_hessian2d_as<T, 1, true>(res, rhs, nx, ny, L, wt, transpose, accumulate, s);
  }
  if (vec) return launch_hessian2d_as<T, V, false>(res, rhs, nx, ny, L, wt, transpose, accumulate, s);
  return launch_hessian2d_as<T, 1, false>(res, rhs, nx, ny, L, wt, transpose, accumulate, s);
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_hessian2d_f32(float* res, const float* rhs, size_t nx, size_t ny, size_t L, double w, int components, int transpose, int accumulate, void* stream) {
  return launch_hessian2d<float>(res, rhs, nx, ny, L, w, components, transpose, accumulate, stream);
}
int prost_hip_hessian2d_f64(double* res, const double* rhs, size_t nx, size_t ny, size_t L, double w, int components, int transpose, int accumulate, void* stream) {
  return launch_hessian2d<double>(res, rhs, nx, ny, L, w, components, transpose, accumulate, stream);
}
}  // extern "C"
