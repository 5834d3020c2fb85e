// kernels_linop_tensor_gradient2d.hip -- BlockTensorGradient2D: res (+)= K rhs and res (+)= K^T rhs for K = T grad, the gradient of L
// channels of an ny x nx grid weighted per pixel by a scalar, by one weight per axis or by a symmetric 2 x 2 tensor, without a matrix.
// The arithmetic, its order and the marches are include/prost/linop/tensor_gradient2d.hpp, which also runs on the host
// (tests/host/tensor_gradient2d_harness.cpp).  This file decides who reads what.
//
// Vector kernels: the planar column march of grad_fwd_vec_kernel / grad_adj_vec_kernel (kernels_linop.hip).  A lane owns VEC
// consecutive rows (16 bytes), a workgroup of 256 a strip of 256 VEC rows and a chunk of 12 / 6 / 3 / 1 columns of one channel; the
// mode k, the direction and the accumulation are template parameters.  Forward looks ahead: u of column x + 1 is the vector loaded for
// the next step, u of row y + 1 comes from the adjacent lane by a DPP wave shift, and only the last lane of a wave reads one extra
// scalar.  The adjoint looks back at computed values: the flux qx of column x - 1 stays in registers (at the first column of a chunk it
// is computed from gx, gy and the tensor of the halo column), the flux qy of row row0 - 1 is the adjacent lane's last flux, and the
// first lane of a wave computes it from the five scalars at row0 - 1.  Element kernels (one row per lane, everything from memory) take
// the heights that are no multiple of VEC and res, rhs or tensor pointers that are not 16-byte aligned.  No LDS, no scratch, no
// atomics: a repeated call repeats its bits.  Resource table and the all-channels variant that was measured: docs/rounds/r29.md.
#include <cmath>

#include "elementwise.hpp"
#include "fused_op.hpp"
#include "prost/linop/tensor_gradient2d.hpp"

namespace prost_hip {

namespace tg2 = prost::tensor_gradient2d;

/// VEC rows as one 16-byte access; the row neighbours from the adjacent lanes
template <class T, int VEC> struct TensorGradVecMover {
  __device__ __forceinline__ void load(const T* p, T (&v)[VEC], int) const { ldv<T, VEC>(p, v); }
  __device__ __forceinline__ void store(T* p, const T (&v)[VEC], int) const { stv<T, VEC>(p, v); }
  __device__ __forceinline__ T below(const T (&v)[VEC], const T* column, size_t row0, size_t ny, bool active) const { return row_below<T, VEC>(v, column, row0, ny, active); }
  __device__ __forceinline__ T up(T last) const { return lane_up(last); }
  __device__ __forceinline__ bool reads_above(size_t row0, bool active) const { return (threadIdx.x & (kWave - 1)) == 0 && active && row0 > 0; }
};
/// one row per lane, any alignment; the row neighbours from memory
template <class T> struct TensorGradElemMover {
  __device__ __forceinline__ void load(const T* p, T (&v)[1], int) const { v[0] = p[0]; }
  __device__ __forceinline__ void store(T* p, const T (&v)[1], int) const { p[0] = v[0]; }
  __device__ __forceinline__ T below(const T (&)[1], const T* column, size_t row0, size_t ny, bool active) const { return active && row0 + 1 < ny ? column[row0 + 1] : (T)0; }
  __device__ __forceinline__ T up(T) const { return (T)0; }
  __device__ __forceinline__ bool reads_above(size_t row0, bool active) const { return active && row0 > 0; }
};

// res and rhs are not __restrict__ here: the marches read res in the accumulating forms through the same Mover
template <class T, int VEC, int K, bool ADJ, bool ACC>
__global__ void __launch_bounds__(kBlock) tensor_grad2d_kernel(T* res, const T* rhs, const T* tensor, size_t nx, size_t ny, size_t L, unsigned strips, unsigned chunks, int cols) {
  const unsigned strip = blockIdx.x % strips, chunk = (blockIdx.x / strips) % chunks;
  const size_t c = blockIdx.x / (strips * chunks);
  const size_t row0 = ((size_t)strip * kBlock + threadIdx.x) * VEC;
  const size_t x0 = (size_t)chunk * cols, x1 = x0 + cols < nx ? x0 + cols : nx;
  typedef typename std::conditional<VEC == 1, TensorGradElemMover<T>, TensorGradVecMover<T, VEC>>::type Mover;
  const Mover m;
  if (ADJ) tg2::AdjointMarch<T, VEC, K, ACC>(m, res, rhs, tensor, nx, ny, L, c, row0, x0, x1);
  else tg2::ForwardMarch<T, VEC, K, ACC>(m, res, rhs, tensor, nx, ny, L, c, row0, x0, x1);
}

template <class T, int VEC, int K>
static int launch_tensor_grad2d_as(T* res, const T* rhs, const T* tensor, size_t nx, size_t ny, size_t L, int transpose, int accumulate, hipStream_t s) {
  const size_t strips = (ny + (size_t)kBlock * VEC - 1) / ((size_t)kBlock * VEC);
  const int cols = tg2::PickColumns(nx, strips, L);
  const size_t chunks = (nx + cols - 1) / cols, blocks = strips * chunks * L;
  if (blocks >= (1ull << 31)) { set_error("tensor_gradient2d: more than 2^31 - 1 workgroups"); return 1; }
#define GO(ADJv, ACCv) PH_LAUNCH((tensor_grad2d_kernel<T, VEC, K, ADJv, ACCv>), dim3((unsigned)blocks), dim3(kBlock), 0, s, res, rhs, tensor, nx, ny, L, (unsigned)strips, (unsigned)chunks, cols)
  if (!transpose) { if (accumulate) GO(false, true); else GO(false, false); }
  else { if (accumulate) GO(true, true); else GO(true, false); }
#undef GO
  PH_LAUNCH_END("tensor_gradient2d kernel");
}

template <class T, int VEC>
static int launch_tensor_grad2d_mode(T* res, const T* rhs, const T* tensor, size_t nx, size_t ny, size_t L, int mode, int transpose, int accumulate, hipStream_t s) {
  if (mode == 1) return launch_tensor_grad2d_as<T, VEC, 1>(res, rhs, tensor, nx, ny, L, transpose, accumulate, s);
  if (mode == 2) return launch_tensor_grad2d_as<T, VEC, 2>(res, rhs, tensor, nx, ny, L, transpose, accumulate, s);
  return launch_tensor_grad2d_as<T, VEC, 3>(res, rhs, tensor, nx, ny, L, transpose, accumulate, s);
}

template <class T>
static int launch_tensor_grad2d(T* res, const T* rhs, const T* tensor, size_t nx, size_t ny, size_t L, int mode, int transpose, int accumulate, void* stream) {
  if (nx == 0 || ny == 0 || L == 0) { set_error("tensor_gradient2d: nx, ny and L have to be at least 1"); return 1; }
  if (mode < 1 || mode > tg2::kMaxMode) { set_error("tensor_gradient2d: the mode (planes of the tensor) has to be 1, 2 or 3"); return 1; }
  if (!res || !rhs || !tensor) { set_error("tensor_gradient2d: null pointer"); return 1; }
  if (2.0L * (long double)nx * (long double)ny * (long double)L > 9007199254740992.0L) { set_error("tensor_gradient2d: 2 L nx ny has to stay within 2^53"); return 1; }
  constexpr int V = VecOf<T>::N;
  hipStream_t s = as_stream(stream);
  if (ny % V == 0 && aligned16(res) && aligned16(rhs) && aligned16(tensor)) return launch_tensor_grad2d_mode<T, V>(res, rhs, tensor, nx, ny, L, mode, transpose, accumulate, s);
  return launch_tensor_grad2d_mode<T, 1>(res, rhs, tensor, nx, ny, L, mode, transpose, accumulate, s);
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_linop_tensor_gradient2d_f32(float* res, const float* rhs, const float* tensor, size_t nx, size_t ny, size_t L, int mode, int transpose, int accumulate, void* stream) {
  return launch_tensor_grad2d<float>(res, rhs, tensor, nx, ny, L, mode, transpose, accumulate, stream);
}
int prost_hip_linop_tensor_gradient2d_f64(double* res, const double* rhs, const double* tensor, size_t nx, size_t ny, size_t L, int mode, int transpose, int accumulate, void* stream) {
  return launch_tensor_grad2d<double>(res, rhs, tensor, nx, ny, L, mode, transpose, accumulate, stream);
}
}  // extern "C"
