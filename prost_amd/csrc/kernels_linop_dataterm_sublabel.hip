// kernels_linop_dataterm_sublabel.hip -- BlockDatatermSublabel: [r ; s] (+)= K [u ; w] and [u ; w] (+)= K^T [r ; s] for the coupling
// of the sublabel-accurate data term, without a matrix.  The reference ships no kernel for it (its users bolt one on); the arithmetic,
// with its order of operations, is include/prost/linop/dataterm_sublabel.hpp, which also runs on the host
// (tests/host/dataterm_sublabel_harness.cpp).  This file decides who reads what.
//
// Lanes run over pixels, workgroups of 256.  A lane marches over the k = L - 1 planes with the running sum in registers, so every
// access is a plane access and consecutive lanes touch consecutive addresses.  Vector instance: one 16-byte access per lane and plane
// (4 fp32 or 2 fp64 pixels), taken when res and rhs are 16-byte aligned and N is a multiple of the pixels per access (every plane then
// starts aligned).  Element instance: one pixel per lane, everything else -- a block at an odd offset of the operator, a ragged N.
// gamma: k values of T in device memory, read with a wave-uniform index; it is declared apart from res (__restrict__), which lets the
// compiler fetch it with scalar loads although stores to res lie in between.  L is a run-time value.  No LDS, no scratch, no atomics: a
// repeated call repeats its bits.  A lane reads plane i before it writes plane i and never returns to it: res may be rhs.
// Resource table: docs/rounds/r17.md.
#include "common.hpp"
#include "prost/linop/dataterm_sublabel.hpp"

namespace prost_hip {

namespace dts = prost::dataterm_sublabel;

/// one 16-byte access: 4 fp32 or 2 fp64 neighbouring pixels of a plane
struct VectorAccess {
  static __device__ __forceinline__ void Load(const float* p, float (&v)[4]) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  }
  static __device__ __forceinline__ void Store(float* p, const float (&v)[4]) { *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]); }
  static __device__ __forceinline__ void Load(const double* p, double (&v)[2]) {
    const double2 q = *reinterpret_cast<const double2*>(p);
    v[0] = q.x; v[1] = q.y;
  }
  static __device__ __forceinline__ void Store(double* p, const double (&v)[2]) { *reinterpret_cast<double2*>(p) = make_double2(v[0], v[1]); }
};

template <class T, int W, bool TRANSPOSE, bool ACC, class A>
__global__ void __launch_bounds__(kBlock) dataterm_sublabel_kernel(T* res, const T* rhs, size_t npixels, size_t k, const T* __restrict__ gamma, T delta) {
  const size_t p = ((size_t)blockIdx.x * kBlock + threadIdx.x) * W;
  if (p >= npixels) return;              // npixels is a multiple of W: a live lane owns W whole pixels
  if (TRANSPOSE) dts::Adjoint<T, W, ACC, A>(res, rhs, npixels, k, p, delta, gamma);
  else dts::Forward<T, W, ACC, A>(res, rhs, npixels, k, p, delta, gamma);
}

template <class T, int W, class A>
static void launch_instance(T* res, const T* rhs, size_t npixels, size_t k, const T* gamma, T delta, int transpose, int accumulate, hipStream_t s) {
  const dim3 grid((unsigned)((npixels / W + kBlock - 1) / kBlock)), block(kBlock);
  if (transpose) {
    if (accumulate) PH_LAUNCH((dataterm_sublabel_kernel<T, W, true, true, A>), grid, block, 0, s, res, rhs, npixels, k, gamma, delta);
    else PH_LAUNCH((dataterm_sublabel_kernel<T, W, true, false, A>), grid, block, 0, s, res, rhs, npixels, k, gamma, delta);
  } else {
    if (accumulate) PH_LAUNCH((dataterm_sublabel_kernel<T, W, false, true, A>), grid, block, 0, s, res, rhs, npixels, k, gamma, delta);
    else PH_LAUNCH((dataterm_sublabel_kernel<T, W, false, false, A>), grid, block, 0, s, res, rhs, npixels, k, gamma, delta);
  }
}

template <class T>
static int launch_dataterm_sublabel(T* res, const T* rhs, size_t npixels, size_t L, const T* gamma, double delta, int transpose, int accumulate, void* stream) {
  if (L < 2) { set_error("linop_dataterm_sublabel: L has to be at least 2"); return 1; }
  if (npixels == 0) return 0;
  if (!res || !rhs || !gamma) { set_error("linop_dataterm_sublabel: null pointer"); return 1; }
  const size_t k = L - 1;
  if (npixels > ((size_t)1 << 62) / k) { set_error("linop_dataterm_sublabel: npixels * (L - 1) is too large"); return 1; }
  if ((npixels + kBlock - 1) / kBlock > (size_t)0x7fffffff) { set_error("linop_dataterm_sublabel: npixels has to stay below 2^31 * 256"); return 1; }
  constexpr int W = 16 / sizeof(T);
  hipStream_t s = as_stream(stream);
  const bool vector = (((uintptr_t)res | (uintptr_t)rhs) & (uintptr_t)15) == 0 && npixels % W == 0;
  if (vector) launch_instance<T, W, VectorAccess>(res, rhs, npixels, k, gamma, (T)delta, transpose, accumulate, s);
  else launch_instance<T, 1, dts::ElementAccess>(res, rhs, npixels, k, gamma, (T)delta, transpose, accumulate, s);
  PH_LAUNCH_END("linop_dataterm_sublabel kernel");
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_linop_dataterm_sublabel_f32(float* res, const float* rhs, size_t npixels, size_t L, const float* gamma, double delta, int transpose, int accumulate,
                                          void* stream) {
  return launch_dataterm_sublabel<float>(res, rhs, npixels, L, gamma, delta, transpose, accumulate, stream);
}
int prost_hip_linop_dataterm_sublabel_f64(double* res, const double* rhs, size_t npixels, size_t L, const double* gamma, double delta, int transpose, int accumulate,
                                          void* stream) {
  return launch_dataterm_sublabel<double>(res, rhs, npixels, L, gamma, delta, transpose, accumulate, stream);
}
}  // extern "C"
