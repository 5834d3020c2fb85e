// kernels_prox_epi_conjquad.hip -- ProxIndEpiConjQuad1D: the projection of (y, t) onto the epigraph of the conjugate of one quadratic
// piece, t >= phi*(y) with phi(x) = a x^2 + b x + c on [alpha, beta].  The reference ships no kernel for it (its users bolt one on);
// the arithmetic is include/prost/prox/epi_conjquad.hpp, which also runs on the host (tests/host/epi_conjquad_harness.cpp).  This file
// decides who reads what and keeps the Newton loop of the arc region uniform.
//
// One group per lane, workgroups of 256.  Planar: y at g, t at g + count.  Interleaved: (y, t) at 2 g, 2 g + 1, read and written as
// one 8 / 16-byte access per lane when both pointers are aligned for it (LAYOUT 2); a prox at an odd index of its variable hands in
// arg + index, aligned for one element only, and takes element accesses (LAYOUT 1).  Each coefficient is a pointer to count values
// or NULL with the value in the argument list.  A lane reads its group before it writes it and touches no other: res may be arg.
// The loop is `for (it < cap && __any(pending))`: every lane of a wave leaves it together, finished lanes idle through a predicated
// body.  A lane still pending at the cap writes (y0, max(t0, phi*(y0))) and counts itself in *fallback_counter.  A non-zero *stop
// (the stop word of a device-resident step-size rule) makes the launch return without writing.
// No LDS, no scratch (resource table: docs/rounds/r15.md).
#include "common.hpp"
#include "prost/prox/epi_conjquad.hpp"

namespace prost_hip {

namespace ecq = prost::epi_conjquad;

template <class T> struct Pair;
template <> struct Pair<float> { using type = float2; };
template <> struct Pair<double> { using type = double2; };

template <class T>
struct ConjQuadCoeffs {
  const T* ptr[5];       // a, b, c, alpha, beta: count values each, or NULL
  T val[5];
};

template <class T, int LAYOUT>
__global__ void __launch_bounds__(kBlock) epi_conjquad_kernel(T* res, const T* arg, size_t count, ConjQuadCoeffs<T> co, unsigned* fallback_counter,
                                                             const int* stop) {
  using P2 = typename Pair<T>::type;
  if (stop && *stop) return;
  const size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = g < count;

  T y0 = 0, t0 = 0;
  ecq::Piece<T> p;
  p.Set((T)1, (T)0, (T)0, (T)0, (T)0);
  if (live) {
    if (LAYOUT == 0) { y0 = arg[g]; t0 = arg[g + count]; }
    else if (LAYOUT == 1) { y0 = arg[2 * g]; t0 = arg[2 * g + 1]; }
    else { const P2 v = reinterpret_cast<const P2*>(arg)[g]; y0 = v.x; t0 = v.y; }
    p.Set(co.ptr[0] ? co.ptr[0][g] : co.val[0], co.ptr[1] ? co.ptr[1][g] : co.val[1], co.ptr[2] ? co.ptr[2][g] : co.val[2],
          co.ptr[3] ? co.ptr[3][g] : co.val[3], co.ptr[4] ? co.ptr[4][g] : co.val[4]);
  }
  ecq::Projector<T> st;
  st.Begin(p, y0, t0);           // a dead lane holds (0, 0) above phi* = y^2 / 4: inside, never pending

  for (int it = 0; it < ecq::kStepCap && __any(st.pending); it++)
    if (st.pending) st.Step(p);
  if (st.pending) {
    st.Fallback(p, y0, t0);
    if (fallback_counter) atomicAdd(fallback_counter, 1u);
  }

  if (live) {
    if (LAYOUT == 0) { res[g] = st.y; res[g + count] = st.t; }
    else if (LAYOUT == 1) { res[2 * g] = st.y; res[2 * g + 1] = st.t; }
    else { P2 v; v.x = st.y; v.y = st.t; reinterpret_cast<P2*>(res)[g] = v; }
  }
}

template <class T>
static int launch_epi_conjquad(T* res, const T* arg, size_t count, int interleaved, const T* const (&ptr)[5], const double (&val)[5],
                               unsigned* fallback_counter, const int* stop, void* stream) {
  if (count == 0) return 0;
  if (!res || !arg) { set_error("prox_ind_epi_conjquad_1d: null pointer"); return 1; }
  const size_t blocks = (count + kBlock - 1) / kBlock;
  if (blocks > (size_t)0x7fffffff) { set_error("prox_ind_epi_conjquad_1d: count has to stay below 2^31 * 256"); return 1; }
  ConjQuadCoeffs<T> co;
  for (int i = 0; i < 5; i++) { co.ptr[i] = ptr[i]; co.val[i] = (T)val[i]; }
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)blocks), block(kBlock);
  const bool aligned = (((uintptr_t)res | (uintptr_t)arg) & (uintptr_t)(2 * sizeof(T) - 1)) == 0;
  if (!interleaved) PH_LAUNCH((epi_conjquad_kernel<T, 0>), grid, block, 0, s, res, arg, count, co, fallback_counter, stop);
  else if (!aligned) PH_LAUNCH((epi_conjquad_kernel<T, 1>), grid, block, 0, s, res, arg, count, co, fallback_counter, stop);
  else PH_LAUNCH((epi_conjquad_kernel<T, 2>), grid, block, 0, s, res, arg, count, co, fallback_counter, stop);
  PH_LAUNCH_END("ind_epi_conjquad_1d kernel");
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_epi_conjquad_step_cap(int dtype, int* cap) {
  if (dtype != 0 && dtype != 1) { set_error("epi_conjquad_step_cap: dtype is 0 (fp32) or 1 (fp64)"); return 1; }
  if (cap) *cap = ecq::kStepCap;
  return 0;
}
int prost_hip_prox_ind_epi_conjquad_1d_f32(float* res, const float* arg, size_t count, int interleaved, const float* a_ptr, double a_val, const float* b_ptr,
                                           double b_val, const float* c_ptr, double c_val, const float* alpha_ptr, double alpha_val, const float* beta_ptr,
                                           double beta_val, unsigned* fallback_counter, const int* stop_dev, void* stream) {
  const float* const ptr[5] = {a_ptr, b_ptr, c_ptr, alpha_ptr, beta_ptr};
  const double val[5] = {a_val, b_val, c_val, alpha_val, beta_val};
  return launch_epi_conjquad<float>(res, arg, count, interleaved, ptr, val, fallback_counter, stop_dev, stream);
}
int prost_hip_prox_ind_epi_conjquad_1d_f64(double* res, const double* arg, size_t count, int interleaved, const double* a_ptr, double a_val, const double* b_ptr,
                                           double b_val, const double* c_ptr, double c_val, const double* alpha_ptr, double alpha_val, const double* beta_ptr,
                                           double beta_val, unsigned* fallback_counter, const int* stop_dev, void* stream) {
  const double* const ptr[5] = {a_ptr, b_ptr, c_ptr, alpha_ptr, beta_ptr};
  const double val[5] = {a_val, b_val, c_val, alpha_val, beta_val};
  return launch_epi_conjquad<double>(res, arg, count, interleaved, ptr, val, fallback_counter, stop_dev, stream);
}
}  // extern "C"
