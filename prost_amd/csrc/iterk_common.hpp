// iterk_common.hpp -- what the two files of the K-iteration kernels share: kernels_fused_iterk.hip (the single-wave pipeline and the
// host side) and kernels_fused_iterk_lw.hip (one level per wavefront, built with flags of its own: prost_amd/csrc/Makefile).
#pragma once
#include "fused_common.hpp"
#include "iterk_levelwave.hpp"

#include <type_traits>

#ifndef ITERK_NT
#define ITERK_NT true
#endif
#ifndef ITERK_LOAD_AUX
#define ITERK_LOAD_AUX 0
#endif

namespace prost_hip {

typedef int idx_t;
typedef __attribute__((address_space(3))) void lds_void_k;
typedef const __attribute__((address_space(1))) void glb_void_k;

struct LevelStep {
  float tauT, rD, step, sigS, theta, opt;       // tau T, 1 / (1 + step), step = c a^2 tau T, sigma S, theta, 1 + theta
  UniformDiv sq;                                // exact class: the divisor 1. + step of Function1DSquare and its reciprocal, in double
};
template <int K>
struct StepsK {
  LevelStep s[K];
  float tau_last, sigma_last;                   // residual transforms of the last iteration
};

template <int N> using int_c = std::integral_constant<int, N>;
template <int A, int B, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (A < B) { f(int_c<A>()); static_for<A + 1, B>(f); }
}

// one launch of the level-per-wavefront family (kernels_fused_iterk_lw.hip; K = 3 and 4): the instance for (g_fn, per-pixel b), or,
// with `place` set, the K = 4 / square / per-pixel-b instance that records where its waves ran.  Returns 0 or the error code of `fail`.
template <int K>
int launch_iterk_levelwave(int g_fn, bool b_per_pixel, int ring, dim3 grid, hipStream_t s, float* x_out, float* y_out, const float* x, const float* y,
                           const FusedArgs<float>& a, const StepsK<K>& sp, const PdhgRecord<float>* rec, unsigned* place);

}  // namespace prost_hip
