// prox_spectral.hpp -- what the two kernel files of the spectral proxes share (kernels_prox_spectral.hip: one group per lane;
// kernels_prox_eigen_nxn.hip: several lanes per matrix): the kernel argument block, the step / stop-word read, the scalar function
// as a run-time id, and the launch geometry of the cooperative kernel.
#pragma once
#include "common.hpp"
#include "device_math.hpp"

namespace prost_hip {

/// the scalar function as a run-time id: one scalar branch per wavefront (fn is a kernel argument)
struct RtFun1D {
  int fn;
  __device__ __forceinline__ double operator()(double x0, double tau, double alpha, double beta) const { return f1d_apply<double>(fn, x0, tau, alpha, beta); }
};

template <class T>
struct SpectralArgs {
  T* res; const T* arg; const T* tau_diag;
  T tau; const T* step; const int* stop;       // step != null: the scalar step is *step, and *stop != 0 ends the kernel
  bool invert_tau;
  size_t count;
  int fn;
  const T* cp[7]; T cv[7];                     // per-group coefficient vectors (or null) and the scalar values
};

template <class T, int N> struct alignas(sizeof(T) * N) SpPack { T v[N]; };

template <class T>
__device__ __forceinline__ bool spectral_step(const SpectralArgs<T>& p, T& tau) {
  tau = p.tau;
  if (p.step == nullptr) return true;
  if (*p.stop != 0) return false;
  tau = *p.step;
  return true;
}

/// Geometry of the cooperative eigen_nxn kernel for an n x n matrix (6 <= n <= 32; the launcher uses it for n >= kEigenCoopMinN).
/// m = n rounded up to even (an odd n plays with a bye); `lanes` lanes own one matrix: the smallest power of two that holds the
/// (m/2)^2 blocks of a round, between 16 and 64; 256 / lanes matrices per workgroup; A and V^T as m x m doubles each in LDS.
/// n = 32: 64 lanes, 4 matrices, 4 * 2 * 32 * 32 * 8 = 64 KiB -- there is no room for anything else, which is why the rotations
/// of a round travel between lanes through cross-lane reads, not through LDS.
struct EigenCoopPlan { int m, lanes, matrices; size_t lds_bytes; };
inline EigenCoopPlan eigen_coop_plan(int n) {
  EigenCoopPlan g;
  g.m = n + (n & 1);
  const int blocks = (g.m / 2) * (g.m / 2);
  g.lanes = 16;
  while (g.lanes < blocks && g.lanes < 64) g.lanes *= 2;
  g.matrices = kBlock / g.lanes;
  g.lds_bytes = (size_t)g.matrices * 2 * g.m * g.m * sizeof(double);
  return g;
}
constexpr int kEigenCoopMinN = 6;              // below: one matrix per lane in registers (kernels_prox_spectral.hip)

/// defined in kernels_prox_eigen_nxn.hip; p is complete, n in [kEigenCoopMinN, 32]
template <class T> int launch_eigen_nxn_coop(const SpectralArgs<T>& p, int n, bool interleaved, hipStream_t s);

}  // namespace prost_hip
