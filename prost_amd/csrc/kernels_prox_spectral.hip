// kernels_prox_spectral.hip -- the spectral proxes: functions of the singular values of an n x 2 matrix
// (elem_operation:singular_nx2:*) and of the eigenvalues of a symmetric 2x2 / 3x3 matrix (elem_operation:eigen_2x2:*,
// elem_operation:eigen_3x3:*).  The arithmetic is the public functor surface (include/prost/prox/elemop/
// elem_operation_singular_nx2.hpp, _eigen_2x2.hpp, _eigen_3x3.hpp over spectral_common.hpp); this file is the gfx950 kernel
// around it and the C ABI entry points prost_hip_prox_spectral_f32 / _f64.
//
// The generic functor kernel (prox_elem_operation.inl) keeps a group in registers up to 8 components; a 3x3 matrix has 9
// and would run one group per lane over HBM, reading every component twice.  Here:
//   * one group per lane, the WHOLE group in registers (DIM is a template argument: 2, 4, 6, 8, 10, 12 for singular_nx2,
//     4 and 9 for the eigen operations), the decomposition in fp64 registers, the scalar function a wave-uniform switch;
//   * planar layout: component i of 64 consecutive groups is 64 consecutive values -- every load and store instruction of a
//     wavefront is one contiguous 256-byte (fp32) / 512-byte (fp64) run;
//   * interleaved layout: the 256 groups of a workgroup are ONE contiguous run of 256 * DIM values.  It moves between HBM and
//     an LDS tile in 16-byte accesses per lane (1 KiB per wavefront instruction), and every lane picks its group out of the
//     tile -- a 36-byte stride per lane straight from HBM would fetch every cache line nine times over;
//   * only tau_diag[first component of the group] is read (diagsteps = false: the preconditioner is constant over a group);
//   * the step is a host value or, inside a batch of iterations whose step-size rule runs on the device, a device scalar
//     next to a stop word (Prox::StepView): a raised stop word ends the kernel before it touches the result.
// singular_nx2 with dim > 12 streams the group twice over HBM (once for M^T M, once for the product), one group per lane.
// No device synchronisation; launch-configuration errors surface through hipGetLastError.
#include "prox_spectral.hpp"
#include "prost/prox/elemop/elem_operation_eigen_2x2.hpp"
#include "prost/prox/elemop/elem_operation_eigen_3x3.hpp"
#include "prost/prox/elemop/elem_operation_eigen_nxn.hpp"
#include "prost/prox/elemop/elem_operation_mass_norm.hpp"
#include "prost/prox/elemop/elem_operation_singular_nx2.hpp"

namespace prost_hip {

struct RtFun2D {
  int fn;
  __device__ __forceinline__ void operator()(double y1, double y2, double& x1, double& x2, double tau, double alpha, double beta) const {
    if (fn == PROST_FN2D_IND_L1_BALL) prost::Function2DIndL1Ball<double>()(y1, y2, x1, x2, tau, alpha, beta);
    else if (fn == PROST_FN2D_MOREAU_IND_L1_BALL) prost::Function2DMoreau<double, prost::Function2DIndL1Ball<double>>()(y1, y2, x1, x2, tau, alpha, beta);
    else {
      x1 = f1d_apply<double>(fn, y1, tau, alpha, beta);
      x2 = f1d_apply<double>(fn, y2, tau, alpha, beta);
    }
  }
};

template <class T, int OP, int DIM>
__device__ __forceinline__ void spectral_apply(T (&r)[DIM], const T (&a)[DIM], double tau, const T* c, int fn) {
  if constexpr (OP == PROST_SPECTRAL_SINGULAR_NX2) prost::elemop::SingularNx2Apply<T, double>(r, a, (size_t)(DIM / 2), tau, c, RtFun2D{fn});
  else if constexpr (OP == PROST_SPECTRAL_EIGEN_2X2) prost::elemop::Eigen2x2Apply<T>(r, a, tau, c, RtFun1D{fn});
  else if constexpr (OP == PROST_SPECTRAL_EIGEN_3X3) prost::elemop::Eigen3x3Apply<T>(r, a, tau, c, RtFun1D{fn});
  else if constexpr (OP == PROST_SPECTRAL_EIGEN_NXN) {
    // a symmetrised matrix and a symmetric result read the same row by row and column by column: n = 2, 3 are the existing operations
    if constexpr (DIM == 4) prost::elemop::Eigen2x2Apply<T>(r, a, tau, c, RtFun1D{fn});
    else if constexpr (DIM == 9) prost::elemop::Eigen3x3Apply<T>(r, a, tau, c, RtFun1D{fn});
    else prost::elemop::EigenNApply<T, DIM == 1 ? 1 : DIM == 16 ? 4 : 5>(r, a, tau, c, RtFun1D{fn});
  } else if constexpr (OP == PROST_SPECTRAL_MASS4) prost::elemop::MassNormApply<T, 4, false>(r, a, tau);
  else if constexpr (OP == PROST_SPECTRAL_IND_COMASS4_BALL) prost::elemop::MassNormApply<T, 4, true>(r, a, tau);
  else if constexpr (OP == PROST_SPECTRAL_MASS5) prost::elemop::MassNormApply<T, 5, false>(r, a, tau);
  else prost::elemop::MassNormApply<T, 5, true>(r, a, tau);
}

/// the scalar step of a group: for the mass operations the cost (coefficient 0) is a weight on it, multiplied in T
template <class T, int OP>
__device__ __forceinline__ T spectral_group_tau(T tau_scal, const T* c) {
  if constexpr (OP >= PROST_SPECTRAL_MASS4) return tau_scal * c[0];
  else return tau_scal;
}

// 256 * DIM contiguous values between HBM and the LDS tile of a workgroup; `valid` of them exist (the last workgroup).
// 16 bytes per lane and access where the HBM side is 16-byte aligned (a workgroup's run starts a multiple of 16 bytes behind the operand)
template <class T, int DIM, bool LOAD>
__device__ __forceinline__ void spectral_tile_copy(T* tile, T* hbm, size_t valid) {
  constexpr int V = 16 / (int)sizeof(T);
  const bool wide = (reinterpret_cast<uintptr_t>(hbm) & 15u) == 0;
  constexpr int kTrips = (DIM + V - 1) / V, kUnroll = DIM > 12 ? 1 : kTrips;      // the 4x4 / 5x5 tiles: a rolled loop, fewer scalar registers
#pragma unroll kUnroll
  for (int it = 0; it < kTrips; it++) {
    const int i = (it * kBlock + (int)threadIdx.x) * V;
    if (i >= kBlock * DIM) continue;
    if (wide && (size_t)(i + V) <= valid) {
      if (LOAD) *reinterpret_cast<SpPack<T, V>*>(tile + i) = *reinterpret_cast<const SpPack<T, V>*>(hbm + i);
      else *reinterpret_cast<SpPack<T, V>*>(hbm + i) = *reinterpret_cast<const SpPack<T, V>*>(tile + i);
    } else {
#pragma unroll
      for (int j = 0; j < V; j++)
        if ((size_t)(i + j) < valid) { if (LOAD) tile[i + j] = hbm[i + j]; else hbm[i + j] = tile[i + j]; }
    }
  }
}

template <class T, int OP, int DIM, bool INTERLEAVED>
__global__ void __launch_bounds__(kBlock) spectral_kernel(SpectralArgs<T> p) {
  T tau_scal;
  if (!spectral_step(p, tau_scal)) return;                 // the same in every lane of the grid
  const size_t g0 = (size_t)blockIdx.x * kBlock, g = g0 + threadIdx.x;
  const bool live = g < p.count;
  T a[DIM], r[DIM];
  if constexpr (INTERLEAVED) {
    __shared__ alignas(16) T tile[kBlock * DIM];
    const size_t valid = (p.count - g0 < (size_t)kBlock ? p.count - g0 : (size_t)kBlock) * DIM;
    spectral_tile_copy<T, DIM, true>(tile, const_cast<T*>(p.arg) + g0 * DIM, valid);
    __syncthreads();
    if (live) {
#pragma unroll
      for (int k = 0; k < DIM; k++) a[k] = tile[threadIdx.x * DIM + k];
      T c[7];
#pragma unroll
      for (int k = 0; k < 7; k++) c[k] = p.cp[k] != nullptr ? p.cp[k][g] : p.cv[k];
      spectral_apply<T, OP, DIM>(r, a, prost::elemop::SpectralStep(spectral_group_tau<T, OP>(tau_scal, c), p.tau_diag[g * DIM], p.invert_tau), c, p.fn);
#pragma unroll
      for (int k = 0; k < DIM; k++) tile[threadIdx.x * DIM + k] = r[k];      // a lane overwrites the slots it has read itself
    }
    __syncthreads();
    spectral_tile_copy<T, DIM, false>(tile, p.res + g0 * DIM, valid);
  } else {
    if (!live) return;
    if constexpr (DIM > 12) {
      // 25 component offsets k * count kept as wave-uniform 64-bit values would not fit the scalar registers: the address walks in the lane
      const T* ap = p.arg + g;
#pragma unroll
      for (int k = 0; k < DIM; k++) { a[k] = *ap; ap += p.count; asm volatile("" : "+v"(ap)); }
    } else {
#pragma unroll
      for (int k = 0; k < DIM; k++) a[k] = p.arg[g + p.count * k];
    }
    T c[7];
#pragma unroll
    for (int k = 0; k < 7; k++) c[k] = p.cp[k] != nullptr ? p.cp[k][g] : p.cv[k];
    spectral_apply<T, OP, DIM>(r, a, prost::elemop::SpectralStep(spectral_group_tau<T, OP>(tau_scal, c), p.tau_diag[g], p.invert_tau), c, p.fn);
    if constexpr (DIM > 12) {
      T* rp = p.res + g;
#pragma unroll
      for (int k = 0; k < DIM; k++) { *rp = r[k]; rp += p.count; asm volatile("" : "+v"(rp)); }
    } else {
#pragma unroll
      for (int k = 0; k < DIM; k++) p.res[g + p.count * k] = r[k];
    }
  }
}

// singular_nx2 of any even dim: one group per lane, views over HBM, the group read twice
template <class T>
__global__ void __launch_bounds__(kBlock) spectral_nx2_stream_kernel(SpectralArgs<T> p, size_t dim, bool interleaved) {
  T tau_scal;
  if (!spectral_step(p, tau_scal)) return;
  const size_t g = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (g >= p.count) return;
  prost::Vector<T> res(p.count, dim, interleaved, g, p.res);
  const prost::Vector<const T> arg(p.count, dim, interleaved, g, p.arg);
  T c[7];
#pragma unroll
  for (int k = 0; k < 7; k++) c[k] = p.cp[k] != nullptr ? p.cp[k][g] : p.cv[k];
  prost::elemop::SingularNx2Apply<T, double>(res, arg, dim / 2, prost::elemop::SpectralStep(tau_scal, p.tau_diag[interleaved ? g * dim : g], p.invert_tau), c, RtFun2D{p.fn});
}

template <class T, int OP, int DIM>
static void launch_instance(const SpectralArgs<T>& p, bool interleaved, unsigned grid, hipStream_t s) {
  if (interleaved) hipLaunchKernelGGL((spectral_kernel<T, OP, DIM, true>), dim3(grid), dim3(kBlock), 0, s, p);
  else hipLaunchKernelGGL((spectral_kernel<T, OP, DIM, false>), dim3(grid), dim3(kBlock), 0, s, p);
}

template <class T>
static int launch_spectral(int op, int fn, T* res, const T* arg, const T* tau_diag, double tau, const T* step_dev, const int* stop_dev, int invert_tau,
                           size_t count, size_t dim, int interleaved, const T* const* coeff_ptr, const double* coeff_val, void* stream) {
  const bool fn1d = fn >= 0 && fn < PROST_FN_COUNT;
  const bool fn2d = fn == PROST_FN2D_IND_L1_BALL || fn == PROST_FN2D_MOREAU_IND_L1_BALL;
  int n_side = 0;
  if (op == PROST_SPECTRAL_SINGULAR_NX2) {
    if (!(fn1d || fn2d)) { set_error("prox_spectral: unknown function id"); return 1; }
    if (dim == 0 || dim % 2 != 0) { set_error("prox_spectral: singular_nx2 needs an even dim"); return 1; }
  } else if (op == PROST_SPECTRAL_EIGEN_2X2 || op == PROST_SPECTRAL_EIGEN_3X3) {
    if (!fn1d) { set_error("prox_spectral: unknown function id"); return 1; }
    if (dim != (op == PROST_SPECTRAL_EIGEN_2X2 ? 4u : 9u)) { set_error("prox_spectral: eigen_2x2 needs dim 4, eigen_3x3 dim 9"); return 1; }
  } else if (op == PROST_SPECTRAL_EIGEN_NXN) {
    if (!fn1d) { set_error("prox_spectral: unknown function id"); return 1; }
    n_side = prost::elemop::EigenNxNSide(dim);
    if (n_side < 1 || n_side > prost::elemop::kEigenNxNMax) { set_error("prox_spectral: eigen_nxn needs dim = n * n with 1 <= n <= 32"); return 1; }
  } else if (op == PROST_SPECTRAL_MASS4 || op == PROST_SPECTRAL_IND_COMASS4_BALL) {
    if (dim != 6) { set_error("prox_spectral: mass4 and ind_comass4_ball need dim 6"); return 1; }
  } else if (op == PROST_SPECTRAL_MASS5 || op == PROST_SPECTRAL_IND_COMASS5_BALL) {
    if (dim != 10) { set_error("prox_spectral: mass5 and ind_comass5_ball need dim 10"); return 1; }
  } else { set_error("prox_spectral: unknown operation id"); return 1; }
  if ((step_dev == nullptr) != (stop_dev == nullptr)) { set_error("prox_spectral: the device step and the stop word come together"); return 1; }
  if (count == 0) return 0;
  const size_t blocks = (count + kBlock - 1) / kBlock;
  if (blocks > 0x7FFFFFFFu) { set_error("prox_spectral: too many groups for one launch"); return 1; }
  SpectralArgs<T> p;
  p.res = res; p.arg = arg; p.tau_diag = tau_diag;
  p.tau = (T)tau; p.step = step_dev; p.stop = stop_dev;
  p.invert_tau = invert_tau != 0;
  p.count = count; p.fn = fn;
  for (int k = 0; k < 7; k++) { p.cp[k] = coeff_ptr ? coeff_ptr[k] : nullptr; p.cv[k] = (T)coeff_val[k]; }
  const unsigned grid = (unsigned)blocks;
  hipStream_t s = as_stream(stream);
  const bool il = interleaved != 0;
  if (op == PROST_SPECTRAL_EIGEN_2X2) launch_instance<T, PROST_SPECTRAL_EIGEN_2X2, 4>(p, il, grid, s);
  else if (op == PROST_SPECTRAL_EIGEN_3X3) launch_instance<T, PROST_SPECTRAL_EIGEN_3X3, 9>(p, il, grid, s);
  else if (op == PROST_SPECTRAL_EIGEN_NXN) {
    if (n_side >= kEigenCoopMinN) return launch_eigen_nxn_coop<T>(p, n_side, il, s);         // several lanes per matrix, A and V^T in LDS
    switch (n_side) {
      case 1: launch_instance<T, PROST_SPECTRAL_EIGEN_NXN, 1>(p, il, grid, s); break;
      case 2: launch_instance<T, PROST_SPECTRAL_EIGEN_NXN, 4>(p, il, grid, s); break;
      case 3: launch_instance<T, PROST_SPECTRAL_EIGEN_NXN, 9>(p, il, grid, s); break;
      case 4: launch_instance<T, PROST_SPECTRAL_EIGEN_NXN, 16>(p, il, grid, s); break;
      default: launch_instance<T, PROST_SPECTRAL_EIGEN_NXN, 25>(p, il, grid, s); break;
    }
  }
  else if (op == PROST_SPECTRAL_MASS4) launch_instance<T, PROST_SPECTRAL_MASS4, 6>(p, il, grid, s);
  else if (op == PROST_SPECTRAL_IND_COMASS4_BALL) launch_instance<T, PROST_SPECTRAL_IND_COMASS4_BALL, 6>(p, il, grid, s);
  else if (op == PROST_SPECTRAL_MASS5) launch_instance<T, PROST_SPECTRAL_MASS5, 10>(p, il, grid, s);
  else if (op == PROST_SPECTRAL_IND_COMASS5_BALL) launch_instance<T, PROST_SPECTRAL_IND_COMASS5_BALL, 10>(p, il, grid, s);
  else switch (dim) {
    case 2: launch_instance<T, PROST_SPECTRAL_SINGULAR_NX2, 2>(p, il, grid, s); break;
    case 4: launch_instance<T, PROST_SPECTRAL_SINGULAR_NX2, 4>(p, il, grid, s); break;
    case 6: launch_instance<T, PROST_SPECTRAL_SINGULAR_NX2, 6>(p, il, grid, s); break;
    case 8: launch_instance<T, PROST_SPECTRAL_SINGULAR_NX2, 8>(p, il, grid, s); break;
    case 10: launch_instance<T, PROST_SPECTRAL_SINGULAR_NX2, 10>(p, il, grid, s); break;
    case 12: launch_instance<T, PROST_SPECTRAL_SINGULAR_NX2, 12>(p, il, grid, s); break;
    default: hipLaunchKernelGGL((spectral_nx2_stream_kernel<T>), dim3(grid), dim3(kBlock), 0, s, p, dim, il); break;
  }
  PH_LAUNCH_END("prox_spectral kernel");
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_prox_spectral_f32(int op, int fn, float* res, const float* arg, const float* tau_diag, double tau, const float* step_dev, const int* stop_dev,
                                int invert_tau, size_t count, size_t dim, int interleaved, const float* const* coeff_ptr, const double* coeff_val, void* stream) {
  return launch_spectral<float>(op, fn, res, arg, tau_diag, tau, step_dev, stop_dev, invert_tau, count, dim, interleaved, coeff_ptr, coeff_val, stream);
}
int prost_hip_prox_spectral_f64(int op, int fn, double* res, const double* arg, const double* tau_diag, double tau, const double* step_dev, const int* stop_dev,
                                int invert_tau, size_t count, size_t dim, int interleaved, const double* const* coeff_ptr, const double* coeff_val, void* stream) {
  return launch_spectral<double>(op, fn, res, arg, tau_diag, tau, step_dev, stop_dev, invert_tau, count, dim, interleaved, coeff_ptr, coeff_val, stream);
}
int prost_hip_prox_eigen_nxn_plan(size_t n, int dtype, int* lanes_per_matrix, int* matrices_per_workgroup, size_t* lds_bytes) {
  if (n < 1 || n > (size_t)prost::elemop::kEigenNxNMax) { set_error("prox_eigen_nxn_plan: n has to be in 1..32"); return 1; }
  if (dtype != 0 && dtype != 1) { set_error("prox_eigen_nxn_plan: dtype is 0 (fp32) or 1 (fp64)"); return 1; }
  int lanes = 1, matrices = kBlock;
  size_t lds = (size_t)kBlock * n * n * (dtype == 0 ? sizeof(float) : sizeof(double));        // the tile of the interleaved layout
  if ((int)n >= kEigenCoopMinN) {
    const EigenCoopPlan g = eigen_coop_plan((int)n);
    lanes = g.lanes; matrices = g.matrices; lds = g.lds_bytes;
  }
  if (lanes_per_matrix) *lanes_per_matrix = lanes;
  if (matrices_per_workgroup) *matrices_per_workgroup = matrices;
  if (lds_bytes) *lds_bytes = lds;
  return 0;
}
}  // extern "C"
