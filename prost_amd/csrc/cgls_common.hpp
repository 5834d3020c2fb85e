// cgls_common.hpp -- what the CGLS kernel files share: the device record of the CG scalars, the partial-sum regions of the
// workspace and the scalars a round kernel takes (kernels_cgls.hip: staged rounds, rounds with the operator inside, ADMM and normest
// stages; kernels_cgls_pixel.hip: the two-launch pixel rounds).
#pragma once
#include "reduce.hpp"

namespace prost_hip {

struct CgState {
  double gamma, norms0, norms, normx, xmax, alpha, neg_alpha, beta;
  double tol;                      // stopping tolerance and epoch of the current solve: set by INIT_X, so that the
  int epoch;                       // STEP launches take no per-solve argument (they can be replayed from a HIP graph)
  int done, k, indefinite, flag;
};

enum { kRegionX = 0, kRegionS, kRegionP, kRegionQ, kRegions };          // partial-sum regions of the workspace
// a region holds one slot per workgroup: (hi, lo) of ONE sum, compact (stride 2: kernels with a single sum), or
// (a.hi, a.lo, b.hi, b.lo) (stride 4: the staged kernels and the residual stages, which carry two sums) -- reduce.hpp, dd_t
__host__ __device__ inline double* region(double* ws, int r) { return ws + (size_t)r * 4 * kReduceBlocks; }

struct RoundScalars { double shift, eps; unsigned g_a, g_b; int* host_done; };

}  // namespace prost_hip
