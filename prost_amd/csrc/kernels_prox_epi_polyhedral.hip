// kernels_prox_epi_polyhedral.hip -- ProxIndEpiPolyhedral: the projection of (x_1 .. x_d, y) onto the epigraph of a max-affine
// function, y >= max_i <a_i, x> - b_i, one small quadratic program per group.  The reference ships no kernel for it (its users
// bolt one on); the arithmetic is include/prost/prox/epi_polyhedral.hpp, a dual active-set projection that also runs on the host
// (tests/host/epi_polyhedral_harness.cpp).  This file decides which lane reads which constraint and keeps the step loop uniform.
//
// G = lanes_per_group lanes share a group (a power of two from prost_hip_epi_polyhedral_plan, chosen from the longest constraint
// list of the prox; sub-groups are aligned inside a wave).  One step:
//   scan    lane l looks at constraints l, l + G, ..: adjacent lanes read adjacent constraints.  The lists are re-read every step
//           (they come from L1 / L2 after the first; keeping a share in registers would cost 4 (d + 1) registers of a budget
//           the DIM = 4 double instance already fills).
//   argmax  (violation, index) through __shfl_xor over the G lanes, ties to the lower index; the index is then taken from the
//           sub-group's first lane, so that every lane of a group holds the same state whatever the data
//   solve   every lane loads the chosen constraint (one address per group) and runs ActiveSet::Step redundantly; when the scan
//           finds nothing, ActiveSet::Polish once, and one more scan
// The loop is `while (__any(!done))`: every shuffle executes with all 64 lanes in the loop, finished groups idle through
// predicated bodies.  Work is bounded: a group stops after StepCap(k, DIM) steps, writes the feasible point (x0, max(y0, max_i
// <a_i, x0> - b_i)) and counts itself in *fallback_counter.  k is clamped to max_count, so the bound holds for any cnt array.
// No LDS, no scratch (resource table: docs/rounds/r14.md).
#include "common.hpp"
#include "prost/prox/epi_polyhedral.hpp"

#include <limits>

namespace prost_hip {

namespace ep = prost::epi;

template <class T, int DIM>
__global__ void __launch_bounds__(kBlock) epi_polyhedral_kernel(T* res, const T* arg, size_t count, bool interleaved, const T* __restrict__ a,
                                                               const T* __restrict__ b, const int32_t* __restrict__ cnt,
                                                               const int32_t* __restrict__ idx, int max_count, int lanes_log2,
                                                               unsigned* fallback_counter) {
  constexpr int D = DIM - 1;
  const int G = 1 << lanes_log2;
  const size_t t = (size_t)blockIdx.x * kBlock + threadIdx.x;
  const size_t g = t >> lanes_log2;
  const int sub = (int)(t & (size_t)(G - 1));
  const int lane = (int)(threadIdx.x & (kWave - 1));
  const bool live = g < count;

  int k = 0;
  size_t s0 = 0;
  T z0[DIM];
#pragma unroll
  for (int j = 0; j < DIM; j++) z0[j] = 0;
  if (live) {
    k = cnt[g];
    k = k < 0 ? 0 : (k > max_count ? max_count : k);
    s0 = (size_t)idx[g];
#pragma unroll
    for (int j = 0; j < DIM; j++) z0[j] = interleaved ? arg[g * DIM + j] : arg[g + count * j];
  }
  ep::ActiveSet<T, DIM> st;
  st.Init(z0);
  const int cap = ep::StepCap(k, DIM);
  bool done = !live || k == 0, capped = false;
  const T lowest = -std::numeric_limits<T>::infinity();

  while (__any(!done)) {
    T bv = lowest;
    int bi = -1;
    if (!done && !st.pending) {
      for (int i = sub; i < k; i += G) {
        T ai[D], v;
#pragma unroll
        for (int j = 0; j < D; j++) ai[j] = a[(s0 + i) * D + j];
        if (ep::Violation<T, DIM>(st.z, ai, b[s0 + i], v) && v > bv) { bv = v; bi = i; }
      }
    }
    for (int off = G >> 1; off > 0; off >>= 1) {
      const T ov = __shfl_xor(bv, off);
      const int oi = __shfl_xor(bi, off);
      if (oi >= 0 && (bi < 0 || ov > bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
    }
    bi = __shfl(bi, lane & ~(G - 1));
    if (!done) {
      if (!st.pending) {
        if (bi < 0) done = st.polished || !st.Polish();           // the polished point is scanned once more
        else {
          T ai[D];
#pragma unroll
          for (int j = 0; j < D; j++) ai[j] = a[(s0 + bi) * D + j];
          st.Begin(ai, b[s0 + bi]);
        }
      }
      if (!done && st.pending) {
        if (st.steps >= cap) { capped = true; done = true; }
        else if (st.Step() == ep::kStuck) { capped = true; done = true; }
      }
    }
  }

  if (__any(capped)) {
    T worst = lowest;
    if (capped) {
      for (int i = sub; i < k; i += G) {
        T s = 0;
#pragma unroll
        for (int j = 0; j < D; j++) s += a[(s0 + i) * D + j] * z0[j];
        s -= b[s0 + i];
        worst = s > worst ? s : worst;
      }
    }
    for (int off = G >> 1; off > 0; off >>= 1) {
      const T o = __shfl_xor(worst, off);
      worst = o > worst ? o : worst;
    }
    if (capped) {
      ep::Fallback<T, DIM>(z0, worst, st.z);
      if (sub == 0 && fallback_counter) atomicAdd(fallback_counter, 1u);
    }
  }

  if (live && sub == 0) {
#pragma unroll
    for (int j = 0; j < DIM; j++) {
      if (interleaved) res[g * DIM + j] = st.z[j];
      else res[g + count * j] = st.z[j];
    }
  }
}

static bool epi_plan(size_t max_count, size_t dim, int& lanes) {
  if (dim < (size_t)ep::kMinDim || dim > (size_t)ep::kMaxDim || max_count >= ((size_t)1 << 31)) return false;
  lanes = ep::LanesPerGroup(max_count);
  return true;
}

template <class T>
static int launch_epi_polyhedral(T* res, const T* arg, size_t count, size_t dim, int interleaved, const T* a, const T* b, const int32_t* cnt,
                                 const int32_t* idx, size_t max_count, unsigned* fallback_counter, void* stream) {
  int lanes = 1;
  if (!epi_plan(max_count, dim, lanes)) { set_error("prox_ind_epi_polyhedral: dim has to be between 2 and 4 and max_count below 2^31"); return 1; }
  if (count == 0) return 0;
  if (count >= ((size_t)1 << 31)) { set_error("prox_ind_epi_polyhedral: count has to be below 2^31"); return 1; }
  if (!res || !arg || !cnt || !idx || (max_count > 0 && (!a || !b))) { set_error("prox_ind_epi_polyhedral: null pointer"); return 1; }
  int lanes_log2 = 0;
  while ((1 << lanes_log2) < lanes) lanes_log2++;
  const size_t blocks = (count * (size_t)lanes + kBlock - 1) / kBlock;       // < 2^31 * 64 / 256
  hipStream_t s = as_stream(stream);
  const dim3 grid((unsigned)blocks), block(kBlock);
  const bool il = interleaved != 0;
  const int mc = (int)max_count;
  if (dim == 2) PH_LAUNCH((epi_polyhedral_kernel<T, 2>), grid, block, 0, s, res, arg, count, il, a, b, cnt, idx, mc, lanes_log2, fallback_counter);
  else if (dim == 3) PH_LAUNCH((epi_polyhedral_kernel<T, 3>), grid, block, 0, s, res, arg, count, il, a, b, cnt, idx, mc, lanes_log2, fallback_counter);
  else PH_LAUNCH((epi_polyhedral_kernel<T, 4>), grid, block, 0, s, res, arg, count, il, a, b, cnt, idx, mc, lanes_log2, fallback_counter);
  PH_LAUNCH_END("ind_epi_polyhedral kernel");
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_epi_polyhedral_plan(size_t max_count, size_t dim, int dtype, int* lanes_per_group, int* step_cap_a, int* step_cap_b) {
  if (dtype != 0 && dtype != 1) { set_error("epi_polyhedral_plan: dtype is 0 (fp32) or 1 (fp64)"); return 1; }
  int lanes = 1;
  if (!epi_plan(max_count, dim, lanes)) { set_error("epi_polyhedral_plan: dim has to be between 2 and 4 and max_count below 2^31"); return 1; }
  if (lanes_per_group) *lanes_per_group = lanes;
  if (step_cap_a) *step_cap_a = ep::kStepCapA;
  if (step_cap_b) *step_cap_b = ep::kStepCapB;
  return 0;
}
int prost_hip_prox_ind_epi_polyhedral_f32(float* res, const float* arg, size_t count, size_t dim, int interleaved, const float* a, const float* b,
                                          const int32_t* cnt, const int32_t* idx, size_t max_count, unsigned* fallback_counter, void* stream) {
  return launch_epi_polyhedral<float>(res, arg, count, dim, interleaved, a, b, cnt, idx, max_count, fallback_counter, stream);
}
int prost_hip_prox_ind_epi_polyhedral_f64(double* res, const double* arg, size_t count, size_t dim, int interleaved, const double* a, const double* b,
                                          const int32_t* cnt, const int32_t* idx, size_t max_count, unsigned* fallback_counter, void* stream) {
  return launch_epi_polyhedral<double>(res, arg, count, dim, interleaved, a, b, cnt, idx, max_count, fallback_counter, stream);
}
}  // extern "C"
