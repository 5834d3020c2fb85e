// kernels_prox_range.hip -- the dense solve of ProxIndRange (reference: src/prox/prox_ind_range.cu, cusolverDn<t>potrf / potrs):
// a blocked Cholesky factorisation of the n x n matrix A'A, run once, and L L' z = t for one right-hand side, run per evaluation.
// The per-block arithmetic is include/prost/prox/potrs_blocks.hpp (host and device templates, run on the host by
// tests/host/potrs_blocks_harness.cpp); this file decides which lane runs which row and where the barriers stand.
//
// Factorisation (prost_hip_range_potrf_*): fp64 for both data types -- T = double in place, T = float on a copy in the workspace --
// right-looking, block columns of kNB = 64, three launches per block column:
//   diag      one 64-lane workgroup, the block in LDS: unblocked Cholesky (a lane per row), then the inverse of the block in place;
//             the inverse and its transpose go to the side array `dinv` as T (zero-padded to 64 x 64), and as fp64 to the workspace
//   panel     a lane per row below the block: the row times the transposed inverse
//   trailing  64 x 64 tiles of the lower triangle to the right, 16 entries per lane
// A pivot that is not a positive finite number stores its index in *status (preset to -1 by the first launch) and every later
// launch returns at once: nothing waits, nothing loops.  The last launch writes L (upper triangle zero) and U = L' as T.
//
// Solve (prost_hip_range_potrs_*), all arithmetic in T.  Block step k of a sweep: z_k = Dinv_k r_k (a 64 x 64 product: four partial
// sums per row, added in a fixed order), then every remaining row i loses M[i, block k] z_k, again as four partial sums of 16 columns.
// The forward sweep reads L downwards, the backward sweep reads U = L' upwards: both walk a column along consecutive rows, so the
// lanes of a wave read consecutive addresses.  Two tiers (prost_hip_range_potrs_plan):
//   small (n <= 512 in fp32, 320 in fp64: measured)  one launch, one workgroup of 1024 lanes, the vector in LDS, barriers between block steps, both sweeps
//   large              one launch per block step, 64 rows per workgroup.  EVERY workgroup recomputes z_k from the inverted block
//                      (16 / 32 KiB, from L2) and updates its own rows; workgroup 0 stores z_k.  The forward sweep consumes v and
//                      stores the solved blocks to the workspace, the backward sweep consumes the workspace and stores to v, so no
//                      launch reads an entry that the same launch writes from another workgroup.
// No workgroup waits for another inside a launch: no flags, no counters, no atomics; every dependency is a kernel boundary.  The
// summation order depends on (n, tier) only, so a repeated call repeats its bits.
#include "common.hpp"
#include "prost/prox/potrs_blocks.hpp"

namespace prost_hip {

namespace pb = prost::potrs;
constexpr int kNB = pb::kNB;
constexpr int kRangeSmallMaxN = 1024;        // the small tier's vector and partial sums: (1024 + 1024) * sizeof(T) of LDS
constexpr int kRangeSmallThreads = 1024;
// where the plan changes tier.  Measured (docs/rounds/r12.md §5): the small tier costs 0.028 / 0.039 ms at n = 250 and 0.305 / 0.471 ms at
// n = 1024 (fp32 / fp64: one workgroup streams n^2 values), the large tier 0.044 ms and 0.147 / 0.156 ms (4.6 - 5.5 us per launch); the
// two lines cross near n = 500 (fp32) and n = 300 (fp64).  tier = 1 may still be forced up to kRangeSmallMaxN.
constexpr int kRangeSmallPlanN32 = 512, kRangeSmallPlanN64 = 320;
static_assert(kRangeSmallMaxN % kNB == 0 && kBlock == pb::kGroups * kNB, "block geometry");

struct RangePlan { int tier, launches; size_t lds_bytes, ws_bytes; };
static bool range_plan(size_t n, size_t elem, RangePlan& p) {
  if (n < 1 || n >= ((size_t)1 << 31) / n) return false;
  const size_t nblk = pb::NumBlocks(n);
  p.ws_bytes = (nblk * kNB * elem + 15) / 16 * 16;
  if (n <= (elem == sizeof(float) ? (size_t)kRangeSmallPlanN32 : (size_t)kRangeSmallPlanN64)) { p.tier = 1; p.launches = 1; p.lds_bytes = (size_t)(kRangeSmallMaxN + kRangeSmallThreads) * elem; }
  else { p.tier = 2; p.launches = (int)(2 * nblk); p.lds_bytes = (size_t)(2 * kNB + kBlock) * elem; }
  return true;
}

// ------------------------------------------------------------------------------------------
// factorisation
// ------------------------------------------------------------------------------------------
template <class T>
__global__ void __launch_bounds__(kBlock) potrf_begin_kernel(double* W, const T* A, size_t nn, int* status, int copy) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *status = -1;
  if (copy)
    for (size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x; e < nn; e += (size_t)gridDim.x * kBlock) W[e] = (double)A[e];
}

template <class T>
__global__ void __launch_bounds__(kNB) potrf_diag_kernel(double* __restrict__ W, size_t n, size_t k, double* __restrict__ dinv_f, T* __restrict__ dinv, int* status) {
  constexpr int LD = kNB + 1;                  // odd stride: a row walk and a column walk both spread over the banks
  __shared__ double D[kNB * LD];
  __shared__ int s_ok;
  if (*status >= 0) return;                    // the same in every lane of the grid
  const int r = (int)threadIdx.x;
  const size_t c0 = k * kNB;
  const int nb = n - c0 < (size_t)kNB ? (int)(n - c0) : kNB;
  for (int c = 0; c < kNB; c++) D[r + c * LD] = (r < nb && c <= r) ? W[(c0 + r) + (c0 + c) * n] : 0.;
  __syncthreads();
  for (int j = 0; j < nb; j++) {
    if (r == j) s_ok = pb::CholPivot(D, LD, j) ? 1 : 0;
    __syncthreads();
    if (!s_ok) {                               // uniform: s_ok is next written two barriers further on
      if (r == 0) *status = (int)(c0 + j);
      return;
    }
    if (r > j && r < nb) pb::CholScaleRow(D, LD, j, r);
    __syncthreads();
    if (r > j && r < nb) pb::CholUpdateRow(D, LD, j, r);
    __syncthreads();
  }
  for (int c = 0; c < nb; c++)
    if (r < nb && c <= r) W[(c0 + r) + (c0 + c) * n] = D[r + c * LD];
  for (int j = nb - 1; j >= 0; j--) {
    const bool below = r > j && r < nb;
    const double v = below ? pb::TrtiRow(D, LD, j, r) : 0.;
    const double d = pb::TrtiDiag(D, LD, j);
    __syncthreads();                           // every row has read column j
    if (below) D[r + j * LD] = v;
    if (r == j) D[j + j * LD] = d;
    __syncthreads();
  }
  for (int c = 0; c < kNB; c++) {
    dinv_f[r + c * kNB] = D[r + c * LD];
    dinv[r + c * kNB] = (T)D[r + c * LD];
    dinv[kNB * kNB + r + c * kNB] = (T)D[c + r * LD];
  }
}

__global__ void __launch_bounds__(kBlock) potrf_panel_kernel(double* __restrict__ W, size_t n, size_t k, const double* __restrict__ dinv_f, const int* status) {
  __shared__ double Di[kNB * kNB];
  if (*status >= 0) return;
  for (int e = (int)threadIdx.x; e < kNB * kNB; e += kBlock) Di[e] = dinv_f[e];
  __syncthreads();
  const size_t c0 = k * kNB, row = c0 + kNB + (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (row >= n) return;                        // (after the only barrier)
  for (int c = kNB - 1; c >= 0; c--) W[row + (c0 + c) * n] = pb::PanelEntry(W, n, row, c0, Di, kNB, c);
}

__global__ void __launch_bounds__(kBlock) potrf_trailing_kernel(double* __restrict__ W, size_t n, size_t k, const int* status) {
  if (*status >= 0 || blockIdx.y > blockIdx.x) return;                    // tiles above the diagonal have nothing to do
  const size_t c0 = k * kNB, r0 = c0 + kNB;
  const size_t row = r0 + (size_t)blockIdx.x * kNB + (threadIdx.x & (kNB - 1));
  const size_t colb = r0 + (size_t)blockIdx.y * kNB + (size_t)(threadIdx.x / kNB) * pb::kGroup;
  if (row >= n) return;
  for (int q = 0; q < pb::kGroup; q++) {
    const size_t col = colb + q;
    if (col <= row) W[row + col * n] -= pb::TrailingDot(W, n, row, col, c0, kNB);   // reads columns c0 .. c0 + 63 only: no launch-mate writes them
  }
}

// W may be L itself (T = double): an entry is read by the lane that overwrites it
template <class T>
__global__ void __launch_bounds__(kBlock) potrf_finish_kernel(const double* W, T* L, T* __restrict__ U, size_t n, const int* status) {
  if (*status >= 0) return;
  const size_t nn = n * n;
  for (size_t e = (size_t)blockIdx.x * kBlock + threadIdx.x; e < nn; e += (size_t)gridDim.x * kBlock) {
    const size_t c = e / n, i = e - c * n;
    const double v = i >= c ? W[e] : 0.;
    L[e] = (T)v;
    U[c + i * n] = (T)v;
  }
}

static size_t potrf_workspace_bytes(size_t n, size_t elem) {
  return (size_t)kNB * kNB * sizeof(double) + (elem == sizeof(double) ? 0 : n * n * sizeof(double));
}

template <class T>
static int launch_potrf(T* L, T* U, T* dinv, void* workspace, int* status, size_t n, void* stream) {
  RangePlan p;
  if (!range_plan(n, sizeof(T), p)) { set_error("range_potrf: n has to be at least 1 with n * n < 2^31"); return 1; }
  if (!L || !U || !dinv || !workspace || !status) { set_error("range_potrf: null pointer"); return 1; }
  hipStream_t s = as_stream(stream);
  double* dinv_f = static_cast<double*>(workspace);
  constexpr bool copy = sizeof(T) != sizeof(double);
  double* W = copy ? dinv_f + kNB * kNB : reinterpret_cast<double*>(L);
  const size_t nblk = pb::NumBlocks(n);
  hipLaunchKernelGGL((potrf_begin_kernel<T>), dim3(copy ? grid_for(n * n) : 1), dim3(kBlock), 0, s, W, L, n * n, status, (int)copy);
  for (size_t k = 0; k < nblk; k++) {
    hipLaunchKernelGGL((potrf_diag_kernel<T>), dim3(1), dim3(kNB), 0, s, W, n, k, dinv_f, dinv + k * 2 * kNB * kNB, status);
    const size_t r0 = (k + 1) * kNB;
    if (r0 >= n) break;
    const size_t below = n - r0, tiles = (below + kNB - 1) / kNB;
    hipLaunchKernelGGL(potrf_panel_kernel, dim3((unsigned)((below + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, W, n, k, dinv_f, status);
    hipLaunchKernelGGL(potrf_trailing_kernel, dim3((unsigned)tiles, (unsigned)tiles), dim3(kBlock), 0, s, W, n, k, status);
  }
  hipLaunchKernelGGL((potrf_finish_kernel<T>), dim3(grid_for(n * n)), dim3(kBlock), 0, s, W, L, U, n, status);
  PH_LAUNCH_END("range_potrf kernels");
}

// ------------------------------------------------------------------------------------------
// solve
// ------------------------------------------------------------------------------------------
// z = Dk r for one inverted block (64 x 64, zero-padded): lanes 0 .. 255 form the partial sums, lanes 0 .. 63 add them.  s_z may be
// s_in: every partial sum is formed before the first barrier.
template <class T>
__device__ __forceinline__ void block_solve(const T* __restrict__ Dk, const T* s_in, T* s_z, T* s_part) {
  const int tid = (int)threadIdx.x;
  if (tid < kBlock) s_part[tid] = pb::BlockRow(Dk, (size_t)kNB, (size_t)(tid & (kNB - 1)), (size_t)0, tid / kNB, kNB, s_in);
  __syncthreads();
  if (tid < kNB) s_z[tid] = pb::Combine4(s_part[tid], s_part[kNB + tid], s_part[2 * kNB + tid], s_part[3 * kNB + tid]);
  __syncthreads();
}
// vec[i] -= M[i, col0 .. col0 + nb) z for the rows r0 <= i < r1, THREADS / 4 rows per pass.  The trip count is the same in every lane.
template <class T, int THREADS>
__device__ __forceinline__ void rows_update(const T* __restrict__ M, size_t n, size_t col0, int nb, size_t r0, size_t r1, T* vec, const T* s_z, T* s_part) {
  constexpr int RP = THREADS / pb::kGroups;
  const int rl = (int)threadIdx.x % RP, g = (int)threadIdx.x / RP;
  for (size_t base = r0; base < r1; base += RP) {
    const size_t i = base + rl;
    s_part[g * RP + rl] = i < r1 ? pb::BlockRow(M, n, i, col0, g, nb, s_z) : (T)0;
    __syncthreads();
    if (g == 0 && i < r1) vec[i] = vec[i] - pb::Combine4(s_part[rl], s_part[RP + rl], s_part[2 * RP + rl], s_part[3 * RP + rl]);
    __syncthreads();
  }
}

template <class T>
__global__ void __launch_bounds__(kRangeSmallThreads) potrs_small_kernel(T* __restrict__ v, const T* __restrict__ L, const T* __restrict__ U, const T* __restrict__ dinv, size_t n) {
  __shared__ T s_vec[kRangeSmallMaxN];
  __shared__ T s_part[kRangeSmallThreads];
  const size_t nblk = pb::NumBlocks(n);        // n <= kRangeSmallMaxN (checked at the launch): nblk * kNB <= kRangeSmallMaxN
  for (size_t i = threadIdx.x; i < nblk * kNB; i += kRangeSmallThreads) s_vec[i] = i < n ? v[i] : (T)0;
  __syncthreads();
  for (size_t k = 0; k < nblk; k++) {
    const size_t c0 = k * kNB;
    const int nb = n - c0 < (size_t)kNB ? (int)(n - c0) : kNB;
    block_solve<T>(dinv + k * 2 * kNB * kNB, s_vec + c0, s_vec + c0, s_part);
    rows_update<T, kRangeSmallThreads>(L, n, c0, nb, c0 + kNB, n, s_vec, s_vec + c0, s_part);
  }
  for (size_t k = nblk; k-- > 0;) {
    const size_t c0 = k * kNB;
    const int nb = n - c0 < (size_t)kNB ? (int)(n - c0) : kNB;
    block_solve<T>(dinv + k * 2 * kNB * kNB + kNB * kNB, s_vec + c0, s_vec + c0, s_part);
    rows_update<T, kRangeSmallThreads>(U, n, c0, nb, 0, c0, s_vec, s_vec + c0, s_part);
  }
  for (size_t i = threadIdx.x; i < n; i += kRangeSmallThreads) v[i] = s_vec[i];
}

// block step k of one sweep: vin holds the right-hand side (block k final, the remaining rows partly updated), vout takes block k of
// the solution.  vin and vout are different arrays.
template <class T>
__global__ void __launch_bounds__(kBlock) potrs_step_kernel(T* __restrict__ vin, T* __restrict__ vout, const T* __restrict__ M, const T* __restrict__ Dk, size_t n, size_t k, int backward) {
  __shared__ T s_in[kNB], s_z[kNB], s_part[kBlock];
  const int tid = (int)threadIdx.x;
  const size_t c0 = k * kNB;
  const int nb = n - c0 < (size_t)kNB ? (int)(n - c0) : kNB;
  if (tid < kNB) s_in[tid] = tid < nb ? vin[c0 + tid] : (T)0;
  __syncthreads();
  block_solve<T>(Dk, s_in, s_z, s_part);
  if (blockIdx.x == 0 && tid < nb) vout[c0 + tid] = s_z[tid];
  const size_t lo = backward ? 0 : c0 + kNB, hi = backward ? c0 : n;
  const size_t base = lo + (size_t)blockIdx.x * kNB;
  if (base < hi) rows_update<T, kBlock>(M, n, c0, nb, base, base + kNB < hi ? base + kNB : hi, vin, s_z, s_part);      // one pass; uniform in the workgroup
}

template <class T>
static int launch_potrs(T* v, const T* L, const T* U, const T* dinv, void* workspace, size_t n, int tier, void* stream) {
  RangePlan p;
  if (!range_plan(n, sizeof(T), p)) { set_error("range_potrs: n has to be at least 1 with n * n < 2^31"); return 1; }
  if (tier != 0 && tier != 1 && tier != 2) { set_error("range_potrs: tier is 0 (the plan's), 1 (small) or 2 (large)"); return 1; }
  if (tier == 1 && n > (size_t)kRangeSmallMaxN) { set_error("range_potrs: n is too large for the small tier"); return 1; }
  if (tier == 0) tier = p.tier;
  if (!v || !L || !U || !dinv || (tier == 2 && !workspace)) { set_error("range_potrs: null pointer"); return 1; }
  hipStream_t s = as_stream(stream);
  if (tier == 1) {
    PH_LAUNCH((potrs_small_kernel<T>), dim3(1), dim3(kRangeSmallThreads), 0, s, v, L, U, dinv, n);
    PH_LAUNCH_END("range_potrs small kernel");
  }
  T* w = static_cast<T*>(workspace);
  const size_t nblk = pb::NumBlocks(n);
  for (size_t k = 0; k < nblk; k++) {
    const size_t lo = (k + 1) * kNB, rows = lo < n ? n - lo : 0;
    const unsigned grid = rows ? (unsigned)((rows + kNB - 1) / kNB) : 1u;
    hipLaunchKernelGGL((potrs_step_kernel<T>), dim3(grid), dim3(kBlock), 0, s, v, w, L, dinv + k * 2 * kNB * kNB, n, k, 0);
  }
  for (size_t k = nblk; k-- > 0;) {
    const unsigned grid = k ? (unsigned)k : 1u;                          // k * kNB rows above the block, 64 per workgroup
    hipLaunchKernelGGL((potrs_step_kernel<T>), dim3(grid), dim3(kBlock), 0, s, w, v, U, dinv + k * 2 * kNB * kNB + kNB * kNB, n, k, 1);
  }
  PH_LAUNCH_END("range_potrs step kernels");
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_range_potrs_plan(size_t n, int dtype, int* tier, int* nb, int* launches_per_solve, size_t* lds_bytes, size_t* workspace_bytes) {
  if (dtype != 0 && dtype != 1) { set_error("range_potrs_plan: dtype is 0 (fp32) or 1 (fp64)"); return 1; }
  RangePlan p;
  if (!range_plan(n, dtype ? sizeof(double) : sizeof(float), p)) { set_error("range_potrs_plan: n has to be at least 1 with n * n < 2^31"); return 1; }
  if (tier) *tier = p.tier;
  if (nb) *nb = kNB;
  if (launches_per_solve) *launches_per_solve = p.launches;
  if (lds_bytes) *lds_bytes = p.lds_bytes;
  if (workspace_bytes) *workspace_bytes = p.ws_bytes;
  return 0;
}
size_t prost_hip_range_dinv_elements(size_t n) { return pb::NumBlocks(n) * 2 * kNB * kNB; }
size_t prost_hip_range_potrf_workspace_bytes_f32(size_t n) { return potrf_workspace_bytes(n, sizeof(float)); }
size_t prost_hip_range_potrf_workspace_bytes_f64(size_t n) { return potrf_workspace_bytes(n, sizeof(double)); }
size_t prost_hip_range_potrs_workspace_bytes_f32(size_t n) { RangePlan p; return range_plan(n, sizeof(float), p) ? p.ws_bytes : 0; }
size_t prost_hip_range_potrs_workspace_bytes_f64(size_t n) { RangePlan p; return range_plan(n, sizeof(double), p) ? p.ws_bytes : 0; }
int prost_hip_range_potrf_f32(float* L, float* U, float* dinv, void* ws, int* status, size_t n, void* s) { return launch_potrf<float>(L, U, dinv, ws, status, n, s); }
int prost_hip_range_potrf_f64(double* L, double* U, double* dinv, void* ws, int* status, size_t n, void* s) { return launch_potrf<double>(L, U, dinv, ws, status, n, s); }
int prost_hip_range_potrs_f32(float* v, const float* L, const float* U, const float* dinv, void* ws, size_t n, int tier, void* s) { return launch_potrs<float>(v, L, U, dinv, ws, n, tier, s); }
int prost_hip_range_potrs_f64(double* v, const double* L, const double* U, const double* dinv, void* ws, size_t n, int tier, void* s) { return launch_potrs<double>(v, L, U, dinv, ws, n, tier, s); }
}  // extern "C"
