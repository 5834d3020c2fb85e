// kernels_linop_fanbeam2d.hip -- BlockFanbeam2D: res (+)= K rhs and res (+)= K^T rhs for the fan-beam projector K (a point source, a
// flat or an equiangular detector; Joseph's method) of L image planes, without a matrix.  The arithmetic, with its order of operations,
// the three tables and the candidate window of the adjoint, is include/prost/linop/fanbeam2d.hpp, which also runs on the host
// (tests/host/fanbeam2d_harness.cpp).  This file decides who reads what; it follows kernels_linop_radon2d.hip.
//
// Forward: a wavefront (one per workgroup) owns 64 consecutive bins of one view of one plane, so the view's table row is wave-uniform
// and read with scalar loads; a lane reads its bin's row, runs the prologue of its ray once (two divisions) and marches the ray over
// the driving lines with one running sum, eight lines' loads in flight.  At a column-driven view the lanes read one column at
// near-consecutive addresses: direct loads.  At a row-driven view they read one row across the columns, a cache line each: there the
// image goes through LDS in slabs of 16 rows by up to 128 columns (forward_sum_rows below).  The rays of a fan diverge, so the width
// of a slab is not the parallel figure: each slab's column range is measured, a minimum and a maximum over the wave of the rays'
// positions on its first and last row, and a slab wider than 128 columns is read from memory directly.
// Adjoint: a lane owns a pixel, the lanes of a wave 64 consecutive rows of one column, so stores are coalesced along y.  The lane loops
// over the views (table rows through scalar loads), locates its candidate bins with one division and the inverse map, and runs the
// prologue of each of its 2 m + 2 candidates; neighbouring pixels gather the same or neighbouring sinogram words.
// Planes are the grid's y axis.  No scratch, no atomics: a repeated call repeats its bits.  Resource table: docs/rounds/r34.md.
#include <cstring>

#include "common.hpp"
#include "prost/linop/fanbeam2d.hpp"

namespace prost_hip {

namespace f2d = prost::fanbeam2d;

static_assert(sizeof(f2d::Geometry) == sizeof(prost_hip_fanbeam2d_geometry), "geometry record");
static_assert(f2d::kBinsPerWave == kWave && f2d::kViewWidth == PROST_HIP_FANBEAM2D_VIEW_WIDTH && f2d::kBinWidth == PROST_HIP_FANBEAM2D_BIN_WIDTH &&
                  f2d::kInverseWidth == PROST_HIP_FANBEAM2D_INVERSE_WIDTH && f2d::kMaxMargin == PROST_HIP_FANBEAM2D_MAX_MARGIN,
              "table and tile constants");

namespace {

constexpr unsigned kMaxPlaneGrid = 65535;
constexpr int kSlabRows = f2d::kSlabRows, kSlabPitch = kSlabRows + 1, kSlabColumns = f2d::kSlabColumns;
static_assert(kWave % kSlabRows == 0 && f2d::kForwardBatch <= kSlabRows && kSlabRows % f2d::kForwardBatch == 0, "a wave stages whole columns, a batch stays inside a slab");

template <class T> __device__ __forceinline__ T wave_min(T v) {
#pragma unroll
  for (int s = 1; s < kWave; s *= 2) { const T o = __shfl_xor(v, s, kWave); v = o < v ? o : v; }
  return v;
}
template <class T> __device__ __forceinline__ T wave_max(T v) {
#pragma unroll
  for (int s = 1; s < kWave; s *= 2) { const T o = __shfl_xor(v, s, kWave); v = o > v ? o : v; }
  return v;
}

/// one ray of a row-driven view, with the image read through LDS.  A ray's position r + p t is monotone in t (every operation is), so
/// on the rows t0 .. t0 + 15 it stays between its values on the first and the last of them; the minimum and the maximum of those over
/// the wave bound the columns the wave's rays can touch there, floor(min) .. floor(max) + 1.  Up to kSlabColumns such columns are staged
/// with coalesced loads along y (four columns of 16 rows per wave instruction, eight instructions in flight) at an odd column pitch, so
/// lanes with neighbouring i0 read different banks and i0, i0 + 1 are one pitch apart.  A wider slab is read from memory directly.  The
/// running sum, the weights and their order are ForwardSum's: the same bits.
template <class T>
__device__ __forceinline__ T forward_sum_rows(const f2d::Ray<T>& ray, const T* plane, const f2d::Geometry& g, T* slab) {
  constexpr int kStageColumns = kWave / kSlabRows, kStageBatch = 8;
  const int ny = g.ny, nx = g.nx, lane = threadIdx.x;
  const int srow = lane % kSlabRows, scol = lane / kSlabRows;
  const T p = ray.p, c = ray.c, r = ray.r;
  T acc = -(T)0;
  for (int t0 = 0; t0 < ny; t0 += kSlabRows) {
    const int rows = ny - t0 < kSlabRows ? ny - t0 : kSlabRows;
    const T fa = f2d::Position(r, p * (T)t0), fb = f2d::Position(r, p * (T)(t0 + rows - 1));
    const T lo = floor(wave_min(fa < fb ? fa : fb)), hi = floor(wave_max(fa < fb ? fb : fa)) + (T)1;
    const int x0 = __builtin_amdgcn_readfirstlane(lo > (T)0 ? (lo < (T)nx ? (int)lo : nx) : 0);
    const int x1 = __builtin_amdgcn_readfirstlane(hi < (T)(nx - 1) ? (hi >= (T)0 ? (int)hi : -1) : nx - 1);
    const int width = x1 - x0 + 1;
    if (width <= 0) continue;                        // wave-uniform: these rows hold no entry of these rays
    const bool staged = width <= kSlabColumns;
    if (staged) {
      __syncthreads();                               // the reads of the slab before
      const int yr = t0 + (srow < rows ? srow : rows - 1);
      for (int c0 = scol; c0 < width; c0 += kStageColumns * kStageBatch) {
        T v[kStageBatch];
#pragma unroll
        for (int u = 0; u < kStageBatch; u++) {
          const int cx = c0 + u * kStageColumns < width ? c0 + u * kStageColumns : width - 1;
          v[u] = plane[(size_t)yr + (size_t)(x0 + cx) * (size_t)ny];
        }
#pragma unroll
        for (int u = 0; u < kStageBatch; u++) PROST_F2D_PIN(v[u]);
#pragma unroll
        for (int u = 0; u < kStageBatch; u++)
          if (c0 + u * kStageColumns < width && srow < rows) slab[(c0 + u * kStageColumns) * kSlabPitch + srow] = v[u];
      }
      __syncthreads();
    }
    for (int k0 = 0; k0 < rows; k0 += f2d::kForwardBatch) {
      T a0[f2d::kForwardBatch], a1[f2d::kForwardBatch], v0[f2d::kForwardBatch], v1[f2d::kForwardBatch];
      bool has0[f2d::kForwardBatch], has1[f2d::kForwardBatch];
#pragma unroll
      for (int k = 0; k < f2d::kForwardBatch; k++) {
        const int kk = k0 + k < rows ? k0 + k : rows - 1, t = t0 + kk;
        T w0, w1;
        const int i0 = f2d::Weights(f2d::Position(r, p * (T)t), nx, w0, w1);
        has0[k] = k0 + k < rows && i0 >= 0 && w0 != (T)0;
        has1[k] = k0 + k < rows && i0 >= -1 && i0 + 1 < nx && w1 != (T)0;
        a0[k] = c * w0;
        a1[k] = c * w1;
        int j0 = has0[k] ? i0 : x0, j1 = has1[k] ? i0 + 1 : x0;
        j0 = j0 < x0 ? x0 : (j0 > x1 ? x1 : j0);                                  // x0 .. x1: inside the slab, inside the plane (an entry
        j1 = j1 < x0 ? x0 : (j1 > x1 ? x1 : j1);                                  // is inside already: the clamp changes no value used)
        if (staged) {
          v0[k] = slab[(j0 - x0) * kSlabPitch + kk];
          v1[k] = slab[(j1 - x0) * kSlabPitch + kk];
        } else {
          v0[k] = plane[t + j0 * ny];
          v1[k] = plane[t + j1 * ny];
        }
      }
#pragma unroll
      for (int k = 0; k < f2d::kForwardBatch; k++) { PROST_F2D_PIN(v0[k]); PROST_F2D_PIN(v1[k]); }
#pragma unroll
      for (int k = 0; k < f2d::kForwardBatch; k++) {
        if (has0[k]) acc = acc + a0[k] * v0[k];
        if (has1[k]) acc = acc + a1[k] * v1[k];
      }
    }
  }
  return acc;
}

/// one wavefront per workgroup: 64 consecutive bins of one view, the planes on the grid's y axis
template <class T, bool ACC>
__global__ void __launch_bounds__(kWave) fanbeam2d_forward_kernel(T* res, const T* rhs, const f2d::Geometry g, const T* __restrict__ table, unsigned chunks) {
  __shared__ T slab[kSlabColumns * kSlabPitch];
  const unsigned a = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const int d = (int)(chunk * kWave) + (int)threadIdx.x, dc = d < g.ndet ? d : g.ndet - 1;   // a lane past the detector repeats the last bin and stores nothing
  const T* __restrict__ e = table + (size_t)a * f2d::kViewWidth;
  const T* __restrict__ bin = f2d::BinTable(table, g) + (size_t)dc * f2d::kBinWidth;
  const bool column = e[f2d::kAxis] != (T)0;                                          // wave-uniform
  const f2d::Ray<T> ray = f2d::Prologue(e, bin[f2d::kSinGamma], bin[f2d::kCosGamma]);
  const size_t plane = (size_t)g.ny * (size_t)g.nx, sino = (size_t)g.ndet * (size_t)g.na;
  for (unsigned c = blockIdx.y; c < (unsigned)g.planes; c += gridDim.y) {
    T v;
    if (column) v = f2d::ForwardSum<T>(e, ray, rhs + (size_t)c * plane, g);
    else v = forward_sum_rows<T>(ray, rhs + (size_t)c * plane, g, slab);
    if (d < g.ndet) {
      T* o = res + (size_t)c * sino + (size_t)a * (size_t)g.ndet + (size_t)d;
      *o = ACC ? *o + v : v;
    }
  }
}

template <class T, int M, bool ACC>
__global__ void __launch_bounds__(kBlock) fanbeam2d_adjoint_kernel(T* res, const T* rhs, const f2d::Geometry g, const T* __restrict__ table, unsigned tiles_y) {
  constexpr unsigned kWaves = kBlock / kWave;
  const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + threadIdx.x / kWave);
  const unsigned x = wave / tiles_y, y = (wave % tiles_y) * kWave + threadIdx.x % kWave;
  if (x >= (unsigned)g.nx || y >= (unsigned)g.ny) return;
  const size_t plane = (size_t)g.ny * (size_t)g.nx, sino = (size_t)g.ndet * (size_t)g.na;
  for (unsigned c = blockIdx.y; c < (unsigned)g.planes; c += gridDim.y) {
    const T v = f2d::AdjointSum<T, M>(table, rhs + (size_t)c * sino, g, (int)y, (int)x);
    T* o = res + (size_t)c * plane + (size_t)y + (size_t)x * (size_t)g.ny;
    *o = ACC ? *o + v : v;
  }
}

template <class T, int M>
int launch_adjoint(const f2d::Geometry& g, const T* table, T* res, const T* rhs, int accumulate, hipStream_t s, dim3 grid, unsigned tiles_y) {
  const dim3 block(kBlock);
  if (accumulate) PH_LAUNCH((fanbeam2d_adjoint_kernel<T, M, true>), grid, block, 0, s, res, rhs, g, table, tiles_y);
  else PH_LAUNCH((fanbeam2d_adjoint_kernel<T, M, false>), grid, block, 0, s, res, rhs, g, table, tiles_y);
  PH_LAUNCH_END("fanbeam2d adjoint kernel");
}

template <class T>
int launch_fanbeam2d(const prost_hip_fanbeam2d_geometry* geometry, const T* table, T* res, const T* rhs, int accumulate, void* stream) {
  if (!geometry) { set_error("fanbeam2d: null geometry"); return 1; }
  f2d::Geometry g;
  std::memcpy(&g, geometry, sizeof(g));
  if (g.ny < 1 || g.nx < 1 || g.ny > f2d::kMaxSide || g.nx > f2d::kMaxSide) { set_error("fanbeam2d: nx and ny have to be 1 .. 8192"); return 1; }
  if (g.na < 1 || g.na > f2d::kMaxViews) { set_error("fanbeam2d: the view count has to be 1 .. 4096"); return 1; }
  if (g.ndet < 1 || g.ndet > f2d::kMaxBins || g.planes < 1) { set_error("fanbeam2d: the bin count and the plane count have to be at least 1 (bins below 2^31 - 1024)"); return 1; }
  if (g.m < 1 || g.m > f2d::kMaxMargin) { set_error("fanbeam2d: the window margin has to be 1 .. 5"); return 1; }
  const uint64_t kLimit = (uint64_t)1 << 31;
  if ((uint64_t)g.ndet * (uint64_t)g.na >= kLimit) { set_error("fanbeam2d: a sinogram has to stay below 2^31 elements"); return 1; }
  if (!res || !rhs || !table) { set_error("fanbeam2d: null pointer"); return 1; }
  hipStream_t s = as_stream(stream);
  const unsigned kWaves = kBlock / kWave, planes = (unsigned)g.planes < kMaxPlaneGrid ? (unsigned)g.planes : kMaxPlaneGrid;
  if (!g.transpose) {
    const uint64_t chunks = ((uint64_t)g.ndet + kWave - 1) / kWave, waves = chunks * (uint64_t)g.na;      // below 2^31 / 64 + 4096
    const dim3 grid((unsigned)waves, planes), wave(kWave);
    if (accumulate) PH_LAUNCH((fanbeam2d_forward_kernel<T, true>), grid, wave, 0, s, res, rhs, g, table, (unsigned)chunks);
    else PH_LAUNCH((fanbeam2d_forward_kernel<T, false>), grid, wave, 0, s, res, rhs, g, table, (unsigned)chunks);
    PH_LAUNCH_END("fanbeam2d forward kernel");
  }
  const uint64_t tiles_y = ((uint64_t)g.ny + kWave - 1) / kWave, waves = tiles_y * (uint64_t)g.nx;             // at most 128 * 8192
  const dim3 grid((unsigned)((waves + kWaves - 1) / kWaves), planes);
  switch (g.m) {
    case 1: return launch_adjoint<T, 1>(g, table, res, rhs, accumulate, s, grid, (unsigned)tiles_y);
    case 2: return launch_adjoint<T, 2>(g, table, res, rhs, accumulate, s, grid, (unsigned)tiles_y);
    case 3: return launch_adjoint<T, 3>(g, table, res, rhs, accumulate, s, grid, (unsigned)tiles_y);
    case 4: return launch_adjoint<T, 4>(g, table, res, rhs, accumulate, s, grid, (unsigned)tiles_y);
    default: return launch_adjoint<T, 5>(g, table, res, rhs, accumulate, s, grid, (unsigned)tiles_y);
  }
}

}  // namespace
}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_fanbeam2d_f32(const prost_hip_fanbeam2d_geometry* geometry, const float* table, float* res, const float* rhs, int accumulate, void* stream) {
  return launch_fanbeam2d<float>(geometry, table, res, rhs, accumulate, stream);
}
int prost_hip_fanbeam2d_f64(const prost_hip_fanbeam2d_geometry* geometry, const double* table, double* res, const double* rhs, int accumulate, void* stream) {
  return launch_fanbeam2d<double>(geometry, table, res, rhs, accumulate, stream);
}
}  // extern "C"
