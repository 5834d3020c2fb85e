// kernels_linop_radon2d.hip -- BlockRadon2D: res (+)= K rhs and res (+)= K^T rhs for the parallel-beam projector K (Joseph's method)
// of L image planes, without a matrix.  The arithmetic, with its order of operations, the per-angle table and the candidate window of
// the adjoint, is include/prost/linop/radon2d.hpp, which also runs on the host (tests/host/radon2d_harness.cpp).  This file decides who
// reads what.
//
// Forward: a wavefront (one per workgroup) owns 64 consecutive bins of one angle of one plane, so the angle's table row is wave-uniform
// and read with scalar loads; a lane marches its ray over the driving lines with one running sum, eight lines' loads in flight.  At a
// column-driven angle the lanes read y-positions q apart in one column, near-consecutive addresses: direct loads.  At a row-driven
// angle they read one row across the columns, ny elements apart, a cache line each: there the image goes through LDS in slabs of 16
// rows by up to 128 columns, staged with coalesced loads along y at an odd column pitch (forward_sum_rows below).
// Adjoint: a lane owns a pixel, the lanes of a wave 64 consecutive rows of one column, so stores are coalesced along y.  The lane loops
// over the angles (table rows through scalar loads) and gathers its 2 m + 2 candidate bins, which for neighbouring pixels are the same
// or neighbouring sinogram words.
// Planes are the grid's y axis.  No scratch, no atomics: a repeated call repeats its bits.  Resource table: docs/rounds/r23.md.
#include <cstring>

#include "common.hpp"
#include "prost/linop/radon2d.hpp"

namespace prost_hip {

namespace r2d = prost::radon2d;

static_assert(sizeof(r2d::Geometry) == sizeof(prost_hip_radon2d_geometry), "geometry record");
static_assert(r2d::kBinsPerWave == kWave && r2d::kTableWidth == PROST_HIP_RADON2D_TABLE_WIDTH, "table and tile constants");

constexpr unsigned kMaxPlaneGrid = 65535;
constexpr int kSlabRows = r2d::kSlabRows, kSlabPitch = kSlabRows + 1, kSlabColumns = r2d::kSlabColumns;
static_assert(kWave % kSlabRows == 0 && r2d::kForwardBatch <= kSlabRows && kSlabRows % r2d::kForwardBatch == 0, "a wave stages whole columns, a batch stays inside a slab");

/// one ray of a row-driven angle, with the image read through LDS.  The wave's rays d_lo .. d_hi cross the rows t0 .. t0 + 15 inside
/// the columns floor(f_min) .. floor(f_max) + 1: every operation of the position is monotone in d and in t, so the four corners of
/// (d, t) bound f.  Up to kSlabColumns such columns are staged with coalesced loads along y (four columns of 16 rows per wave
/// instruction, eight instructions in flight) at an odd column pitch, so lanes with neighbouring i0 read different banks and i0, i0 + 1
/// are one pitch apart.  A slab that would be wider (spacing above 1) is read from memory directly.  The running sum, the weights and
/// their order are ForwardSum's: the same bits.
template <class T>
__device__ __forceinline__ T forward_sum_rows(const T* __restrict__ e, const T* plane, const r2d::Geometry& g, int d, int d_lo, int d_hi, T* slab) {
  constexpr int kStageColumns = kWave / kSlabRows, kStageBatch = 8;
  const int ny = g.ny, nx = g.nx, lane = threadIdx.x;
  const int srow = lane % kSlabRows, scol = lane / kSlabRows;
  const T p = e[r2d::kP], c = e[r2d::kC], base = r2d::Base(e, d), base_lo = r2d::Base(e, d_lo), base_hi = r2d::Base(e, d_hi);
  T acc = -(T)0;
  for (int t0 = 0; t0 < ny; t0 += kSlabRows) {
    const int rows = ny - t0 < kSlabRows ? ny - t0 : kSlabRows;
    const T pa = p * (T)t0, pb = p * (T)(t0 + rows - 1);
    const T f0 = r2d::Position(base_lo, pa), f1 = r2d::Position(base_lo, pb), f2 = r2d::Position(base_hi, pa), f3 = r2d::Position(base_hi, pb);
    const T m01 = f0 < f1 ? f0 : f1, m23 = f2 < f3 ? f2 : f3, M01 = f0 < f1 ? f1 : f0, M23 = f2 < f3 ? f3 : f2;
    const T lo = floor(m01 < m23 ? m01 : m23), hi = floor(M01 < M23 ? M23 : M01) + (T)1;
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
        for (int u = 0; u < kStageBatch; u++) PROST_R2D_PIN(v[u]);
#pragma unroll
        for (int u = 0; u < kStageBatch; u++)
          if (c0 + u * kStageColumns < width && srow < rows) slab[(c0 + u * kStageColumns) * kSlabPitch + srow] = v[u];
      }
      __syncthreads();
    }
    for (int k0 = 0; k0 < rows; k0 += r2d::kForwardBatch) {
      T a0[r2d::kForwardBatch], a1[r2d::kForwardBatch], v0[r2d::kForwardBatch], v1[r2d::kForwardBatch];
      bool has0[r2d::kForwardBatch], has1[r2d::kForwardBatch];
#pragma unroll
      for (int k = 0; k < r2d::kForwardBatch; k++) {
        const int kk = k0 + k < rows ? k0 + k : rows - 1, t = t0 + kk;
        T w0, w1;
        const int i0 = r2d::Weights(r2d::Position(base, p * (T)t), nx, w0, w1);
        has0[k] = k0 + k < rows && i0 >= 0 && w0 != (T)0;
        has1[k] = k0 + k < rows && i0 >= -1 && i0 + 1 < nx && w1 != (T)0;
        a0[k] = c * w0;
        a1[k] = c * w1;
        const int j0 = has0[k] ? i0 : x0, j1 = has1[k] ? i0 + 1 : x0;          // x0 .. x1: inside the slab, inside the plane
        if (staged) {
          v0[k] = slab[(j0 - x0) * kSlabPitch + kk];
          v1[k] = slab[(j1 - x0) * kSlabPitch + kk];
        } else {
          v0[k] = plane[t + j0 * ny];
          v1[k] = plane[t + j1 * ny];
        }
      }
#pragma unroll
      for (int k = 0; k < r2d::kForwardBatch; k++) { PROST_R2D_PIN(v0[k]); PROST_R2D_PIN(v1[k]); }
#pragma unroll
      for (int k = 0; k < r2d::kForwardBatch; k++) {
        if (has0[k]) acc = acc + a0[k] * v0[k];
        if (has1[k]) acc = acc + a1[k] * v1[k];
      }
    }
  }
  return acc;
}

/// one wavefront per workgroup: 64 consecutive bins of one angle, the planes on the grid's y axis
template <class T, bool ACC>
__global__ void __launch_bounds__(kWave) radon2d_forward_kernel(T* res, const T* rhs, const r2d::Geometry g, const T* __restrict__ table, unsigned chunks) {
  __shared__ T slab[kSlabColumns * kSlabPitch];
  const unsigned a = blockIdx.x / chunks, chunk = blockIdx.x % chunks;
  const int d_lo = (int)(chunk * kWave), d_hi = d_lo + kWave - 1 < g.ndet ? d_lo + kWave - 1 : g.ndet - 1;
  const int d = d_lo + (int)threadIdx.x, dc = d < g.ndet ? d : g.ndet - 1;             // a lane past the detector repeats the last bin and stores nothing
  const T* __restrict__ e = table + (size_t)a * r2d::kTableWidth;
  const bool column = e[r2d::kAxis] != (T)0;                                          // wave-uniform
  const size_t plane = (size_t)g.ny * (size_t)g.nx, sino = (size_t)g.ndet * (size_t)g.na;
  for (unsigned c = blockIdx.y; c < (unsigned)g.planes; c += gridDim.y) {
    T v;
    if (column) v = r2d::ForwardSum<T>(e, rhs + (size_t)c * plane, g, dc);
    else v = forward_sum_rows<T>(e, rhs + (size_t)c * plane, g, dc, d_lo, d_hi, slab);
    if (d < g.ndet) {
      T* o = res + (size_t)c * sino + (size_t)a * (size_t)g.ndet + (size_t)d;
      *o = ACC ? *o + v : v;
    }
  }
}

template <class T, int M, bool ACC>
__global__ void __launch_bounds__(kBlock) radon2d_adjoint_kernel(T* res, const T* rhs, const r2d::Geometry g, const T* __restrict__ table, unsigned tiles_y) {
  constexpr unsigned kWaves = kBlock / kWave;
  const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + threadIdx.x / kWave);
  const unsigned x = wave / tiles_y, y = (wave % tiles_y) * kWave + threadIdx.x % kWave;
  if (x >= (unsigned)g.nx || y >= (unsigned)g.ny) return;
  const size_t plane = (size_t)g.ny * (size_t)g.nx, sino = (size_t)g.ndet * (size_t)g.na;
  for (unsigned c = blockIdx.y; c < (unsigned)g.planes; c += gridDim.y) {
    const T v = r2d::AdjointSum<T, M>(table, rhs + (size_t)c * sino, g, (int)y, (int)x);
    T* o = res + (size_t)c * plane + (size_t)y + (size_t)x * (size_t)g.ny;
    *o = ACC ? *o + v : v;
  }
}

template <class T>
static int launch_radon2d(const prost_hip_radon2d_geometry* geometry, const T* table, T* res, const T* rhs, int accumulate, void* stream) {
  if (!geometry) { set_error("radon2d: null geometry"); return 1; }
  r2d::Geometry g;
  std::memcpy(&g, geometry, sizeof(g));
  if (g.ny < 1 || g.nx < 1 || g.ny > r2d::kMaxSide || g.nx > r2d::kMaxSide) { set_error("radon2d: nx and ny have to be 1 .. 8192"); return 1; }
  if (g.na < 1 || g.na > r2d::kMaxAngles) { set_error("radon2d: the angle count has to be 1 .. 4096"); return 1; }
  if (g.ndet < 1 || g.ndet > r2d::kMaxBins || g.planes < 1) { set_error("radon2d: the bin count and the plane count have to be at least 1 (bins below 2^31 - 1024)"); return 1; }
  if (g.m < 1 || g.m > r2d::kMaxMargin) { set_error("radon2d: the window margin has to be 1 or 2 (spacing 0.5 .. 8)"); return 1; }
  const uint64_t kLimit = (uint64_t)1 << 31;
  if ((uint64_t)g.ndet * (uint64_t)g.na >= kLimit) { set_error("radon2d: a sinogram has to stay below 2^31 elements"); return 1; }
  if (!res || !rhs || !table) { set_error("radon2d: null pointer"); return 1; }
  hipStream_t s = as_stream(stream);
  const dim3 block(kBlock);
  const unsigned kWaves = kBlock / kWave, planes = (unsigned)g.planes < kMaxPlaneGrid ? (unsigned)g.planes : kMaxPlaneGrid;
  if (!g.transpose) {
    const uint64_t chunks = ((uint64_t)g.ndet + kWave - 1) / kWave, waves = chunks * (uint64_t)g.na;      // below 2^31 / 64 + 4096
    const dim3 grid((unsigned)waves, planes), wave(kWave);
    if (accumulate) PH_LAUNCH((radon2d_forward_kernel<T, true>), grid, wave, 0, s, res, rhs, g, table, (unsigned)chunks);
    else PH_LAUNCH((radon2d_forward_kernel<T, false>), grid, wave, 0, s, res, rhs, g, table, (unsigned)chunks);
    PH_LAUNCH_END("radon2d forward kernel");
  }
  const uint64_t tiles_y = ((uint64_t)g.ny + kWave - 1) / kWave, waves = tiles_y * (uint64_t)g.nx;             // at most 128 * 8192
  const dim3 grid((unsigned)((waves + kWaves - 1) / kWaves), planes);
#define PROST_R2D_ADJOINT(M, ACC) PH_LAUNCH((radon2d_adjoint_kernel<T, M, ACC>), grid, block, 0, s, res, rhs, g, table, (unsigned)tiles_y)
  if (g.m == 1) { if (accumulate) PROST_R2D_ADJOINT(1, true); else PROST_R2D_ADJOINT(1, false); }
  else { if (accumulate) PROST_R2D_ADJOINT(2, true); else PROST_R2D_ADJOINT(2, false); }
#undef PROST_R2D_ADJOINT
  PH_LAUNCH_END("radon2d adjoint kernel");
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_radon2d_f32(const prost_hip_radon2d_geometry* geometry, const float* table, float* res, const float* rhs, int accumulate, void* stream) {
  return launch_radon2d<float>(geometry, table, res, rhs, accumulate, stream);
}
int prost_hip_radon2d_f64(const prost_hip_radon2d_geometry* geometry, const double* table, double* res, const double* rhs, int accumulate, void* stream) {
  return launch_radon2d<double>(geometry, table, res, rhs, accumulate, stream);
}
}  // extern "C"
