// kernels_linop_sample2d.hip -- BlockSample2D: res (+)= K rhs and res (+)= K^T rhs for bilinear resampling K of L image planes at M
// positions, without a matrix.  The arithmetic, with its order of operations and the bucket tables of the adjoint, is
// include/prost/linop/sample2d.hpp, which also runs on the host (tests/host/sample2d_harness.cpp).  This file decides who reads what.
//
// Forward: a lane owns a sample.  It reads fx and fy coalesced, forms the four weights and the four clamped offsets once, and loops over
// the planes: four loads issued unconditionally from always-valid addresses, then selected, then added in slot order.  The stores are
// coalesced along the samples.
// Adjoint: a lane owns a pixel, the lanes of a wave 64 consecutive rows of one column (coalesced stores, and neighbouring lanes read
// neighbouring words of cell_start), four waves per workgroup, planes on the grid's y axis.  The lane walks the two contiguous stretches
// of `order` that hold the four cells reaching its pixel and gathers rhs[order[k]], four samples' loads in flight: a finite count read
// from the table, no step cap.  Many samples in one cell serialise in one lane: slow, correct.
// No scratch, no atomics: a repeated call repeats its bits.  Resource table: docs/rounds/r24.md.
#include <cstring>

#include "common.hpp"
#include "prost/linop/sample2d.hpp"

namespace prost_hip {

namespace s2d = prost::sample2d;

static_assert(sizeof(s2d::Geometry) == sizeof(prost_hip_sample2d_geometry), "geometry record");
static_assert(s2d::kSamplesPerWave == kWave && s2d::kRowsPerWave == kWave, "tile constants");

constexpr unsigned kMaxPlaneGrid = 65535;

template <class T, bool ACC>
__global__ void __launch_bounds__(kBlock) sample2d_forward_kernel(T* res, const T* rhs, const s2d::Geometry g, const T* __restrict__ px, const T* __restrict__ py) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= (unsigned)g.m) return;
  const s2d::Row<T> r = s2d::MakeRow<T>(px[i], py[i], g.ny, g.nx);
  const size_t plane = (size_t)g.ny * (size_t)g.nx, m = (size_t)g.m;
  for (int c = 0; c < g.planes; c++) {
    const T v = s2d::ForwardSum<T>(r, rhs + (size_t)c * plane);
    T* o = res + (size_t)c * m + i;
    *o = ACC ? *o + v : v;
  }
}

template <class T, bool ACC>
__global__ void __launch_bounds__(kBlock) sample2d_adjoint_kernel(T* res, const T* rhs, const s2d::Geometry g, const T* __restrict__ px, const T* __restrict__ py,
                                                                   const int32_t* __restrict__ order, const int32_t* __restrict__ cell_start, unsigned tiles_y) {
  constexpr unsigned kWaves = kBlock / kWave;
  const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * kWaves + threadIdx.x / kWave);
  const unsigned xx = wave / tiles_y, yy = (wave % tiles_y) * kWave + threadIdx.x % kWave;
  if (xx >= (unsigned)g.nx || yy >= (unsigned)g.ny) return;
  const size_t plane = (size_t)g.ny * (size_t)g.nx, m = (size_t)g.m;
  for (unsigned c = blockIdx.y; c < (unsigned)g.planes; c += gridDim.y) {
    const T v = s2d::AdjointSum<T>(px, py, order, cell_start, rhs + (size_t)c * m, g.ny, (int)yy, (int)xx);
    T* o = res + (size_t)c * plane + (size_t)yy + (size_t)xx * (size_t)g.ny;
    *o = ACC ? *o + v : v;
  }
}

template <class T>
static int launch_sample2d(const prost_hip_sample2d_geometry* geometry, const T* pos_x, const T* pos_y, const int32_t* order, const int32_t* cell_start, T* res,
                           const T* rhs, int accumulate, void* stream) {
  if (!geometry) { set_error("sample2d: null geometry"); return 1; }
  s2d::Geometry g;
  std::memcpy(&g, geometry, sizeof(g));
  if (g.ny < 1 || g.nx < 1 || g.ny > s2d::kMaxSide || g.nx > s2d::kMaxSide) { set_error("sample2d: nx and ny have to be 1 .. 16384"); return 1; }
  if (g.m < 1 || g.planes < 1) { set_error("sample2d: the sample count and the plane count have to be at least 1"); return 1; }
  const uint64_t kLimit = (uint64_t)1 << 31;
  if ((uint64_t)g.m >= kLimit || (uint64_t)g.ny * (uint64_t)g.nx >= kLimit) { set_error("sample2d: the samples and the pixels of a plane have to stay below 2^31"); return 1; }
  if (!res || !rhs || !pos_x || !pos_y || !order || !cell_start) { set_error("sample2d: null pointer"); return 1; }
  hipStream_t s = as_stream(stream);
  const dim3 block(kBlock);
  if (!g.transpose) {
    const dim3 grid((unsigned)(((uint64_t)g.m + kBlock - 1) / kBlock));               // at most 2^23
    if (accumulate) PH_LAUNCH((sample2d_forward_kernel<T, true>), grid, block, 0, s, res, rhs, g, pos_x, pos_y);
    else PH_LAUNCH((sample2d_forward_kernel<T, false>), grid, block, 0, s, res, rhs, g, pos_x, pos_y);
    PH_LAUNCH_END("sample2d forward kernel");
  }
  const unsigned kWaves = kBlock / kWave, planes = (unsigned)g.planes < kMaxPlaneGrid ? (unsigned)g.planes : kMaxPlaneGrid;
  const uint64_t tiles_y = ((uint64_t)g.ny + kWave - 1) / kWave, waves = tiles_y * (uint64_t)g.nx;      // at most 256 * 16384
  const dim3 grid((unsigned)((waves + kWaves - 1) / kWaves), planes);
  if (accumulate) PH_LAUNCH((sample2d_adjoint_kernel<T, true>), grid, block, 0, s, res, rhs, g, pos_x, pos_y, order, cell_start, (unsigned)tiles_y);
  else PH_LAUNCH((sample2d_adjoint_kernel<T, false>), grid, block, 0, s, res, rhs, g, pos_x, pos_y, order, cell_start, (unsigned)tiles_y);
  PH_LAUNCH_END("sample2d adjoint kernel");
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_sample2d_f32(const prost_hip_sample2d_geometry* geometry, const float* pos_x, const float* pos_y, const int32_t* order, const int32_t* cell_start,
                           float* res, const float* rhs, int accumulate, void* stream) {
  return launch_sample2d<float>(geometry, pos_x, pos_y, order, cell_start, res, rhs, accumulate, stream);
}
int prost_hip_sample2d_f64(const prost_hip_sample2d_geometry* geometry, const double* pos_x, const double* pos_y, const int32_t* order, const int32_t* cell_start,
                           double* res, const double* rhs, int accumulate, void* stream) {
  return launch_sample2d<double>(geometry, pos_x, pos_y, order, cell_start, res, rhs, accumulate, stream);
}
}  // extern "C"
