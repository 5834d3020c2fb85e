// kernels_linop_conv2d.hip -- BlockConv2D: res (+)= K rhs and res (+)= K^T rhs for one small window applied at every pixel of L image
// planes (zero padding), without a matrix.  The arithmetic, with its order of operations, is include/prost/linop/conv2d.hpp, which
// also runs on the host (tests/host/conv2d_harness.cpp).  This file decides who reads what.
//
// A workgroup of 256 owns a tile of 64 x 16 outputs of one plane: lanes along y, the contiguous axis, the four waves along x, every
// lane with 4 neighbouring outputs along x in registers.  The source tile with its (ky - 1, kx - 1) halo is staged in LDS once,
// out-of-range cells as zeros, so the march has no bounds tests; its column pitch is 94 elements for every window, so a tap's LDS
// offset is known when the table is made and the 4 reads of a tap differ by constants.  Consecutive lanes read consecutive LDS
// words: no bank conflicts for any tap.  The tap table (offset, value) is a __restrict__ device array read with a wave-uniform index.
// LDS: 94 (15 + kx) sizeof(T) bytes, 34 592 at 31 x 31 in fp64 (four workgroups per CU).  The two directions share the instances:
// only the geometry record and the table differ.  No scratch, no atomics: a repeated call repeats its bits.
// Resource table: docs/rounds/r18.md.
#include <cstring>

#include "common.hpp"
#include "prost/linop/conv2d.hpp"

namespace prost_hip {

namespace c2d = prost::conv2d;

static_assert(sizeof(c2d::Geometry) == sizeof(prost_hip_conv2d_geometry), "geometry record");
static_assert(sizeof(c2d::Tap<float>) == sizeof(prost_hip_conv2d_tap_f32) && sizeof(c2d::Tap<double>) == sizeof(prost_hip_conv2d_tap_f64), "tap record");
static_assert(c2d::kPitch == PROST_HIP_CONV2D_PITCH && c2d::kMaxWindow == PROST_HIP_CONV2D_MAX_WINDOW, "tile constants");
static_assert(c2d::kPitch <= 2 * kWave, "a lane stages at most two rows of a column");
static_assert(c2d::kTileY == kWave && c2d::kTileX == (kBlock / kWave) * c2d::kOutputs, "a lane per output row, four outputs along x per lane");

template <class T, bool ACC>
__global__ void __launch_bounds__(kBlock) conv2d_kernel(T* res, const T* rhs, const c2d::Geometry g, const c2d::Tap<T>* __restrict__ taps, int ntaps,
                                                        unsigned tiles_y, unsigned tiles_x) {
  extern __shared__ __align__(16) unsigned char conv2d_lds[];
  T* tile = reinterpret_cast<T*>(conv2d_lds);
  unsigned b = blockIdx.x;
  const unsigned by = b % tiles_y;
  b /= tiles_y;
  const unsigned bx = b % tiles_x, plane = b / tiles_x;
  const int y0 = (int)by * c2d::kTileY, x0 = (int)bx * c2d::kTileX;
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const T* src = rhs + (size_t)plane * (size_t)g.sny * (size_t)g.snx;
  const int rows = c2d::kTileY + g.ky - 1, cols = c2d::kTileX + g.kx - 1;
  // a wave stages every fourth column, kStageColumns of them at a time, a lane rows `lane` and `lane + 64` (rows <= 94).  The loads of
  // a batch are unconditional (SourceIndex names the nearest element of the plane for a cell outside it) and all issued before the
  // first value is looked at; the empty asm statements keep the compiler from moving a load back under its `inside` test, where
  // every lane would wait for one load after the other.
  constexpr int kWaves = kBlock / kWave, kStageColumns = 4;
  for (int lx0 = wave; lx0 < cols; lx0 += kWaves * kStageColumns) {
    T v[kStageColumns][2];
    bool inside[kStageColumns][2];
#pragma unroll
    for (int u = 0; u < kStageColumns; u++)
#pragma unroll
      for (int h = 0; h < 2; h++) {
        const int lx = lx0 + u * kWaves < cols ? lx0 + u * kWaves : cols - 1, ly = lane + h * kWave < rows ? lane + h * kWave : rows - 1;
        v[u][h] = src[c2d::SourceIndex(g, y0, x0, ly, lx, inside[u][h])];
      }
#pragma unroll
    for (int u = 0; u < kStageColumns; u++)
#pragma unroll
      for (int h = 0; h < 2; h++) asm volatile("" : "+v"(v[u][h]));
#pragma unroll
    for (int u = 0; u < kStageColumns; u++)
#pragma unroll
      for (int h = 0; h < 2; h++)
        if (lx0 + u * kWaves < cols && lane + h * kWave < rows) tile[lane + h * kWave + (lx0 + u * kWaves) * c2d::kPitch] = inside[u][h] ? v[u][h] : (T)0;
  }
  __syncthreads();
  const int tx = wave * c2d::kOutputs;
  if (x0 + tx >= g.dnx) return;              // wave-uniform: a wave past the right edge of the plane
  T acc[c2d::kOutputs];
  c2d::March<T, c2d::kOutputs>(acc, tile + lane + tx * c2d::kPitch, taps, ntaps);
  c2d::Store<T, c2d::kOutputs, ACC>(res + (size_t)plane * (size_t)g.dny * (size_t)g.dnx, g, y0 + lane, x0 + tx, acc);
}

template <class T, class TapRecord>
static int launch_conv2d(const prost_hip_conv2d_geometry* geometry, const TapRecord* taps, size_t ntaps, T* res, const T* rhs, int accumulate, void* stream) {
  if (!geometry) { set_error("conv2d: null geometry"); return 1; }
  c2d::Geometry g;
  std::memcpy(&g, geometry, sizeof(g));
  if (g.ky < 1 || g.kx < 1 || g.ky > c2d::kMaxWindow || g.kx > c2d::kMaxWindow) { set_error("conv2d: the window has to be 1 x 1 to 31 x 31"); return 1; }
  if (g.sny < 1 || g.snx < 1 || g.dny < 1 || g.dnx < 1 || g.planes < 1) { set_error("conv2d: plane sizes and the plane count have to be at least 1"); return 1; }
  if (g.oy < 0 || g.ox < 0 || g.oy >= g.ky || g.ox >= g.kx) { set_error("conv2d: the crop offset has to lie inside the window"); return 1; }
  if (ntaps < 1 || ntaps > (size_t)(g.ky * g.kx)) { set_error("conv2d: the tap count has to be 1 .. ky kx"); return 1; }
  if ((uint64_t)g.sny * (uint64_t)g.snx >= ((uint64_t)1 << 31) || (uint64_t)g.dny * (uint64_t)g.dnx >= ((uint64_t)1 << 31)) {
    set_error("conv2d: a plane has to stay below 2^31 elements"); return 1;
  }
  if (!res || !rhs || !taps) { set_error("conv2d: null pointer"); return 1; }
  const uint64_t tiles_y = ((uint64_t)g.dny + c2d::kTileY - 1) / c2d::kTileY, tiles_x = ((uint64_t)g.dnx + c2d::kTileX - 1) / c2d::kTileX;
  const uint64_t blocks = tiles_y * tiles_x * (uint64_t)g.planes;
  if (blocks > (uint64_t)0x7fffffff) { set_error("conv2d: more than 2^31 - 1 tiles"); return 1; }
  const size_t lds = (size_t)c2d::kPitch * (size_t)(c2d::kTileX + g.kx - 1) * sizeof(T);
  const c2d::Tap<T>* table = reinterpret_cast<const c2d::Tap<T>*>(taps);
  const dim3 grid((unsigned)blocks), block(kBlock);
  hipStream_t s = as_stream(stream);
  if (accumulate) PH_LAUNCH((conv2d_kernel<T, true>), grid, block, lds, s, res, rhs, g, table, (int)ntaps, (unsigned)tiles_y, (unsigned)tiles_x);
  else PH_LAUNCH((conv2d_kernel<T, false>), grid, block, lds, s, res, rhs, g, table, (int)ntaps, (unsigned)tiles_y, (unsigned)tiles_x);
  PH_LAUNCH_END("conv2d kernel");
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_conv2d_f32(const prost_hip_conv2d_geometry* geometry, const prost_hip_conv2d_tap_f32* taps, size_t ntaps, float* res, const float* rhs,
                         int accumulate, void* stream) {
  return launch_conv2d<float>(geometry, taps, ntaps, res, rhs, accumulate, stream);
}
int prost_hip_conv2d_f64(const prost_hip_conv2d_geometry* geometry, const prost_hip_conv2d_tap_f64* taps, size_t ntaps, double* res, const double* rhs,
                         int accumulate, void* stream) {
  return launch_conv2d<double>(geometry, taps, ntaps, res, rhs, accumulate, stream);
}
}  // extern "C"
