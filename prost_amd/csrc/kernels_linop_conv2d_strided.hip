// kernels_linop_conv2d_strided.hip -- BlockConv2DStrided: res (+)= K rhs and res (+)= K^T rhs for K = S B, one small window applied
// at every pixel of L image planes (zero padding) and every (sy, sx)-th result kept, without a matrix.  The arithmetic, with its order
// of operations, the tile table and the staging rules, is include/prost/linop/conv2d_strided.hpp, which also runs on the host
// (tests/host/conv2d_strided_harness.cpp).  This file decides who reads what.
//
// Forward: a workgroup of 256 owns a tile of ty x tx outputs of one plane (conv2d_strided::kTiles, the first entry whose source tile
// fits 64 KiB: 64 x 16 with four outputs along x per lane down to 32 x 4 with one), lanes along y.  Output row t reads source rows
// t sy + const, so the source tile is staged de-interleaved by row residue: every tap reads consecutive LDS words for consecutive
// lanes, at any stride.  The tap record holds the sub-plane and position of its cell as one offset.
// Adjoint: a workgroup owns 64 sy x 16 destination pixels; a lane owns sy consecutive rows of four neighbouring columns, one
// accumulator per row residue, one tap sub-list per residue class (ry, rx) (wave-uniform: the four waves own four columns each).  All
// residues read the staged source rows lane + const of the natural layout -- consecutive words again -- and the sy results of a
// column are contiguous in memory: one 8- or 16-byte store where the address allows, element stores otherwise.
// Staging loads are unconditional and batched (clamp the index, load, select zero).  No scratch, no atomics: a repeated call repeats
// its bits.  Resource table: docs/rounds/r21.md.
#include <cstring>

#include "common.hpp"
#include "prost/linop/conv2d_strided.hpp"

namespace prost_hip {

namespace c2s = prost::conv2d_strided;

static_assert(sizeof(c2s::Geometry) == sizeof(prost_hip_conv2d_strided_geometry), "geometry record");
static_assert(sizeof(c2s::Tap<float>) == sizeof(prost_hip_conv2d_tap_f32) && sizeof(c2s::Tap<double>) == sizeof(prost_hip_conv2d_tap_f64), "tap record");
static_assert(c2s::kThreads == kBlock && c2s::kAdjLanes == kWave && c2s::kMaxStride == PROST_HIP_CONV2D_STRIDED_MAX_STRIDE, "tile constants");
static_assert(c2s::kAdjLanes + c2s::kMaxWindow - 1 <= 2 * kWave, "a lane stages at most two rows of an adjoint column");

// a wave stages every fourth column, kStageColumns of them at a time, a lane two rows 64 apart, row pair after row pair.  The loads
// of a batch are unconditional (`index` names the nearest element of the plane for a cell outside it) and all issued before the first
// value is looked at; the empty asm statements keep the compiler from moving a load back under its `inside` test.
template <class T, class Index, class Cell>
__device__ __forceinline__ void stage_tile(T* tile, const T* src, int rows, int cols, int lane, int wave, Index index, Cell cell) {
  constexpr int kWaves = kBlock / kWave, kStageColumns = 4;
  for (int ly0 = lane; ly0 - lane < rows; ly0 += 2 * kWave)
    for (int lx0 = wave; lx0 < cols; lx0 += kWaves * kStageColumns) {
      T v[kStageColumns][2];
      bool inside[kStageColumns][2];
#pragma unroll
      for (int u = 0; u < kStageColumns; u++)
#pragma unroll
        for (int h = 0; h < 2; h++) {
          const int lx = lx0 + u * kWaves < cols ? lx0 + u * kWaves : cols - 1, ly = ly0 + h * kWave < rows ? ly0 + h * kWave : rows - 1;
          v[u][h] = src[index(ly, lx, inside[u][h])];
        }
#pragma unroll
      for (int u = 0; u < kStageColumns; u++)
#pragma unroll
        for (int h = 0; h < 2; h++) asm volatile("" : "+v"(v[u][h]));
#pragma unroll
      for (int u = 0; u < kStageColumns; u++)
#pragma unroll
        for (int h = 0; h < 2; h++)
          if (lx0 + u * kWaves < cols && ly0 + h * kWave < rows) tile[cell(ly0 + h * kWave, lx0 + u * kWaves)] = inside[u][h] ? v[u][h] : (T)0;
    }
}

template <class T, int R, bool ACC>
__global__ void __launch_bounds__(kBlock) conv2d_strided_forward_kernel(T* res, const T* rhs, const c2s::Geometry g, const c2s::Tap<T>* __restrict__ taps, int ntaps,
                                                                        int tile_y, int tile_x, unsigned tiles_y, unsigned tiles_x) {
  extern __shared__ __align__(16) unsigned char conv2d_strided_lds[];
  T* tile = reinterpret_cast<T*>(conv2d_strided_lds);
  unsigned b = blockIdx.x;
  const unsigned by = b % tiles_y;
  b /= tiles_y;
  const unsigned bx = b % tiles_x, plane = b / tiles_x;
  const int y0 = (int)by * tile_y, x0 = (int)bx * tile_x;
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const T* src = rhs + (size_t)plane * (size_t)g.ny * (size_t)g.nx;
  const int rows = c2s::ForwardRows(tile_y, g.ky, g.sy), cols = c2s::ForwardColumns(tile_x, g.kx, g.sx), sub = c2s::SubPitch(tile_y, g.ky, g.sy);
  stage_tile(tile, src, rows, cols, lane, wave, [&](int ly, int lx, bool& inside) { return c2s::ForwardSourceIndex(g, y0, x0, ly, lx, inside); },
             [&](int ly, int lx) { return c2s::ForwardCell(ly, lx, g.sy, sub); });
  __syncthreads();
  const int ty = (int)threadIdx.x & (tile_y - 1), tx = ((int)threadIdx.x / tile_y) * R;      // tile_y is 64 or 32
  if (tx >= tile_x || x0 + tx >= g.mx) return;
  const int xstep = g.sx * g.sy * sub;
  T acc[R];
  c2s::ForwardMarch<T, R>(acc, tile + ty + tx * xstep, xstep, taps, ntaps);
  c2s::ForwardStore<T, R, ACC>(res + (size_t)plane * (size_t)g.my * (size_t)g.mx, g, y0 + ty, x0 + tx, acc);
}

/// the SY results of a lane and column: one vector access where all rows exist and the address allows, else one element at a time
template <class T, int SY, bool ACC>
__device__ __forceinline__ void adjoint_store(T* plane, const c2s::Geometry& g, int v, int u, const T (&acc)[SY]) {
  if constexpr (SY == 2 || SY == 4) {
    constexpr int kBytes = SY * sizeof(T) > 16 ? 16 : SY * sizeof(T), kN = kBytes / (int)sizeof(T);
    typedef T Vec __attribute__((ext_vector_type(kN)));
    T* p = plane + (size_t)v + (size_t)u * (size_t)g.ny;
    if (u < g.nx && v + SY <= g.ny && reinterpret_cast<uintptr_t>(p) % kBytes == 0) {
#pragma unroll
      for (int q = 0; q < SY / kN; q++) {
        Vec* pv = reinterpret_cast<Vec*>(p) + q;
        Vec val;
        if (ACC) val = *pv;
#pragma unroll
        for (int e = 0; e < kN; e++) val[e] = ACC ? val[e] + acc[q * kN + e] : acc[q * kN + e];
        *pv = val;
      }
      return;
    }
  }
  c2s::AdjointStoreElements<T, SY, ACC>(plane, g, v, u, acc);
}

template <class T, int SY, bool ACC>
__global__ void __launch_bounds__(kBlock) conv2d_strided_adjoint_kernel(T* res, const T* rhs, const c2s::Geometry g, const c2s::Tap<T>* __restrict__ taps,
                                                                        unsigned tiles_y, unsigned tiles_x) {
  extern __shared__ __align__(16) unsigned char conv2d_strided_lds[];
  T* tile = reinterpret_cast<T*>(conv2d_strided_lds);
  unsigned b = blockIdx.x;
  const unsigned by = b % tiles_y;
  b /= tiles_y;
  const unsigned bx = b % tiles_x, plane = b / tiles_x;
  const int v0 = (int)by * c2s::kAdjLanes * SY, u0 = (int)bx * c2s::kAdjColumns;
  const int lane = threadIdx.x % kWave, wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
  const T* src = rhs + (size_t)plane * (size_t)g.my * (size_t)g.mx;
  const int pitch = c2s::AdjointPitch(g), cols = c2s::AdjointColumns(g, u0), X0 = c2s::AdjointFirstColumn(g, u0);
  stage_tile(tile, src, pitch, cols, lane, wave, [&](int ly, int lx, bool& inside) { return c2s::AdjointSourceIndex(g, v0, u0, ly, lx, inside); },
             [&](int ly, int lx) { return ly + lx * pitch; });
  __syncthreads();
  const int v = v0 + lane * SY;
  T* dst = res + (size_t)plane * (size_t)g.ny * (size_t)g.nx;
#pragma unroll
  for (int r = 0; r < c2s::kAdjOutputs; r++) {
    const int u = u0 + wave * c2s::kAdjOutputs + r;
    if (u >= g.nx) break;                    // wave-uniform
    T acc[SY];
    c2s::AdjointMarch<T, SY>(acc, tile + lane, g, u, X0, pitch, taps);
    if (v < g.ny) adjoint_store<T, SY, ACC>(dst, g, v, u, acc);
  }
}

template <class T, class TapRecord>
static int launch_conv2d_strided(const prost_hip_conv2d_strided_geometry* geometry, const TapRecord* taps, size_t ntaps, T* res, const T* rhs, int accumulate,
                                 void* stream) {
  if (!geometry) { set_error("conv2d_strided: null geometry"); return 1; }
  c2s::Geometry g;
  std::memcpy(&g, geometry, sizeof(g));
  if (g.ky < 1 || g.kx < 1 || g.ky > c2s::kMaxWindow || g.kx > c2s::kMaxWindow) { set_error("conv2d_strided: the window has to be 1 x 1 to 31 x 31"); return 1; }
  if (g.sy < 1 || g.sx < 1 || g.sy > c2s::kMaxStride || g.sx > c2s::kMaxStride) { set_error("conv2d_strided: the stride has to be 1 .. 4 per axis"); return 1; }
  if (g.py < 0 || g.px < 0 || g.py >= g.sy || g.px >= g.sx) { set_error("conv2d_strided: the phase has to be 0 .. stride - 1"); return 1; }
  if (g.ny < 1 || g.nx < 1 || g.my < 1 || g.mx < 1 || g.planes < 1) { set_error("conv2d_strided: plane sizes and the plane count have to be at least 1"); return 1; }
  if (g.oy < 0 || g.ox < 0 || g.oy >= g.ky || g.ox >= g.kx) { set_error("conv2d_strided: the crop offset has to lie inside the window"); return 1; }
  if (ntaps < 1 || ntaps > (size_t)(g.ky * g.kx)) { set_error("conv2d_strided: the tap count has to be 1 .. ky kx"); return 1; }
  if (g.class_start[0] != 0 || g.class_start[c2s::kClasses] != (int32_t)ntaps) { set_error("conv2d_strided: the class table has to run from 0 to the tap count"); return 1; }
  for (int c = 0; c < c2s::kClasses; c++)
    if (g.class_start[c] > g.class_start[c + 1]) { set_error("conv2d_strided: the class table has to ascend"); return 1; }
  const uint64_t kLimit = (uint64_t)1 << 31;
  if ((uint64_t)g.ny * (uint64_t)g.nx >= kLimit || (uint64_t)g.my * (uint64_t)g.mx >= kLimit) { set_error("conv2d_strided: a plane has to stay below 2^31 elements"); return 1; }
  if ((uint64_t)g.ny + 1024 >= kLimit || (uint64_t)g.nx + 1024 >= kLimit || (uint64_t)g.my * (uint64_t)g.sy + 1024 >= kLimit || (uint64_t)g.mx * (uint64_t)g.sx + 1024 >= kLimit) {
    set_error("conv2d_strided: a side of a plane has to stay below 2^31 - 1024"); return 1;
  }
  if (!res || !rhs || !taps) { set_error("conv2d_strided: null pointer"); return 1; }
  const c2s::Tap<T>* table = reinterpret_cast<const c2s::Tap<T>*>(taps);
  hipStream_t s = as_stream(stream);
  const dim3 block(kBlock);
  if (!g.transpose) {
    const int pick = c2s::PickTile(sizeof(T), g.sy, g.sx, g.ky, g.kx);
    if (pick < 0) { set_error("conv2d_strided: no tile fits the LDS"); return 1; }
    const c2s::Tile tl = c2s::kTiles[pick];
    const uint64_t tiles_y = ((uint64_t)g.my + tl.ty - 1) / tl.ty, tiles_x = ((uint64_t)g.mx + tl.tx - 1) / tl.tx, blocks = tiles_y * tiles_x * (uint64_t)g.planes;
    if (blocks > (uint64_t)0x7fffffff) { set_error("conv2d_strided: more than 2^31 - 1 tiles"); return 1; }
    const size_t lds = c2s::ForwardLdsElements(tl, g.ky, g.kx, g.sy, g.sx) * sizeof(T);
    const dim3 grid((unsigned)blocks);
#define PROST_C2S_FORWARD(R, ACC) \
  PH_LAUNCH((conv2d_strided_forward_kernel<T, R, ACC>), grid, block, lds, s, res, rhs, g, table, (int)ntaps, tl.ty, tl.tx, (unsigned)tiles_y, (unsigned)tiles_x)
    if (tl.outputs == 4) { if (accumulate) PROST_C2S_FORWARD(4, true); else PROST_C2S_FORWARD(4, false); }
    else if (tl.outputs == 2) { if (accumulate) PROST_C2S_FORWARD(2, true); else PROST_C2S_FORWARD(2, false); }
    else { if (accumulate) PROST_C2S_FORWARD(1, true); else PROST_C2S_FORWARD(1, false); }
#undef PROST_C2S_FORWARD
    PH_LAUNCH_END("conv2d_strided forward kernel");
  }
  const uint64_t rows_per_tile = (uint64_t)c2s::kAdjLanes * (uint64_t)g.sy;
  const uint64_t tiles_y = ((uint64_t)g.ny + rows_per_tile - 1) / rows_per_tile, tiles_x = ((uint64_t)g.nx + c2s::kAdjColumns - 1) / c2s::kAdjColumns;
  const uint64_t blocks = tiles_y * tiles_x * (uint64_t)g.planes;
  if (blocks > (uint64_t)0x7fffffff) { set_error("conv2d_strided: more than 2^31 - 1 tiles"); return 1; }
  const size_t lds = (size_t)c2s::AdjointPitch(g) * (size_t)c2s::AdjointColumnBound(g) * sizeof(T);
  if (lds > c2s::kLdsLimit) { set_error("conv2d_strided: the adjoint tile does not fit the LDS"); return 1; }
  const dim3 grid((unsigned)blocks);
#define PROST_C2S_ADJOINT(SY, ACC) PH_LAUNCH((conv2d_strided_adjoint_kernel<T, SY, ACC>), grid, block, lds, s, res, rhs, g, table, (unsigned)tiles_y, (unsigned)tiles_x)
  switch (g.sy) {
    case 1: if (accumulate) PROST_C2S_ADJOINT(1, true); else PROST_C2S_ADJOINT(1, false); break;
    case 2: if (accumulate) PROST_C2S_ADJOINT(2, true); else PROST_C2S_ADJOINT(2, false); break;
    case 3: if (accumulate) PROST_C2S_ADJOINT(3, true); else PROST_C2S_ADJOINT(3, false); break;
    default: if (accumulate) PROST_C2S_ADJOINT(4, true); else PROST_C2S_ADJOINT(4, false); break;
  }
#undef PROST_C2S_ADJOINT
  PH_LAUNCH_END("conv2d_strided adjoint kernel");
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_conv2d_strided_f32(const prost_hip_conv2d_strided_geometry* geometry, const prost_hip_conv2d_tap_f32* taps, size_t ntaps, float* res, const float* rhs,
                                 int accumulate, void* stream) {
  return launch_conv2d_strided<float>(geometry, taps, ntaps, res, rhs, accumulate, stream);
}
int prost_hip_conv2d_strided_f64(const prost_hip_conv2d_strided_geometry* geometry, const prost_hip_conv2d_tap_f64* taps, size_t ntaps, double* res, const double* rhs,
                                 int accumulate, void* stream) {
  return launch_conv2d_strided<double>(geometry, taps, ntaps, res, rhs, accumulate, stream);
}
}  // extern "C"
