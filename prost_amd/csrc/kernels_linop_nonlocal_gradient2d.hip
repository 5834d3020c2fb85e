// kernels_linop_nonlocal_gradient2d.hip -- BlockNonlocalGradient2D: res (+)= K rhs and res (+)= K^T rhs for the nonlocal gradient
// (K u)_m[p] = w_m(p) (u[p + d_m] - u[p]) of L channels of an ny x nx grid, M displacements inside a window of reach 15 and one weight
// plane per displacement shared by all channels, without a matrix.  The arithmetic, its order, the tile table and the cells a lane walks
// are include/prost/linop/nonlocal_gradient2d.hpp, which also runs on the host (tests/host/nonlocal_gradient2d_harness.cpp).  This file
// decides who reads what.
//
// A workgroup of 256 lanes owns a tile of 64 x 16 pixels and the channels of one pass (the header's tile table: as many as keep the
// staged tiles within 64 KiB, four at most); y runs across the lanes.  The displacements are a kernel argument (M int8 pairs by value),
// so the walk over m reads them through scalar loads.  Forward: the tile of u with a halo of the block's actual reach is staged in LDS
// once per channel of the pass, then each lane walks m, loads its weights once and uses them for every channel it holds: compulsory
// traffic (M + M L + L) N values, not (2 M L + L) N.  Adjoint: a gather -- the outgoing terms as one access at p, the incoming terms
// at p - d_m straight from memory (the neighbouring tiles' lines are in the cache): the vector kernels load the aligned pair of 16-byte
// groups that holds them and pick by dy mod the vector width, which is the same for every lane; no LDS, no atomics, a repeated call
// repeats its bits.  Vector kernels: a lane owns 16 bytes of a column (heights that are a multiple of the vector width; res, rhs
// and weights 16-byte aligned); element kernels: one row per lane, any alignment.  Resource table and rates: docs/rounds/r30.md.
#include <cmath>

#include "elementwise.hpp"
#include "fused_op.hpp"
#include "prost/linop/nonlocal_gradient2d.hpp"

namespace prost_hip {

namespace nlg2 = prost::nonlocal_gradient2d;

/// v[j] = j + S < W ? a[j + S] : b[j + S - W]: the W values that start S values into the aligned pair (a, b)
template <class T, int W, int S>
__device__ __forceinline__ void pick_shifted(const T (&a)[W], const T (&b)[W], T (&v)[W]) {
#pragma unroll
  for (int j = 0; j < W; j++) v[j] = j + S < W ? a[(j + S) % W] : b[(j + S) % W];
}

/// W rows as one access of W values (16 bytes, or one element)
template <class T, int W> struct NonlocalMover {
  __device__ __forceinline__ void load(const T* p, T (&v)[W], int) const { ldv<T, W>(p, v); }
  __device__ __forceinline__ void store(T* p, const T (&v)[W], int) const { stv<T, W>(p, v); }
  /// the W rows from row0 - dy on of column xq.  They straddle two aligned groups of W rows unless dy is a multiple of W; heights and
  /// row0 are multiples of W here, so a group lies in one column, it lies in the grid as soon as one of its rows does, and the shift
  /// into the pair depends on dy alone: it is the same for every lane, and so is the branch.  Two 16-byte loads instead of W
  /// element loads 16 bytes apart; a group outside the grid is not loaded, and its rows are never selected.
  __device__ __forceinline__ void gather(const T* plane, long xq, long row0, int dy, long nx, long ny, T (&v)[W]) const {
    if (W == 1) {
      const long row = row0 - dy;
      v[0] = xq >= 0 && xq < nx && row >= 0 && row < ny ? plane[(size_t)xq * (size_t)ny + (size_t)row] : (T)0;
      return;
    }
    const int shift = ((-dy) % W + W) % W;
    const long first = row0 - dy - shift;               // a multiple of W
    const bool xin = xq >= 0 && xq < nx;
    T a[W], b[W];
#pragma unroll
    for (int j = 0; j < W; j++) { a[j] = (T)0; b[j] = (T)0; }
    if (xin && first >= 0 && first + W <= ny) ldv<T, W>(plane + (size_t)xq * (size_t)ny + (size_t)first, a);
    if (shift != 0 && xin && first + W >= 0 && first + 2 * W <= ny) ldv<T, W>(plane + (size_t)xq * (size_t)ny + (size_t)(first + W), b);
    if (shift == 0) pick_shifted<T, W, 0>(a, b, v);
    else if (shift == 1) pick_shifted<T, W, 1 % W>(a, b, v);
    else if (shift == 2) pick_shifted<T, W, 2 % W>(a, b, v);
    else pick_shifted<T, W, 3 % W>(a, b, v);
  }
};

extern __shared__ __align__(16) unsigned char nonlocal_lds[];

// res and rhs are not __restrict__ here: the accumulating forms read res through the same Mover
template <class T, int W, bool ADJ, bool ACC>
__global__ void __launch_bounds__(nlg2::kThreads) nonlocal_grad2d_kernel(T* res, const T* rhs, const T* weights, const nlg2::Offsets offsets, int M, size_t nx, size_t ny, size_t L,
                                                                         unsigned tiles_y, unsigned tiles_x, int pass, int ry, int rx) {
  const unsigned by = blockIdx.x % tiles_y, bx = (blockIdx.x / tiles_y) % tiles_x;
  const size_t c0 = (size_t)(blockIdx.x / (tiles_y * tiles_x)) * (size_t)pass;
  const int C = L - c0 < (size_t)pass ? (int)(L - c0) : pass;
  const nlg2::Tile t = {(long)by * nlg2::kTileY, (long)bx * nlg2::kTileX, nlg2::kTileY, nlg2::kTileX, ry, rx};
  const NonlocalMover<T, W> mv;
  T* staged = reinterpret_cast<T*>(nonlocal_lds);
  if (!ADJ) {
    nlg2::StageTile<T>(staged, t, rhs, nx, ny, c0, C, (int)threadIdx.x, nlg2::kThreads);
    __syncthreads();
  }
  for (int step = 0; step < nlg2::Steps<W>(t, nlg2::kThreads); step++) {
    size_t row0, x;
    if (!nlg2::CellOf<W>(t, (int)threadIdx.x, nlg2::kThreads, step, row0, x)) continue;
    if (ADJ) nlg2::AdjointCell<T, W, ACC>(mv, res, rhs, weights, offsets, M, nx, ny, L, c0, C, row0, x);
    else nlg2::ForwardCell<T, W, ACC>(mv, res, staged, t, weights, offsets, M, nx, ny, L, c0, C, row0, x);
  }
}

template <class T, int W>
static int launch_nonlocal_grad2d_as(T* res, const T* rhs, const T* weights, const nlg2::Offsets& offsets, int M, size_t nx, size_t ny, size_t L, int transpose,
                                     int accumulate, hipStream_t s) {
  int ry, rx;
  nlg2::Reach(offsets, M, ry, rx);
  const int pass = nlg2::PassChannels(ry > rx ? ry : rx, sizeof(T));
  const size_t tiles_y = (ny + nlg2::kTileY - 1) / nlg2::kTileY, tiles_x = (nx + nlg2::kTileX - 1) / nlg2::kTileX, passes = (L + pass - 1) / pass;
  if (tiles_y >= (1ull << 31) || tiles_x >= (1ull << 31) || (long double)tiles_y * (long double)tiles_x * (long double)passes >= 2147483648.0L) {
    set_error("nonlocal_gradient2d: more than 2^31 - 1 workgroups");
    return 1;
  }
  const size_t blocks = tiles_y * tiles_x * passes;
  const size_t lds = transpose ? 0 : (size_t)pass * nlg2::TileValues(nlg2::kTileY, nlg2::kTileX, ry, rx) * sizeof(T);
  if (lds > nlg2::kLdsLimit) { set_error("nonlocal_gradient2d: the staged tiles exceed 64 KiB"); return 1; }
#define GO(ADJv, ACCv) PH_LAUNCH((nonlocal_grad2d_kernel<T, W, ADJv, ACCv>), dim3((unsigned)blocks), dim3(nlg2::kThreads), lds, s, res, rhs, weights, offsets, M, nx, ny, L, (unsigned)tiles_y, (unsigned)tiles_x, pass, ry, rx)
  if (!transpose) { if (accumulate) GO(false, true); else GO(false, false); }
  else { if (accumulate) GO(true, true); else GO(true, false); }
#undef GO
  PH_LAUNCH_END("nonlocal_gradient2d kernel");
}

template <class T>
static int launch_nonlocal_grad2d(T* res, const T* rhs, const T* weights, size_t nx, size_t ny, size_t L, int M, const signed char* offsets, int transpose, int accumulate,
                                  void* stream) {
  if (nx == 0 || ny == 0 || L == 0) { set_error("nonlocal_gradient2d: nx, ny and L have to be at least 1"); return 1; }
  if (M < 1 || M > nlg2::kMaxOffsets) { set_error("nonlocal_gradient2d: the number of offsets has to be 1 .. 64"); return 1; }
  if (!res || !rhs || !weights || !offsets) { set_error("nonlocal_gradient2d: null pointer"); return 1; }
  if ((long double)M * (long double)nx * (long double)ny * (long double)L > 9007199254740992.0L) { set_error("nonlocal_gradient2d: M L nx ny has to stay within 2^53"); return 1; }
  nlg2::Offsets o = {};
  for (int m = 0; m < M; m++) {
    o.dy[m] = offsets[2 * m];
    o.dx[m] = offsets[2 * m + 1];
    if (o.dy[m] < -nlg2::kMaxReach || o.dy[m] > nlg2::kMaxReach || o.dx[m] < -nlg2::kMaxReach || o.dx[m] > nlg2::kMaxReach) {
      set_error("nonlocal_gradient2d: an offset reaches beyond 15");
      return 1;
    }
    if (o.dy[m] == 0 && o.dx[m] == 0) { set_error("nonlocal_gradient2d: the offset (0, 0) is no displacement"); return 1; }
  }
  constexpr int V = VecOf<T>::N;
  hipStream_t s = as_stream(stream);
  if (ny % V == 0 && aligned16(res) && aligned16(rhs) && aligned16(weights)) return launch_nonlocal_grad2d_as<T, V>(res, rhs, weights, o, M, nx, ny, L, transpose, accumulate, s);
  return launch_nonlocal_grad2d_as<T, 1>(res, rhs, weights, o, M, nx, ny, L, transpose, accumulate, s);
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_linop_nonlocal_gradient2d_f32(float* res, const float* rhs, const float* weights, size_t nx, size_t ny, size_t L, int M, const signed char* offsets, int transpose,
                                            int accumulate, void* stream) {
  return launch_nonlocal_grad2d<float>(res, rhs, weights, nx, ny, L, M, offsets, transpose, accumulate, stream);
}
int prost_hip_linop_nonlocal_gradient2d_f64(double* res, const double* rhs, const double* weights, size_t nx, size_t ny, size_t L, int M, const signed char* offsets, int transpose,
                                            int accumulate, void* stream) {
  return launch_nonlocal_grad2d<double>(res, rhs, weights, nx, ny, L, M, offsets, transpose, accumulate, stream);
}
}  // extern "C"
