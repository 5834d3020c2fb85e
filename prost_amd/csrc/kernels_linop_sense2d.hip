// kernels_linop_sense2d.hip -- BlockSense2D: res (+)= K rhs and res (+)= K^T rhs for the multi-coil Fourier operator of parallel MRI,
// K u = [ F (sigma_c . u) ]_c, without a matrix, without an intermediate field of C images and without a separate pointwise launch.  The
// arithmetic -- the complex products, the order of the coil sum, and through fft2d.hpp the tree, the table, the passes and the scaling -- is
// include/prost/linop/sense2d.hpp, which also runs on the host (tests/host/sense2d_harness.cpp).  The tiles, their LDS layout, the stage
// loop and the conditions of the 16-byte accesses are those of kernels_linop_fft2d.hip (fft2d_tile.hpp).  This file adds the two fused
// passes:
//
//   forward, first pass (the y pass, or the only pass): sense2d_forward_kernel.  The grid's plane axis runs over the L C range images
//       j = l C + c.  A lane reads rhs of image l and the map of coil c at the same offsets, forms z = sigma u and writes it into LDS;
//       everything after the load is fft2d's pass.  With two passes the second one IS fft2d's x pass on L C images (fft2d_launch_pass).
//   transpose, last pass (the x pass, or the only pass): sense2d_sum_kernel.  With two passes the first one IS fft2d's y pass on L C
//       images into the work buffer.  A workgroup owns one tile of image l and loops over the coils: it loads the tile of range image
//       l C + c, runs the stages, and each lane takes its own output elements from LDS, scales them by s, forms the term with the
//       conjugate map and adds it to accumulators in registers -- 8 complex values per lane with the small tile, 32 (fp32) or 16 (fp64)
//       with the large one; a lane holds the same elements in every coil.  One store (or read-add-store) after the last coil.
//
// No atomics, no scratch, no reduction launch: a repeated call repeats its bits.  16 bytes per lane when res / work, rhs AND the maps are
// 16-byte aligned and a contiguous run of the tile holds that many values (fft_tile_wide).
//
// Tile choice of the coil-summing pass (launch_sum_pass): the small tile for the y pass and for nx <= 512, else fft2d's large one.  The
// pass has only (lines / B) x L workgroups because the coils are summed inside the workgroup, so a smaller slab trades coalescing for
// workgroups: measured with L = 1 in fp32, the small tile (32 workgroups at 256 x 256, 128 at 512 x 512) is 2.1 to 2.4 times faster than
// the large one (8 and 32 workgroups) and at 2048 x 2048 (a slab of one row) 1.75 times slower.  The record's tile selector forces either.
// Measured (docs/rounds/r33.md): the forward product costs what fft2d on the L C images costs; the transposed product is still 2 to 3
// times slower than fft2d plus a pointwise pass at 256 x 256 to 512 x 512 and 1.07 times at 2048 x 2048 x 4.
#include <cstring>

#include "fft2d_tile.hpp"
#include "prost/linop/sense2d.hpp"

namespace prost_hip {

namespace s2d = prost::sense2d;

static_assert(sizeof(s2d::Geometry) == sizeof(prost_hip_sense2d_geometry), "geometry record");

/// blockIdx.x: a tile of 2^lb lines; blockIdx.y: range image j = l C + c.  src: the L domain images; dst: the L C range images (res, or the
/// work buffer with MODE == kToWork)
template <class T, bool XPASS, int MODE, int ELEMS, int W>
__global__ void __launch_bounds__(kBlock) sense2d_forward_kernel(T* dst, const T* src, const T* __restrict__ maps, const s2d::Geometry g, const T* __restrict__ table, T s,
                                                                 int lm, int lb, int pitch, int ltab) {
  __shared__ T re[ELEMS], im[ELEMS];
  const size_t N = (size_t)g.ny * (size_t)g.nx, L = (size_t)g.planes, C = (size_t)g.coils, J = L * C;
  const int count = 1 << (lm + lb);
  const size_t base = fft_tile_base<XPASS>(blockIdx.x, lm, lb);
  for (size_t j = blockIdx.y; j < J; j += gridDim.y) {
    const size_t l = j / C, c = j - l * C;
    const T *ur = src + l * N + base, *ui = src + (L + l) * N + base, *mr = maps + c * N + base, *mi = maps + (C + c) * N + base;
    for (int f = (int)threadIdx.x * W; f < count; f += kBlock * W) {
      const size_t at = fft_tile_at<XPASS>(f, lb, g.ny);
      const int in = fft_tile_in<XPASS>(f, lm, pitch);
      const FftPack<T, W> vr = *reinterpret_cast<const FftPack<T, W>*>(ur + at), vi = *reinterpret_cast<const FftPack<T, W>*>(ui + at);
      const FftPack<T, W> wr = *reinterpret_cast<const FftPack<T, W>*>(mr + at), wi = *reinterpret_cast<const FftPack<T, W>*>(mi + at);
#pragma unroll
      for (int w = 0; w < W; w++) {
        const f2d::Cx<T> u = {vr.v[w], vi.v[w]};
        const f2d::Cx<T> z = s2d::Product<T>(u, wr.v[w], wi.v[w]);
        re[in + w] = z.re; im[in + w] = z.im;
      }
    }
    __syncthreads();
    fft_tile_stages<T, false, XPASS, ELEMS>(re, im, lm, lb, pitch, table, ltab);
    T *dr = dst + j * N + base, *di = dst + (J + j) * N + base;
    for (int f = (int)threadIdx.x * W; f < count; f += kBlock * W) {
      const size_t at = fft_tile_at<XPASS>(f, lb, g.ny);
      const int in = fft_tile_in<XPASS>(f, lm, pitch);
      FftPack<T, W> vr, vi;
      if (MODE == kFinalAdd) { vr = *reinterpret_cast<const FftPack<T, W>*>(dr + at); vi = *reinterpret_cast<const FftPack<T, W>*>(di + at); }
#pragma unroll
      for (int w = 0; w < W; w++) { fft_store<T, MODE>(&vr.v[w], re[in + w], s); fft_store<T, MODE>(&vi.v[w], im[in + w], s); }
      *reinterpret_cast<FftPack<T, W>*>(dr + at) = vr; *reinterpret_cast<FftPack<T, W>*>(di + at) = vi;
    }
    __syncthreads();
  }
}

/// blockIdx.x: a tile of 2^lb lines; blockIdx.y: domain image l.  src: the L C range images (rhs, or the work buffer behind fft2d's y
/// pass); dst: the L domain images of res
template <class T, bool XPASS, bool ACC, int ELEMS, int W>
__global__ void __launch_bounds__(kBlock) sense2d_sum_kernel(T* dst, const T* src, const T* __restrict__ maps, const s2d::Geometry g, const T* __restrict__ table, T s, int lm,
                                                             int lb, int pitch, int ltab) {
  __shared__ T re[ELEMS], im[ELEMS];
  constexpr int kPer = ELEMS / kBlock / W;                         // packs a lane holds: ELEMS / kBlock complex accumulators
  const size_t N = (size_t)g.ny * (size_t)g.nx, L = (size_t)g.planes, C = (size_t)g.coils, J = L * C;
  const int count = 1 << (lm + lb);
  const size_t base = fft_tile_base<XPASS>(blockIdx.x, lm, lb);
  for (size_t l = blockIdx.y; l < L; l += gridDim.y) {
    FftPack<T, W> ar[kPer], ai[kPer];
    for (size_t c = 0; c < C; c++) {
      const size_t j = l * C + c;
      const T *sr = src + j * N + base, *si = src + (J + j) * N + base, *mr = maps + c * N + base, *mi = maps + (C + c) * N + base;
      for (int f = (int)threadIdx.x * W; f < count; f += kBlock * W) {
        const size_t at = fft_tile_at<XPASS>(f, lb, g.ny);
        const int in = fft_tile_in<XPASS>(f, lm, pitch);
        const FftPack<T, W> vr = *reinterpret_cast<const FftPack<T, W>*>(sr + at), vi = *reinterpret_cast<const FftPack<T, W>*>(si + at);
#pragma unroll
        for (int w = 0; w < W; w++) { re[in + w] = vr.v[w]; im[in + w] = vi.v[w]; }
      }
      __syncthreads();
      fft_tile_stages<T, true, XPASS, ELEMS>(re, im, lm, lb, pitch, table, ltab);
#pragma unroll
      for (int i = 0; i < kPer; i++) {
        const int f = ((int)threadIdx.x + i * kBlock) * W;
        if (f < count) {
          const size_t at = fft_tile_at<XPASS>(f, lb, g.ny);
          const int in = fft_tile_in<XPASS>(f, lm, pitch);
          const FftPack<T, W> wr = *reinterpret_cast<const FftPack<T, W>*>(mr + at), wi = *reinterpret_cast<const FftPack<T, W>*>(mi + at);
#pragma unroll
          for (int w = 0; w < W; w++) {
            const f2d::Cx<T> v = {re[in + w] * s, im[in + w] * s};
            const f2d::Cx<T> t = s2d::ConjProduct<T>(v, wr.v[w], wi.v[w]);
            if (c == 0) { ar[i].v[w] = t.re; ai[i].v[w] = t.im; }
            else { ar[i].v[w] = ar[i].v[w] + t.re; ai[i].v[w] = ai[i].v[w] + t.im; }
          }
        }
      }
      __syncthreads();                                             // the next coil's tile overwrites re / im
    }
    T *dr = dst + l * N + base, *di = dst + (L + l) * N + base;
#pragma unroll
    for (int i = 0; i < kPer; i++) {
      const int f = ((int)threadIdx.x + i * kBlock) * W;
      if (f < count) {
        const size_t at = fft_tile_at<XPASS>(f, lb, g.ny);
        FftPack<T, W> vr = ar[i], vi = ai[i];
        if (ACC) {
          const FftPack<T, W> pr = *reinterpret_cast<const FftPack<T, W>*>(dr + at), pi = *reinterpret_cast<const FftPack<T, W>*>(di + at);
#pragma unroll
          for (int w = 0; w < W; w++) { vr.v[w] = pr.v[w] + vr.v[w]; vi.v[w] = pi.v[w] + vi.v[w]; }
        }
        *reinterpret_cast<FftPack<T, W>*>(dr + at) = vr; *reinterpret_cast<FftPack<T, W>*>(di + at) = vi;
      }
    }
  }
}

/// kSlabAuto: the small tile up to nx = 512, where it was measured 2.1 to 2.4 times faster than fft2d's large tile in fp32 and 1.45 times
/// in fp64 (four times the workgroups), fft2d's choice beyond: at nx = 2048 the small tile is a slab of one row and 1.75 times slower;
/// nx = 1024 was not measured (docs/rounds/r33.md)
constexpr int kSumSmallTileMaxNx = 512;
static bool sum_pass_small_tile(const s2d::Geometry& g) { return g.nx <= kSumSmallTileMaxNx; }

static unsigned plane_grid(long images) { return (unsigned long)images < kFftMaxPlaneGrid ? (unsigned)images : kFftMaxPlaneGrid; }

template <class T, bool XPASS, int MODE, int ELEMS>
static void launch_forward_tile(T* dst, const T* src, const T* maps, const s2d::Geometry& g, const T* table, hipStream_t stream) {
  const FftTileShape t = fft_tile_shape<XPASS>(s2d::RangeGeometry(g, false), ELEMS);
  const dim3 grid(t.tiles, plane_grid((long)g.planes * g.coils)), block(kBlock);
  const T s = f2d::Scale<T>(g.ny, g.nx);
  constexpr int kWide = 16 / (int)sizeof(T);
  if (fft_tile_wide<T>(t, {dst, src, maps}))
    PH_LAUNCH((sense2d_forward_kernel<T, XPASS, MODE, ELEMS, kWide>), grid, block, 0, stream, dst, src, maps, g, table, s, t.lm, t.lb, t.pitch, t.ltab);
  else PH_LAUNCH((sense2d_forward_kernel<T, XPASS, MODE, ELEMS, 1>), grid, block, 0, stream, dst, src, maps, g, table, s, t.lm, t.lb, t.pitch, t.ltab);
}
template <class T, bool XPASS, int MODE>
static void launch_forward_pass(T* dst, const T* src, const T* maps, const s2d::Geometry& g, const T* table, hipStream_t stream) {
  if constexpr (!XPASS) {
    launch_forward_tile<T, XPASS, MODE, kFftSmallTile>(dst, src, maps, g, table, stream);
  } else {
    if (fft_small_tile<XPASS>(s2d::RangeGeometry(g, false))) launch_forward_tile<T, XPASS, MODE, kFftSmallTile>(dst, src, maps, g, table, stream);
    else launch_forward_tile<T, XPASS, MODE, FftTile<T>::kLarge>(dst, src, maps, g, table, stream);
  }
}

template <class T, bool XPASS, bool ACC, int ELEMS>
static void launch_sum_tile(T* dst, const T* src, const T* maps, const s2d::Geometry& g, const T* table, hipStream_t stream) {
  const FftTileShape t = fft_tile_shape<XPASS>(s2d::RangeGeometry(g, true), ELEMS);
  const dim3 grid(t.tiles, plane_grid(g.planes)), block(kBlock);
  const T s = f2d::Scale<T>(g.ny, g.nx);
  constexpr int kWide = 16 / (int)sizeof(T);
  if (fft_tile_wide<T>(t, {dst, src, maps}))
    PH_LAUNCH((sense2d_sum_kernel<T, XPASS, ACC, ELEMS, kWide>), grid, block, 0, stream, dst, src, maps, g, table, s, t.lm, t.lb, t.pitch, t.ltab);
  else PH_LAUNCH((sense2d_sum_kernel<T, XPASS, ACC, ELEMS, 1>), grid, block, 0, stream, dst, src, maps, g, table, s, t.lm, t.lb, t.pitch, t.ltab);
}
/// the tile of the coil-summing pass.  g.slab (the record's tile selector): kSlabAuto the choice of this file, kSlabSmall the small tile
/// whatever nx is (a slab of 2048 / nx rows), kSlabFft2d fft2d's choice.  The bits do not depend on it: every line runs the same tree
enum { kSlabAuto = 0, kSlabSmall = 1, kSlabFft2d = 2 };
template <class T, bool XPASS, bool ACC>
static void launch_sum_pass(T* dst, const T* src, const T* maps, const s2d::Geometry& g, const T* table, hipStream_t stream) {
  if constexpr (!XPASS) {
    launch_sum_tile<T, XPASS, ACC, kFftSmallTile>(dst, src, maps, g, table, stream);
  } else {
    const bool small = g.slab == kSlabSmall || (g.slab == kSlabAuto ? sum_pass_small_tile(g) : fft_small_tile<XPASS>(s2d::RangeGeometry(g, true)));
    if (small) launch_sum_tile<T, XPASS, ACC, kFftSmallTile>(dst, src, maps, g, table, stream);
    else launch_sum_tile<T, XPASS, ACC, FftTile<T>::kLarge>(dst, src, maps, g, table, stream);
  }
}

template <class T>
static bool launch_sense2d_forward(const s2d::Geometry& g, const T* table, const T* maps, T* work, T* res, const T* rhs, bool acc, hipStream_t s) {
  if (g.ny > 1 && g.nx > 1) {
    launch_forward_pass<T, false, kToWork>(work, rhs, maps, g, table, s);
    return fft2d_launch_pass<T>(false, true, acc ? kFinalAdd : kFinal, res, work, s2d::RangeGeometry(g, false), table, s);
  } else if (g.ny > 1) {
    if (acc) launch_forward_pass<T, false, kFinalAdd>(res, rhs, maps, g, table, s);
    else launch_forward_pass<T, false, kFinal>(res, rhs, maps, g, table, s);
  } else {                                                         // ny == 1: the x pass alone (nx == 1: no stage, the pointwise product)
    if (acc) launch_forward_pass<T, true, kFinalAdd>(res, rhs, maps, g, table, s);
    else launch_forward_pass<T, true, kFinal>(res, rhs, maps, g, table, s);
  }
  return true;
}
template <class T>
static bool launch_sense2d_transpose(const s2d::Geometry& g, const T* table, const T* maps, T* work, T* res, const T* rhs, bool acc, hipStream_t s) {
  if (g.ny > 1 && g.nx > 1) {
    if (!fft2d_launch_pass<T>(true, false, kToWork, work, rhs, s2d::RangeGeometry(g, true), table, s)) return false;
    if (acc) launch_sum_pass<T, true, true>(res, work, maps, g, table, s);
    else launch_sum_pass<T, true, false>(res, work, maps, g, table, s);
  } else if (g.ny > 1) {
    if (acc) launch_sum_pass<T, false, true>(res, rhs, maps, g, table, s);
    else launch_sum_pass<T, false, false>(res, rhs, maps, g, table, s);
  } else {
    if (acc) launch_sum_pass<T, true, true>(res, rhs, maps, g, table, s);
    else launch_sum_pass<T, true, false>(res, rhs, maps, g, table, s);
  }
  return true;
}

template <class T>
static int launch_sense2d(const prost_hip_sense2d_geometry* geometry, const T* table, const T* maps, T* work, T* res, const T* rhs, int accumulate, void* stream) {
  if (!geometry) { set_error("sense2d: null geometry"); return 1; }
  s2d::Geometry g;
  std::memcpy(&g, geometry, sizeof(g));
  if (!f2d::IsSide(g.ny) || !f2d::IsSide(g.nx)) { set_error("sense2d: nx and ny have to be powers of two from 1 to 2048"); return 1; }
  if (g.planes < 1) { set_error("sense2d: the image count has to be at least 1"); return 1; }
  if (g.coils < 1 || g.coils > s2d::kMaxCoils) { set_error("sense2d: the coil count has to be from 1 to 64"); return 1; }
  if (2 * (uint64_t)g.planes * (uint64_t)g.coils * (uint64_t)g.ny * (uint64_t)g.nx >= ((uint64_t)1 << 31)) { set_error("sense2d: 2 L C nx ny has to stay below 2^31"); return 1; }
  if (g.slab < 0 || g.slab > 2) { set_error("sense2d: the tile selector has to be 0, 1 or 2"); return 1; }
  if (!table || !maps || !work || !res || !rhs) { set_error("sense2d: null pointer"); return 1; }
  hipStream_t s = as_stream(stream);
  const bool launched = g.transpose ? launch_sense2d_transpose<T>(g, table, maps, work, res, rhs, accumulate != 0, s)
                                    : launch_sense2d_forward<T>(g, table, maps, work, res, rhs, accumulate != 0, s);
  if (!launched) { set_error("sense2d: fft2d has no such pass"); return 1; }
  PH_LAUNCH_END("sense2d kernel");
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_sense2d_f32(const prost_hip_sense2d_geometry* geometry, const float* table, const float* maps, float* work, float* res, const float* rhs, int accumulate,
                          void* stream) {
  return launch_sense2d<float>(geometry, table, maps, work, res, rhs, accumulate, stream);
}
int prost_hip_sense2d_f64(const prost_hip_sense2d_geometry* geometry, const double* table, const double* maps, double* work, double* res, const double* rhs, int accumulate,
                          void* stream) {
  return launch_sense2d<double>(geometry, table, maps, work, res, rhs, accumulate, stream);
}
}  // extern "C"
