// kernels_linop_fft2d.hip -- BlockFFT2D: res (+)= K rhs and res (+)= K^T rhs for the unitary 2-D discrete Fourier transform K of L
// complex images, without a matrix and without a library.  The arithmetic -- the radix-2 tree, the twiddle table, which products are
// skipped, the order of the passes, the scaling -- is include/prost/linop/fft2d.hpp, which also runs on the host
// (tests/host/fft2d_harness.cpp).  This file decides who holds what.
//
// A workgroup of 256 lanes owns a tile of B whole lines of m points in LDS, real and imaginary parts in two static arrays.  Two tile
// sizes: 2048 complex values (16 KiB in fp32, 32 KiB in fp64: ten or five workgroups on a CU, one tile's loads overlap another's
// stages) and 64 KiB (8192 values in fp32, 4096 in fp64: two workgroups on a CU).  A stage of the tree is one step: every lane reads
// the two inputs of its butterflies (4 with the small tile, 16 / 8 with the large one, in registers), the workgroup synchronises, every
// lane writes its two outputs, the workgroup synchronises.  One array pair serves every stage; there is no permutation pass
// (fft2d.hpp: Stockham order).
//
//   y pass (lines contiguous):  the small tile; B consecutive columns, a contiguous stretch of B ny values per plane, read and written
//       coalesced, line after line in LDS.  Butterflies: j fastest.
//   x pass (lines of stride ny): the tile is a slab of B consecutive y and all nx, B = min(tile / nx, ny), read and written coalesced
//       along y: the small tile while it holds 16 rows (nx <= 128), else the large one (B = 32 .. 4 in fp32, 16 .. 2 in fp64: at
//       nx = 2048 in fp64 a row of the slab is 16 bytes, and the pass is far from coalesced).  In LDS element e of line b sits at
//       e B + b: butterflies b fastest, so both reads of a wave are contiguous.
//
// Global accesses: 16 bytes per lane (four fp32 or two fp64 values, consecutive in memory and in LDS) when src and dst of the pass are
// 16-byte aligned and a contiguous run of the tile -- a line of the y pass, the B rows of a slab of the x pass -- holds that many values;
// one value per lane otherwise (an odd element offset of the block inside the solver's vectors, a side of 2 in fp32).
//
// LDS banking (MI355X: ds_read_b32 / ds_write_b32 serve two groups of 32 lanes over 32 banks, ds_read_b64 two groups of 32 over 64
// banks, ds_write_b64 four groups of 16 over 32 banks).  The reads of a stage are contiguous over the lanes of a group: free of
// conflicts (y pass with lines shorter than 64: the lines are pitched at 3 m / 2, which puts the half-lines a group reads on distinct
// banks).  The writes go to runs of h values with gaps of h: for h below the group width two lanes of a group share a bank.  On
// ds_write_b32 a 2-way conflict costs nothing (the store's transfer to the LDS takes longer than its two array cycles); on
// ds_write_b64 the stages with h < 16 take 8 array cycles for 6 of transfer.  Nothing here was measured with counters.
//
// The last pass multiplies by s and stores (or adds to) res; with both passes the first one writes the block's work buffer.  Planes on
// the grid's y axis.  No scratch, no atomics: a repeated call repeats its bits.  Resource table: docs/rounds/r25.md.
#include <cstring>

#include "fft2d_tile.hpp"

namespace prost_hip {

static_assert(sizeof(f2d::Geometry) == sizeof(prost_hip_fft2d_geometry), "geometry record");

/// XPASS: lines of nx points at stride ny, the tile's lines are y0 .. y0 + B - 1; else lines of ny contiguous points, the tile's lines are
/// columns x0 .. x0 + B - 1
/// blockIdx.x: a tile of 2^lb lines.  W: values a lane moves per global access, 1 or 16 / sizeof(T); the launcher picks 16 bytes when src and
/// dst are 16-byte aligned and a contiguous run of the tile (a line of the y pass, the B rows of a slab) holds at least W values
template <class T, bool INV, bool XPASS, int MODE, int ELEMS, int W>
__global__ void __launch_bounds__(kBlock) fft2d_pass_kernel(T* dst, const T* src, const f2d::Geometry g, const T* __restrict__ table, T s, int lm, int lb,
                                                            int pitch, int ltab) {
  __shared__ T re[ELEMS], im[ELEMS];
  const size_t N = (size_t)g.ny * (size_t)g.nx, L = (size_t)g.planes;
  const int count = 1 << (lm + lb), m1 = (1 << lm) - 1, b1 = (1 << lb) - 1;
  // offset of the tile's first value inside a plane
  const size_t base = XPASS ? ((size_t)blockIdx.x << lb) : ((size_t)blockIdx.x << (lb + lm));
  for (size_t c = blockIdx.y; c < L; c += gridDim.y) {
    const T *sr = src + c * N + base, *si = src + (L + c) * N + base;
    // f .. f + W - 1 stay inside one contiguous run, in memory and in LDS
    for (int f = (int)threadIdx.x * W; f < count; f += kBlock * W) {
      const size_t at = XPASS ? (size_t)(f >> lb) * (size_t)g.ny + (size_t)(f & b1) : (size_t)f;
      const int in = XPASS ? f : (f >> lm) * pitch + (f & m1);
      const FftPack<T, W> vr = *reinterpret_cast<const FftPack<T, W>*>(sr + at), vi = *reinterpret_cast<const FftPack<T, W>*>(si + at);
#pragma unroll
      for (int w = 0; w < W; w++) { re[in + w] = vr.v[w]; im[in + w] = vi.v[w]; }
    }
    __syncthreads();
    fft_tile_stages<T, INV, XPASS, ELEMS>(re, im, lm, lb, pitch, table, ltab);
    T *dr = dst + c * N + base, *di = dst + (L + c) * N + base;
    for (int f = (int)threadIdx.x * W; f < count; f += kBlock * W) {
      const size_t at = XPASS ? (size_t)(f >> lb) * (size_t)g.ny + (size_t)(f & b1) : (size_t)f;
      const int in = XPASS ? f : (f >> lm) * pitch + (f & m1);
      FftPack<T, W> vr, vi;
      if (MODE == kFinalAdd) { vr = *reinterpret_cast<const FftPack<T, W>*>(dr + at); vi = *reinterpret_cast<const FftPack<T, W>*>(di + at); }
#pragma unroll
      for (int w = 0; w < W; w++) { fft_store<T, MODE>(&vr.v[w], re[in + w], s); fft_store<T, MODE>(&vi.v[w], im[in + w], s); }
      *reinterpret_cast<FftPack<T, W>*>(dr + at) = vr; *reinterpret_cast<FftPack<T, W>*>(di + at) = vi;
    }
    __syncthreads();
  }
}

template <class T, bool INV, bool XPASS, int MODE, int ELEMS>
static void launch_fft2d_tile(T* dst, const T* src, const f2d::Geometry& g, const T* table, hipStream_t stream) {
  const FftTileShape t = fft_tile_shape<XPASS>(g, ELEMS);
  const unsigned planes = (unsigned)g.planes < kFftMaxPlaneGrid ? (unsigned)g.planes : kFftMaxPlaneGrid;
  const dim3 grid(t.tiles, planes), block(kBlock);
  const T s = f2d::Scale<T>(g.ny, g.nx);
  constexpr int kWide = 16 / (int)sizeof(T);
  if (fft_tile_wide<T>(t, {dst, src})) PH_LAUNCH((fft2d_pass_kernel<T, INV, XPASS, MODE, ELEMS, kWide>), grid, block, 0, stream, dst, src, g, table, s, t.lm, t.lb, t.pitch, t.ltab);
  else PH_LAUNCH((fft2d_pass_kernel<T, INV, XPASS, MODE, ELEMS, 1>), grid, block, 0, stream, dst, src, g, table, s, t.lm, t.lb, t.pitch, t.ltab);
}

/// the tile of a pass: fft_small_tile (fft2d_tile.hpp)
template <class T, bool INV, bool XPASS, int MODE>
static void launch_fft2d_pass(T* dst, const T* src, const f2d::Geometry& g, const T* table, hipStream_t stream) {
  if constexpr (!XPASS) {
    launch_fft2d_tile<T, INV, XPASS, MODE, kFftSmallTile>(dst, src, g, table, stream);
  } else {
    if (fft_small_tile<XPASS>(g)) launch_fft2d_tile<T, INV, XPASS, MODE, kFftSmallTile>(dst, src, g, table, stream);
    else launch_fft2d_tile<T, INV, XPASS, MODE, FftTile<T>::kLarge>(dst, src, g, table, stream);
  }
}

template <class T, bool INV>
static void launch_fft2d_dir(const f2d::Geometry& g, const T* table, T* work, T* res, const T* rhs, bool acc, hipStream_t s) {
  if (g.ny > 1 && g.nx > 1) {
    launch_fft2d_pass<T, INV, false, kToWork>(work, rhs, g, table, s);
    if (acc) launch_fft2d_pass<T, INV, true, kFinalAdd>(res, work, g, table, s);
    else launch_fft2d_pass<T, INV, true, kFinal>(res, work, g, table, s);
  } else if (g.ny > 1) {
    if (acc) launch_fft2d_pass<T, INV, false, kFinalAdd>(res, rhs, g, table, s);
    else launch_fft2d_pass<T, INV, false, kFinal>(res, rhs, g, table, s);
  } else {                                                         // ny == 1: the x pass alone (nx == 1: no stage, the identity)
    if (acc) launch_fft2d_pass<T, INV, true, kFinalAdd>(res, rhs, g, table, s);
    else launch_fft2d_pass<T, INV, true, kFinal>(res, rhs, g, table, s);
  }
}

template <class T, bool INV, bool XPASS>
static void launch_fft2d_mode(int mode, T* dst, const T* src, const f2d::Geometry& g, const T* table, hipStream_t s) {
  if constexpr (!XPASS)                                            // the x pass is always the last one
    if (mode == kToWork) { launch_fft2d_pass<T, INV, XPASS, kToWork>(dst, src, g, table, s); return; }
  if (mode == kFinal) launch_fft2d_pass<T, INV, XPASS, kFinal>(dst, src, g, table, s);
  else launch_fft2d_pass<T, INV, XPASS, kFinalAdd>(dst, src, g, table, s);
}
/// one pass on its own, for kernels_linop_sense2d.hip (fft2d_tile.hpp): the launches above, nothing else.  The x pass is always the last
/// pass and has no instance that writes the work buffer: that combination, and a mode that is none of the three, is refused (false, no launch)
template <class T>
bool fft2d_launch_pass(bool inverse, bool xpass, int mode, T* dst, const T* src, const f2d::Geometry& g, const T* table, hipStream_t s) {
  if ((mode != kToWork && mode != kFinal && mode != kFinalAdd) || (xpass && mode == kToWork)) return false;
  if (inverse) { if (xpass) launch_fft2d_mode<T, true, true>(mode, dst, src, g, table, s); else launch_fft2d_mode<T, true, false>(mode, dst, src, g, table, s); }
  else { if (xpass) launch_fft2d_mode<T, false, true>(mode, dst, src, g, table, s); else launch_fft2d_mode<T, false, false>(mode, dst, src, g, table, s); }
  return true;
}
template bool fft2d_launch_pass<float>(bool, bool, int, float*, const float*, const f2d::Geometry&, const float*, hipStream_t);
template bool fft2d_launch_pass<double>(bool, bool, int, double*, const double*, const f2d::Geometry&, const double*, hipStream_t);

template <class T>
static int launch_fft2d(const prost_hip_fft2d_geometry* geometry, const T* table, T* work, T* res, const T* rhs, int accumulate, void* stream) {
  if (!geometry) { set_error("fft2d: null geometry"); return 1; }
  f2d::Geometry g;
  std::memcpy(&g, geometry, sizeof(g));
  if (!f2d::IsSide(g.ny) || !f2d::IsSide(g.nx)) { set_error("fft2d: nx and ny have to be powers of two from 1 to 2048"); return 1; }
  if (g.planes < 1) { set_error("fft2d: the plane count has to be at least 1"); return 1; }
  if (2 * (uint64_t)g.planes * (uint64_t)g.ny * (uint64_t)g.nx >= ((uint64_t)1 << 31)) { set_error("fft2d: 2 L nx ny has to stay below 2^31"); return 1; }
  if (!table || !work || !res || !rhs) { set_error("fft2d: null pointer"); return 1; }
  hipStream_t s = as_stream(stream);
  if (g.transpose) launch_fft2d_dir<T, true>(g, table, work, res, rhs, accumulate != 0, s);
  else launch_fft2d_dir<T, false>(g, table, work, res, rhs, accumulate != 0, s);
  PH_LAUNCH_END("fft2d kernel");
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_fft2d_f32(const prost_hip_fft2d_geometry* geometry, const float* table, float* work, float* res, const float* rhs, int accumulate, void* stream) {
  return launch_fft2d<float>(geometry, table, work, res, rhs, accumulate, stream);
}
int prost_hip_fft2d_f64(const prost_hip_fft2d_geometry* geometry, const double* table, double* work, double* res, const double* rhs, int accumulate, void* stream) {
  return launch_fft2d<double>(geometry, table, work, res, rhs, accumulate, stream);
}
}  // extern "C"
