// fft2d_tile.hpp -- the tile machinery of kernels_linop_fft2d.hip, shared with kernels_linop_sense2d.hip: the LDS addressing, the stage
// loop, the store of the last pass, the 16-byte packs, the tile choice and the conditions of the wide accesses.  What a tile is, how it
// is banked and why: the head comment of kernels_linop_fft2d.hip.  The arithmetic is include/prost/linop/fft2d.hpp.
#pragma once
#include <cstdint>
#include <initializer_list>

#include "common.hpp"
#include "prost/linop/fft2d.hpp"

namespace prost_hip {

namespace f2d = prost::fft2d;

constexpr unsigned kFftMaxPlaneGrid = 65535;
enum { kToWork = 0, kFinal = 1, kFinalAdd = 2 };

constexpr int kFftSmallTile = 2048;                          ///< complex values: 16 KiB of LDS in fp32, 32 KiB in fp64; one longest line
template <class T> struct FftTile {
  static constexpr int kLarge = 32768 / (int)sizeof(T);     ///< complex values of the large tile: 64 KiB of LDS
};
constexpr int kFftSlab = 16;                                 ///< lines the x pass wants side by side: 64 contiguous bytes per row in fp32
static_assert(kFftSmallTile >= f2d::kMaxSide && FftTile<double>::kLarge >= 2 * f2d::kMaxSide, "a tile holds the longest line, the large one two");

/// LDS address of element e of line b
template <bool XPASS> __device__ __forceinline__ int fft_at(int b, int e, int lb, int pitch) { return XPASS ? (e << lb) + b : b * pitch + e; }

/// the stages of B = 2^lb lines of m = 2^lm points held in re / im
template <class T, bool INV, bool XPASS, int ELEMS>
__device__ __forceinline__ void fft_tile_stages(T* re, T* im, int lm, int lb, int pitch, const T* __restrict__ table, int ltab) {
  constexpr int kPer = ELEMS / 2 / kBlock;                   // butterflies of a lane per stage
  if (lm == 0) return;
  const int nb = 1 << (lm + lb - 1), half = 1 << (lm - 1);
  for (int lh = 0; lh < lm; lh++) {
    const int h = 1 << lh;
    f2d::Cx<T> a[kPer], b[kPer];
#pragma unroll
    for (int u = 0; u < kPer; u++) {
      const int idx = (int)threadIdx.x + u * kBlock;
      if (idx < nb) {
        const int line = XPASS ? (idx & ((1 << lb) - 1)) : (idx >> (lm - 1)), j = XPASS ? (idx >> lb) : (idx & (half - 1));
        const int ia = fft_at<XPASS>(line, j, lb, pitch), ib = fft_at<XPASS>(line, j + half, lb, pitch);
        a[u].re = re[ia]; a[u].im = im[ia]; b[u].re = re[ib]; b[u].im = im[ib];
      }
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < kPer; u++) {
      const int idx = (int)threadIdx.x + u * kBlock;
      if (idx < nb) {
        const int line = XPASS ? (idx & ((1 << lb) - 1)) : (idx >> (lm - 1)), j = XPASS ? (idx >> lb) : (idx & (half - 1));
        const int k = j & (h - 1), e0 = k + ((j >> lh) << (lh + 1));
        const int w = k << (ltab - lh - 1);                  // below half the table
        const f2d::Cx<T> t = f2d::Twiddled<T, INV>(b[u], k, h, table[2 * w], table[2 * w + 1]);
        const int o0 = fft_at<XPASS>(line, e0, lb, pitch), o1 = fft_at<XPASS>(line, e0 + h, lb, pitch);
        re[o0] = a[u].re + t.re; im[o0] = a[u].im + t.im;
        re[o1] = a[u].re - t.re; im[o1] = a[u].im - t.im;
      }
    }
    __syncthreads();
  }
}

template <class T, int MODE> __device__ __forceinline__ void fft_store(T* o, T v, T s) {
  if (MODE == kToWork) { *o = v; return; }
  const T scaled = v * s;
  *o = MODE == kFinalAdd ? *o + scaled : scaled;
}

/// W values of T, 16 bytes when W > 1: one global access of a lane
template <class T, int W> struct alignas(sizeof(T) * W) FftPack { T v[W]; };

/// where value f of a tile sits: `at` elements behind the tile's first value in its plane, `in` in LDS.  f .. f + W - 1 stay inside one
/// contiguous run, in memory and in LDS.  These three helpers MIRROR the expressions that fft2d_pass_kernel (kernels_linop_fft2d.hip) writes
/// out inline for base, at and in -- that kernel is left as round 25 pinned it -- and have to change together with them: the passes of
/// sense2d read what fft2d's passes wrote and the reverse (tests/test_gpu_sense2d.py holds the two to each other bit for bit)
template <bool XPASS> __device__ __forceinline__ size_t fft_tile_at(int f, int lb, int ny) {
  return XPASS ? (size_t)(f >> lb) * (size_t)ny + (size_t)(f & ((1 << lb) - 1)) : (size_t)f;
}
template <bool XPASS> __device__ __forceinline__ int fft_tile_in(int f, int lm, int pitch) { return XPASS ? f : (f >> lm) * pitch + (f & ((1 << lm) - 1)); }
/// offset of the first value of tile `tile` inside a plane
template <bool XPASS> __device__ __forceinline__ size_t fft_tile_base(unsigned tile, int lm, int lb) {
  return XPASS ? ((size_t)tile << lb) : ((size_t)tile << (lb + lm));
}

/// how a pass is cut into tiles of ELEMS complex values: XPASS: lines of nx points at stride ny, a tile is a slab of B consecutive y and all
/// nx; else lines of ny contiguous points, a tile is B consecutive columns
struct FftTileShape {
  int lm, lb, pitch, ltab;      ///< log2 of the line length and of B; the pitch of a line in LDS (y pass); log2 of the table size
  unsigned tiles;               ///< lines / B: the grid's x axis
  int run;                      ///< values of a contiguous run of the tile: a line of the y pass, the B rows of a slab
};
template <bool XPASS> inline FftTileShape fft_tile_shape(const f2d::Geometry& g, int tile) {
  const int m = XPASS ? g.nx : g.ny, lines = XPASS ? g.ny : g.nx;
  const int cap = (!XPASS && m < 64) ? tile / 2 : tile;            // short contiguous lines are pitched at 3 m / 2
  const int B = cap / m < lines ? cap / m : lines;
  FftTileShape t;
  t.pitch = (!XPASS && m < 64) ? m + m / 2 : m;
  t.lm = f2d::Log2(m); t.lb = f2d::Log2(B); t.ltab = f2d::Log2(f2d::TableSize(g.ny, g.nx));
  t.tiles = (unsigned)(lines / B);
  t.run = XPASS ? B : m;
  return t;
}
/// 16 bytes per lane where the pointers allow: every plane and every run then starts on a multiple of 16 bytes, since a run's length (a
/// power of two, at least 16 / sizeof(T)) divides every offset in front of it
template <class T> inline bool fft_tile_wide(const FftTileShape& t, std::initializer_list<const void*> pointers) {
  uintptr_t bits = 0;
  for (const void* p : pointers) bits |= reinterpret_cast<uintptr_t>(p);
  return t.run >= 16 / (int)sizeof(T) && bits % 16 == 0;
}
/// the y pass takes small tiles: its lines are contiguous, and 5 to 10 workgroups on a CU overlap one tile's loads with another's stages.
/// The x pass takes the small tile while it holds kFftSlab lines (nx <= 128), else the large one
template <bool XPASS> inline bool fft_small_tile(const f2d::Geometry& g) { return !XPASS || g.nx * kFftSlab <= kFftSmallTile; }

/// one pass of fft2d over g.planes images as kernels_linop_fft2d.hip launches it (defined there): mode kToWork (y pass only), kFinal or
/// kFinalAdd; false, and nothing is launched, for the x pass with kToWork or an unknown mode
template <class T> bool fft2d_launch_pass(bool inverse, bool xpass, int mode, T* dst, const T* src, const f2d::Geometry& g, const T* table, hipStream_t stream);

}  // namespace prost_hip
