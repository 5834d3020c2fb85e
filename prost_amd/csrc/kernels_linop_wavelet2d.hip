// kernels_linop_wavelet2d.hip -- BlockWavelet2D: res (+)= K rhs and res (+)= K^T rhs for the orthogonal, periodised, separable
// multi-level wavelet transform K of L real planes, without a matrix.  The arithmetic -- the taps, the order of every sum, the order of
// the passes and of the levels, the limits, the slots of the work buffer -- is include/prost/linop/wavelet2d.hpp, which also runs on
// the host (tests/host/wavelet2d_harness.cpp).  This file decides who holds what.
//
// One launch per level does both passes of that level.  A workgroup of 256 lanes owns kWvTY x kWvTX = 32 x 16 positions of each of the
// four sub-bands, a tile of 64 x 32 pixels of the level's corner.
//   forward:    it stages the tile with its periodic halo (T - 2 more rows and columns, wrapped mod my / mx) in LDS, filters along y
//               into a second LDS array (lows above highs), filters that along x and stores its piece of the four sub-bands: the three
//               detail bands to res, the low-low band to the work buffer (to res at the last level).
//   transposed: a gather.  It stages the T/2 - 1 lows and highs in front of its own of every band (wrapped mod my/2, mx/2), the low-low
//               band from the work buffer, the others from rhs; runs the x pass into the second array and the y pass from there, and
//               stores 64 x 32 pixels of the corner to the work buffer (to res at level 0).
// Nothing between the two passes of a level goes through global memory.  LDS: 78 x 46 + 46 x 64 values, 25.5 KiB in fp32 and 51 KiB in
// fp64, static.
//
// Tail: once a plane's corner holds at most wavelet2d::kTailValues = 4096 values (64 x 64), one launch with a workgroup per plane
// finishes all remaining levels between two LDS arrays of 4096 values (32 KiB in fp32, 64 KiB in fp64) and stores the corner once; the
// transpose begins with it.  A 2048 x 2048 transform at 8 levels is 5 launches + 1 instead of 8.  geometry.no_tail turns it off.
//
// Global accesses run along y.  WL (loads) and WS (stores) are the values a lane moves per access, 1 or 16 bytes' worth (4 in fp32,
// 2 in fp64); each kernel launch decides each of the two for its own pointers: 16 bytes when the pointers, the column heights and the
// plane strides of that side are multiples of 16 bytes and every run of the tile -- the 2 ty unwrapped rows of a staged column, the
// ty lows and ty highs of a stored one -- holds whole groups (the corner's height, for the band stores and band loads half of it, a
// multiple of the group); one value otherwise (an odd element offset of the block inside the solver's vectors, heights such as 90 or
// 100).  The wrapped halo rows are always read one by one.
//
// Taps travel as a kernel argument (Taps<T>, 32 values) and are read with scalar loads.  Planes on the grid's y axis (the tail: x).
// No scratch, no atomics: a repeated call repeats its bits.  A plane never reads another plane.  Resource table: docs/rounds/r27.md.
#include <cstring>
#include <type_traits>

#include "common.hpp"
#include "prost/linop/wavelet2d.hpp"

namespace prost_hip {

namespace w2d = prost::wavelet2d;

static_assert(sizeof(w2d::Geometry) == sizeof(prost_hip_wavelet2d_geometry), "geometry record");

constexpr unsigned kWvMaxPlaneGrid = 65535;
constexpr int kWvTY = 32, kWvTX = 16;                                      ///< positions of a sub-band per tile
constexpr int kWvInY = 2 * kWvTY + w2d::kMaxTaps - 2, kWvInX = 2 * kWvTX + w2d::kMaxTaps - 2;   ///< 78 x 46: the staged tile, either direction
constexpr int kWvIn = kWvInY * kWvInX;
constexpr int kWvMid = kWvInX * 2 * kWvTY;                                 ///< forward 46 x 64; transposed 32 x 78 is smaller
static_assert(2 * kWvTX * kWvInY <= kWvMid, "the transposed intermediate fits");
static_assert((kWvIn + kWvMid) * sizeof(double) <= 65536 && 2 * w2d::kTailValues * sizeof(double) <= 65536, "static LDS of at most 64 KiB");
static_assert((2 * kWvTY) % 4 == 0, "tiles begin on whole groups of 16 bytes");

/// one level (or the tail) of one call
template <class T> struct WvArgs {
  const T* src;           ///< forward: the corner; transposed: rhs, the three detail bands (and the low-low band at the deepest level)
  const T* ll_src;        ///< transposed: the low-low band
  T* ll_dst;              ///< forward: where the low-low band goes; transposed: where the corner goes
  T* res;                 ///< forward: where the detail bands go (quadrant layout, column height ny)
  int my, mx;             ///< the corner
  int src_ld, lls_ld, ll_ld, res_ld;                       ///< column heights of src, ll_src, ll_dst, res
  size_t src_plane, lls_plane, ll_plane, res_plane;        ///< plane strides
  int planes, ntaps, tiles_y;
  int acc, ll_acc;        ///< res / ll_dst: store res + value
  int nlevels;            ///< the tail: levels to run
};

/// W consecutive values: one global access of a lane
template <class T, int W> struct alignas(sizeof(T) * W) WvPack { T v[W]; };
template <class T, int W> __device__ __forceinline__ WvPack<T, W> wv_load(const T* p) { return *reinterpret_cast<const WvPack<T, W>*>(p); }
template <class T, int W> __device__ __forceinline__ void wv_store(T* p, WvPack<T, W> v, int acc) {
  if (acc) {
    const WvPack<T, W> old = wv_load<T, W>(p);
#pragma unroll
    for (int w = 0; w < W; w++) v.v[w] = old.v[w] + v.v[w];
  }
  *reinterpret_cast<WvPack<T, W>*>(p) = v;
}

template <class T, int WL, int WS>
__global__ void __launch_bounds__(kBlock) wavelet2d_forward_level_kernel(const WvArgs<T> a, const w2d::Taps<T> w) {
  __shared__ alignas(16) T in[kWvIn];
  __shared__ alignas(16) T mid[kWvMid];
  const bool py = a.my > 1, px = a.mx > 1;
  const int hy = py ? a.my / 2 : 1, hx = px ? a.mx / 2 : 1;
  const int ky0 = ((int)blockIdx.x % a.tiles_y) * kWvTY, kx0 = ((int)blockIdx.x / a.tiles_y) * kWvTX;
  const int ty = hy - ky0 < kWvTY ? hy - ky0 : kWvTY, tx = hx - kx0 < kWvTX ? hx - kx0 : kWvTX;
  const int iy = py ? 2 * ty + a.ntaps - 2 : 1, ix = px ? 2 * tx + a.ntaps - 2 : 1;      // staged rows and columns
  const int ry = py ? 2 * ty : 1;                                                          // rows of mid; the staged rows that do not wrap
  const int y0 = py ? 2 * ky0 : 0, x0 = px ? 2 * kx0 : 0;
  const int tid = (int)threadIdx.x, T_ = a.ntaps;
  for (size_t c = blockIdx.y; c < (size_t)a.planes; c += gridDim.y) {
    const T* src = a.src + c * a.src_plane;
    const int nvl = ry / WL;                                   // WL > 1: the launcher saw to it that WL divides ry
    for (int f = tid; f < ix * nvl; f += kBlock) {
      const int cx = f / nvl, r = (f - cx * nvl) * WL;
      int gx = x0 + cx;
      if (gx >= a.mx) gx -= a.mx;
      const WvPack<T, WL> v = wv_load<T, WL>(src + (size_t)gx * (size_t)a.src_ld + (size_t)(y0 + r));
#pragma unroll
      for (int e = 0; e < WL; e++) in[cx * iy + r + e] = v.v[e];
    }
    const int halo = iy - ry;                                  // the rows behind the tile, wrapped
    for (int f = tid; f < ix * halo; f += kBlock) {
      const int cx = f / halo, r = ry + (f - cx * halo);
      int gy = y0 + r, gx = x0 + cx;
      if (gy >= a.my) gy -= a.my;
      if (gx >= a.mx) gx -= a.mx;
      in[cx * iy + r] = src[(size_t)gx * (size_t)a.src_ld + (size_t)gy];
    }
    __syncthreads();
    if (py) {
      for (int f = tid; f < ix * ty; f += kBlock) {
        const int cx = f / ty, k = f - cx * ty;
        const T* line = in + cx * iy + 2 * k;
        T lo, hi;
        w2d::Analysis<T>(w, T_, [&](int t) { return line[t]; }, lo, hi);
        mid[cx * ry + k] = lo; mid[cx * ry + ty + k] = hi;
      }
    } else {
      for (int f = tid; f < ix; f += kBlock) mid[f] = in[f];
    }
    __syncthreads();
    T* ll = a.ll_dst + c * a.ll_plane;
    T* res = a.res + c * a.res_plane;
    const int nvs = ry / WS;                                   // WS > 1: WS divides ty, a group is all lows or all highs
    for (int f = tid; f < tx * nvs; f += kBlock) {
      const int kx = f / nvs, r = (f - kx * nvs) * WS;
      const int gy = py ? (r < ty ? ky0 + r : hy + ky0 + (r - ty)) : 0;
      WvPack<T, WS> lo, hi;
#pragma unroll
      for (int e = 0; e < WS; e++) {
        if (px) {
          const T* line = mid + 2 * kx * ry + r + e;
          w2d::Analysis<T>(w, T_, [&](int t) { return line[t * ry]; }, lo.v[e], hi.v[e]);
        } else {
          lo.v[e] = mid[r + e]; hi.v[e] = (T)0;
        }
      }
      const int gx = kx0 + kx;
      if (gy < hy) wv_store<T, WS>(ll + (size_t)gx * (size_t)a.ll_ld + (size_t)gy, lo, a.ll_acc);
      else wv_store<T, WS>(res + (size_t)gx * (size_t)a.res_ld + (size_t)gy, lo, a.acc);
      if (px) wv_store<T, WS>(res + (size_t)(hx + gx) * (size_t)a.res_ld + (size_t)gy, hi, a.acc);
    }
    __syncthreads();
  }
}

template <class T, int WL, int WS>
__global__ void __launch_bounds__(kBlock) wavelet2d_transposed_level_kernel(const WvArgs<T> a, const w2d::Taps<T> w) {
  __shared__ alignas(16) T in[kWvIn];
  __shared__ alignas(16) T mid[kWvMid];
  const bool py = a.my > 1, px = a.mx > 1;
  const int hy = py ? a.my / 2 : 1, hx = px ? a.mx / 2 : 1;
  const int ky0 = ((int)blockIdx.x % a.tiles_y) * kWvTY, kx0 = ((int)blockIdx.x / a.tiles_y) * kWvTX;
  const int ty = hy - ky0 < kWvTY ? hy - ky0 : kWvTY, tx = hx - kx0 < kWvTX ? hx - kx0 : kWvTX;
  const int halo = a.ntaps / 2 - 1;
  const int hly = py ? halo : 0;                                              // halo rows in front of the lows and of the highs
  const int sy = py ? ty + halo : 1, sx = px ? tx + halo : 1;                 // staged lows (and highs) per axis
  const int iy = py ? 2 * sy : 1, ix = px ? 2 * sx : 1;
  const int oy = py ? 2 * ty : 1, ox = px ? 2 * tx : 1;                       // pixels of the corner this tile stores
  const int bands = py ? 2 : 1;
  const int tid = (int)threadIdx.x, T_ = a.ntaps;
  for (size_t c = blockIdx.y; c < (size_t)a.planes; c += gridDim.y) {
    const T* src = a.src + c * a.src_plane;
    const T* lls = a.ll_src + c * a.lls_plane;
    // staged column cx: low kx0 - halo + cx (cx < sx) or the high of the same index, wrapped
    auto column = [&](int cx) {
      if (!px) return 0;
      int k = kx0 - halo + (cx < sx ? cx : cx - sx);
      if (k < 0) k += hx;
      return cx < sx ? k : hx + k;
    };
    // the tile's own rows: ty lows from ky0 and ty highs from hy + ky0, staged behind their halos
    const int nvl = (py ? ty : 1) / WL;                        // WL > 1: WL divides ty
    for (int f = tid; f < ix * bands * nvl; f += kBlock) {
      const int cx = f / (bands * nvl), rest = f - cx * (bands * nvl), band = rest / nvl, r = (rest - band * nvl) * WL;
      const int gx = column(cx), gy = (py ? ky0 : 0) + r + band * hy;
      const T* from = (gy < hy && gx < hx) ? lls + (size_t)gx * (size_t)a.lls_ld : src + (size_t)gx * (size_t)a.src_ld;
      const WvPack<T, WL> v = wv_load<T, WL>(from + gy);
#pragma unroll
      for (int e = 0; e < WL; e++) in[cx * iy + band * sy + hly + r + e] = v.v[e];
    }
    for (int f = tid; f < ix * 2 * hly; f += kBlock) {
      const int cx = f / (2 * hly), rest = f - cx * (2 * hly), band = rest / hly, r = rest - band * hly;
      int k = ky0 - halo + r;
      if (k < 0) k += hy;
      const int gx = column(cx), gy = k + band * hy;
      in[cx * iy + band * sy + r] = (gy < hy && gx < hx) ? lls[(size_t)gx * (size_t)a.lls_ld + (size_t)gy] : src[(size_t)gx * (size_t)a.src_ld + (size_t)gy];
    }
    __syncthreads();
    // the x pass first: every staged row, the tile's ox columns.  Staged position s holds low kx0 - halo + s, so output column n of the
    // tile is output n + 2 halo of a line that begins at the staged halo, and no index wraps
    if (px) {
      for (int f = tid; f < ox * iy; f += kBlock) {
        const int n = f / iy, r = f - n * iy;
        const T* line = in + r;
        mid[f] = w2d::Synthesis<T>(w, T_, n + 2 * halo, sx, [&](int k) { return line[k * iy]; }, [&](int k) { return line[(sx + k) * iy]; });
      }
    } else {
      for (int f = tid; f < iy; f += kBlock) mid[f] = in[f];
    }
    __syncthreads();
    T* dst = a.ll_dst + c * a.ll_plane;
    const int nvs = oy / WS;                                   // WS > 1: WS divides 2 ty
    for (int f = tid; f < ox * nvs; f += kBlock) {
      const int n = f / nvs, r = (f - n * nvs) * WS;
      const T* line = mid + n * iy;
      WvPack<T, WS> v;
#pragma unroll
      for (int e = 0; e < WS; e++)
        v.v[e] = py ? w2d::Synthesis<T>(w, T_, r + e + 2 * halo, sy, [&](int k) { return line[k]; }, [&](int k) { return line[sy + k]; }) : line[0];
      const int gy = (py ? 2 * ky0 : 0) + r, gx = (px ? 2 * kx0 : 0) + n;
      wv_store<T, WS>(dst + (size_t)gx * (size_t)a.ll_ld + (size_t)gy, v, a.ll_acc);
    }
    __syncthreads();
  }
}

/// the remaining a.nlevels levels of a corner of at most kTailValues values, a workgroup per plane; lines keep the column height my in LDS
template <class T, bool INV, int WL, int WS>
__global__ void __launch_bounds__(kBlock) wavelet2d_tail_kernel(const WvArgs<T> a, const w2d::Taps<T> w) {
  __shared__ alignas(16) T A[w2d::kTailValues];
  __shared__ alignas(16) T B[w2d::kTailValues];
  const int tid = (int)threadIdx.x, T_ = a.ntaps, ld = a.my, count = a.my * a.mx;
  for (size_t c = blockIdx.x; c < (size_t)a.planes; c += gridDim.x) {
    const T* src = a.src + c * a.src_plane;
    for (int f = tid * WL; f < count; f += kBlock * WL) {      // WL > 1: WL divides my, a group stays inside its column
      const int gx = f / ld, gy = f - gx * ld;
      const WvPack<T, WL> v = wv_load<T, WL>(src + (size_t)gx * (size_t)a.src_ld + (size_t)gy);
#pragma unroll
      for (int e = 0; e < WL; e++) A[f + e] = v.v[e];
    }
    __syncthreads();
    for (int i = 0; i < a.nlevels; i++) {
      const int l = INV ? a.nlevels - 1 - i : i;
      const int cy = w2d::CornerSide(a.my, l), cx = w2d::CornerSide(a.mx, l);
      const bool py = cy > 1, px = cx > 1;
      const int hy = py ? cy / 2 : 1, hx = px ? cx / 2 : 1;
      if (!INV) {
        if (py) {
          for (int f = tid; f < hy * cx; f += kBlock) {
            const int col = f / hy, k = f - col * hy;
            const T* line = A + col * ld;
            T lo, hi;
            w2d::Analysis<T>(w, T_, [&](int t) { int e = 2 * k + t; if (e >= cy) e -= cy; return line[e]; }, lo, hi);
            B[col * ld + k] = lo; B[col * ld + hy + k] = hi;
          }
        } else {
          for (int f = tid; f < cx; f += kBlock) B[f * ld] = A[f * ld];
        }
        __syncthreads();
        if (px) {
          for (int f = tid; f < cy * hx; f += kBlock) {
            const int k = f / cy, r = f - k * cy;
            const T* line = B + r;
            T lo, hi;
            w2d::Analysis<T>(w, T_, [&](int t) { int e = 2 * k + t; if (e >= cx) e -= cx; return line[e * ld]; }, lo, hi);
            A[k * ld + r] = lo; A[(hx + k) * ld + r] = hi;
          }
        } else {
          for (int f = tid; f < cy; f += kBlock) A[f] = B[f];
        }
        __syncthreads();
      } else {
        if (px) {
          for (int f = tid; f < cy * cx; f += kBlock) {
            const int n = f / cy, r = f - n * cy;
            const T* line = A + r;
            B[n * ld + r] = w2d::Synthesis<T>(w, T_, n, hx, [&](int k) { return line[k * ld]; }, [&](int k) { return line[(hx + k) * ld]; });
          }
        } else {
          for (int f = tid; f < cy; f += kBlock) B[f] = A[f];
        }
        __syncthreads();
        if (py) {
          for (int f = tid; f < cy * cx; f += kBlock) {
            const int col = f / cy, n = f - col * cy;
            const T* line = B + col * ld;
            A[col * ld + n] = w2d::Synthesis<T>(w, T_, n, hy, [&](int k) { return line[k]; }, [&](int k) { return line[hy + k]; });
          }
        } else {
          for (int f = tid; f < cx; f += kBlock) A[f * ld] = B[f * ld];
        }
        __syncthreads();
      }
    }
    T* dst = a.ll_dst + c * a.ll_plane;
    for (int f = tid * WS; f < count; f += kBlock * WS) {
      const int gx = f / ld, gy = f - gx * ld;
      WvPack<T, WS> v;
#pragma unroll
      for (int e = 0; e < WS; e++) v.v[e] = A[f + e];
      wv_store<T, WS>(dst + (size_t)gx * (size_t)a.ll_ld + (size_t)gy, v, a.ll_acc);
    }
    __syncthreads();
  }
}

/// where the corner level l acts on lives: rhs / res for l = 0, else slot (l - 1) mod 2 of the work buffer, packed
template <class T> struct WvPlace { T* p; int ld; size_t plane; };
template <class T> static WvPlace<T> wv_corner(const w2d::Geometry& g, T* outer, T* work, int l) {
  if (l == 0) return {outer, g.ny, (size_t)g.ny * (size_t)g.nx};
  T* slot = ((l - 1) & 1) ? work + w2d::WorkSlot0(g) : work;
  return {slot, w2d::CornerSide(g.ny, l), w2d::CornerSize(g.ny, g.nx, l)};
}

/// every column and every plane behind p begins on a multiple of 16 bytes
template <class T> static bool wv_wide(const T* p, int ld, size_t plane) {
  constexpr int kWide = 16 / (int)sizeof(T);
  return reinterpret_cast<uintptr_t>(p) % 16 == 0 && ld % kWide == 0 && plane % kWide == 0;
}

/// launch(WL, WS) with 16 bytes per lane on the sides that allow it (integral constants)
template <class T, class F> static void wv_dispatch(bool wide_loads, bool wide_stores, F launch) {
  using Wide = std::integral_constant<int, 16 / (int)sizeof(T)>;
  using One = std::integral_constant<int, 1>;
  if (wide_loads && wide_stores) launch(Wide{}, Wide{});
  else if (wide_loads) launch(Wide{}, One{});
  else if (wide_stores) launch(One{}, Wide{});
  else launch(One{}, One{});
}

template <class T>
static void launch_wavelet2d_plan(const w2d::Geometry& g, const w2d::Taps<T>& w, T* work, T* res, const T* rhs, int acc, hipStream_t stream) {
  constexpr int kWide = 16 / (int)sizeof(T);
  const int tail = w2d::TailStart(g);
  const size_t N = (size_t)g.ny * (size_t)g.nx;
  const unsigned planes = (unsigned)g.planes < kWvMaxPlaneGrid ? (unsigned)g.planes : kWvMaxPlaneGrid;
  WvArgs<T> a;
  std::memset(&a, 0, sizeof(a));
  a.planes = g.planes; a.ntaps = g.ntaps; a.acc = acc;
  a.res = res; a.res_ld = g.ny; a.res_plane = N;
  auto level_grid = [&]() {
    const int hy = a.my > 1 ? a.my / 2 : 1, hx = a.mx > 1 ? a.mx / 2 : 1;
    a.tiles_y = (hy + kWvTY - 1) / kWvTY;
    return dim3((unsigned)(a.tiles_y * ((hx + kWvTX - 1) / kWvTX)), planes);
  };
  if (!g.transpose) {
    for (int l = 0; l < g.levels; l++) {
      // the corner comes from rhs (l = 0) or its slot; the low-low band goes to the next corner's slot, at the end to res
      const WvPlace<T> from = wv_corner<T>(g, const_cast<T*>(rhs), work, l);
      a.src = from.p; a.src_ld = from.ld; a.src_plane = from.plane;
      a.my = w2d::CornerSide(g.ny, l); a.mx = w2d::CornerSide(g.nx, l);
      const bool whole = a.my % kWide == 0, halves = a.my % (2 * kWide) == 0;      // groups in a corner's column, in a band's column
      if (l == tail) {
        a.nlevels = g.levels - l; a.ll_dst = res; a.ll_ld = g.ny; a.ll_plane = N; a.ll_acc = acc;
        const bool wl = whole && wv_wide<T>(a.src, a.src_ld, a.src_plane), ws = whole && wv_wide<T>(res, g.ny, N);
        wv_dispatch<T>(wl, ws, [&](auto WL, auto WS) { PH_LAUNCH((wavelet2d_tail_kernel<T, false, decltype(WL)::value, decltype(WS)::value>), dim3(planes), dim3(kBlock), 0, stream, a, w); });
        return;
      }
      const bool last = l == g.levels - 1;
      const WvPlace<T> to = last ? WvPlace<T>{res, g.ny, N} : wv_corner<T>(g, res, work, l + 1);
      a.ll_dst = to.p; a.ll_ld = to.ld; a.ll_plane = to.plane; a.ll_acc = last ? acc : 0;
      const bool wl = whole && wv_wide<T>(a.src, a.src_ld, a.src_plane);
      const bool ws = halves && wv_wide<T>(res, g.ny, N) && wv_wide<T>(a.ll_dst, a.ll_ld, a.ll_plane);
      const dim3 grid = level_grid();
      wv_dispatch<T>(wl, ws, [&](auto WL, auto WS) { PH_LAUNCH((wavelet2d_forward_level_kernel<T, decltype(WL)::value, decltype(WS)::value>), grid, dim3(kBlock), 0, stream, a, w); });
    }
  } else {
    a.src = rhs; a.src_ld = g.ny; a.src_plane = N;
    if (tail < g.levels) {
      const WvPlace<T> to = wv_corner<T>(g, res, work, tail);
      a.my = w2d::CornerSide(g.ny, tail); a.mx = w2d::CornerSide(g.nx, tail);
      a.nlevels = g.levels - tail; a.ll_dst = to.p; a.ll_ld = to.ld; a.ll_plane = to.plane; a.ll_acc = tail == 0 ? acc : 0;
      const bool whole = a.my % kWide == 0;
      const bool wl = whole && wv_wide<T>(rhs, g.ny, N), ws = whole && wv_wide<T>(a.ll_dst, a.ll_ld, a.ll_plane);
      wv_dispatch<T>(wl, ws, [&](auto WL, auto WS) { PH_LAUNCH((wavelet2d_tail_kernel<T, true, decltype(WL)::value, decltype(WS)::value>), dim3(planes), dim3(kBlock), 0, stream, a, w); });
    }
    for (int l = (tail < g.levels ? tail : g.levels) - 1; l >= 0; l--) {
      // the low-low band is corner l + 1 (at the deepest level: rhs itself); the corner goes to its slot, at level 0 to res
      const WvPlace<T> from = l == g.levels - 1 ? WvPlace<T>{const_cast<T*>(rhs), g.ny, N} : wv_corner<T>(g, res, work, l + 1);
      const WvPlace<T> to = wv_corner<T>(g, res, work, l);
      a.my = w2d::CornerSide(g.ny, l); a.mx = w2d::CornerSide(g.nx, l);
      a.ll_src = from.p; a.ll_dst = to.p; a.ll_ld = to.ld; a.ll_plane = to.plane; a.ll_acc = l == 0 ? acc : 0;
      a.lls_ld = from.ld; a.lls_plane = from.plane;
      const bool whole = a.my % kWide == 0, halves = a.my % (2 * kWide) == 0;
      const bool wl = halves && wv_wide<T>(rhs, g.ny, N) && wv_wide<T>(a.ll_src, a.lls_ld, a.lls_plane);
      const bool ws = whole && wv_wide<T>(a.ll_dst, a.ll_ld, a.ll_plane);
      const dim3 grid = level_grid();
      wv_dispatch<T>(wl, ws, [&](auto WL, auto WS) { PH_LAUNCH((wavelet2d_transposed_level_kernel<T, decltype(WL)::value, decltype(WS)::value>), grid, dim3(kBlock), 0, stream, a, w); });
    }
  }
}

template <class T>
static int launch_wavelet2d(const prost_hip_wavelet2d_geometry* geometry, const T* taps, T* work, T* res, const T* rhs, int accumulate, void* stream) {
  if (!geometry) { set_error("wavelet2d: null geometry"); return 1; }
  w2d::Geometry g;
  std::memcpy(&g, geometry, sizeof(g));
  if (const char* why = w2d::CheckShape(g.ny, g.nx, g.planes, g.levels, g.ntaps)) { set_error(std::string("wavelet2d: ") + why); return 1; }
  if (!taps || !work || !res || !rhs) { set_error("wavelet2d: null pointer"); return 1; }
  w2d::Taps<T> w;
  for (int t = 0; t < w2d::kMaxTaps; t++) { w.h[t] = (T)0; w.g[t] = (T)0; }
  for (int t = 0; t < g.ntaps; t++) { w.h[t] = taps[t]; w.g[t] = (t & 1) ? -taps[g.ntaps - 1 - t] : taps[g.ntaps - 1 - t]; }
  launch_wavelet2d_plan<T>(g, w, work, res, rhs, accumulate != 0 ? 1 : 0, as_stream(stream));
  PH_LAUNCH_END("wavelet2d kernel");
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_wavelet2d_f32(const prost_hip_wavelet2d_geometry* geometry, const float* taps, float* work, float* res, const float* rhs, int accumulate, void* stream) {
  return launch_wavelet2d<float>(geometry, taps, work, res, rhs, accumulate, stream);
}
int prost_hip_wavelet2d_f64(const prost_hip_wavelet2d_geometry* geometry, const double* taps, double* work, double* res, const double* rhs, int accumulate, void* stream) {
  return launch_wavelet2d<double>(geometry, taps, work, res, rhs, accumulate, stream);
}
}  // extern "C"
