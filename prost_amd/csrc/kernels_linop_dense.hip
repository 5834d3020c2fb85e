// kernels_linop_dense.hip -- the dense blocks for gfx950: kron(K, I_d), kron(I_d, K) for a small dense K and the general dense
// matrix-vector product (reference: src/linop/block_dense_kron_id.cu, block_id_kron_dense.cu, block_dense.cu).
//
// K is column-major, nrows x ncols, of type T on the device.  One product serves the forward and the transposed call: output row r,
// inner index i, coefficient K[r sr + i si] with (sr, si) = (1, nrows) forward and (nrows, 1) transposed.  Both Kronecker kernels form
// every output as the reference does: a sum of type T that starts at 0, products added in ascending i (one rounding per product and per
// add, -ffp-contract=off), then one add into res -- bit-identical to the reference's expressions.  No MFMA, no split of the i range.
#include "common.hpp"
#include "fused_op.hpp"

namespace prost_hip {

// the coefficients of one row tile at inner index i: wave-uniform, read through the constant address space (scalar loads) at 32-bit
// offsets from the tile's first coefficient (K has fewer than 2^31 entries, checked at the launch).  Rows past the end of K repeat its
// last row; their sums are never stored.
template <int RT>
__device__ __forceinline__ void coeff_offsets(size_t r0, size_t rows, size_t sr, unsigned (&off)[RT]) {
  const unsigned last = rows - r0 < (size_t)RT ? (unsigned)(rows - r0) - 1u : (unsigned)RT - 1u;
#pragma unroll
  for (int r = 0; r < RT; r++) off[r] = ((unsigned)r < last ? (unsigned)r : last) * (unsigned)sr;
}
template <class T, int RT>
__device__ __forceinline__ void load_coeffs(const PROST_CONSTANT T* __restrict__ tile_i, const unsigned (&off)[RT], T (&k)[RT]) {
#pragma unroll
  for (int r = 0; r < RT; r++) k[r] = tile_i[off[r]];
}

// ------------------------------------------------------------------------------------------
// kron(K, I_d): res[r d + p] (+)= sum_i K[r, i] rhs[i d + p]  (BlockDenseKronIdKernel, block_dense_kron_id.cu:28-65).
// A lane owns V consecutive p (V = 16 bytes where d and both pointers allow, else 1), streams rhs[i d + p] once per row tile in
// ascending i and keeps RT x V sums in registers; blockIdx.y walks the row tiles (the operand is re-read per tile, not per row).
// ------------------------------------------------------------------------------------------
template <class T, bool ACC, int V, int RT>
__global__ void __launch_bounds__(kBlock) dense_kron_id_kernel(T* __restrict__ res, const T* __restrict__ rhs, size_t d, size_t rows, size_t inner,
                                                               const T* __restrict__ K, size_t sr, size_t si) {
  typedef T TV __attribute__((ext_vector_type(V)));
  const PROST_CONSTANT T* cK = as_constant(K);
  const size_t dvec = d / V;
  const size_t tiles = (rows + RT - 1) / RT;
  for (size_t tile = blockIdx.y; tile < tiles; tile += gridDim.y) {
    const size_t r0 = tile * RT;
    unsigned off[RT];
    coeff_offsets<RT>(r0, rows, sr, off);
    const unsigned nvalid = rows - r0 < (size_t)RT ? (unsigned)(rows - r0) : (unsigned)RT;
    for (size_t pv = (size_t)blockIdx.x * kBlock + threadIdx.x; pv < dvec; pv += (size_t)gridDim.x * kBlock) {
      const size_t p = pv * V;
      T sum[RT][V];
#pragma unroll
      for (int r = 0; r < RT; r++)
#pragma unroll
        for (int j = 0; j < V; j++) sum[r][j] = 0;
      for (size_t i = 0; i < inner; i++) {
        T k[RT];
        load_coeffs<T, RT>(cK + r0 * sr + i * si, off, k);
        T x[V];
        if (V > 1) {
          const TV xv = *reinterpret_cast<const TV*>(rhs + i * d + p);
#pragma unroll
          for (int j = 0; j < V; j++) x[j] = xv[j];
        } else x[0] = rhs[i * d + p];
#pragma unroll
        for (int r = 0; r < RT; r++)
#pragma unroll
          for (int j = 0; j < V; j++) sum[r][j] += k[r] * x[j];
      }
      T* out = res + r0 * d + p;
#pragma unroll
      for (int r = 0; r < RT; r++, out += d) {
        if ((unsigned)r < nvalid) {
          if (V > 1) {
            TV o;
            if (ACC) o = *reinterpret_cast<TV*>(out);
#pragma unroll
            for (int j = 0; j < V; j++) o[j] = (ACC ? o[j] : (T)0) + sum[r][j];
            *reinterpret_cast<TV*>(out) = o;
          } else out[0] = (ACC ? out[0] : (T)0) + sum[r][0];
        }
      }
    }
  }
}

template <class T, bool ACC, int V>
static void launch_dense_kron_id_rt(T* res, const T* rhs, size_t d, size_t rows, size_t inner, const T* K, size_t sr, size_t si, hipStream_t s) {
  const size_t dvec = d / V;
  size_t gx = (dvec + kBlock - 1) / kBlock;
  if (gx > (size_t)kMaxGridStride) gx = kMaxGridStride;
  const int rt = rows <= 4 ? 4 : rows <= 8 ? 8 : 16;
  const size_t tiles = (rows + rt - 1) / rt;
  // enough workgroups to fill the chip when the identity is short: the row tiles spread over blockIdx.y
  size_t gy = gx >= 2048 ? 1 : (2048 + gx - 1) / gx;
  if (gy > tiles) gy = tiles;
  if (gy > 65535) gy = 65535;
  const dim3 grid((unsigned)gx, (unsigned)gy), block(kBlock);
  if (rt == 4) hipLaunchKernelGGL((dense_kron_id_kernel<T, ACC, V, 4>), grid, block, 0, s, res, rhs, d, rows, inner, K, sr, si);
  else if (rt == 8) hipLaunchKernelGGL((dense_kron_id_kernel<T, ACC, V, 8>), grid, block, 0, s, res, rhs, d, rows, inner, K, sr, si);
  else hipLaunchKernelGGL((dense_kron_id_kernel<T, ACC, V, 16>), grid, block, 0, s, res, rhs, d, rows, inner, K, sr, si);
}

// ------------------------------------------------------------------------------------------
// kron(I_d, K): res[p rows + r] (+)= sum_i K[r, i] rhs[p inner + i]  (BlockIdKronDenseKernel, block_id_kron_dense.cu:28-65).
// A workgroup takes `groups` consecutive p at a time: their operands and their outputs are contiguous ranges, moved between global
// memory and LDS with 16-byte accesses where the pointers allow.  In LDS a group's operands sit `inner | 1` apart and its outputs
// `rows | 1` apart (odd strides: the lanes of a wave, one group each, hit distinct banks).  A wave takes (row tile, 64 groups) items:
// the row tile is wave-uniform, so K comes through scalar loads as above; a lane keeps RT sums over its group's operands.
// kIdKronLdsBytes bounds the plan: K with (inner | 1) + (rows | 1) > kIdKronLdsBytes / sizeof(T) / 4 (fewer than 4 groups fit) goes
// to the plain kernel below.
// ------------------------------------------------------------------------------------------
constexpr int kIdKronLdsBytes = 48 * 1024;
template <class T, bool ACC, int RT>
__global__ void __launch_bounds__(kBlock) id_kron_dense_kernel(T* __restrict__ res, const T* __restrict__ rhs, size_t d, unsigned rows, unsigned inner,
                                                               unsigned groups, const T* __restrict__ K, size_t sr, size_t si, int in_vec, int out_vec) {
  constexpr int V = 16 / sizeof(T);
  typedef T TV __attribute__((ext_vector_type(V)));
  __shared__ __attribute__((aligned(16))) T s_buf[kIdKronLdsBytes / sizeof(T)];
  const PROST_CONSTANT T* cK = as_constant(K);
  const unsigned in_stride = inner | 1u, out_stride = rows | 1u;
  T* __restrict__ s_in = s_buf;
  T* __restrict__ s_out = s_buf + (size_t)groups * in_stride;
  const unsigned wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), lane = threadIdx.x % kWave;
  const unsigned row_tiles = (rows + RT - 1) / RT, chunks = (groups + kWave - 1) / kWave;
  const size_t tiles = (d + groups - 1) / groups;
  for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const size_t j0 = tile * groups;
    const unsigned ng = d - j0 < groups ? (unsigned)(d - j0) : groups;
    const unsigned n_in = ng * inner, n_out = ng * rows;
    const T* __restrict__ src = rhs + j0 * inner;
    T* __restrict__ dst = res + j0 * rows;
    __syncthreads();                                                  // the previous tile's reads of s_out
    for (unsigned k = V * threadIdx.x; k < n_in; k += V * kBlock) {
      T x[V];
      if (in_vec && k + V <= n_in) {
        const TV xv = *reinterpret_cast<const TV*>(src + k);
#pragma unroll
        for (int e = 0; e < V; e++) x[e] = xv[e];
      } else {
#pragma unroll
        for (int e = 0; e < V; e++) x[e] = k + e < n_in ? src[k + e] : (T)0;
      }
      unsigned q = k / inner, m = k % inner;
#pragma unroll
      for (int e = 0; e < V; e++) {
        if (k + e < n_in) s_in[q * in_stride + m] = x[e];
        if (++m == inner) { m = 0; q++; }
      }
    }
    __syncthreads();
    for (unsigned w = wave; w < row_tiles * chunks; w += kBlock / kWave) {
      const unsigned r0 = (w % row_tiles) * RT, g = (w / row_tiles) * kWave + lane;
      if (g < ng) {
        const T* __restrict__ xs = s_in + g * in_stride;
        unsigned off[RT];
        coeff_offsets<RT>(r0, rows, sr, off);
        T sum[RT];
#pragma unroll
        for (int r = 0; r < RT; r++) sum[r] = 0;
        for (unsigned i = 0; i < inner; i++) {
          T k[RT];
          load_coeffs<T, RT>(cK + r0 * sr + i * si, off, k);
          const T x = xs[i];
#pragma unroll
          for (int r = 0; r < RT; r++) sum[r] += k[r] * x;
        }
#pragma unroll
        for (int r = 0; r < RT; r++)
          if (r0 + r < rows) s_out[g * out_stride + r0 + r] = sum[r];
      }
    }
    __syncthreads();
    for (unsigned k = V * threadIdx.x; k < n_out; k += V * kBlock) {
      T y[V];
      unsigned q = k / rows, m = k % rows;
#pragma unroll
      for (int e = 0; e < V; e++) {
        y[e] = k + e < n_out ? s_out[q * out_stride + m] : (T)0;
        if (++m == rows) { m = 0; q++; }
      }
      if (out_vec && k + V <= n_out) {
        TV o;
        if (ACC) o = *reinterpret_cast<TV*>(dst + k);
#pragma unroll
        for (int e = 0; e < V; e++) o[e] = (ACC ? o[e] : (T)0) + y[e];
        *reinterpret_cast<TV*>(dst + k) = o;
      } else {
#pragma unroll
        for (int e = 0; e < V; e++)
          if (k + e < n_out) dst[k + e] = (ACC ? dst[k + e] : (T)0) + y[e];
      }
    }
  }
}

// the plain kernel for K too large for the plan above: one output per lane, the reference's own loop
template <class T, bool ACC>
__global__ void __launch_bounds__(kBlock) id_kron_dense_plain_kernel(T* __restrict__ res, const T* __restrict__ rhs, size_t d, size_t rows, size_t inner,
                                                                     const T* __restrict__ K, size_t sr, size_t si) {
  const size_t total = d * rows;
  for (size_t tx = (size_t)blockIdx.x * kBlock + threadIdx.x; tx < total; tx += (size_t)gridDim.x * kBlock) {
    const size_t r = tx % rows, ofs = (tx / rows) * inner;
    T sum = 0;
    for (size_t i = 0; i < inner; i++) sum += K[r * sr + i * si] * rhs[ofs + i];
    res[tx] = (ACC ? res[tx] : (T)0) + sum;
  }
}

template <class T, bool ACC>
static int launch_kron_dense(bool id_first, T* res, const T* rhs, size_t d, size_t nrows, size_t ncols, const T* K, int transpose, void* stream) {
  if (d == 0 || nrows == 0 || ncols == 0) return 0;
  if (!res || !rhs || !K) { set_error("dense kronecker product: null pointer"); return 1; }
  if (nrows >= ((size_t)1 << 31) / ncols) { set_error("dense kronecker product: K has 2^31 entries or more"); return 1; }
  hipStream_t s = as_stream(stream);
  const size_t rows = transpose ? ncols : nrows, inner = transpose ? nrows : ncols;
  const size_t sr = transpose ? nrows : 1, si = transpose ? 1 : nrows;
  constexpr size_t V = 16 / sizeof(T);
  const bool res16 = reinterpret_cast<uintptr_t>(res) % 16 == 0, rhs16 = reinterpret_cast<uintptr_t>(rhs) % 16 == 0;
  if (!id_first) {
    if (res16 && rhs16 && d % V == 0) launch_dense_kron_id_rt<T, ACC, (int)V>(res, rhs, d, rows, inner, K, sr, si, s);
    else launch_dense_kron_id_rt<T, ACC, 1>(res, rhs, d, rows, inner, K, sr, si, s);
    PH_LAUNCH_END("dense kronecker kernel (identity last)");
  }
  const size_t lds_elems = kIdKronLdsBytes / sizeof(T), per_group = (inner | 1) + (rows | 1);
  if (per_group * 4 <= lds_elems) {
    // groups per tile: a multiple of 4 (tile starts keep the alignment of the base pointers whatever rows / inner are), whole waves of
    // groups where that many fit
    size_t groups = lds_elems / per_group;
    if (groups > 8 * kBlock) groups = 8 * kBlock;                           // (a small K: several groups per lane, fewer barriers per byte)
    groups &= groups >= (size_t)kWave ? ~(size_t)(kWave - 1) : ~(size_t)3;
    const size_t tiles = (d + groups - 1) / groups;
    const unsigned grid = (unsigned)(tiles < 768 ? tiles : 768);          // resident workgroups (3 per CU by LDS) that walk the tiles
    const int rt = rows <= 4 ? 4 : rows <= 8 ? 8 : 16;
    if (rt == 4) hipLaunchKernelGGL((id_kron_dense_kernel<T, ACC, 4>), dim3(grid), dim3(kBlock), 0, s, res, rhs, d, (unsigned)rows, (unsigned)inner, (unsigned)groups, K, sr, si, (int)rhs16, (int)res16);
    else if (rt == 8) hipLaunchKernelGGL((id_kron_dense_kernel<T, ACC, 8>), dim3(grid), dim3(kBlock), 0, s, res, rhs, d, (unsigned)rows, (unsigned)inner, (unsigned)groups, K, sr, si, (int)rhs16, (int)res16);
    else hipLaunchKernelGGL((id_kron_dense_kernel<T, ACC, 16>), dim3(grid), dim3(kBlock), 0, s, res, rhs, d, (unsigned)rows, (unsigned)inner, (unsigned)groups, K, sr, si, (int)rhs16, (int)res16);
    PH_LAUNCH_END("dense kronecker kernel (identity first, LDS tiles)");
  }
  hipLaunchKernelGGL((id_kron_dense_plain_kernel<T, ACC>), dim3(grid_for(d * rows)), dim3(kBlock), 0, s, res, rhs, d, rows, inner, K, sr, si);
  PH_LAUNCH_END("dense kronecker kernel (identity first, plain)");
}

// ------------------------------------------------------------------------------------------
// dense matrix-vector product, A column-major nrows x ncols (cublas<t>gemv with alpha = beta = 1, block_dense.cu:82-188).
// No floating-point atomics: where the work is split, each part writes its partial sums to the workspace and a second kernel adds them in
// ascending part order, so the result is the same from run to run.
//   forward: one-wave workgroups, lanes along the rows (a column segment is one coalesced read), blockIdx.y = part of the column range
//   adjoint: one wave per column, lanes stride over the rows (coalesced), shuffle reduction; blockIdx.y = part of the row range
// ------------------------------------------------------------------------------------------
static size_t gemv_parts(size_t out_waves, size_t inner, size_t inner_per_part) {
  if (out_waves >= 2048) return 1;
  size_t parts = (4096 + out_waves - 1) / out_waves;
  const size_t most = (inner + inner_per_part - 1) / inner_per_part;
  if (parts > most) parts = most;
  if (parts > 1024) parts = 1024;
  return parts < 1 ? 1 : parts;
}
static size_t gemv_parts_fwd(size_t nrows, size_t ncols) { return gemv_parts((nrows + kWave - 1) / kWave, ncols, 8); }
static size_t gemv_parts_adj(size_t nrows, size_t ncols) { return gemv_parts(ncols, nrows, 256); }

// out: res itself (parts == 1; ACC decides += or =) or the workspace slice of this part (plain store)
template <class T, bool ACC, int V>
__global__ void __launch_bounds__(kWave) gemv_fwd_kernel(T* __restrict__ out, const T* __restrict__ rhs, size_t nrows, size_t ncols,
                                                        const T* __restrict__ A, size_t cols_per_part) {
  typedef T TV __attribute__((ext_vector_type(V)));
  const size_t r = ((size_t)blockIdx.x * kWave + threadIdx.x) * V;
  if (r >= nrows) return;
  const size_t c0 = (size_t)blockIdx.y * cols_per_part;
  const size_t c1 = c0 + cols_per_part < ncols ? c0 + cols_per_part : ncols;
  T* __restrict__ o = out + (size_t)blockIdx.y * nrows + r;
  T sum[V];
#pragma unroll
  for (int j = 0; j < V; j++) sum[j] = 0;
  size_t c = c0;
  for (; c + 4 <= c1; c += 4) {                                          // four column segments in flight
    TV a[4];
    T x[4];
#pragma unroll
    for (int u = 0; u < 4; u++) { a[u] = *reinterpret_cast<const TV*>(A + (c + u) * nrows + r); x[u] = rhs[c + u]; }
#pragma unroll
    for (int u = 0; u < 4; u++)
#pragma unroll
      for (int j = 0; j < V; j++) sum[j] += a[u][j] * x[u];
  }
  for (; c < c1; c++) {
    const TV a = *reinterpret_cast<const TV*>(A + c * nrows + r);
    const T x = rhs[c];
#pragma unroll
    for (int j = 0; j < V; j++) sum[j] += a[j] * x;
  }
  TV ov;
  if (ACC) ov = *reinterpret_cast<TV*>(o);
#pragma unroll
  for (int j = 0; j < V; j++) ov[j] = (ACC ? ov[j] : (T)0) + sum[j];
  *reinterpret_cast<TV*>(o) = ov;
}

template <class T, bool ACC, int V>
__global__ void __launch_bounds__(kBlock) gemv_adj_kernel(T* __restrict__ out, const T* __restrict__ rhs, size_t nrows, size_t ncols,
                                                         const T* __restrict__ A, size_t rows_per_part) {
  typedef T TV __attribute__((ext_vector_type(V)));
  const size_t c = (size_t)blockIdx.x * (kBlock / kWave) + threadIdx.x / kWave;
  if (c >= ncols) return;                                                  // (whole waves leave: the shuffles below stay among live lanes)
  const unsigned lane = threadIdx.x % kWave;
  const size_t r0 = (size_t)blockIdx.y * rows_per_part;
  const size_t r1 = r0 + rows_per_part < nrows ? r0 + rows_per_part : nrows;
  const T* __restrict__ col = A + c * nrows;
  T s0 = 0, s1 = 0;
  size_t r = r0 + (size_t)lane * V;
  for (; r + (size_t)kWave * V < r1; r += 2 * (size_t)kWave * V) {       // two segments in flight, a sum each
    const TV a0 = *reinterpret_cast<const TV*>(col + r), x0 = *reinterpret_cast<const TV*>(rhs + r);
    const TV a1 = *reinterpret_cast<const TV*>(col + r + (size_t)kWave * V), x1 = *reinterpret_cast<const TV*>(rhs + r + (size_t)kWave * V);
#pragma unroll
    for (int j = 0; j < V; j++) { s0 += a0[j] * x0[j]; s1 += a1[j] * x1[j]; }
  }
  if (r < r1) {
    const TV a0 = *reinterpret_cast<const TV*>(col + r), x0 = *reinterpret_cast<const TV*>(rhs + r);
#pragma unroll
    for (int j = 0; j < V; j++) s0 += a0[j] * x0[j];
  }
  T sum = s0 + s1;
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) sum += __shfl_down(sum, o, kWave);
  if (lane == 0) {
    T* __restrict__ dst = out + (size_t)blockIdx.y * ncols + c;
    *dst = (ACC ? *dst : (T)0) + sum;
  }
}

// res[k] (+)= ((part 0 + part 1) + part 2) + ...
template <class T, bool ACC>
__global__ void __launch_bounds__(kBlock) gemv_combine_kernel(T* __restrict__ res, const T* __restrict__ ws, size_t n, size_t parts) {
  const size_t k = (size_t)blockIdx.x * kBlock + threadIdx.x;
  if (k >= n) return;
  T sum = ws[k];
  for (size_t p = 1; p < parts; p++) sum += ws[p * n + k];
  res[k] = (ACC ? res[k] : (T)0) + sum;
}

template <class T, bool ACC>
static int launch_gemv(T* res, const T* rhs, size_t nrows, size_t ncols, const T* A, int transpose, void* workspace, void* stream) {
  const size_t n_out = transpose ? ncols : nrows;
  if (n_out == 0) return 0;
  if (!res || !A || (!rhs && (transpose ? nrows : ncols))) { set_error("dense gemv: null pointer"); return 1; }
  hipStream_t s = as_stream(stream);
  if ((transpose ? nrows : ncols) == 0) {
    if (!ACC) PH_CHECK(hipMemsetAsync(res, 0, n_out * sizeof(T), s));
    return 0;
  }
  constexpr size_t V = 16 / sizeof(T);
  const size_t parts = transpose ? gemv_parts_adj(nrows, ncols) : gemv_parts_fwd(nrows, ncols);
  if (parts > 1 && !workspace) { set_error("dense gemv: this shape needs the workspace (prost_hip_dense_gemv_workspace_bytes)"); return 1; }
  T* out = parts > 1 ? static_cast<T*>(workspace) : res;
  const bool a16 = reinterpret_cast<uintptr_t>(A) % 16 == 0 && nrows % V == 0;
  if (!transpose) {
    const size_t cpp = (ncols + parts - 1) / parts;
    const bool vec = a16 && reinterpret_cast<uintptr_t>(out) % 16 == 0;
    const size_t gx = ((nrows + (vec ? V : 1) - 1) / (vec ? V : 1) + kWave - 1) / kWave;
    if (gx >= ((size_t)1 << 31)) { set_error("dense gemv: too many rows"); return 1; }
    const dim3 grid((unsigned)gx, (unsigned)parts), block(kWave);
    // (a part's slice of the workspace starts at part * nrows: 16-byte aligned with the workspace because nrows % V == 0 on the vector path)
    if (parts > 1) {
      if (vec) hipLaunchKernelGGL((gemv_fwd_kernel<T, false, (int)V>), grid, block, 0, s, out, rhs, nrows, ncols, A, cpp);
      else hipLaunchKernelGGL((gemv_fwd_kernel<T, false, 1>), grid, block, 0, s, out, rhs, nrows, ncols, A, cpp);
    } else {
      if (vec) hipLaunchKernelGGL((gemv_fwd_kernel<T, ACC, (int)V>), grid, block, 0, s, out, rhs, nrows, ncols, A, cpp);
      else hipLaunchKernelGGL((gemv_fwd_kernel<T, ACC, 1>), grid, block, 0, s, out, rhs, nrows, ncols, A, cpp);
    }
  } else {
    size_t rpp = (nrows + parts - 1) / parts;
    const bool vec = a16 && reinterpret_cast<uintptr_t>(rhs) % 16 == 0;
    if (vec) rpp = (rpp + V - 1) / V * V;                                 // part starts stay 16-byte aligned
    const size_t gx = (ncols + kBlock / kWave - 1) / (kBlock / kWave);
    if (gx >= ((size_t)1 << 31)) { set_error("dense gemv: too many columns"); return 1; }
    const dim3 grid((unsigned)gx, (unsigned)parts), block(kBlock);
    if (parts > 1) {
      if (vec) hipLaunchKernelGGL((gemv_adj_kernel<T, false, (int)V>), grid, block, 0, s, out, rhs, nrows, ncols, A, rpp);
      else hipLaunchKernelGGL((gemv_adj_kernel<T, false, 1>), grid, block, 0, s, out, rhs, nrows, ncols, A, rpp);
    } else {
      if (vec) hipLaunchKernelGGL((gemv_adj_kernel<T, ACC, (int)V>), grid, block, 0, s, out, rhs, nrows, ncols, A, rpp);
      else hipLaunchKernelGGL((gemv_adj_kernel<T, ACC, 1>), grid, block, 0, s, out, rhs, nrows, ncols, A, rpp);
    }
  }
  if (parts > 1) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(e, "dense gemv kernel");
    hipLaunchKernelGGL((gemv_combine_kernel<T, ACC>), dim3(grid_for(n_out)), dim3(kBlock), 0, s, res, out, n_out, parts);
  }
  PH_LAUNCH_END("dense gemv kernel");
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
#define PROST_DENSE_KRON(NAME, IDF)                                                                                                                 \
  int prost_hip_##NAME##_acc_f32(float* r, const float* x, size_t d, size_t m, size_t n, const float* K, int t, void* s) { return launch_kron_dense<float, true>(IDF, r, x, d, m, n, K, t, s); }      \
  int prost_hip_##NAME##_acc_f64(double* r, const double* x, size_t d, size_t m, size_t n, const double* K, int t, void* s) { return launch_kron_dense<double, true>(IDF, r, x, d, m, n, K, t, s); }  \
  int prost_hip_##NAME##_f32(float* r, const float* x, size_t d, size_t m, size_t n, const float* K, int t, void* s) { return launch_kron_dense<float, false>(IDF, r, x, d, m, n, K, t, s); }         \
  int prost_hip_##NAME##_f64(double* r, const double* x, size_t d, size_t m, size_t n, const double* K, int t, void* s) { return launch_kron_dense<double, false>(IDF, r, x, d, m, n, K, t, s); }
PROST_DENSE_KRON(dense_kron_id, false)
PROST_DENSE_KRON(id_kron_dense, true)
#undef PROST_DENSE_KRON

int prost_hip_dense_gemv_acc_f32(float* r, const float* x, size_t m, size_t n, const float* A, int t, void* ws, void* s) { return launch_gemv<float, true>(r, x, m, n, A, t, ws, s); }
int prost_hip_dense_gemv_acc_f64(double* r, const double* x, size_t m, size_t n, const double* A, int t, void* ws, void* s) { return launch_gemv<double, true>(r, x, m, n, A, t, ws, s); }
int prost_hip_dense_gemv_f32(float* r, const float* x, size_t m, size_t n, const float* A, int t, void* ws, void* s) { return launch_gemv<float, false>(r, x, m, n, A, t, ws, s); }
int prost_hip_dense_gemv_f64(double* r, const double* x, size_t m, size_t n, const double* A, int t, void* ws, void* s) { return launch_gemv<double, false>(r, x, m, n, A, t, ws, s); }
size_t prost_hip_dense_gemv_workspace_bytes(size_t nrows, size_t ncols) {
  const size_t fwd = gemv_parts_fwd(nrows, ncols), adj = gemv_parts_adj(nrows, ncols);
  const size_t a = fwd > 1 ? fwd * nrows : 0, b = adj > 1 ? adj * ncols : 0;
  return (a > b ? a : b) * sizeof(double);
}
}  // extern "C"
