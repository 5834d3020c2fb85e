// CPU harness for what the in-tree linear-operator blocks hand to the kernel C ABI (tests/test_linop_product_trace.py).  The host
// sources common.cpp and linop.cpp are compiled into this translation unit as they are; include/prost_hip.h is replaced by a
// recording mock, as in pdhg_launch_trace_harness.cpp.  Nothing is computed: the mock's "device" memory is host memory, an H2D copy is
// a memcpy, and every mocked call appends one line to a trace -- the entry point, every pointer as the ORDINAL of the allocation it
// points into (prost_hip_malloc numbers them in the order they are made) plus its byte offset ("-" is null), every size and int
// argument, every double in %a, and for every device array the call is given (CSR arrays, pattern tables, anchors, gamma, tap tables,
// per-angle tables, positions and buckets, twiddle tables, tensor planes, ...) and every host record (the geometry records, the wavelet
// taps) its length and a 64-bit FNV-1a digest of its bytes.  Per placement the host-only answers follow:
// sizes, gpu_mem_amount, describe / stencil_shape / uniform_sums, and every row and column sum at alpha 1 and 2 (runs of equal values
// as COUNTxVALUE) with whether the bulk forms add exactly those.
//
// Every block runs alone at (0, 0), as the second of two copies stacked below the first, and as the second of two copies side by
// side: LinearOperator's exclusive, first-writer and accumulate paths then reach all four evaluation virtuals at offset pointers.
// Before Initialize() every product is tried once, and the text of the exception is printed where a block has such a guard.
// Only public interfaces are used, so two versions of linop.cpp / blocks.hpp that print the same traces make the same ABI calls.
//
//   linop_product_trace_harness --list          names of all scenarios
//   linop_product_trace_harness all             every scenario, each behind a line "@ <name>"
//   linop_product_trace_harness <name> ...      the named scenarios
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <string>
#include <vector>

#include "prost_hip.h"

static std::vector<std::string> g_log;
static void logf(const char* fmt, ...) {
  char buf[1024];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
  g_log.push_back(buf);
}
// allocations in the order they were made; a pointer prints as the ordinal of the allocation that holds it (+ byte offset)
struct Allocation { size_t bytes; int ordinal; };
static std::map<uintptr_t, Allocation> g_allocs;
static int g_next_ordinal = 0;
static std::string P(const void* p) {
  if (!p) return "-";
  auto it = g_allocs.upper_bound((uintptr_t)p);
  if (it == g_allocs.begin()) return "?";
  --it;
  const size_t off = (uintptr_t)p - it->first;
  if (off >= it->second.bytes) return "?";
  char buf[48];
  if (off) snprintf(buf, sizeof(buf), "#%d+%zu", it->second.ordinal, off); else snprintf(buf, sizeof(buf), "#%d", it->second.ordinal);
  return buf;
}
static unsigned long long Fnv(const void* p, size_t bytes) {
  unsigned long long h = 14695981039346656037ull;
  for (size_t i = 0; i < bytes; i++) h = (h ^ ((const unsigned char*)p)[i]) * 1099511628211ull;
  return h;
}
// a device array of `count` elements of `elem` bytes: where it is, how long it is, what it holds
static std::string A(const void* p, size_t count, size_t elem) {
  if (!p) return "-";
  char buf[64];
  snprintf(buf, sizeof(buf), "[%zux%zu fnv=%016llx]", count, elem, Fnv(p, count * elem));
  return P(p) + buf;
}
static const char* R(const std::string& s) { static std::string keep[64]; static int k = 0; keep[k & 63] = s; return keep[k++ & 63].c_str(); }      // (a logf call prints up to 21)
#define PP(p) R(P(p))
#define AA(p, n, e) R(A(p, n, e))

// ---- the products: one line each ------------------------------------------------------------------------------------------------
static int grad(const char* name, const void* r, const void* x, size_t nx, size_t ny, size_t L, int lf, int acc) {
  logf("%s res=%s rhs=%s nx=%zu ny=%zu L=%zu label_first=%d acc=%d", name, PP(r), PP(x), nx, ny, L, lf, acc); return 0;
}
static int diags(const char* name, const void* r, const void* x, size_t nrows, size_t ncols, size_t nd, const int64_t* off, const float* fac, int quirk) {
  logf("%s res=%s rhs=%s nrows=%zu ncols=%zu ndiags=%zu offsets=%s factors=%s quirk=%d", name, PP(r), PP(x), nrows, ncols, nd, AA(off, nd, 8), AA(fac, nd, 4), quirk); return 0;
}
static int csr(const char* name, size_t e, const void* r, const void* x, size_t nrows, size_t nnz, const void* val, const int32_t* ptr, const int32_t* ind) {
  logf("%s res=%s rhs=%s nrows=%zu nnz=%zu val=%s ptr=%s ind=%s", name, PP(r), PP(x), nrows, nnz, AA(val, nnz, e), AA(ptr, nrows + 1, 4), AA(ind, nnz, 4)); return 0;
}
static int pattern(const char* name, size_t e, const void* r, const void* x, size_t nrows, const uint16_t* ids, const int32_t* anchor, bool anchored, const int32_t* pptr,
                   const int32_t* rel, const void* pval, int npat, int nent, int acc) {
  const size_t padded = (nrows + 3) / 4 * 4;
  logf("%s res=%s rhs=%s nrows=%zu ids=%s%s%s pptr=%s rel=%s pval=%s npatterns=%d nentries=%d acc=%d", name, PP(r), PP(x), nrows, AA(ids, padded, 2), anchored ? " anchor=" : "",
       anchored ? AA(anchor, padded, 4) : "", AA(pptr, (size_t)npat + 1, 4), AA(rel, (size_t)nent, 4), AA(pval, (size_t)nent, e), npat, nent, acc);
  return 0;
}
static int kron_sparse(const char* name, const void* r, const void* x, size_t d, size_t nrows, long ncols, const float* val, const int32_t* ptr, const int32_t* ind) {
  const size_t nnz = ptr ? (size_t)ptr[nrows] : 0;
  char nc[32] = "";
  if (ncols >= 0) snprintf(nc, sizeof(nc), " ncols=%ld", ncols);
  logf("%s res=%s rhs=%s diaglength=%zu nrows=%zu%s val=%s ptr=%s ind=%s", name, PP(r), PP(x), d, nrows, nc, AA(val, nnz, 4), AA(ptr, nrows + 1, 4), AA(ind, nnz, 4)); return 0;
}
static int kron_dense(const char* name, size_t e, const void* r, const void* x, size_t d, size_t nrows, size_t ncols, const void* data, int transpose) {
  logf("%s res=%s rhs=%s diaglength=%zu nrows=%zu ncols=%zu data=%s transpose=%d", name, PP(r), PP(x), d, nrows, ncols, AA(data, nrows * ncols, e), transpose); return 0;
}
static int gemv(const char* name, size_t e, const void* r, const void* x, size_t nrows, size_t ncols, const void* data, int transpose, const void* ws) {
  logf("%s res=%s rhs=%s nrows=%zu ncols=%zu data=%s transpose=%d workspace=%s", name, PP(r), PP(x), nrows, ncols, AA(data, nrows * ncols, e), transpose, PP(ws)); return 0;
}
static int sublabel(const char* name, size_t e, const void* r, const void* x, size_t npixels, size_t L, const void* gamma, double delta, int transpose, int acc) {
  logf("%s res=%s rhs=%s npixels=%zu L=%zu gamma=%s delta=%a transpose=%d acc=%d", name, PP(r), PP(x), npixels, L, AA(gamma, L - 1, e), delta, transpose, acc); return 0;
}
static int conv(const char* name, size_t tap_bytes, const prost_hip_conv2d_geometry* g, const void* taps, size_t ntaps, const void* r, const void* x, int acc) {
  logf("%s geometry=host[%zu fnv=%016llx] taps=%s ntaps=%zu res=%s rhs=%s acc=%d", name, sizeof(*g), Fnv(g, sizeof(*g)), AA(taps, ntaps, tap_bytes), ntaps, PP(r), PP(x), acc); return 0;
}
// a record or array the ABI reads on the host before the call returns
static std::string H(const void* p, size_t bytes) {
  char buf[64];
  snprintf(buf, sizeof(buf), "host[%zu fnv=%016llx]", bytes, Fnv(p, bytes));
  return buf;
}
#define HH(p, n) R(H(p, n))
static int conv_strided(const char* name, size_t tap_bytes, const prost_hip_conv2d_strided_geometry* g, const void* taps, size_t ntaps, const void* r, const void* x, int acc) {
  logf("%s geometry=%s transpose=%d taps=%s ntaps=%zu res=%s rhs=%s acc=%d", name, HH(g, sizeof(*g)), (int)g->transpose, AA(taps, ntaps, tap_bytes), ntaps, PP(r), PP(x), acc); return 0;
}
static int radon(const char* name, size_t e, const prost_hip_radon2d_geometry* g, const void* table, const void* r, const void* x, int acc) {
  logf("%s geometry=%s transpose=%d table=%s res=%s rhs=%s acc=%d", name, HH(g, sizeof(*g)), (int)g->transpose, AA(table, (size_t)g->na * PROST_HIP_RADON2D_TABLE_WIDTH, e), PP(r), PP(x),
       acc); return 0;
}
static int sample(const char* name, size_t e, const prost_hip_sample2d_geometry* g, const void* px, const void* py, const int32_t* order, const int32_t* cell_start, const void* r,
                  const void* x, int acc) {
  const size_t m = (size_t)g->m, cells = ((size_t)g->ny + 1) * ((size_t)g->nx + 1);
  logf("%s geometry=%s transpose=%d pos_x=%s pos_y=%s order=%s cell_start=%s res=%s rhs=%s acc=%d", name, HH(g, sizeof(*g)), (int)g->transpose, AA(px, m, e), AA(py, m, e),
       AA(order, m, 4), AA(cell_start, cells + 1, 4), PP(r), PP(x), acc); return 0;
}
static int fft(const char* name, size_t e, const prost_hip_fft2d_geometry* g, const void* table, const void* work, const void* r, const void* x, int acc) {
  const size_t n = (size_t)(g->ny > g->nx ? g->ny : g->nx), values = 2 * (size_t)g->planes * (size_t)g->ny * (size_t)g->nx;
  logf("%s geometry=%s transpose=%d table=%s work=%s res=%s rhs=%s acc=%d", name, HH(g, sizeof(*g)), (int)g->transpose, AA(table, 2 * n, e), AA(work, values, e), PP(r), PP(x), acc);
  return 0;
}
// planes (C(1) + C(2)) values, C(j) the corner of a plane after j levels (a side of 1 stays 1)
static size_t WaveletWorkValues(const prost_hip_wavelet2d_geometry* g) {
  auto side = [](int n, int j) { return (size_t)(n > 1 ? n >> j : 1); };
  return (size_t)g->planes * (side(g->ny, 1) * side(g->nx, 1) + side(g->ny, 2) * side(g->nx, 2));
}
static int wavelet(const char* name, size_t e, const prost_hip_wavelet2d_geometry* g, const void* taps, const void* work, size_t work_values, const void* r, const void* x, int acc) {
  logf("%s geometry=%s transpose=%d taps=%s work=%s res=%s rhs=%s acc=%d", name, HH(g, sizeof(*g)), (int)g->transpose, HH(taps, (size_t)g->ntaps * e), AA(work, work_values, e), PP(r),
       PP(x), acc); return 0;
}
static int tensorgrad(const char* name, size_t e, const void* r, const void* x, const void* tensor, size_t nx, size_t ny, size_t L, int mode, int transpose, int acc) {
  logf("%s res=%s rhs=%s tensor=%s nx=%zu ny=%zu L=%zu mode=%d transpose=%d acc=%d", name, PP(r), PP(x), AA(tensor, (size_t)mode * nx * ny, e), nx, ny, L, mode, transpose, acc); return 0;
}
static int symgrad(const char* name, const void* r, const void* x, size_t nx, size_t ny, size_t L, double w, int transpose, int acc) {
  logf("%s res=%s rhs=%s nx=%zu ny=%zu L=%zu w=%a transpose=%d acc=%d", name, PP(r), PP(x), nx, ny, L, w, transpose, acc); return 0;
}

extern "C" {
const char* prost_hip_last_error(void) { return ""; }
int prost_hip_malloc(void** p, size_t bytes) {
  *p = calloc(bytes ? bytes : 1, 1);
  g_allocs[(uintptr_t)*p] = {bytes ? bytes : 1, g_next_ordinal++};
  logf("malloc %s %zu bytes", PP(*p), bytes);
  return 0;
}
int prost_hip_free(void* p) { logf("free %s", PP(p)); g_allocs.erase((uintptr_t)p); free(p); return 0; }
int prost_hip_memcpy_h2d(void* d, const void* s, size_t n, void*) { memcpy(d, s, n); logf("h2d %s %zu bytes fnv=%016llx", PP(d), n, Fnv(s, n)); return 0; }
int prost_hip_memcpy_d2h(void* d, const void* s, size_t n, void*) { memcpy(d, s, n); logf("d2h %s %zu bytes", PP(s), n); return 0; }
int prost_hip_memcpy_d2d(void* d, const void* s, size_t n, void*) { memmove(d, s, n); logf("d2d %s from %s %zu bytes", PP(d), PP(s), n); return 0; }
int prost_hip_memset(void* d, int v, size_t n, void*) { memset(d, v, n); logf("memset %s %d %zu bytes", PP(d), v, n); return 0; }
int prost_hip_stream_synchronize(void*) { logf("stream_synchronize"); return 0; }
size_t prost_hip_dense_gemv_workspace_bytes(size_t nrows, size_t ncols) { return 16 * (nrows + ncols); }

#define LINOP_MOCKS(T, S)                                                                                                                                                   \
  int prost_hip_scale_##S(T* x, size_t n, double beta, void*) { logf("scale_" #S " x=%s n=%zu beta=%a", PP(x), n, beta); return 0; }                                       \
  int prost_hip_fill_##S(T* x, double v, size_t n, void*) { logf("fill_" #S " x=%s value=%a n=%zu", PP(x), v, n); return 0; }                                              \
  int prost_hip_grad2d_fwd_##S(T* r, const T* x, size_t nx, size_t ny, size_t L, int lf, int acc, void*) { return grad("grad2d_fwd_" #S, r, x, nx, ny, L, lf, acc); }       \
  int prost_hip_grad2d_adj_##S(T* r, const T* x, size_t nx, size_t ny, size_t L, int lf, int acc, void*) { return grad("grad2d_adj_" #S, r, x, nx, ny, L, lf, acc); }       \
  int prost_hip_grad3d_fwd_##S(T* r, const T* x, size_t nx, size_t ny, size_t L, int lf, int acc, void*) { return grad("grad3d_fwd_" #S, r, x, nx, ny, L, lf, acc); }       \
  int prost_hip_grad3d_adj_##S(T* r, const T* x, size_t nx, size_t ny, size_t L, int lf, int acc, void*) { return grad("grad3d_adj_" #S, r, x, nx, ny, L, lf, acc); }       \
  int prost_hip_diags_fwd_##S(T* r, const T* x, size_t m, size_t n, size_t nd, const int64_t* o, const float* f, void*) { return diags("diags_fwd_" #S, r, x, m, n, nd, o, f, -1); } \
  int prost_hip_diags_adj_##S(T* r, const T* x, size_t m, size_t n, size_t nd, const int64_t* o, const float* f, int q, void*) { return diags("diags_adj_" #S, r, x, m, n, nd, o, f, q); } \
  int prost_hip_csr_spmv_acc_##S(T* r, const T* x, size_t m, size_t nnz, const T* v, const int32_t* p, const int32_t* i, void*) { return csr("csr_spmv_acc_" #S, sizeof(T), r, x, m, nnz, v, p, i); } \
  int prost_hip_csr_spmv_##S(T* r, const T* x, size_t m, size_t nnz, const T* v, const int32_t* p, const int32_t* i, void*) { return csr("csr_spmv_" #S, sizeof(T), r, x, m, nnz, v, p, i); } \
  int prost_hip_pattern_spmv_tab_##S(T* r, const T* x, size_t m, const uint16_t* ids, const int32_t* pp, const int32_t* rel, const T* pv, int np, int ne, int acc, void*) { \
    return pattern("pattern_spmv_" #S, sizeof(T), r, x, m, ids, nullptr, false, pp, rel, pv, np, ne, acc);                                                                  \
  }                                                                                                                                                                         \
  int prost_hip_pattern_spmv_anchored_##S(T* r, const T* x, size_t m, const uint16_t* ids, const int32_t* an, const int32_t* pp, const int32_t* rel, const T* pv, int np,   \
                                          int ne, int acc, void*) {                                                                                                         \
    return pattern("pattern_spmv_anchored_" #S, sizeof(T), r, x, m, ids, an, true, pp, rel, pv, np, ne, acc);                                                               \
  }                                                                                                                                                                         \
  int prost_hip_sparse_kron_id_acc_##S(T* r, const T* x, size_t d, size_t m, const float* v, const int32_t* p, const int32_t* i, void*) { return kron_sparse("sparse_kron_id_acc_" #S, r, x, d, m, -1, v, p, i); } \
  int prost_hip_sparse_kron_id_##S(T* r, const T* x, size_t d, size_t m, const float* v, const int32_t* p, const int32_t* i, void*) { return kron_sparse("sparse_kron_id_" #S, r, x, d, m, -1, v, p, i); } \
  int prost_hip_id_kron_sparse_acc_##S(T* r, const T* x, size_t d, size_t m, size_t n, const float* v, const int32_t* p, const int32_t* i, void*) { return kron_sparse("id_kron_sparse_acc_" #S, r, x, d, m, (long)n, v, p, i); } \
  int prost_hip_id_kron_sparse_##S(T* r, const T* x, size_t d, size_t m, size_t n, const float* v, const int32_t* p, const int32_t* i, void*) { return kron_sparse("id_kron_sparse_" #S, r, x, d, m, (long)n, v, p, i); } \
  int prost_hip_dense_kron_id_acc_##S(T* r, const T* x, size_t d, size_t m, size_t n, const T* a, int t, void*) { return kron_dense("dense_kron_id_acc_" #S, sizeof(T), r, x, d, m, n, a, t); } \
  int prost_hip_dense_kron_id_##S(T* r, const T* x, size_t d, size_t m, size_t n, const T* a, int t, void*) { return kron_dense("dense_kron_id_" #S, sizeof(T), r, x, d, m, n, a, t); } \
  int prost_hip_id_kron_dense_acc_##S(T* r, const T* x, size_t d, size_t m, size_t n, const T* a, int t, void*) { return kron_dense("id_kron_dense_acc_" #S, sizeof(T), r, x, d, m, n, a, t); } \
  int prost_hip_id_kron_dense_##S(T* r, const T* x, size_t d, size_t m, size_t n, const T* a, int t, void*) { return kron_dense("id_kron_dense_" #S, sizeof(T), r, x, d, m, n, a, t); } \
  int prost_hip_dense_gemv_acc_##S(T* r, const T* x, size_t m, size_t n, const T* a, int t, void* ws, void*) { return gemv("dense_gemv_acc_" #S, sizeof(T), r, x, m, n, a, t, ws); } \
  int prost_hip_dense_gemv_##S(T* r, const T* x, size_t m, size_t n, const T* a, int t, void* ws, void*) { return gemv("dense_gemv_" #S, sizeof(T), r, x, m, n, a, t, ws); } \
  int prost_hip_linop_dataterm_sublabel_##S(T* r, const T* x, size_t np, size_t L, const T* g, double delta, int t, int acc, void*) {                                       \
    return sublabel("linop_dataterm_sublabel_" #S, sizeof(T), r, x, np, L, g, delta, t, acc);                                                                               \
  }                                                                                                                                                                         \
  int prost_hip_conv2d_##S(const prost_hip_conv2d_geometry* g, const prost_hip_conv2d_tap_##S* taps, size_t nt, T* r, const T* x, int acc, void*) {                         \
    return conv("conv2d_" #S, sizeof(prost_hip_conv2d_tap_##S), g, taps, nt, r, x, acc);                                                                                    \
  }                                                                                                                                                                         \
  int prost_hip_linop_sym_gradient2d_##S(T* r, const T* x, size_t nx, size_t ny, size_t L, double w, int t, int acc, void*) { return symgrad("linop_sym_gradient2d_" #S, r, x, nx, ny, L, w, t, acc); } \
  int prost_hip_conv2d_strided_##S(const prost_hip_conv2d_strided_geometry* g, const prost_hip_conv2d_tap_##S* taps, size_t nt, T* r, const T* x, int acc, void*) {         \
    return conv_strided("conv2d_strided_" #S, sizeof(prost_hip_conv2d_tap_##S), g, taps, nt, r, x, acc);                                                                    \
  }                                                                                                                                                                         \
  int prost_hip_radon2d_##S(const prost_hip_radon2d_geometry* g, const T* table, T* r, const T* x, int acc, void*) { return radon("radon2d_" #S, sizeof(T), g, table, r, x, acc); } \
  int prost_hip_sample2d_##S(const prost_hip_sample2d_geometry* g, const T* px, const T* py, const int32_t* o, const int32_t* cs, T* r, const T* x, int acc, void*) {        \
    return sample("sample2d_" #S, sizeof(T), g, px, py, o, cs, r, x, acc);                                                                                                  \
  }                                                                                                                                                                         \
  int prost_hip_fft2d_##S(const prost_hip_fft2d_geometry* g, const T* table, T* work, T* r, const T* x, int acc, void*) { return fft("fft2d_" #S, sizeof(T), g, table, work, r, x, acc); } \
  int prost_hip_wavelet2d_##S(const prost_hip_wavelet2d_geometry* g, const T* taps, T* work, T* r, const T* x, int acc, void*) {                                           \
    return wavelet("wavelet2d_" #S, sizeof(T), g, taps, work, WaveletWorkValues(g), r, x, acc);                                                                            \
  }                                                                                                                                                                         \
  int prost_hip_linop_tensor_gradient2d_##S(T* r, const T* x, const T* tensor, size_t nx, size_t ny, size_t L, int mode, int t, int acc, void*) {                           \
    return tensorgrad("linop_tensor_gradient2d_" #S, sizeof(T), r, x, tensor, nx, ny, L, mode, t, acc);                                                                     \
  }
LINOP_MOCKS(float, f32)
LINOP_MOCKS(double, f64)
#undef LINOP_MOCKS
int prost_hip_negate_f32(float* x, size_t n, void*) { logf("negate_f32 x=%s n=%zu", PP(x), n); return 0; }
int prost_hip_negate_f64(double* x, size_t n, int via_float, void*) { logf("negate_f64 x=%s n=%zu via_float=%d", PP(x), n, via_float); return 0; }
}  // extern "C"

#include "../../prost_amd/csrc/host/common.cpp"
#include "../../prost_amd/csrc/host/linop.cpp"

using namespace prost;

// ---- host-only answers ----------------------------------------------------------------------------------------------------------
template <typename T>
static std::string Runs(const std::vector<T>& v) {          // runs of equal values as COUNTxVALUE
  std::string out;
  char buf[64];
  for (size_t i = 0; i < v.size();) {
    size_t j = i;
    while (j < v.size() && std::memcmp(&v[j], &v[i], sizeof(T)) == 0) j++;
    snprintf(buf, sizeof(buf), "%s%zux%a", i ? " " : "", j - i, (double)v[i]);
    out += buf;
    i = j;
  }
  return out;
}
static void LogDesc(const char* what, size_t index, bool answer, const BlockDesc& d) {
  if (!answer) { logf("-- block %zu %s: no", index, what); return; }
  logf("-- block %zu %s: kind=%d nx=%zu ny=%zu L=%zu label_first=%d nnz=%zu val=%s ptr=%s ind=%s val_t=%s ptr_t=%s ind_t=%s pointwise_planes=%zu ids=%s pptr=%s rel=%s pval=%s anchor=%s "
       "ids_t=%s pptr_t=%s rel_t=%s pval_t=%s anchor_t=%s",
       index, what, (int)d.kind, d.nx, d.ny, d.L, (int)d.label_first, d.nnz, PP(d.val), PP(d.ptr), PP(d.ind), PP(d.val_t), PP(d.ptr_t), PP(d.ind_t), d.pointwise_planes, PP(d.ids),
       PP(d.pptr), PP(d.rel), PP(d.pval), PP(d.anchor), PP(d.ids_t), PP(d.pptr_t), PP(d.rel_t), PP(d.pval_t), PP(d.anchor_t));
}
template <typename T>
static void LogBlocks(const LinearOperator<T>& op) {
  for (size_t i = 0; i < op.blocks().size(); i++) {
    const Block<T>& b = *op.blocks()[i];
    BlockDesc d, s;
    const bool described = b.describe(d), stencil = b.stencil_shape(s);
    LogDesc("describe", i, described, d);
    LogDesc("stencil_shape", i, stencil, s);
    T row = -1, col = -1;
    const bool uniform = b.uniform_sums((T)1, (T)1, row, col);
    logf("-- block %zu at (%zu, %zu) %zu x %zu gpu_mem_amount=%zu uniform_sums=%d row=%a col=%a", i, b.row(), b.col(), b.nrows(), b.ncols(), b.gpu_mem_amount(), (int)uniform,
         (double)row, (double)col);
  }
}
template <typename T>
static void LogSums(const LinearOperator<T>& op) {
  T row = -1, col = -1;
  const bool uniform = op.uniform_sums((T)1, (T)1, row, col);
  logf("-- operator %zu x %zu gpu_mem_amount=%zu uniform_sums=%d row=%a col=%a", op.nrows(), op.ncols(), op.gpu_mem_amount(), (int)uniform, (double)row, (double)col);
  for (int a = 1; a <= 2; a++) {
    std::vector<T> one(op.nrows()), bulk(op.nrows(), (T)7);
    for (size_t r = 0; r < one.size(); r++) one[r] = op.row_sum(r, (T)a);
    op.row_sums(bulk, (T)a);
    g_log.push_back("-- row_sum alpha=" + std::to_string(a) + " row_sums_equal=" + std::to_string((int)(std::memcmp(one.data(), bulk.data(), one.size() * sizeof(T)) == 0)) + ": " + Runs(one));
    one.assign(op.ncols(), 0); bulk.assign(op.ncols(), (T)7);
    for (size_t c = 0; c < one.size(); c++) one[c] = op.col_sum(c, (T)a);
    op.col_sums(bulk, (T)a);
    g_log.push_back("-- col_sum alpha=" + std::to_string(a) + " col_sums_equal=" + std::to_string((int)(std::memcmp(one.data(), bulk.data(), one.size() * sizeof(T)) == 0)) + ": " + Runs(one));
  }
}
template <typename T>
static void Products(const char* when, LinearOperator<T>& op, device_vector<T>& x, device_vector<T>& y) {
  auto shared = std::shared_ptr<LinearOperator<T>>(&op, [](LinearOperator<T>*) {});
  DualLinearOperator<T> dual(shared);
  for (int which = 0; which < 4; which++)
    for (int beta = 0; beta <= 1; beta++) {
      if (which >= 2 && !strcmp(when, "before Initialize")) continue;
      const char* names[] = {"Eval", "EvalAdjoint", "Dual::Eval", "Dual::EvalAdjoint"};
      logf("-- %s beta=%d (%s)", names[which], beta, when);
      try {
        if (which == 0) op.Eval(y, x, (T)beta);
        else if (which == 1) op.EvalAdjoint(x, y, (T)beta);
        else if (which == 2) dual.Eval(x, y, (T)beta);
        else dual.EvalAdjoint(y, x, (T)beta);
      } catch (const std::exception& e) {
        logf("-- EXCEPTION %s", e.what());
      }
    }
}

template <typename T> using Make = std::function<Block<T>*(size_t row, size_t col)>;

template <typename T>
static void Placement(const char* name, const Make<T>& make, int copies, bool below) {
  if (!g_allocs.empty()) { std::fprintf(stderr, "allocations left over\n"); std::exit(4); }
  g_next_ordinal = 0;
  {
    LinearOperator<T> op;
    std::shared_ptr<Block<T>> first(make(0, 0));
    op.AddBlock(first);
    if (copies == 2) op.AddBlock(std::shared_ptr<Block<T>>(below ? make(first->nrows(), 0) : make(0, first->ncols())));
    op.InitializeHost();
    logf("-- placement %s: %zu x %zu", name, op.nrows(), op.ncols());
    device_vector<T> x(op.ncols()), y(op.nrows());
    Products("before Initialize", op, x, y);
    logf("-- Initialize");
    op.Initialize();
    LogBlocks(op);
    LogSums(op);
    Products("initialized", op, x, y);
    logf("-- Release");
    op.Release();
    LogBlocks(op);
  }
}
template <typename T>
static void RunBlock(const Make<T>& make) {
  Placement<T>("alone", make, 1, false);
  Placement<T>("second of two, below", make, 2, true);
  Placement<T>("second of two, to the right", make, 2, false);
}

// ---- scenarios -----------------------------------------------------------------------------------------------------------------
struct Csc { int m = 0, n = 0; std::vector<double> val; std::vector<int32_t> ptr, ind; };
static Csc MakeCsc(int m, int n, const std::function<bool(int, int, double&)>& entry) {
  Csc c; c.m = m; c.n = n; c.ptr.push_back(0);
  for (int col = 0; col < n; col++) {
    for (int row = 0; row < m; row++) { double v = 0; if (entry(row, col, v)) { c.val.push_back(v); c.ind.push_back(row); } }
    c.ptr.push_back((int32_t)c.val.size());
  }
  return c;
}
// small multiples of 1/4 from a fixed linear congruential sequence, a function of (row, col) alone
static double Value(int row, int col) {
  uint32_t s = (uint32_t)(row * 131 + col * 31 + 7);
  for (int i = 0; i < 3; i++) s = s * 1664525u + 1013904223u;
  const int k = (int)((s >> 16) % 33) - 16;
  return (k ? k : 17) * 0.25;
}
static bool Kept(int row, int col) {
  uint32_t s = (uint32_t)(row * 57 + col * 13 + 3);
  for (int i = 0; i < 3; i++) s = s * 1664525u + 1013904223u;
  return ((s >> 16) & 3) != 0;
}
template <typename T> static std::vector<T> As(const std::vector<double>& v) { return std::vector<T>(v.begin(), v.end()); }
template <typename T> static Block<T>* Sparse(const Csc& c, size_t row, size_t col) {
  return BlockSparse<T>::CreateFromCSC(row, col, c.m, c.n, (int)c.val.size(), As<T>(c.val), c.ptr, c.ind);
}
template <typename T> static Block<T>* KronSparse(bool id_first, const Csc& c, size_t row, size_t col) {
  return BlockKronSparse<T>::CreateFromCSC(id_first, row, col, 4, c.m, c.n, (int)c.val.size(), As<T>(c.val), c.ptr, c.ind);
}
static std::vector<double> DenseData(int m, int n) {
  std::vector<double> d;
  for (int col = 0; col < n; col++) for (int row = 0; row < m; row++) d.push_back(Value(row, col));
  return d;
}

struct Scenario { std::string name; std::function<void()> run; };
template <typename T>
static void Add(std::vector<Scenario>& all, const std::string& name, const Make<T>& make) {
  all.push_back({name + (sizeof(T) == 4 ? ".f32" : ".f64"), [make]() { RunBlock<T>(make); }});
}
#define BLOCK(NAME, EXPR)                                                                                \
  Add<float>(all, NAME, [=](size_t row, size_t col) -> Block<float>* { typedef float T; return EXPR; }); \
  Add<double>(all, NAME, [=](size_t row, size_t col) -> Block<double>* { typedef double T; return EXPR; });

static std::vector<Scenario> AllScenarios() {
  std::vector<Scenario> all;
  for (int lf = 0; lf <= 1; lf++) {
    BLOCK("gradient2d.label_first" + std::to_string(lf), new BlockGradient2D<T>(row, col, 3, 4, 2, lf != 0))
    BLOCK("gradient3d.label_first" + std::to_string(lf), new BlockGradient3D<T>(row, col, 3, 4, 2, lf != 0))
  }
  const Csc random = MakeCsc(5, 7, [](int r, int c, double& v) { v = Value(r, c); return Kept(r, c); });
  const Csc difference = MakeCsc(300, 300, [](int r, int c, double& v) { v = c == r ? -1 : 1; return r < 299 && (c == r || c == r + 1); });
  const Csc pairs = MakeCsc(300, 600, [](int r, int c, double& v) { v = c == 2 * r ? 0.5 : -1.5; return c == 2 * r || c == 2 * r + 1; });
  const Csc empty = MakeCsc(4, 6, [](int, int, double&) { return false; });
  const Csc small = MakeCsc(2, 3, [](int r, int c, double& v) { v = Value(r + 2, c + 5); return !(r == 1 && c == 1); });
  BLOCK("sparse.random5x7", Sparse<T>(random, row, col))
  BLOCK("sparse.difference300", Sparse<T>(difference, row, col))
  BLOCK("sparse.pairs300x600", Sparse<T>(pairs, row, col))
  BLOCK("sparse.empty4x6", Sparse<T>(empty, row, col))
  BLOCK("sparse_kron_id", KronSparse<T>(false, small, row, col))
  BLOCK("id_kron_sparse", KronSparse<T>(true, small, row, col))
  BLOCK("dense", BlockDense<T>::CreateFromColFirstData(row, col, 3, 5, As<T>(DenseData(3, 5))))
  BLOCK("dense_kron_id", BlockKronDense<T>::CreateFromColFirstData(false, 4, row, col, 2, 3, As<T>(DenseData(2, 3))))
  BLOCK("id_kron_dense", BlockKronDense<T>::CreateFromColFirstData(true, 4, row, col, 2, 3, As<T>(DenseData(2, 3))))
  BLOCK("dataterm_sublabel", BlockDatatermSublabel<T>::Create(row, col, 2, 3, 4, 0.0, 1.0))
  BLOCK("conv2d", BlockConv2D<T>::Create(row, col, 4, 5, 2, DenseData(3, 2), 3, 2, "same"))
  BLOCK("sym_gradient2d", BlockSymGradient2D<T>::Create(row, col, 3, 4, 2, 0.5))
  // the blocks added after sym_gradient2d: the smallest shapes that reach every branch of their host code
  std::vector<double> window = DenseData(3, 3);
  window[4] = 0;                                         // one zero tap
  BLOCK("conv2d_strided", BlockConv2DStrided<T>::Create(row, col, 7, 5, 2, window, 3, 3, "same", 2, 2, 1, 0))
  // a row-marched, a column-marched and an obtuse angle; the default detector length 2 ceil(hypot(6, 5) / 2) + 1
  BLOCK("radon2d", BlockRadon2D<T>::Create(row, col, 6, 5, 2, std::vector<double>{0, 0.7, 2.2}, 9, 1, 0.25))
  // a pixel centre, two positions in one cell, one in the border strip [-1, 0), one outside (a zero row), two more
  const std::vector<double> sx = {2, 1.25, 1.75, -0.5, 7, 3.5, 0.25}, sy = {1, 0.5, 0.25, 1.5, 2, 2.5, 2.875};
  BLOCK("sample2d", BlockSample2D<T>::Create(row, col, 5, 4, 2, sx, sy))
  BLOCK("fft2d", BlockFFT2D<T>::Create(row, col, 4, 8, 2))
  const std::vector<double> db2 = {0.48296291314453416, 0.83651630373780790, 0.22414386804201339, -0.12940952255126037};
  BLOCK("wavelet2d", BlockWavelet2D<T>::Create(row, col, 8, 4, 2, db2, 1))
  std::vector<double> tensor3 = DenseData(12, 3), tensor1 = DenseData(12, 1);
  tensor3[17] = 0;                                       // an edge that is switched off
  BLOCK("tensor_gradient2d.k3", BlockTensorGradient2D<T>::Create(row, col, 4, 3, 2, 3, tensor3))
  BLOCK("tensor_gradient2d.k1", BlockTensorGradient2D<T>::Create(row, col, 4, 3, 2, 1, tensor1))
  BLOCK("diags", new BlockDiags<T>(row, col, 4, 5, 3, std::vector<int64_t>{1, -1, 0}, As<T>(std::vector<double>{0.5, -2, 1.25})))
  BLOCK("zero", new BlockZero<T>(row, col, 3, 4))
  return all;
}

int main(int argc, char** argv) {
  const std::vector<Scenario> all = AllScenarios();
  if (argc < 2 || !strcmp(argv[1], "--list")) { for (const Scenario& s : all) std::printf("%s\n", s.name.c_str()); return 0; }
  for (int a = 1; a < argc; a++) {
    bool found = false;
    for (const Scenario& s : all)
      if (!strcmp(argv[a], "all") || s.name == argv[a]) {
        g_log.clear();
        s.run();
        std::printf("@ %s\n", s.name.c_str());
        for (const std::string& l : g_log) std::printf("%s\n", l.c_str());
        found = true;
      }
    if (!found) { std::fprintf(stderr, "no scenario %s\n", argv[a]); return 2; }
  }
  return 0;
}
