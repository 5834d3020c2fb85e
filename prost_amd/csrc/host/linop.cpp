// linop.cpp -- blocks and the block container of the prost host library (calls prost_hip.h only).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <atomic>
#include <cstring>
#include <mutex>
#include <sstream>
#include <thread>
#include <unordered_map>

#include "hipapi.hpp"
#include "prost/linop/blocks.hpp"
#include "prost/linop/conv2d.hpp"
#include "prost/linop/dataterm_sublabel.hpp"
#include "prost/linop/linearoperator.hpp"

namespace prost {

// ---- Block defaults: non-accumulating = zero fill + accumulate ----
template <typename T>
void Block<T>::EvalLocal(T* rb, T* re, const T* xb, const T* xe) {
  CheckHip(Api<T>::scale(rb, (size_t)(re - rb), 0.0, CurrentStream()), "scale");
  EvalLocalAdd(rb, re, xb, xe);
}
template <typename T>
void Block<T>::EvalAdjointLocal(T* rb, T* re, const T* xb, const T* xe) {
  CheckHip(Api<T>::scale(rb, (size_t)(re - rb), 0.0, CurrentStream()), "scale");
  EvalAdjointLocalAdd(rb, re, xb, xe);
}
template class Block<float>;
template class Block<double>;

// ---- gradient blocks ----
template <typename T, int D>
void BlockGradient<T, D>::Product(T* r, const T* x, bool transpose, bool accumulate) {
  const auto fn = D == 2 ? (transpose ? Api<T>::grad2d_adj : Api<T>::grad2d_fwd) : (transpose ? Api<T>::grad3d_adj : Api<T>::grad3d_fwd);
  const char* name = D == 2 ? (transpose ? "grad2d_adj" : "grad2d_fwd") : (transpose ? "grad3d_adj" : "grad3d_fwd");
  CheckHip(fn(r, x, nx_, ny_, L_, label_first_, accumulate ? 1 : 0, CurrentStream()), name);
}
template <typename T, int D> void BlockGradient<T, D>::row_sums(T* out, T) const { ParallelFor(this->nrows(), [&](size_t b, size_t e) { for (size_t r = b; r < e; r++) out[r] += 2; }); }
template <typename T, int D> void BlockGradient<T, D>::col_sums(T* out, T) const { ParallelFor(this->ncols(), [&](size_t b, size_t e) { for (size_t c = b; c < e; c++) out[c] += 2 * D; }); }
template class BlockGradient<float, 2>;
template class BlockGradient<double, 2>;
template class BlockGradient<float, 3>;
template class BlockGradient<double, 3>;

// ---- sparse block ----
template <typename T>
BlockSparse<T>* BlockSparse<T>::CreateFromCSC(size_t row, size_t col, int m, int n, int nnz, const std::vector<T>& val,
                                              const std::vector<int32_t>& ptr, const std::vector<int32_t>& ind) {
  return CreateFromCSC(row, col, m, n, nnz, std::vector<T>(val), std::vector<int32_t>(ptr), std::vector<int32_t>(ind));
}
template <typename T>
BlockSparse<T>* BlockSparse<T>::CreateFromCSC(size_t row, size_t col, int m, int n, int nnz, std::vector<T>&& val, std::vector<int32_t>&& ptr,
                                              std::vector<int32_t>&& ind) {
  BlockSparse<T>* b = new BlockSparse<T>(row, col, m, n);
  b->nnz_ = nnz;
  // the CSC arrays of K are the CSR arrays of K^T; K itself in CSR comes from one transposition
  Side &k = b->side_[0], &kt = b->side_[1];
  k.rows = m; kt.rows = n;
  kt.host_ind = std::move(ind); kt.host_ptr = std::move(ptr); kt.host_val = std::move(val);
  k.host_ind.resize(nnz); k.host_val.resize(nnz); k.host_ptr.resize(m + 1);
  csr2csc<T>(n, m, nnz, kt.host_val.data(), kt.host_ind.data(), kt.host_ptr.data(), k.host_val.data(), k.host_ind.data(), k.host_ptr.data());
  return b;
}
template <typename V>
template <typename T>
T CsrSide<V>::AbsPowSum(size_t row, T alpha) const {
  T sum = 0;
  for (int32_t i = host_ptr[row]; i < host_ptr[row + 1]; i++) sum += std::pow(std::abs(host_val[i]), alpha);
  return sum;
}
// Rows of a CSR matrix as repeated (column - row, value) sequences.  Returns false -- the matrix stays CSR -- when it is small (< 256
// rows), when its rows are not made of few sequences (more than a quarter of up to 4096 sampled rows differ; > 4096 sequences in all, or
// a table of > 65536 entries), or on a signature collision.
namespace {
bool g_sparse_patterns = true;
template <typename T>
struct HostRowPatterns { std::vector<uint16_t> ids; std::vector<int32_t> pptr, rel, anchor; std::vector<T> val; };
template <typename T>
bool BuildRowPatterns(size_t nrows, const std::vector<int32_t>& ptr, const std::vector<int32_t>& ind, const std::vector<T>& val, HostRowPatterns<T>& out, bool anchored = false) {
  // anchored: offsets count from the row's FIRST COLUMN instead of from the row number (matrices between different geometries)
  auto base_of = [&](size_t r) -> int32_t { return anchored ? (ptr[r + 1] > ptr[r] ? ind[ptr[r]] : 0) : (int32_t)r; };
  constexpr size_t kMinRows = 256, kMaxPatterns = 4096, kMaxTable = (size_t)1 << 16;
  if (nrows < kMinRows || ptr.size() != nrows + 1) return false;
  const size_t kSample = std::min<size_t>(4096, nrows), kMaxSampled = kSample / 4;
  std::vector<uint64_t> sig(nrows);
  ParallelFor(nrows, [&](size_t lo, size_t hi) {
    for (size_t r = lo; r < hi; r++) {
      uint64_t h = 1469598103934665603ull ^ (uint64_t)(ptr[r + 1] - ptr[r]);
      for (int32_t j = ptr[r]; j < ptr[r + 1]; j++) {
        uint64_t bits = 0;
        std::memcpy(&bits, &val[j], sizeof(T));
        h = (h ^ (uint64_t)(uint32_t)(ind[j] - base_of(r))) * 1099511628211ull; h ^= h >> 29;
        h = (h ^ bits) * 1099511628211ull; h ^= h >> 31;
      }
      sig[r] = h;
    }
  });
  {   // unstructured matrices leave here after a look at 4096 evenly spaced rows
    std::vector<uint64_t> smp(kSample);
    for (size_t i = 0; i < kSample; i++) smp[i] = sig[i * (nrows / kSample)];
    std::sort(smp.begin(), smp.end());
    if ((size_t)(std::unique(smp.begin(), smp.end()) - smp.begin()) > kMaxSampled) return false;
  }
  // distinct signatures and the first row of each (per sub-range, merged), numbered in row order; then every row looks its number
  // up and is compared with the first row of its pattern, entry by entry (equal signatures of different rows: the matrix stays CSR)
  std::unordered_map<uint64_t, size_t> first;
  std::mutex merge;
  std::atomic<bool> ok(true);
  ParallelFor(nrows, [&](size_t lo, size_t hi) {
    std::unordered_map<uint64_t, size_t> local;
    for (size_t r = lo; r < hi && ok.load(std::memory_order_relaxed); r++) {
      if (local.emplace(sig[r], r).second && local.size() > kMaxPatterns) ok = false;
    }
    std::lock_guard<std::mutex> g(merge);
    for (const auto& kv : local) { auto it = first.emplace(kv.first, kv.second).first; if (kv.second < it->second) it->second = kv.second; }
  });
  if (!ok || first.size() > kMaxPatterns) return false;
  std::vector<std::pair<size_t, uint64_t>> order;
  order.reserve(first.size());
  for (const auto& kv : first) order.emplace_back(kv.second, kv.first);
  std::sort(order.begin(), order.end());
  std::unordered_map<uint64_t, uint32_t> number;
  std::vector<size_t> rep(order.size());
  out.pptr.assign(1, 0); out.rel.clear(); out.val.clear();
  for (size_t k = 0; k < order.size(); k++) {
    const size_t r = order[k].first;
    number.emplace(order[k].second, (uint32_t)k);
    rep[k] = r;
    for (int32_t j = ptr[r]; j < ptr[r + 1]; j++) { out.rel.push_back(ind[j] - base_of(r)); out.val.push_back(val[j]); }
    out.pptr.push_back((int32_t)out.rel.size());
    if (out.rel.size() > kMaxTable) return false;
  }
  if (out.rel.empty()) return false;                                  // a matrix without entries: nothing to tabulate
  out.ids.assign((nrows + 3) / 4 * 4, 0);
  ParallelFor(nrows, [&](size_t lo, size_t hi) {
    for (size_t r = lo; r < hi; r++) {
      const uint32_t id = number.find(sig[r])->second;
      const size_t q = rep[id];
      const int32_t len = ptr[r + 1] - ptr[r];
      bool same = len == ptr[q + 1] - ptr[q];
      for (int32_t j = 0; same && j < len; j++)
        same = ind[ptr[r] + j] - base_of(r) == ind[ptr[q] + j] - base_of(q) && std::memcmp(&val[ptr[r] + j], &val[ptr[q] + j], sizeof(T)) == 0;
      if (!same) { ok = false; return; }
      out.ids[r] = (uint16_t)id;
    }
  });
  if (!ok) return false;
  out.anchor.clear();
  if (anchored) {
    // an empty row continues the run of the row above it, so that the 4 rows of a lane keep consecutive anchors across it
    out.anchor.assign((nrows + 3) / 4 * 4, 0);
    for (size_t r = 0; r < nrows; r++) out.anchor[r] = ptr[r + 1] > ptr[r] ? ind[ptr[r]] : (r ? out.anchor[r - 1] + 1 : 0);
  }
  return true;
}
}  // namespace
static bool g_stencil_recognition = true;
template <typename T> void BlockSparse<T>::SetStencilRecognition(bool on) { g_stencil_recognition = on; }

/// Is K, entry for entry, spmat_gradient2d(nx, ny, L) -- rows [0, L n): forward differences along x (-1 at the pixel, +1 one column
/// on, nothing in the last column), rows [L n, 2 L n): along y (-1, +1 one row down, nothing in the last row), n = nx ny, label l in
/// columns [l n, (l + 1) n) (spmat_gradient2d.m:7-14)?  ny is read off row 0, n off the first empty row, then every row is checked.
template <typename T>
void BlockSparse<T>::DetectGradient2D() {
  grad_nx_ = grad_ny_ = grad_L_ = 0;
  const std::vector<int32_t>&host_ptr_ = side_[0].host_ptr, &host_ind_ = side_[0].host_ind;
  const std::vector<T>& host_val_ = side_[0].host_val;
  const size_t m = this->nrows(), n = this->ncols();
  if (!g_stencil_recognition || m != 2 * n || n < 4 || host_ptr_.size() != m + 1) return;
  if (host_ptr_[1] - host_ptr_[0] != 2 || host_ind_[0] != 0 || host_val_[0] != (T)-1 || host_val_[1] != (T)1) return;
  const size_t ny = (size_t)host_ind_[1];
  if (ny < 2 || ny >= n) return;
  size_t first_empty = n;
  for (size_t r = 0; r < n; r++) if (host_ptr_[r + 1] == host_ptr_[r]) { first_empty = r; break; }
  const size_t img = first_empty + ny;
  if (first_empty == n || img > n || n % img != 0 || img % ny != 0 || img / ny < 2) return;
  std::atomic<bool> ok(true);
  auto row_is = [&](size_t r, size_t c0, bool two) {
    const int32_t b = host_ptr_[r], e = host_ptr_[r + 1];
    if (!two) return e == b;
    return e - b == 2 && (size_t)host_ind_[b] == c0 && host_val_[b] == (T)-1 && host_val_[b + 1] == (T)1;
  };
  ParallelFor(n, [&](size_t lo, size_t hi) {
    for (size_t q = lo; q < hi && ok.load(std::memory_order_relaxed); q++) {
      const size_t p = q % img;
      const bool dx = p < img - ny, dy = p % ny < ny - 1;
      if (!row_is(q, q, dx) || (dx && (size_t)host_ind_[host_ptr_[q] + 1] != q + ny) ||
          !row_is(n + q, q, dy) || (dy && (size_t)host_ind_[host_ptr_[n + q] + 1] != q + 1)) { ok = false; return; }
    }
  });
  if (!ok) return;
  grad_ny_ = ny; grad_nx_ = img / ny; grad_L_ = n / img;
}

template <typename T> void BlockSparse<T>::SetPatternCompression(bool on) { g_sparse_patterns = on; }
template <typename T> bool BlockSparse<T>::pattern_compression() { return g_sparse_patterns; }

template <typename T>
void BlockSparse<T>::Initialize() {
  for (Side& s : side_) s.pat.on = false;
  DetectGradient2D();
  DetectPointwise();
  for (Side& s : side_) {
    HostRowPatterns<T> h;
    // (offsets from the row number first -- 2 bytes per row; then from the row's first column -- 6 bytes per row, for matrices that map
    // between different geometries: convmtx2 of example_deblurring.m)
    if (!g_sparse_patterns || !(BuildRowPatterns<T>(s.rows, s.host_ptr, s.host_ind, s.host_val, h) || BuildRowPatterns<T>(s.rows, s.host_ptr, s.host_ind, s.host_val, h, true))) continue;
    RowPatterns& p = s.pat;
    p.ids = h.ids; p.pptr = h.pptr; p.rel = h.rel; p.val = h.val;
    p.anchor.clear();
    if (!h.anchor.empty()) p.anchor = h.anchor;
    p.count = h.pptr.size() - 1;
    p.on = true;
  }
  // the CSR arrays of a product that runs from row patterns stay on the host (a 4096^2 gradient: 0.5 GB of upload each)
  for (Side& s : side_) if (!s.pat.on) s.Upload();
}
template <typename T>
bool BlockSparse<T>::describe(BlockDesc& d) const {
  if (nnz_ == 0) return false;
  for (const Side& s : side_) if (!s.pat.on && s.val.size() != nnz_) return false;          // before Initialize()
  d.kind = BlockDesc::kSparse; d.nnz = nnz_;
  auto fill = [](const Side& s, const void*& val, const int32_t*& ptr, const int32_t*& ind, const uint16_t*& ids, const int32_t*& pptr, const int32_t*& rel, const void*& pval,
                 const int32_t*& anchor) {
    if (s.pat.on) { ids = s.pat.ids.data(); pptr = s.pat.pptr.data(); rel = s.pat.rel.data(); pval = s.pat.val.data(); anchor = s.pat.anchor.size() ? s.pat.anchor.data() : nullptr; }
    else { val = s.val.data(); ptr = s.ptr.data(); ind = s.ind.data(); }
  };
  fill(side_[0], d.val, d.ptr, d.ind, d.ids, d.pptr, d.rel, d.pval, d.anchor);
  fill(side_[1], d.val_t, d.ptr_t, d.ind_t, d.ids_t, d.pptr_t, d.rel_t, d.pval_t, d.anchor_t);
  d.pointwise_planes = pointwise_planes_;
  return true;
}
/// K couples the channels of one pixel: nrows x (L nrows), row i = L entries at columns i, i + nrows, ..., i + (L - 1) nrows -- the
/// shape of [diag(Ix) diag(Iy)] (a warp / data-term matrix of a multi-channel model).  The two-launch CG rounds of the ADMM backend
/// (prost_hip_cgls_pixel_round) read such a block as a per-pixel table of L values.
template <typename T>
void BlockSparse<T>::DetectPointwise() {
  pointwise_planes_ = 0;
  const std::vector<int32_t>&host_ptr_ = side_[0].host_ptr, &host_ind_ = side_[0].host_ind;
  const size_t m = this->nrows(), n = this->ncols();
  if (m == 0 || n % m != 0 || host_ptr_.size() != m + 1) return;
  const size_t L = n / m;
  if (L < 1 || L > 4 || nnz_ != L * m) return;
  std::atomic<bool> ok(true);
  ParallelFor(m, [&](size_t lo, size_t hi) {
    for (size_t i = lo; i < hi && ok.load(std::memory_order_relaxed); i++) {
      if ((size_t)host_ptr_[i] != i * L || (size_t)host_ptr_[i + 1] != (i + 1) * L) { ok.store(false); return; }
      for (size_t c = 0; c < L; c++)
        if ((size_t)host_ind_[i * L + c] != i + c * m) { ok.store(false); return; }
    }
  });
  if (ok.load()) pointwise_planes_ = L;
}
template <typename T>
void BlockSparse<T>::Release() {
  for (Side& s : side_) s.Clear();
  for (Side& s : side_) { RowPatterns& p = s.pat; p.on = false; p.ids.clear(); p.pptr.clear(); p.rel.clear(); p.val.clear(); p.anchor.clear(); }
}
template <typename T> T BlockSparse<T>::row_sum(size_t row, T alpha) const { return side_[0].AbsPowSum(row, alpha); }
template <typename T> T BlockSparse<T>::col_sum(size_t col, T alpha) const { return side_[1].AbsPowSum(col, alpha); }
// |v|^alpha: alpha == 1 (the default scaling, both for rows and for columns: 2 - alpha == 1) needs no pow -- pow(x, 1) == x
template <typename T>
static void csr_abs_pow_sums(T* out, const CsrSide<T>& s, T alpha) {
  const std::vector<int32_t>& ptr = s.host_ptr;
  const std::vector<T>& val = s.host_val;
  ParallelFor(s.rows, [&](size_t lo, size_t hi) {
    for (size_t r = lo; r < hi; r++) {
      T sum = 0;
      if (alpha == (T)1) { for (int32_t i = ptr[r]; i < ptr[r + 1]; i++) sum += std::abs(val[i]); }
      else { for (int32_t i = ptr[r]; i < ptr[r + 1]; i++) sum += std::pow(std::abs(val[i]), alpha); }
      out[r] += sum;
    }
  });
}
template <typename T> void BlockSparse<T>::row_sums(T* out, T alpha) const { csr_abs_pow_sums<T>(out, side_[0], alpha); }
template <typename T> void BlockSparse<T>::col_sums(T* out, T alpha) const { csr_abs_pow_sums<T>(out, side_[1], alpha); }
template <typename T>
size_t BlockSparse<T>::gpu_mem_amount() const {
  size_t bytes = 0;
  for (const Side& s : side_) if (!s.pat.on) bytes += nnz_ * (sizeof(int32_t) + sizeof(T)) + (s.rows + 1) * sizeof(int32_t);
  for (const Side& s : side_) bytes += s.pat.ids.size() * sizeof(uint16_t) + (s.pat.pptr.size() + s.pat.rel.size() + s.pat.anchor.size()) * sizeof(int32_t) + s.pat.val.size() * sizeof(T);
  return bytes;
}
template <typename T>
void BlockSparse<T>::PatternProduct(const Side& s, T* r, const T* x, int acc) {
  const RowPatterns& p = s.pat;
  if (p.anchor.size())
    CheckHip(Api<T>::pattern_spmv_anchored(r, x, s.rows, p.ids.data(), p.anchor.data(), p.pptr.data(), p.rel.data(), p.val.data(), (int)p.pptr.size() - 1, (int)p.rel.size(), acc, CurrentStream()), "pattern_spmv_anchored");
  else
    CheckHip(Api<T>::pattern_spmv(r, x, s.rows, p.ids.data(), p.pptr.data(), p.rel.data(), p.val.data(), (int)p.pptr.size() - 1, (int)p.rel.size(), acc, CurrentStream()), "pattern_spmv");
}
template <typename T>
void BlockSparse<T>::Product(T* r, const T* x, bool transpose, bool accumulate) {
  const Side& s = side_[transpose];
  if (!s.pat.on && s.val.size() != nnz_ && nnz_) throw Exception("BlockSparse used before Initialize().");
  if (s.pat.on) { PatternProduct(s, r, x, accumulate ? 1 : 0); return; }
  if (accumulate) CheckHip(Api<T>::csr_spmv_acc(r, x, s.rows, nnz_, s.val.data(), s.ptr.data(), s.ind.data(), CurrentStream()), "csr_spmv_acc");
  else CheckHip(Api<T>::csr_spmv(r, x, s.rows, nnz_, s.val.data(), s.ptr.data(), s.ind.data(), CurrentStream()), "csr_spmv");
}
template class BlockSparse<float>;
template class BlockSparse<double>;

// ---- Kronecker blocks ----
template <typename T>
BlockKronSparse<T>* BlockKronSparse<T>::CreateFromCSC(bool id_first, size_t row, size_t col, size_t diaglength, int m, int n, int nnz,
                                                      const std::vector<T>& val, const std::vector<int32_t>& ptr, const std::vector<int32_t>& ind) {
  BlockKronSparse<T>* b = new BlockKronSparse<T>(row, col, (size_t)m * diaglength, (size_t)n * diaglength);
  b->id_first_ = id_first; b->diaglength_ = diaglength; b->mat_nnz_ = nnz;
  CsrSide<float> &k = b->side_[0], &kt = b->side_[1];
  k.rows = m; kt.rows = n;
  kt.host_ind = ind; kt.host_ptr = ptr; kt.host_val = std::vector<float>(val.begin(), val.end());     // block_sparse_kron_id.cu:77-79
  k.host_ind.resize(nnz); k.host_val.resize(nnz); k.host_ptr.resize(m + 1);
  csr2csc<float>(n, m, nnz, kt.host_val.data(), kt.host_ind.data(), kt.host_ptr.data(), k.host_val.data(), k.host_ind.data(), k.host_ptr.data());
  return b;
}
template <typename T> void BlockKronSparse<T>::Initialize() { for (auto& s : side_) s.Upload(); }
template <typename T> void BlockKronSparse<T>::Release() { for (auto& s : side_) s.Clear(); }
template <typename T>
T BlockKronSparse<T>::row_sum(size_t row, T alpha) const { return side_[0].AbsPowSum(id_first_ ? row % side_[0].rows : row / diaglength_, alpha); }
template <typename T>
T BlockKronSparse<T>::col_sum(size_t col, T alpha) const { return side_[1].AbsPowSum(id_first_ ? col % side_[1].rows : col / diaglength_, alpha); }
template <typename T>
size_t BlockKronSparse<T>::gpu_mem_amount() const {
  size_t bytes = 0;
  for (const auto& s : side_) bytes += (s.host_ind.size() + s.host_ptr.size()) * sizeof(int32_t) + s.host_val.size() * sizeof(T);
  return bytes;
}
template <typename T>
void BlockKronSparse<T>::Product(T* r, const T* x, bool transpose, bool accumulate) {
  const CsrSide<float>& s = side_[transpose];
  const size_t mat_cols = side_[!transpose].rows;
  if (s.ptr.size() != s.host_ptr.size()) throw Exception("BlockKronSparse used before Initialize().");
  if (id_first_) {
    const auto fn = accumulate ? Api<T>::id_kron_sparse_acc : Api<T>::id_kron_sparse;
    CheckHip(fn(r, x, diaglength_, s.rows, mat_cols, s.val.data(), s.ptr.data(), s.ind.data(), CurrentStream()), accumulate ? "id_kron_sparse_acc" : "id_kron_sparse");
  } else {
    const auto fn = accumulate ? Api<T>::sparse_kron_id_acc : Api<T>::sparse_kron_id;
    CheckHip(fn(r, x, diaglength_, s.rows, s.val.data(), s.ptr.data(), s.ind.data(), CurrentStream()), accumulate ? "sparse_kron_id_acc" : "sparse_kron_id");
  }
}
template class BlockKronSparse<float>;
template class BlockKronSparse<double>;

// ---- dense blocks ----
template <typename T>
BlockDense<T>* BlockDense<T>::CreateFromColFirstData(size_t row, size_t col, size_t nrows, size_t ncols, const std::vector<T>& data) {
  if (data.size() != nrows * ncols) throw Exception("BlockDense: the data does not have nrows x ncols entries.");
  BlockDense<T>* b = new BlockDense<T>(row, col, nrows, ncols);
  b->host_data_ = data;
  return b;
}
template <typename T>
void BlockDense<T>::Initialize() {
  data_ = host_data_;
  workspace_.resize(prost_hip_dense_gemv_workspace_bytes(this->nrows(), this->ncols()) / sizeof(double));
}
template <typename T>
void BlockDense<T>::Release() { data_.clear(); workspace_.clear(); }
template <typename T>
T BlockDense<T>::row_sum(size_t row, T alpha) const {                 // block_dense.cu:57-64
  T sum = 0;
  for (size_t c = 0; c < this->ncols(); c++) sum += std::pow(std::abs(host_data_[c * this->nrows() + row]), alpha);
  return sum;
}
template <typename T>
T BlockDense<T>::col_sum(size_t col, T alpha) const {                 // :67-74
  T sum = 0;
  for (size_t r = 0; r < this->nrows(); r++) sum += std::pow(std::abs(host_data_[col * this->nrows() + r]), alpha);
  return sum;
}
template <typename T>
size_t BlockDense<T>::gpu_mem_amount() const {
  return host_data_.size() * sizeof(T) + prost_hip_dense_gemv_workspace_bytes(this->nrows(), this->ncols());
}
template <typename T>
void BlockDense<T>::Product(T* r, const T* x, bool transpose, bool acc) {
  if (data_.size() != host_data_.size()) throw Exception("BlockDense used before Initialize().");
  void* ws = workspace_.empty() ? nullptr : (void*)workspace_.data();
  if (acc) CheckHip(Api<T>::dense_gemv_acc(r, x, this->nrows(), this->ncols(), data_.data(), transpose ? 1 : 0, ws, CurrentStream()), "dense_gemv_acc");
  else CheckHip(Api<T>::dense_gemv(r, x, this->nrows(), this->ncols(), data_.data(), transpose ? 1 : 0, ws, CurrentStream()), "dense_gemv");
}
template class BlockDense<float>;
template class BlockDense<double>;

template <typename T>
BlockKronDense<T>* BlockKronDense<T>::CreateFromColFirstData(bool id_first, size_t diaglength, size_t row, size_t col, size_t nrows, size_t ncols,
                                                             const std::vector<T>& data) {
  if (data.size() != nrows * ncols) throw Exception("BlockKronDense: the data does not have nrows x ncols entries.");
  BlockKronDense<T>* b = new BlockKronDense<T>(row, col, nrows * diaglength, ncols * diaglength);
  b->id_first_ = id_first; b->diaglength_ = diaglength; b->mat_nrows_ = nrows; b->mat_ncols_ = ncols;
  b->host_data_ = data;
  return b;
}
template <typename T>
void BlockKronDense<T>::Initialize() { data_ = host_data_; }
template <typename T>
void BlockKronDense<T>::Release() { data_.clear(); }
template <typename T>
T BlockKronDense<T>::row_sum(size_t row, T alpha) const {             // block_dense_kron_id.cu:100-109, block_id_kron_dense.cu:100-109
  row = id_first_ ? row % mat_nrows_ : row / diaglength_;
  T sum = 0;
  for (size_t i = 0; i < mat_ncols_; i++) sum += std::pow(std::abs(host_data_[i * mat_nrows_ + row]), alpha);
  return sum;
}
template <typename T>
T BlockKronDense<T>::col_sum(size_t col, T alpha) const {             // :112-121
  col = id_first_ ? col % mat_ncols_ : col / diaglength_;
  T sum = 0;
  for (size_t i = 0; i < mat_nrows_; i++) sum += std::pow(std::abs(host_data_[i + col * mat_nrows_]), alpha);
  return sum;
}
template <typename T>
size_t BlockKronDense<T>::gpu_mem_amount() const { return host_data_.size() * sizeof(T); }
template <typename T>
void BlockKronDense<T>::Product(T* r, const T* x, bool transpose, bool acc) {
  if (data_.size() != host_data_.size()) throw Exception("BlockKronDense used before Initialize().");
  auto fn = id_first_ ? (acc ? Api<T>::id_kron_dense_acc : Api<T>::id_kron_dense) : (acc ? Api<T>::dense_kron_id_acc : Api<T>::dense_kron_id);
  CheckHip(fn(r, x, diaglength_, mat_nrows_, mat_ncols_, data_.data(), transpose ? 1 : 0, CurrentStream()), id_first_ ? "id_kron_dense" : "dense_kron_id");
}
template class BlockKronDense<float>;
template class BlockKronDense<double>;

// ---- what the matrix-free blocks below share: refusals, argument checks, tap packing, plane sums ----
namespace {
const double kTwo31 = 2147483648.0;            // 2^31: planes are indexed with 32 bits
const double kTwo53 = 9007199254740992.0;      // 2^53: counts and sizes arrive as doubles

/// throws Exception("<block>: <every further argument, streamed>")
template <class... A>
[[noreturn]] void Refuse(const char* block, const A&... text) {
  std::stringstream ss;
  ss << block << ": ";
  (ss << ... << text);
  throw Exception(ss.str());
}
/// how a refusal that depends on the rounding to T ends
template <typename T> const char* PrecisionStop() { return std::is_same<T, float>::value ? " in single precision." : "."; }

typedef std::pair<const char*, double> Named;
/// every value is an integer from 1 to `top`, else "<lead><name> = <value><tail>"
void CheckIntegers(const char* block, std::initializer_list<Named> values, double top, const std::string& tail, const char* lead = "") {
  for (const Named& v : values)
    if (!(v.second >= 1) || v.second != std::floor(v.second) || v.second > top) Refuse(block, lead, v.first, " = ", v.second, tail);
}
void CheckBelowTwo31(const char* block, std::initializer_list<Named> values) { CheckIntegers(block, values, kTwo31 - 1, " has to be a positive integer below 2^31."); }
/// `what`: "the window holds", "the angles hold", ..
void CheckFinite(const char* block, const std::vector<double>& values, const char* what) {
  for (double v : values)
    if (!std::isfinite(v)) Refuse(block, what, " a non-finite value.");
}
/// a declared size (none was declared if both are negative) is rows x cols; `formula` is how the message writes that product
void CheckDeclaredSize(const char* block, double declared_rows, double declared_cols, double rows, double cols, const char* formula, bool square = false) {
  if (!(declared_rows >= 0 || declared_cols >= 0) || (declared_rows == rows && declared_cols == cols)) return;
  if (square) Refuse(block, "the declared size ", declared_rows, " x ", declared_cols, " is not ", formula, " = ", rows, " square.");
  Refuse(block, "the declared size ", declared_rows, " x ", declared_cols, " is not ", formula, " = ", rows, " x ", cols, ".");
}

// the two convolution blocks: the same window, shapes and tap records
void CheckWindow(const char* block, const std::vector<double>& kernel, size_t ky, size_t kx) {
  if (ky == 0 || kx == 0 || kernel.size() != ky * kx) Refuse(block, "the window is empty.");
  if (ky > (size_t)conv2d::kMaxWindow || kx > (size_t)conv2d::kMaxWindow)
    Refuse(block, "the window is ", ky, " x ", kx, ", windows up to ", conv2d::kMaxWindow, " x ", conv2d::kMaxWindow, " are supported.");
  CheckFinite(block, kernel, "the window holds");
}
int ParseShape(const char* block, const std::string& shape) {
  if (shape == "full") return conv2d::kFull;
  if (shape == "same") return conv2d::kSame;
  if (shape == "valid") return conv2d::kValid;
  Refuse(block, "unknown shape '", shape, "' (full, same or valid).");
}
/// the size (my, mx) and crop offset (oy, ox) of the un-decimated convolution
void ConvSize(const char* block, int which, double ny, double nx, size_t ky, size_t kx, long& my, long& mx, long& oy, long& ox) {
  if (!conv2d::OutputSize(which, (long)ny, (long)nx, (long)ky, (long)kx, my, mx, oy, ox))
    Refuse(block, "the window (", ky, " x ", kx, ") is larger than the image (", ny, " x ", nx, "): the valid part is empty.");
}
void CheckPlanes(const char* block, double image, double output) {
  if (image >= kTwo31 || output >= kTwo31) Refuse(block, "a plane of ", std::max(image, output), " elements; it has to stay below 2^31.");
}
/// the tap records as the words that are uploaded, field by field: the padding of the fp64 record stays zero
template <typename T>
std::vector<int32_t> PackTaps(const std::vector<conv2d::Tap<T>>& taps) {
  static_assert(sizeof(conv2d::Tap<T>) % sizeof(int32_t) == 0, "tap record in words");
  const size_t words = sizeof(conv2d::Tap<T>) / sizeof(int32_t);
  std::vector<int32_t> packed(taps.size() * words, 0);
  for (size_t t = 0; t < taps.size(); t++) {
    std::memcpy(&packed[t * words], &taps[t].offset, sizeof(int32_t));
    std::memcpy(reinterpret_cast<char*>(&packed[t * words]) + offsetof(conv2d::Tap<T>, value), &taps[t].value, sizeof(T));
  }
  return packed;
}

/// pixel p of a column-major plane of height ny
struct Pixel {
  int y, x;
  Pixel(size_t p, int ny) : y((int)(p % (size_t)ny)), x((int)(p / (size_t)ny)) {}
};
/// the geometry record of one direction
template <class G> G Directed(G g, bool transpose) { g.transpose = transpose ? 1 : 0; return g; }
/// out[c n + i] += (T)fn(i) for i < n, c < planes: one plane is computed once, on `threads` host threads, and added to every plane
template <typename T, class F>
void AddPlaneSums(T* out, size_t n, size_t planes, F fn, size_t threads = 1) {
  std::vector<T> one(n);
  const size_t parts = std::max<size_t>(std::min(n, threads), 1);
  std::vector<std::thread> th;
  std::exception_ptr err = nullptr;
  std::mutex mu;
  auto run = [&](size_t k) {
    try { for (size_t i = n * k / parts; i < n * (k + 1) / parts; i++) one[i] = (T)fn(i); }
    catch (...) { std::lock_guard<std::mutex> lock(mu); err = std::current_exception(); }
  };
  for (size_t k = 1; k < parts; k++) th.emplace_back(run, k);
  run(0);
  for (auto& t : th) t.join();
  if (err) std::rethrow_exception(err);
  for (size_t c = 0; c < planes; c++)
    for (size_t i = 0; i < n; i++) out[c * n + i] += one[i];
}
/// out[c n + i] += fn(c) for i < n, c < planes: one constant per plane
template <typename T, class F>
void AddPlaneConstants(T* out, size_t n, size_t planes, F fn) {
  for (size_t c = 0; c < planes; c++) {
    const T v = fn(c);
    for (size_t i = 0; i < n; i++) out[c * n + i] += v;
  }
}
}  // namespace

// ---- the coupling of the sublabel-accurate data term ----
template <typename T>
BlockDatatermSublabel<T>* BlockDatatermSublabel<T>::Create(size_t row, size_t col, double nx, double ny, double L, double left, double right,
                                                           double declared_rows, double declared_cols) {
  const char* kName = "BlockDatatermSublabel";
  if (!(L >= 2) || L != std::floor(L) || L > kTwo53) Refuse(kName, "L = ", L, " labels, at least 2 are needed.");
  if (!(nx >= 1) || !(ny >= 1) || nx != std::floor(nx) || ny != std::floor(ny) || nx * ny * (L - 1) > kTwo53 / 4) Refuse(kName, "nx = ", nx, " and ny = ", ny, " have to be at least 1.");
  if (!std::isfinite(left) || !std::isfinite(right)) Refuse(kName, "the bounds left = ", left, " and right = ", right, " have to be finite.");
  if (!(left < right)) Refuse(kName, "left = ", left, " has to be below right = ", right, ".");
  const double size = 2 * nx * ny * (L - 1);
  CheckDeclaredSize(kName, declared_rows, declared_cols, size, size, "2 nx ny (L - 1)", true);
  return new BlockDatatermSublabel<T>(row, col, (size_t)nx * (size_t)ny, (size_t)L, left, right);
}
template <typename T>
BlockDatatermSublabel<T>::BlockDatatermSublabel(size_t row, size_t col, size_t npixels, size_t L, double left, double right)
    : ProductBlock<T>(row, col, 2 * npixels * (L - 1), 2 * npixels * (L - 1)), npixels_(npixels), L_(L), gamma_(L - 1) {
  dataterm_sublabel::Labels<T>(L, left, right, delta_, gamma_.data());
}
template <typename T>
void BlockDatatermSublabel<T>::Initialize() { d_gamma_ = gamma_; }
template <typename T>
void BlockDatatermSublabel<T>::Release() { d_gamma_.clear(); }
template <typename T>
T BlockDatatermSublabel<T>::row_sum(size_t row, T alpha) const {
  const size_t k = L_ - 1, i = (row / npixels_) % k;
  return row < npixels_ * k ? dataterm_sublabel::RowSumR<T>(i, k, delta_, gamma_[i], alpha) : dataterm_sublabel::RowSumS<T>(alpha);
}
template <typename T>
T BlockDatatermSublabel<T>::col_sum(size_t col, T alpha) const {
  const size_t k = L_ - 1, i = (col / npixels_) % k;
  return col < npixels_ * k ? dataterm_sublabel::ColSumU<T>(delta_, alpha) : dataterm_sublabel::ColSumW<T>(i, delta_, gamma_[i], alpha);
}
template <typename T>
void BlockDatatermSublabel<T>::row_sums(T* out, T alpha) const {
  AddPlaneConstants(out, npixels_, 2 * (L_ - 1), [&](size_t i) { return row_sum(i * npixels_, alpha); });
}
template <typename T>
void BlockDatatermSublabel<T>::col_sums(T* out, T alpha) const {
  AddPlaneConstants(out, npixels_, 2 * (L_ - 1), [&](size_t i) { return col_sum(i * npixels_, alpha); });
}
template <typename T>
void BlockDatatermSublabel<T>::Product(T* r, const T* x, bool transpose, bool acc) {
  if (d_gamma_.size() != gamma_.size()) throw Exception("BlockDatatermSublabel used before Initialize().");
  CheckHip(Api<T>::linop_dataterm_sublabel(r, x, npixels_, L_, d_gamma_.data(), (double)delta_, transpose ? 1 : 0, acc ? 1 : 0, CurrentStream()),
           "linop_dataterm_sublabel");
}
template class BlockDatatermSublabel<float>;
template class BlockDatatermSublabel<double>;

// ---- one window at every pixel: 2-D convolution without a matrix ----
template <typename T>
BlockConv2D<T>* BlockConv2D<T>::Create(size_t row, size_t col, double nx, double ny, double L, const std::vector<double>& kernel, size_t ky, size_t kx,
                                       const std::string& shape, double declared_rows, double declared_cols) {
  const char* kName = "BlockConv2D";
  CheckBelowTwo31(kName, {{"nx", nx}, {"ny", ny}, {"L", L}});
  CheckWindow(kName, kernel, ky, kx);
  const int which = ParseShape(kName, shape);
  long my = 0, mx = 0, oy = 0, ox = 0;
  ConvSize(kName, which, ny, nx, ky, kx, my, mx, oy, ox);
  CheckPlanes(kName, nx * ny, (double)my * (double)mx);
  const double rows = L * (double)my * (double)mx, cols = L * ny * nx;
  CheckDeclaredSize(kName, declared_rows, declared_cols, rows, cols, "L my mx x L ny nx");
  std::unique_ptr<BlockConv2D<T>> b(new BlockConv2D<T>(row, col, (size_t)rows, (size_t)cols));
  for (int dir = 0; dir < 2; dir++) {
    b->geometry_[dir] = conv2d::MakeGeometry(which, (long)ny, (long)nx, (long)ky, (long)kx, (long)L, dir == 1);
    b->window_[dir] = conv2d::Window<T>(kernel.data(), (long)ky, (long)kx, dir == 1);
    const std::vector<conv2d::Tap<T>> taps = conv2d::CompactTaps<T>(b->window_[dir], (long)ky, (long)kx);
    b->words_[dir] = PackTaps<T>(taps);
    b->ntaps_ = taps.size();
  }
  if (b->ntaps_ == 0) Refuse(kName, "the window has no non-zero tap", PrecisionStop<T>());
  return b.release();
}
template <typename T>
void BlockConv2D<T>::Initialize() { for (int dir = 0; dir < 2; dir++) d_taps_[dir] = words_[dir]; }
template <typename T>
void BlockConv2D<T>::Release() { for (int dir = 0; dir < 2; dir++) d_taps_[dir].clear(); }
template <typename T>
T BlockConv2D<T>::row_sum(size_t row, T alpha) const {
  const conv2d::Geometry& g = geometry_[0];
  const Pixel at(row % ((size_t)g.dny * (size_t)g.dnx), g.dny);
  return (T)conv2d::SumAt<T>(g, window_[0], (double)alpha, at.y, at.x);
}
template <typename T>
T BlockConv2D<T>::col_sum(size_t col, T alpha) const {
  const conv2d::Geometry& g = geometry_[1];
  const Pixel at(col % ((size_t)g.dny * (size_t)g.dnx), g.dny);
  return (T)conv2d::SumAt<T>(g, window_[1], (double)alpha, at.y, at.x);
}
template <typename T>
void BlockConv2D<T>::row_sums(T* out, T alpha) const { conv2d::RowSums<T>(geometry_[0], window_[0], (double)alpha, out); }
template <typename T>
void BlockConv2D<T>::col_sums(T* out, T alpha) const { conv2d::RowSums<T>(geometry_[1], window_[1], (double)alpha, out); }
template <typename T>
void BlockConv2D<T>::Product(T* r, const T* x, bool transpose, bool acc) {
  const int dir = transpose ? 1 : 0;
  if (d_taps_[dir].size() != words_[dir].size()) throw Exception("BlockConv2D used before Initialize().");
  typedef typename std::conditional<std::is_same<T, float>::value, prost_hip_conv2d_tap_f32, prost_hip_conv2d_tap_f64>::type Record;
  static_assert(sizeof(Record) == sizeof(conv2d::Tap<T>) && sizeof(prost_hip_conv2d_geometry) == sizeof(conv2d::Geometry), "records of prost_hip.h");
  CheckHip(Api<T>::conv2d(reinterpret_cast<const prost_hip_conv2d_geometry*>(&geometry_[dir]), reinterpret_cast<const Record*>(d_taps_[dir].data()), ntaps_, r, x,
                          acc ? 1 : 0, CurrentStream()),
           "conv2d");
}
template class BlockConv2D<float>;
template class BlockConv2D<double>;

// ---- blur and decimate: strided 2-D convolution without a matrix ----
template <typename T>
BlockConv2DStrided<T>* BlockConv2DStrided<T>::Create(size_t row, size_t col, double nx, double ny, double L, const std::vector<double>& kernel, size_t ky, size_t kx,
                                                     const std::string& shape, double sy, double sx, double py, double px, double declared_rows,
                                                     double declared_cols) {
  namespace c2s = conv2d_strided;
  const char* kName = "BlockConv2DStrided";
  const double kMaxSide = kTwo31 - 1024 - conv2d::kMaxWindow;      // sides leave room for a tile's halo
  CheckBelowTwo31(kName, {{"nx", nx}, {"ny", ny}, {"L", L}});
  CheckWindow(kName, kernel, ky, kx);
  const int which = ParseShape(kName, shape);
  CheckIntegers(kName, {{"sy", sy}, {"sx", sx}}, c2s::kMaxStride, " has to be an integer from 1 to " + std::to_string(c2s::kMaxStride) + ".", "the stride ");
  long cy = 0, cx = 0, oy = 0, ox = 0;
  ConvSize(kName, which, ny, nx, ky, kx, cy, cx, oy, ox);
  for (const auto& v : {std::make_pair(Named("py", py), std::min((long)sy, cy)), std::make_pair(Named("px", px), std::min((long)sx, cx))})
    if (!(v.first.second >= 0) || v.first.second != std::floor(v.first.second) || v.first.second >= (double)v.second)
      Refuse(kName, "the phase ", v.first.first, " = ", v.first.second, " has to be an integer from 0 to ", v.second - 1, " (below the stride and the size of the convolution).");
  long my = 0, mx = 0;
  c2s::OutputSize(which, (long)ny, (long)nx, (long)ky, (long)kx, (long)sy, (long)sx, (long)py, (long)px, my, mx, oy, ox);
  CheckPlanes(kName, nx * ny, (double)my * (double)mx);
  if (std::max(nx, ny) >= kMaxSide) Refuse(kName, "a side of ", std::max(nx, ny), " pixels; it has to stay below 2^31 - 1055.");
  const double rows = L * (double)my * (double)mx, cols = L * ny * nx;
  CheckDeclaredSize(kName, declared_rows, declared_cols, rows, cols, "L my mx x L ny nx");
  std::unique_ptr<BlockConv2DStrided<T>> b(new BlockConv2DStrided<T>(row, col, (size_t)rows, (size_t)cols));
  b->window_ = c2s::Window<T>(kernel.data(), (long)ky, (long)kx);
  const int tile = c2s::PickTile(sizeof(T), (int)sy, (int)sx, (int)ky, (int)kx);
  if (tile < 0) Refuse(kName, "no tile of the table fits the window and the stride.");
  for (int dir = 0; dir < 2; dir++) {
    b->geometry_[dir] = c2s::MakeGeometry(which, (long)ny, (long)nx, (long)ky, (long)kx, (long)sy, (long)sx, (long)py, (long)px, (long)L, dir == 1);
    const std::vector<conv2d::Tap<T>> taps = c2s::CompactTaps<T>(b->geometry_[dir], b->window_, tile);
    b->words_[dir] = PackTaps<T>(taps);
    b->ntaps_ = taps.size();
  }
  if (b->ntaps_ == 0) Refuse(kName, "the window has no non-zero tap", PrecisionStop<T>());
  return b.release();
}
template <typename T>
void BlockConv2DStrided<T>::Initialize() { for (int dir = 0; dir < 2; dir++) d_taps_[dir] = words_[dir]; }
template <typename T>
void BlockConv2DStrided<T>::Release() { for (int dir = 0; dir < 2; dir++) d_taps_[dir].clear(); }
template <typename T>
T BlockConv2DStrided<T>::row_sum(size_t row, T alpha) const {
  const conv2d_strided::Geometry& g = geometry_[0];
  const Pixel at(row % ((size_t)g.my * (size_t)g.mx), g.my);
  return (T)conv2d_strided::SumAt<T>(g, window_, (double)alpha, false, at.y, at.x);
}
template <typename T>
T BlockConv2DStrided<T>::col_sum(size_t col, T alpha) const {
  const conv2d_strided::Geometry& g = geometry_[0];
  const Pixel at(col % ((size_t)g.ny * (size_t)g.nx), g.ny);
  return (T)conv2d_strided::SumAt<T>(g, window_, (double)alpha, true, at.y, at.x);
}
template <typename T>
void BlockConv2DStrided<T>::row_sums(T* out, T alpha) const { conv2d_strided::Sums<T>(geometry_[0], window_, (double)alpha, false, out); }
template <typename T>
void BlockConv2DStrided<T>::col_sums(T* out, T alpha) const { conv2d_strided::Sums<T>(geometry_[0], window_, (double)alpha, true, out); }
template <typename T>
void BlockConv2DStrided<T>::Product(T* r, const T* x, bool transpose, bool acc) {
  const int dir = transpose ? 1 : 0;
  if (d_taps_[dir].size() != words_[dir].size()) throw Exception("BlockConv2DStrided used before Initialize().");
  typedef typename std::conditional<std::is_same<T, float>::value, prost_hip_conv2d_tap_f32, prost_hip_conv2d_tap_f64>::type Record;
  static_assert(sizeof(Record) == sizeof(conv2d::Tap<T>) && sizeof(prost_hip_conv2d_strided_geometry) == sizeof(conv2d_strided::Geometry), "records of prost_hip.h");
  CheckHip(Api<T>::conv2d_strided(reinterpret_cast<const prost_hip_conv2d_strided_geometry*>(&geometry_[dir]), reinterpret_cast<const Record*>(d_taps_[dir].data()),
                                  ntaps_, r, x, acc ? 1 : 0, CurrentStream()),
           "conv2d_strided");
}
template class BlockConv2DStrided<float>;
template class BlockConv2DStrided<double>;

// ---- the parallel-beam projector of tomography, without a matrix ----
template <typename T>
BlockRadon2D<T>* BlockRadon2D<T>::Create(size_t row, size_t col, double nx, double ny, double L, const std::vector<double>& angles, double ndet, double spacing, double shift,
                                         double declared_rows, double declared_cols) {
  namespace r2d = radon2d;
  const char* kName = "BlockRadon2D";
  CheckIntegers(kName, {{"nx", nx}, {"ny", ny}}, r2d::kMaxSide, " has to be an integer from 1 to " + std::to_string(r2d::kMaxSide) + ".");
  CheckBelowTwo31(kName, {{"L", L}});
  if (angles.empty()) Refuse(kName, "the angles are empty.");
  if (angles.size() > (size_t)r2d::kMaxAngles) Refuse(kName, angles.size(), " angles, up to ", r2d::kMaxAngles, " are supported.");
  CheckFinite(kName, angles, "the angles hold");
  if (!(spacing >= 0.5 && spacing <= 8)) Refuse(kName, "spacing = ", spacing, " has to be from 0.5 to 8.");
  if (!std::isfinite(shift)) Refuse(kName, "shift = ", shift, " has to be finite.");
  CheckIntegers(kName, {{"ndet", ndet}}, (double)r2d::kMaxBins, " has to be a positive integer below 2^31 - 1024.");
  const double na = (double)angles.size();
  if (ndet * na >= kTwo31) Refuse(kName, "a sinogram of ", ndet * na, " elements; it has to stay below 2^31.");
  const double rows = L * na * ndet, cols = L * ny * nx;
  CheckDeclaredSize(kName, declared_rows, declared_cols, rows, cols, "L na ndet x L ny nx");
  std::unique_ptr<BlockRadon2D<T>> b(new BlockRadon2D<T>(row, col, (size_t)rows, (size_t)cols));
  b->geometry_ = r2d::MakeGeometry((long)ny, (long)nx, (long)L, (long)ndet, (long)angles.size(), spacing, false);
  b->table_ = r2d::MakeTable<T>((long)ny, (long)nx, (long)ndet, spacing, shift, angles);
  for (T v : b->table_)
    if (!std::isfinite(v)) Refuse(kName, "the table of the angles is not finite", PrecisionStop<T>());
  return b.release();
}
template <typename T>
void BlockRadon2D<T>::Initialize() { d_table_ = table_; }
template <typename T>
void BlockRadon2D<T>::Release() { d_table_.clear(); }
template <typename T>
T BlockRadon2D<T>::row_sum(size_t row, T alpha) const {
  const radon2d::Geometry& g = geometry_;
  const Pixel bin(row % ((size_t)g.ndet * (size_t)g.na), g.ndet);      // bin d of angle a at d + a ndet
  return (T)radon2d::RowSum<T>(table_.data(), g, (double)alpha, bin.x, bin.y);
}
template <typename T>
T BlockRadon2D<T>::col_sum(size_t col, T alpha) const {
  const radon2d::Geometry& g = geometry_;
  const Pixel at(col % ((size_t)g.ny * (size_t)g.nx), g.ny);
  return (T)radon2d::ColSum<T>(table_.data(), g, (double)alpha, at.y, at.x);
}
// the sums of one plane are enumerated on several host threads: a ray costs max(nx, ny) steps, a pixel na (2 m + 2)
template <typename T>
void BlockRadon2D<T>::row_sums(T* out, T alpha) const {
  const radon2d::Geometry& g = geometry_;
  const size_t n = (size_t)g.ndet * (size_t)g.na;
  AddPlaneSums(out, n, (size_t)g.planes, [&](size_t p) { return row_sum(p, alpha); }, ParallelChunks(n * (size_t)std::max(g.nx, g.ny)));
}
template <typename T>
void BlockRadon2D<T>::col_sums(T* out, T alpha) const {
  const radon2d::Geometry& g = geometry_;
  const size_t n = (size_t)g.ny * (size_t)g.nx;
  AddPlaneSums(out, n, (size_t)g.planes, [&](size_t p) { return col_sum(p, alpha); }, ParallelChunks(n * (size_t)g.na * (size_t)(2 * g.m + 2)));
}
template <typename T>
void BlockRadon2D<T>::Product(T* r, const T* x, bool transpose, bool acc) {
  if (d_table_.size() != table_.size()) throw Exception("BlockRadon2D used before Initialize().");
  static_assert(sizeof(prost_hip_radon2d_geometry) == sizeof(radon2d::Geometry), "records of prost_hip.h");
  const radon2d::Geometry g = Directed(geometry_, transpose);
  CheckHip(Api<T>::radon2d(reinterpret_cast<const prost_hip_radon2d_geometry*>(&g), d_table_.data(), r, x, acc ? 1 : 0, CurrentStream()), "radon2d");
}
template class BlockRadon2D<float>;
template class BlockRadon2D<double>;

// ---- the fan-beam projector of tomography, without a matrix ----
template <typename T>
BlockFanbeam2D<T>* BlockFanbeam2D<T>::Create(size_t row, size_t col, double nx, double ny, double L, const std::vector<double>& angles, double source_distance,
                                             double detector_distance, double ndet, double spacing, double shift, const std::string& detector, double declared_rows,
                                             double declared_cols) {
  namespace f2d = fanbeam2d;
  const char* kName = "BlockFanbeam2D";
  CheckIntegers(kName, {{"nx", nx}, {"ny", ny}}, f2d::kMaxSide, " has to be an integer from 1 to " + std::to_string(f2d::kMaxSide) + ".");
  CheckBelowTwo31(kName, {{"L", L}});
  if (angles.empty()) Refuse(kName, "the angles are empty.");
  if (angles.size() > (size_t)f2d::kMaxViews) Refuse(kName, angles.size(), " views, up to ", f2d::kMaxViews, " are supported.");
  CheckFinite(kName, angles, "the angles hold");
  if (detector != "flat" && detector != "curved") Refuse(kName, "unknown detector '", detector, "' (flat or curved).");
  if (!(spacing >= 0.5 && spacing <= 8)) Refuse(kName, "spacing = ", spacing, " has to be from 0.5 to 8.");
  if (!std::isfinite(shift)) Refuse(kName, "shift = ", shift, " has to be finite.");
  if (!(source_distance > 0) || !std::isfinite(source_distance)) Refuse(kName, "source_distance = ", source_distance, " has to be positive and finite.");
  if (!(detector_distance > 0) || !std::isfinite(detector_distance)) Refuse(kName, "detector_distance = ", detector_distance, " has to be positive and finite.");
  CheckIntegers(kName, {{"ndet", ndet}}, (double)f2d::kMaxBins, " has to be a positive integer below 2^31 - 1024.");
  const double na = (double)angles.size();
  if (ndet * na >= kTwo31) Refuse(kName, "a sinogram of ", ndet * na, " elements; it has to stay below 2^31.");
  const double rows = L * na * ndet, cols = L * ny * nx;
  CheckDeclaredSize(kName, declared_rows, declared_cols, rows, cols, "L na ndet x L ny nx");
  const f2d::Scanner s = {(long)ny, (long)nx, (long)ndet, source_distance, detector_distance, spacing, shift, detector == "curved"};
  const double closest = f2d::HalfDiagonal(s.nx, s.ny) + 1;
  if (!(source_distance >= closest))
    Refuse(kName, "source_distance = ", source_distance, " puts the source inside the image's circumscribed circle or less than a pixel off it; it has to be at least ", closest, ".");
  const double fan = f2d::MaxFanAngle(s) * (180 / 3.14159265358979323846);
  if (!(fan <= f2d::kMaxFanDegrees)) Refuse(kName, "the outermost ray is ", fan, " degrees off the central ray; half fans up to ", f2d::kMaxFanDegrees, " degrees are supported.");
  const double margin = f2d::MarginOf(s);
  if (!(margin <= f2d::kMaxMargin))
    Refuse(kName, "the candidate window of the adjoint needs a margin of ", margin, " bins, up to ", f2d::kMaxMargin,
           " are supported (a source farther away, a detector nearer to it or a larger spacing).");
  if (!(f2d::Slack<T>(s) <= f2d::kSlack)) Refuse(kName, "source_distance = ", source_distance, " is too far for the candidate window of the adjoint", PrecisionStop<T>());
  std::unique_ptr<BlockFanbeam2D<T>> b(new BlockFanbeam2D<T>(row, col, (size_t)rows, (size_t)cols));
  b->geometry_ = f2d::MakeGeometry(s, (long)L, (long)angles.size(), false);
  b->table_ = f2d::MakeTable<T>(s, angles);
  for (T v : b->table_)
    if (!std::isfinite(v)) Refuse(kName, "the tables are not finite", PrecisionStop<T>());
  return b.release();
}
template <typename T>
void BlockFanbeam2D<T>::Initialize() { d_table_ = table_; }
template <typename T>
void BlockFanbeam2D<T>::Release() { d_table_.clear(); }
template <typename T>
T BlockFanbeam2D<T>::row_sum(size_t row, T alpha) const {
  const fanbeam2d::Geometry& g = geometry_;
  const Pixel bin(row % ((size_t)g.ndet * (size_t)g.na), g.ndet);      // bin d of view a at d + a ndet
  return (T)fanbeam2d::RowSum<T>(table_.data(), g, (double)alpha, bin.x, bin.y);
}
template <typename T>
T BlockFanbeam2D<T>::col_sum(size_t col, T alpha) const {
  const fanbeam2d::Geometry& g = geometry_;
  const Pixel at(col % ((size_t)g.ny * (size_t)g.nx), g.ny);
  return (T)fanbeam2d::ColSum<T>(table_.data(), g, (double)alpha, at.y, at.x);
}
// the sums of one plane are enumerated on several host threads: a ray costs max(nx, ny) steps, a pixel na (2 m + 2) prologues
template <typename T>
void BlockFanbeam2D<T>::row_sums(T* out, T alpha) const {
  const fanbeam2d::Geometry& g = geometry_;
  const size_t n = (size_t)g.ndet * (size_t)g.na;
  AddPlaneSums(out, n, (size_t)g.planes, [&](size_t p) { return row_sum(p, alpha); }, ParallelChunks(n * (size_t)std::max(g.nx, g.ny)));
}
template <typename T>
void BlockFanbeam2D<T>::col_sums(T* out, T alpha) const {
  const fanbeam2d::Geometry& g = geometry_;
  const size_t n = (size_t)g.ny * (size_t)g.nx;
  AddPlaneSums(out, n, (size_t)g.planes, [&](size_t p) { return col_sum(p, alpha); }, ParallelChunks(n * (size_t)g.na * (size_t)(2 * g.m + 2) * 4));
}
template <typename T>
void BlockFanbeam2D<T>::Product(T* r, const T* x, bool transpose, bool acc) {
  if (d_table_.size() != table_.size()) throw Exception("BlockFanbeam2D used before Initialize().");
  static_assert(sizeof(prost_hip_fanbeam2d_geometry) == sizeof(fanbeam2d::Geometry), "records of prost_hip.h");
  const fanbeam2d::Geometry g = Directed(geometry_, transpose);
  CheckHip(Api<T>::fanbeam2d(reinterpret_cast<const prost_hip_fanbeam2d_geometry*>(&g), d_table_.data(), r, x, acc ? 1 : 0, CurrentStream()), "fanbeam2d");
}
template class BlockFanbeam2D<float>;
template class BlockFanbeam2D<double>;

// ---- bilinear resampling at arbitrary positions, without a matrix ----
template <typename T>
BlockSample2D<T>* BlockSample2D<T>::Create(size_t row, size_t col, double nx, double ny, double L, const std::vector<double>& x, const std::vector<double>& y,
                                           double declared_rows, double declared_cols) {
  namespace s2d = sample2d;
  const char* kName = "BlockSample2D";
  CheckIntegers(kName, {{"nx", nx}, {"ny", ny}}, s2d::kMaxSide, " has to be an integer from 1 to " + std::to_string(s2d::kMaxSide) + ".");
  CheckBelowTwo31(kName, {{"L", L}});
  if (x.size() != y.size()) Refuse(kName, x.size(), " x positions and ", y.size(), " y positions.");
  if (x.empty()) Refuse(kName, "the positions are empty.");
  const double m = (double)x.size();
  if (m >= kTwo31 || L * m >= kTwo31) Refuse(kName, "M = ", m, " samples on L = ", L, " planes; M and L M have to stay below 2^31.");
  CheckFinite(kName, x, "the positions hold");
  CheckFinite(kName, y, "the positions hold");
  const double rows = L * m, cols = L * ny * nx;
  CheckDeclaredSize(kName, declared_rows, declared_cols, rows, cols, "L M x L ny nx");
  std::unique_ptr<BlockSample2D<T>> b(new BlockSample2D<T>(row, col, (size_t)rows, (size_t)cols));
  b->geometry_ = s2d::MakeGeometry((long)ny, (long)nx, (long)x.size(), (long)L, false);
  b->pos_x_.assign(x.begin(), x.end());            // rounded once to T
  b->pos_y_.assign(y.begin(), y.end());
  s2d::MakeBuckets<T>(b->pos_x_.data(), b->pos_y_.data(), x.size(), (int)ny, (int)nx, b->order_, b->cell_start_);
  return b.release();
}
template <typename T>
void BlockSample2D<T>::Initialize() { d_pos_x_ = pos_x_; d_pos_y_ = pos_y_; d_order_ = order_; d_cell_start_ = cell_start_; }
template <typename T>
void BlockSample2D<T>::Release() { d_pos_x_.clear(); d_pos_y_.clear(); d_order_.clear(); d_cell_start_.clear(); }
template <typename T>
T BlockSample2D<T>::row_sum(size_t row, T alpha) const {
  return (T)sample2d::RowSum<T>(pos_x_.data(), pos_y_.data(), geometry_, (double)alpha, row % (size_t)geometry_.m);
}
template <typename T>
T BlockSample2D<T>::col_sum(size_t col, T alpha) const {
  const sample2d::Geometry& g = geometry_;
  const Pixel at(col % ((size_t)g.ny * (size_t)g.nx), g.ny);
  return (T)sample2d::ColSum<T>(pos_x_.data(), pos_y_.data(), order_.data(), cell_start_.data(), g, (double)alpha, at.y, at.x);
}
template <typename T>
void BlockSample2D<T>::row_sums(T* out, T alpha) const {
  AddPlaneSums(out, (size_t)geometry_.m, (size_t)geometry_.planes, [&](size_t i) { return row_sum(i, alpha); });
}
template <typename T>
void BlockSample2D<T>::col_sums(T* out, T alpha) const {
  AddPlaneSums(out, (size_t)geometry_.ny * (size_t)geometry_.nx, (size_t)geometry_.planes, [&](size_t p) { return col_sum(p, alpha); });
}
template <typename T>
void BlockSample2D<T>::Product(T* r, const T* x, bool transpose, bool acc) {
  if (d_pos_x_.size() != pos_x_.size() || d_cell_start_.size() != cell_start_.size()) throw Exception("BlockSample2D used before Initialize().");
  static_assert(sizeof(prost_hip_sample2d_geometry) == sizeof(sample2d::Geometry), "records of prost_hip.h");
  const sample2d::Geometry g = Directed(geometry_, transpose);
  CheckHip(Api<T>::sample2d(reinterpret_cast<const prost_hip_sample2d_geometry*>(&g), d_pos_x_.data(), d_pos_y_.data(), d_order_.data(), d_cell_start_.data(), r, x,
                            acc ? 1 : 0, CurrentStream()),
           "sample2d");
}
template class BlockSample2D<float>;
template class BlockSample2D<double>;

// ---- the unitary 2-D Fourier transform, without a matrix ----
template <typename T>
BlockFFT2D<T>* BlockFFT2D<T>::Create(size_t row, size_t col, double nx, double ny, double L, double declared_rows, double declared_cols) {
  const char* kName = "BlockFFT2D";
  for (const Named& v : {Named("nx", nx), Named("ny", ny)})
    if (!(v.second >= 1) || v.second != std::floor(v.second) || v.second > fft2d::kMaxSide || !fft2d::IsSide((long)v.second))
      Refuse(kName, v.first, " = ", v.second, " has to be a power of two from 1 to ", fft2d::kMaxSide, ".");
  CheckBelowTwo31(kName, {{"L", L}});
  const double size = 2 * L * ny * nx;
  if (size >= kTwo31) Refuse(kName, "L = ", L, " images of ", nx, " x ", ny, "; 2 L nx ny has to stay below 2^31.");
  CheckDeclaredSize(kName, declared_rows, declared_cols, size, size, "2 L ny nx x 2 L ny nx");
  std::unique_ptr<BlockFFT2D<T>> b(new BlockFFT2D<T>(row, col, (size_t)size, (size_t)size));
  b->geometry_ = fft2d::MakeGeometry((long)ny, (long)nx, (long)L, false);
  b->table_ = fft2d::MakeTable<T>(fft2d::TableSize((int)ny, (int)nx));
  fft2d::SumTable((int)ny, (int)nx, 1.0, b->sums1_);
  return b.release();
}
template <typename T>
void BlockFFT2D<T>::Initialize() { d_table_ = table_; d_work_.resize(this->nrows(), (T)0); }
template <typename T>
void BlockFFT2D<T>::Release() { d_table_.clear(); d_work_.clear(); }
template <typename T>
T BlockFFT2D<T>::row_sum(size_t row, T alpha) const {
  const fft2d::Geometry& g = geometry_;
  const Pixel at(row % ((size_t)g.ny * (size_t)g.nx), g.ny);
  const int l = fft2d::PeriodLog2(at.y, at.x, g.ny, g.nx);
  return (T)(alpha == (T)1 ? sums1_[l] : fft2d::ClassSum(g.ny, g.nx, (double)alpha, l));      // any other alpha: that one class, g terms
}
template <typename T>
void BlockFFT2D<T>::row_sums(T* out, T alpha) const {
  const fft2d::Geometry& g = geometry_;
  double sums[fft2d::kMaxLog2 + 1];
  fft2d::SumTable(g.ny, g.nx, (double)alpha, sums);
  AddPlaneSums(out, (size_t)g.ny * (size_t)g.nx, 2 * (size_t)g.planes, [&](size_t q) {
    const Pixel at(q, g.ny);
    return sums[fft2d::PeriodLog2(at.y, at.x, g.ny, g.nx)];
  });
}
template <typename T>
void BlockFFT2D<T>::Product(T* r, const T* x, bool transpose, bool acc) {
  if (d_table_.size() != table_.size() || d_work_.size() != this->nrows()) throw Exception("BlockFFT2D used before Initialize().");
  static_assert(sizeof(prost_hip_fft2d_geometry) == sizeof(fft2d::Geometry), "records of prost_hip.h");
  const fft2d::Geometry g = Directed(geometry_, transpose);
  CheckHip(Api<T>::fft2d(reinterpret_cast<const prost_hip_fft2d_geometry*>(&g), d_table_.data(), d_work_.data(), r, x, acc ? 1 : 0, CurrentStream()), "fft2d");
}
template class BlockFFT2D<float>;
template class BlockFFT2D<double>;

// ---- the multi-coil Fourier operator of parallel MRI, without a matrix ----
template <typename T>
BlockSense2D<T>* BlockSense2D<T>::Create(size_t row, size_t col, double nx, double ny, double L, double C, const std::vector<double>& maps, double declared_rows,
                                         double declared_cols) {
  const char* kName = "BlockSense2D";
  for (const Named& v : {Named("nx", nx), Named("ny", ny)})
    if (!(v.second >= 1) || v.second != std::floor(v.second) || v.second > fft2d::kMaxSide || !fft2d::IsSide((long)v.second))
      Refuse(kName, v.first, " = ", v.second, " has to be a power of two from 1 to ", fft2d::kMaxSide, ".");
  CheckBelowTwo31(kName, {{"L", L}});
  CheckIntegers(kName, {{"C", C}}, sense2d::kMaxCoils, " coils; C has to be an integer from 1 to " + std::to_string(sense2d::kMaxCoils) + ".");
  const double N = ny * nx, rows = 2 * L * C * N, cols = 2 * L * N;
  if (rows >= kTwo31) Refuse(kName, "L = ", L, " images of ", nx, " x ", ny, " with C = ", C, " coils; 2 L C nx ny has to stay below 2^31.");
  if ((double)maps.size() != 2 * C * N) Refuse(kName, "the maps hold ", maps.size(), " values, not 2 C = ", 2 * C, " planes of nx ny = ", N, ".");
  CheckDeclaredSize(kName, declared_rows, declared_cols, rows, cols, "2 L C ny nx x 2 L ny nx");
  std::unique_ptr<BlockSense2D<T>> b(new BlockSense2D<T>(row, col, (size_t)rows, (size_t)cols));
  b->geometry_ = sense2d::MakeGeometry((long)ny, (long)nx, (long)L, (long)C, false);
  b->table_ = fft2d::MakeTable<T>(fft2d::TableSize((int)ny, (int)nx));
  b->maps_.resize(maps.size());
  const size_t n = (size_t)N, coils = (size_t)C;
  for (size_t i = 0; i < maps.size(); i++) {
    const T t = (T)maps[i];                         // rounded once
    if (!std::isfinite((double)t))
      Refuse(kName, "value ", i % n, " of the ", i / n < coils ? "real" : "imaginary", " part of map ", (i / n) % coils, ", ", maps[i], ", is not finite", PrecisionStop<T>());
    b->maps_[i] = t;
  }
  b->rows_.resize(coils);
  for (size_t c = 0; c < coils; c++) b->rows_[c] = sense2d::RowBound<T>(b->maps_.data(), b->geometry_, 1.0, (int)c);
  return b.release();
}
template <typename T>
double BlockSense2D<T>::RowBoundOf(double alpha, size_t c) const {
  std::lock_guard<std::mutex> lock(rows_lock_);
  if (alpha != rows_alpha_) {
    for (size_t k = 0; k < rows_.size(); k++) rows_[k] = sense2d::RowBound<T>(maps_.data(), geometry_, alpha, (int)k);
    rows_alpha_ = alpha;
  }
  return rows_[c];
}
template <typename T>
void BlockSense2D<T>::Initialize() { d_table_ = table_; d_maps_ = maps_; d_work_.resize(this->nrows(), (T)0); }
template <typename T>
void BlockSense2D<T>::Release() { d_table_.clear(); d_maps_.clear(); d_work_.clear(); }
template <typename T>
T BlockSense2D<T>::row_sum(size_t row, T alpha) const {
  const sense2d::Geometry& g = geometry_;
  const size_t image = (row / ((size_t)g.ny * (size_t)g.nx)) % ((size_t)g.planes * (size_t)g.coils);      // j = l C + c of the real or the imaginary plane
  return (T)RowBoundOf((double)alpha, image % (size_t)g.coils);
}
template <typename T>
T BlockSense2D<T>::col_sum(size_t col, T alpha) const {
  return (T)sense2d::ColBound<T>(maps_.data(), geometry_, (double)alpha, col % ((size_t)geometry_.ny * (size_t)geometry_.nx));
}
template <typename T>
void BlockSense2D<T>::row_sums(T* out, T alpha) const {
  const sense2d::Geometry& g = geometry_;
  std::vector<double> bound((size_t)g.coils);
  for (int c = 0; c < g.coils; c++) bound[(size_t)c] = RowBoundOf((double)alpha, (size_t)c);
  AddPlaneConstants(out, (size_t)g.ny * (size_t)g.nx, 2 * (size_t)g.planes * (size_t)g.coils, [&](size_t plane) { return (T)bound[plane % (size_t)g.coils]; });
}
template <typename T>
void BlockSense2D<T>::col_sums(T* out, T alpha) const {
  const sense2d::Geometry& g = geometry_;
  AddPlaneSums(out, (size_t)g.ny * (size_t)g.nx, 2 * (size_t)g.planes, [&](size_t p) { return sense2d::ColBound<T>(maps_.data(), g, (double)alpha, p); });
}
template <typename T>
void BlockSense2D<T>::Product(T* r, const T* x, bool transpose, bool acc) {
  if (d_table_.size() != table_.size() || d_maps_.size() != maps_.size() || d_work_.size() != this->nrows()) throw Exception("BlockSense2D used before Initialize().");
  static_assert(sizeof(prost_hip_sense2d_geometry) == sizeof(sense2d::Geometry), "records of prost_hip.h");
  const sense2d::Geometry g = Directed(geometry_, transpose);
  CheckHip(Api<T>::sense2d(reinterpret_cast<const prost_hip_sense2d_geometry*>(&g), d_table_.data(), d_maps_.data(), d_work_.data(), r, x, acc ? 1 : 0, CurrentStream()),
           "sense2d");
}
template class BlockSense2D<float>;
template class BlockSense2D<double>;

// ---- the orthogonal multi-level wavelet transform, without a matrix ----
template <typename T>
BlockWavelet2D<T>* BlockWavelet2D<T>::Create(size_t row, size_t col, double nx, double ny, double L, const std::vector<double>& taps, double levels,
                                             double declared_rows, double declared_cols) {
  namespace w2d = wavelet2d;
  const char* kName = "BlockWavelet2D";
  CheckFinite(kName, taps, "the taps hold");
  if (const char* why = w2d::CheckShape(ny, nx, L, levels, (double)taps.size()))
    Refuse(kName, why, " (nx = ", nx, ", ny = ", ny, ", L = ", L, ", levels = ", levels, ", ", taps.size(), " taps).");
  const double defect = w2d::OrthoDefect(taps.data(), (int)taps.size());
  if (!(defect <= w2d::kOrthoTolerance))
    Refuse(kName, "the taps are not orthonormal: |sum_k h[k] h[k+2l] - delta_l| = ", defect, " for some l, above ", w2d::kOrthoTolerance,
           " (taps rounded from exact values miss by about 1e-15; a table truncated to fewer digits is refused).");
  const double size = L * ny * nx;
  CheckDeclaredSize(kName, declared_rows, declared_cols, size, size, "L ny nx x L ny nx");
  std::unique_ptr<BlockWavelet2D<T>> b(new BlockWavelet2D<T>(row, col, (size_t)size, (size_t)size));
  b->geometry_ = w2d::MakeGeometry((long)ny, (long)nx, (long)L, (long)levels, (long)taps.size(), false);
  b->taps64_ = taps;
  b->taps_.assign(taps.begin(), taps.end());           // rounded once to T
  return b.release();
}
template <typename T>
void BlockWavelet2D<T>::Initialize() { d_work_.resize(wavelet2d::WorkSize(geometry_), (T)0); }
template <typename T>
void BlockWavelet2D<T>::Release() { d_work_.clear(); }
template <typename T>
void BlockWavelet2D<T>::Tables(double alpha) const {
  if (tables_alpha_ == alpha) return;
  const wavelet2d::Geometry& g = geometry_;
  tables_y_ = wavelet2d::AxisTables(g.ny, g.levels, taps64_.data(), g.ntaps, alpha);
  tables_x_ = wavelet2d::AxisTables(g.nx, g.levels, taps64_.data(), g.ntaps, alpha);
  tables_alpha_ = alpha;
}
template <typename T>
T BlockWavelet2D<T>::row_sum(size_t row, T alpha) const {
  const wavelet2d::Geometry& g = geometry_;
  Tables((double)alpha);
  const Pixel at(row % ((size_t)g.ny * (size_t)g.nx), g.ny);
  return (T)wavelet2d::RowSum(g, tables_y_, tables_x_, at.y, at.x);
}
template <typename T>
T BlockWavelet2D<T>::col_sum(size_t col, T alpha) const {
  const wavelet2d::Geometry& g = geometry_;
  Tables((double)alpha);
  const Pixel at(col % ((size_t)g.ny * (size_t)g.nx), g.ny);
  return (T)wavelet2d::ColSum(g, tables_y_, tables_x_, at.y, at.x);
}
template <typename T>
void BlockWavelet2D<T>::row_sums(T* out, T alpha) const {
  AddPlaneSums(out, (size_t)geometry_.ny * (size_t)geometry_.nx, (size_t)geometry_.planes, [&](size_t q) { return row_sum(q, alpha); });
}
template <typename T>
void BlockWavelet2D<T>::col_sums(T* out, T alpha) const {
  AddPlaneSums(out, (size_t)geometry_.ny * (size_t)geometry_.nx, (size_t)geometry_.planes, [&](size_t p) { return col_sum(p, alpha); });
}
template <typename T>
void BlockWavelet2D<T>::Product(T* r, const T* x, bool transpose, bool acc) {
  if (d_work_.size() != wavelet2d::WorkSize(geometry_)) throw Exception("BlockWavelet2D used before Initialize().");
  static_assert(sizeof(prost_hip_wavelet2d_geometry) == sizeof(wavelet2d::Geometry), "records of prost_hip.h");
  const wavelet2d::Geometry g = Directed(geometry_, transpose);
  CheckHip(Api<T>::wavelet2d(reinterpret_cast<const prost_hip_wavelet2d_geometry*>(&g), taps_.data(), d_work_.data(), r, x, acc ? 1 : 0, CurrentStream()), "wavelet2d");
}
template class BlockWavelet2D<float>;
template class BlockWavelet2D<double>;

// ---- the symmetrised gradient of TGV^2, without a matrix ----
template <typename T>
BlockSymGradient2D<T>* BlockSymGradient2D<T>::Create(size_t row, size_t col, double nx, double ny, double L, double w, double declared_rows, double declared_cols) {
  const char* kName = "BlockSymGradient2D";
  CheckIntegers(kName, {{"nx", nx}, {"ny", ny}, {"L", L}}, kTwo53, " has to be a positive integer.");
  if (!std::isfinite(w)) Refuse(kName, "w = ", w, " has to be finite.");
  if (w == 0) Refuse(kName, "w has to be non-zero.");
  const T wt = sym_gradient2d::RoundWeight<T>(w);
  if (wt == (T)0 || !std::isfinite((double)wt)) Refuse(kName, "w = ", w, " is zero or not finite", PrecisionStop<T>());
  const double rows = 3 * L * nx * ny, cols = 2 * L * nx * ny;
  if (!(3 * L * (nx * ny) <= kTwo53) || !(nx * ny <= kTwo53)) Refuse(kName, "3 L nx ny = ", rows, " rows; the size has to stay within 2^53.");
  CheckDeclaredSize(kName, declared_rows, declared_cols, rows, cols, "3 L nx ny x 2 L nx ny");
  return new BlockSymGradient2D<T>(row, col, (size_t)nx, (size_t)ny, (size_t)L, w);
}
template <typename T>
T BlockSymGradient2D<T>::row_sum(size_t row, T alpha) const { return (T)sym_gradient2d::RowSum(row, nx_, ny_, L_, WeightPower(alpha)); }
template <typename T>
T BlockSymGradient2D<T>::col_sum(size_t col, T alpha) const { return (T)sym_gradient2d::ColSum(col, nx_, ny_, L_, WeightPower(alpha)); }
template <typename T>
void BlockSymGradient2D<T>::row_sums(T* out, T alpha) const {
  sym_gradient2d::RowSums<T>(out, nx_, ny_, L_, WeightPower(alpha));
}
template <typename T>
void BlockSymGradient2D<T>::col_sums(T* out, T alpha) const {
  sym_gradient2d::ColSums<T>(out, nx_, ny_, L_, WeightPower(alpha));
}
template <typename T>
void BlockSymGradient2D<T>::Product(T* r, const T* x, bool transpose, bool acc) {
  CheckHip(Api<T>::linop_sym_gradient2d(r, x, nx_, ny_, L_, w_, transpose ? 1 : 0, acc ? 1 : 0, CurrentStream()), "linop_sym_gradient2d");
}
template class BlockSymGradient2D<float>;
template class BlockSymGradient2D<double>;

// ---- K = T grad: the gradient weighted by a per-pixel scalar, axis weights or symmetric tensor, without a matrix ----
template <typename T>
BlockTensorGradient2D<T>* BlockTensorGradient2D<T>::Create(size_t row, size_t col, double nx, double ny, double L, double mode, const std::vector<double>& tensor,
                                                           double declared_rows, double declared_cols) {
  const char* kName = "BlockTensorGradient2D";
  CheckIntegers(kName, {{"nx", nx}, {"ny", ny}, {"L", L}}, kTwo53, " has to be a positive integer.");
  if (!(mode == 1 || mode == 2 || mode == 3)) Refuse(kName, "the tensor has k = ", mode, " planes; k has to be 1 (scalar), 2 (per axis) or 3 (symmetric tensor).");
  const double rows = 2 * L * nx * ny, cols = L * nx * ny;
  if (!(2 * L * (nx * ny) <= kTwo53) || !(nx * ny <= kTwo53)) Refuse(kName, "2 L nx ny = ", rows, " rows; the size has to stay within 2^53.");
  if ((double)tensor.size() != mode * nx * ny) Refuse(kName, "the tensor holds ", tensor.size(), " values, not k = ", mode, " planes of nx ny = ", nx * ny, ".");
  CheckDeclaredSize(kName, declared_rows, declared_cols, rows, cols, "2 L nx ny x L nx ny");
  std::unique_ptr<BlockTensorGradient2D<T>> b(new BlockTensorGradient2D<T>(row, col, (size_t)nx, (size_t)ny, (size_t)L, (int)mode));
  b->tensor_.resize(tensor.size());
  for (size_t i = 0; i < tensor.size(); i++) {
    const T t = (T)tensor[i];                       // rounded once
    if (!std::isfinite((double)t))
      Refuse(kName, "value ", i % (size_t)(nx * ny), " of plane ", i / (size_t)(nx * ny), " of the tensor, ", tensor[i], ", is not finite", PrecisionStop<T>());
    b->tensor_[i] = t;
  }
  return b.release();
}
template <typename T>
void BlockTensorGradient2D<T>::Initialize() { d_tensor_ = tensor_; }
template <typename T>
void BlockTensorGradient2D<T>::Release() { d_tensor_.clear(); }
template <typename T>
T BlockTensorGradient2D<T>::row_sum(size_t row, T alpha) const { return (T)tensor_gradient2d::RowSum(row, tensor_.data(), nx_, ny_, L_, mode_, (double)alpha); }
template <typename T>
T BlockTensorGradient2D<T>::col_sum(size_t col, T alpha) const { return (T)tensor_gradient2d::ColSum(col, tensor_.data(), nx_, ny_, L_, mode_, (double)alpha); }
template <typename T>
void BlockTensorGradient2D<T>::row_sums(T* out, T alpha) const { tensor_gradient2d::RowSums<T>(out, tensor_.data(), nx_, ny_, L_, mode_, (double)alpha); }
template <typename T>
void BlockTensorGradient2D<T>::col_sums(T* out, T alpha) const { tensor_gradient2d::ColSums<T>(out, tensor_.data(), nx_, ny_, L_, mode_, (double)alpha); }
template <typename T>
void BlockTensorGradient2D<T>::Product(T* r, const T* x, bool transpose, bool acc) {
  if (d_tensor_.size() != tensor_.size()) throw Exception("BlockTensorGradient2D used before Initialize().");
  CheckHip(Api<T>::linop_tensor_gradient2d(r, x, d_tensor_.data(), nx_, ny_, L_, mode_, transpose ? 1 : 0, acc ? 1 : 0, CurrentStream()), "linop_tensor_gradient2d");
}
template class BlockTensorGradient2D<float>;
template class BlockTensorGradient2D<double>;

// ---- the nonlocal gradient w_m(p) (u[p + d_m] - u[p]): M displacements, one weight plane each, without a matrix ----
template <typename T>
BlockNonlocalGradient2D<T>* BlockNonlocalGradient2D<T>::Create(size_t row, size_t col, double nx, double ny, double L, const std::vector<double>& offsets,
                                                               const std::vector<double>& weights, double declared_rows, double declared_cols) {
  const char* kName = "BlockNonlocalGradient2D";
  namespace nl = nonlocal_gradient2d;
  CheckIntegers(kName, {{"nx", nx}, {"ny", ny}, {"L", L}}, kTwo53, " has to be a positive integer.");
  if (offsets.empty() || offsets.size() % 2 != 0 || offsets.size() / 2 > (size_t)nl::kMaxOffsets)
    Refuse(kName, "the offsets hold ", offsets.size(), " values; they are M pairs (dy, dx), M from 1 to ", nl::kMaxOffsets, ".");
  CheckFinite(kName, offsets, "the offsets hold");
  const size_t M = offsets.size() / 2;
  for (size_t m = 0; m < M; m++) {
    const double dy = offsets[2 * m], dx = offsets[2 * m + 1];
    if (dy != std::floor(dy) || dx != std::floor(dx)) Refuse(kName, "offset ", m, " = (", dy, ", ", dx, ") is not a pair of integers.");
    if (std::fabs(dy) > nl::kMaxReach || std::fabs(dx) > nl::kMaxReach) Refuse(kName, "offset ", m, " = (", dy, ", ", dx, ") reaches beyond ", nl::kMaxReach, ".");
    if (dy == 0 && dx == 0) Refuse(kName, "offset ", m, " is (0, 0), which is no displacement.");
    for (size_t k = 0; k < m; k++)
      if (offsets[2 * k] == dy && offsets[2 * k + 1] == dx) Refuse(kName, "offsets ", k, " and ", m, " are both (", dy, ", ", dx, "); the offsets have to be distinct.");
  }
  const double rows = (double)M * L * nx * ny, cols = L * nx * ny;
  if (!((double)M * L * (nx * ny) <= kTwo53) || !(nx * ny <= kTwo53)) Refuse(kName, "M L nx ny = ", rows, " rows; the size has to stay within 2^53.");
  if ((double)weights.size() != (double)M * nx * ny) Refuse(kName, "the weights hold ", weights.size(), " values, not M = ", M, " planes of nx ny = ", nx * ny, ".");
  const double tiles = std::ceil(ny / nl::kTileY) * std::ceil(nx / nl::kTileX) * L;        // at least one channel per pass
  if (!(tiles < kTwo31)) Refuse(kName, "a grid of ", ny, " x ", nx, " with ", L, " channels needs up to ", tiles, " workgroups; it has to stay below 2^31.");
  CheckDeclaredSize(kName, declared_rows, declared_cols, rows, cols, "M L nx ny x L nx ny");
  std::unique_ptr<BlockNonlocalGradient2D<T>> b(new BlockNonlocalGradient2D<T>(row, col, (size_t)nx, (size_t)ny, (size_t)L, (int)M));
  b->offsets_ = nl::Offsets();
  b->pairs_.resize(2 * M);
  for (size_t m = 0; m < M; m++) {
    b->offsets_.dy[m] = b->pairs_[2 * m] = (signed char)offsets[2 * m];
    b->offsets_.dx[m] = b->pairs_[2 * m + 1] = (signed char)offsets[2 * m + 1];
  }
  b->weights_.resize(weights.size());
  for (size_t i = 0; i < weights.size(); i++) {
    const T w = (T)weights[i];                      // rounded once
    if (!std::isfinite((double)w))
      Refuse(kName, "value ", i % (size_t)(nx * ny), " of plane ", i / (size_t)(nx * ny), " of the weights, ", weights[i], ", is not finite", PrecisionStop<T>());
    b->weights_[i] = w;
  }
  return b.release();
}
template <typename T>
void BlockNonlocalGradient2D<T>::Initialize() { d_weights_ = weights_; }
template <typename T>
void BlockNonlocalGradient2D<T>::Release() { d_weights_.clear(); }
template <typename T>
T BlockNonlocalGradient2D<T>::row_sum(size_t row, T alpha) const { return (T)nonlocal_gradient2d::RowSum(row, weights_.data(), offsets_, nx_, ny_, L_, (double)alpha); }
template <typename T>
T BlockNonlocalGradient2D<T>::col_sum(size_t col, T alpha) const { return (T)nonlocal_gradient2d::ColSum(col, weights_.data(), offsets_, M_, nx_, ny_, (double)alpha); }
template <typename T>
void BlockNonlocalGradient2D<T>::row_sums(T* out, T alpha) const {
  const size_t N = nx_ * ny_;
  for (int m = 0; m < M_; m++)                      // the L planes of displacement m are the same
    AddPlaneSums(out + (size_t)m * L_ * N, N, L_, [&](size_t p) { return nonlocal_gradient2d::PixelRowSum(weights_.data(), offsets_, m, nx_, ny_, p, (double)alpha); });
}
template <typename T>
void BlockNonlocalGradient2D<T>::col_sums(T* out, T alpha) const {
  AddPlaneSums(out, nx_ * ny_, L_, [&](size_t p) { return nonlocal_gradient2d::PixelColSum(weights_.data(), offsets_, M_, nx_, ny_, p, (double)alpha); });
}
template <typename T>
void BlockNonlocalGradient2D<T>::Product(T* r, const T* x, bool transpose, bool acc) {
  if (d_weights_.size() != weights_.size()) throw Exception("BlockNonlocalGradient2D used before Initialize().");
  CheckHip(Api<T>::linop_nonlocal_gradient2d(r, x, d_weights_.data(), nx_, ny_, L_, M_, pairs_.data(), transpose ? 1 : 0, acc ? 1 : 0, CurrentStream()),
           "linop_nonlocal_gradient2d");
}
template class BlockNonlocalGradient2D<float>;
template class BlockNonlocalGradient2D<double>;

// ---- the second-order differences H = E grad of TV^2, without a matrix ----
template <typename T>
BlockHessian2D<T>* BlockHessian2D<T>::Create(size_t row, size_t col, double nx, double ny, double L, double w, double components, double declared_rows,
                                             double declared_cols) {
  const char* kName = "BlockHessian2D";
  CheckIntegers(kName, {{"nx", nx}, {"ny", ny}, {"L", L}}, kTwo53, " has to be a positive integer.");
  if (!std::isfinite(w)) Refuse(kName, "w = ", w, " has to be finite.");
  if (w == 0) Refuse(kName, "w has to be non-zero.");
  const T wt = hessian2d::RoundWeight<T>(w);
  if (wt == (T)0 || !std::isfinite((double)wt)) Refuse(kName, "w = ", w, " is zero or not finite", PrecisionStop<T>());
  if (!(components == 3 || components == 4)) Refuse(kName, "components = ", components, " has to be 3 (hxx, hyy, hxy) or 4 (hxx, hxy, hxy, hyy).");
  const double rows = components * L * nx * ny, cols = L * nx * ny;
  if (!(components * L * (nx * ny) <= kTwo53) || !(nx * ny <= kTwo53)) Refuse(kName, "components L nx ny = ", rows, " rows; the size has to stay within 2^53.");
  CheckDeclaredSize(kName, declared_rows, declared_cols, rows, cols, "components L nx ny x L nx ny");
  return new BlockHessian2D<T>(row, col, (size_t)nx, (size_t)ny, (size_t)L, w, (int)components);
}
template <typename T>
T BlockHessian2D<T>::row_sum(size_t row, T alpha) const {
  return (T)hessian2d::RowSum(row, nx_, ny_, L_, components_, WeightPower(alpha), hessian2d::TwoPower((double)alpha));
}
template <typename T>
T BlockHessian2D<T>::col_sum(size_t col, T alpha) const {
  return (T)hessian2d::ColSum(col, nx_, ny_, components_, WeightPower(alpha), hessian2d::TwoPower((double)alpha));
}
template <typename T>
void BlockHessian2D<T>::row_sums(T* out, T alpha) const {
  const size_t N = nx_ * ny_;
  for (size_t k = 0; k < (size_t)components_; k++)             // the L planes of component k are the same
    AddPlaneSums(out + k * L_ * N, N, L_, [&](size_t p) { return row_sum(k * L_ * N + p, alpha); });
}
template <typename T>
void BlockHessian2D<T>::col_sums(T* out, T alpha) const {
  AddPlaneSums(out, nx_ * ny_, L_, [&](size_t p) { return col_sum(p, alpha); });
}
template <typename T>
void BlockHessian2D<T>::Product(T* r, const T* x, bool transpose, bool acc) {
  CheckHip(Api<T>::hessian2d(r, x, nx_, ny_, L_, w_, components_, transpose ? 1 : 0, acc ? 1 : 0, CurrentStream()), "hessian2d");
}
template class BlockHessian2D<float>;
template class BlockHessian2D<double>;

// ---- diags block ----
static bool g_diags_quirk = false;
template <typename T> void BlockDiags<T>::SetReferenceGridQuirk(bool on) { g_diags_quirk = on; }
template <typename T> bool BlockDiags<T>::ReferenceGridQuirk() { return g_diags_quirk; }
template <typename T>
BlockDiags<T>::BlockDiags(size_t row, size_t col, size_t nrows, size_t ncols, size_t ndiags, const std::vector<int64_t>& offsets,
                          const std::vector<T>& factors)
    : Block<T>(row, col, nrows, ncols), ndiags_(ndiags), offsets_(offsets) {
  factors_ = std::vector<float>(factors.begin(), factors.end());
  // ascending offsets: the kernels stop at the first diagonal that leaves the matrix.  Selection
  // by pairwise exchange, which is also the order the reference produces for equal offsets
  // (block_diags.cu:110-118).
  for (size_t i = 0; i < ndiags_; i++)
    for (size_t j = i; j < ndiags_; j++)
      if (offsets_[i] > offsets_[j]) { std::swap(offsets_[i], offsets_[j]); std::swap(factors_[i], factors_[j]); }
}
template <typename T>
void BlockDiags<T>::Initialize() {
  if (ndiags_ >= 1024) throw Exception("Out of constant memory. Too many BlockDiags or too many diagonals.");
  d_offsets_ = offsets_;
  d_factors_ = factors_;
}
template <typename T> void BlockDiags<T>::Release() { d_offsets_.clear(); d_factors_.clear(); }
template <typename T>
T BlockDiags<T>::row_sum(size_t row, T alpha) const {
  T sum = 0;
  for (size_t i = 0; i < ndiags_; i++) {
    const long long col = (long long)row + offsets_[i];
    if (col < 0) continue;
    if ((size_t)col >= this->ncols()) break;
    sum += std::pow(std::abs(factors_[i]), alpha);
  }
  return sum;
}
template <typename T>
T BlockDiags<T>::col_sum(size_t col, T alpha) const {
  T sum = 0;
  const long long sc = (long long)col;
  for (size_t i = 0; i < ndiags_; i++) {
    const long long o = offsets_[i];
    if (o <= sc && (sc - o) < (long long)this->nrows() && (sc - o) >= 0) sum += std::pow(std::abs(factors_[i]), alpha);
    if (o > sc) break;
  }
  return sum;
}
template <typename T>
void BlockDiags<T>::EvalLocalAdd(T* r, T*, const T* x, const T*) {
  if (d_offsets_.size() != ndiags_) throw Exception("BlockDiags used before Initialize().");
  CheckHip(Api<T>::diags_fwd(r, x, this->nrows(), this->ncols(), ndiags_, d_offsets_.data(), d_factors_.data(), CurrentStream()), "diags_fwd");
}
template <typename T>
void BlockDiags<T>::EvalAdjointLocalAdd(T* r, T*, const T* x, const T*) {
  if (d_offsets_.size() != ndiags_) throw Exception("BlockDiags used before Initialize().");
  CheckHip(Api<T>::diags_adj(r, x, this->nrows(), this->ncols(), ndiags_, d_offsets_.data(), d_factors_.data(), g_diags_quirk ? 1 : 0, CurrentStream()), "diags_adj");
}
template class BlockDiags<float>;
template class BlockDiags<double>;
template class BlockZero<float>;
template class BlockZero<double>;

// ---- LinearOperator ----
static bool ranges_partition(std::vector<std::pair<size_t, size_t>> r, size_t total) {
  std::sort(r.begin(), r.end());
  size_t pos = 0;
  for (auto& p : r) { if (p.first != pos) return false; pos = p.first + p.second; }
  return pos == total;
}

template <typename T>
void LinearOperator<T>::InitializeHost() {
  nrows_ = ncols_ = 0;
  bool overlap = false;
  for (size_t i = 0; i < blocks_.size(); i++) {
    const Block<T>& a = *blocks_[i];
    nrows_ = std::max(a.row() + a.nrows(), nrows_);
    ncols_ = std::max(a.col() + a.ncols(), ncols_);
    for (size_t j = i + 1; j < blocks_.size(); j++) {
      const Block<T>& b = *blocks_[j];
      const bool cols_meet = a.col() <= b.col() + b.ncols() - 1 && a.col() + a.ncols() - 1 >= b.col();
      const bool rows_meet = a.row() <= b.row() + b.nrows() - 1 && a.row() + a.nrows() - 1 >= b.row();
      overlap |= cols_meet && rows_meet;
    }
  }
  if (overlap) throw Exception("Blocks are overlapping inside the linear operator. Recheck the indices.");
  std::vector<std::pair<size_t, size_t>> rr, cc;
  for (auto& b : blocks_) { rr.emplace_back(b->row(), b->nrows()); cc.emplace_back(b->col(), b->ncols()); }
  rows_exclusive_ = !blocks_.empty() && ranges_partition(rr, nrows_);
  cols_exclusive_ = !blocks_.empty() && ranges_partition(cc, ncols_);
  // first writers and pure accumulators, in list order (the order LinearOperator::Eval accumulates in): a first writer runs its
  // non-accumulating product (0 + sum: the bits of fill + accumulate), nobody fills
  auto plan = [](const std::vector<std::pair<size_t, size_t>>& r, size_t total, std::vector<char>& out) {
    out.clear();
    std::vector<std::pair<size_t, size_t>> done;                      // disjoint [begin, end) ranges already written, sorted
    std::vector<char> p;
    for (const auto& q : r) {
      const size_t b = q.first, e = q.first + q.second;
      size_t covered = 0;
      for (const auto& d : done) { const size_t lo = std::max(b, d.first), hi = std::min(e, d.second); if (lo < hi) covered += hi - lo; }
      if (covered == 0) { p.push_back(0); done.emplace_back(b, e); }
      else if (covered == e - b) p.push_back(1);
      else return;                                                    // partly new: no plan
      // (merge: keep `done` disjoint)
      std::sort(done.begin(), done.end());
      std::vector<std::pair<size_t, size_t>> m;
      for (const auto& d : done) { if (!m.empty() && d.first <= m.back().second) m.back().second = std::max(m.back().second, d.second); else m.push_back(d); }
      done.swap(m);
    }
    if (done.size() == 1 && done[0].first == 0 && done[0].second == total) out.swap(p);
  };
  plan(rr, nrows_, row_plan_);
  plan(cc, ncols_, col_plan_);
}
template <typename T>
void LinearOperator<T>::Initialize() {
  InitializeHost();
  for (auto& b : blocks_) b->Initialize();
}
template <typename T> void LinearOperator<T>::Release() { for (auto& b : blocks_) b->Release(); }

template <typename T>
void LinearOperator<T>::ApplyBeta(device_vector<T>& result, T beta, bool negate_beta) {
  if (beta == 0) CheckHip(Api<T>::scale(result.data(), result.size(), 0.0, CurrentStream()), "scale");
  else if (beta != 1) CheckHip(Api<T>::scale(result.data(), result.size(), negate_beta ? (double)-beta : (double)beta, CurrentStream()), "scale");
}
template <typename T>
void LinearOperator<T>::Eval(device_vector<T>& result, const device_vector<T>& rhs, T beta) {
  if (beta == 0 && rows_exclusive_ && result.size() == nrows_) {        // every row has exactly one writer: no fill pass
    for (auto& b : blocks_) b->Eval(result.data(), rhs.data());
    return;
  }
  if (beta == 0 && !blocks_.empty() && blocks_[0]->row() == 0 && blocks_[0]->nrows() == nrows_ && result.size() == nrows_) {
    // the first block writes every row: it replaces the fill, the others accumulate in the same order as before
    blocks_[0]->Eval(result.data(), rhs.data());
    for (size_t i = 1; i < blocks_.size(); i++) blocks_[i]->EvalAdd(result.data(), rhs.data());
    return;
  }
  if (beta == 0 && row_plan_.size() == blocks_.size() && !blocks_.empty() && result.size() == nrows_) {
    for (size_t i = 0; i < blocks_.size(); i++) { if (row_plan_[i]) blocks_[i]->EvalAdd(result.data(), rhs.data()); else blocks_[i]->Eval(result.data(), rhs.data()); }
    return;
  }
  ApplyBeta(result, beta, false);
  for (auto& b : blocks_) b->EvalAdd(result.data(), rhs.data());
}
template <typename T>
void LinearOperator<T>::EvalAdjoint(device_vector<T>& result, const device_vector<T>& rhs, T beta) {
  if (beta == 0 && cols_exclusive_ && result.size() == ncols_) {
    for (auto& b : blocks_) b->EvalAdjoint(result.data(), rhs.data());
    return;
  }
  if (beta == 0 && !blocks_.empty() && blocks_[0]->col() == 0 && blocks_[0]->ncols() == ncols_ && result.size() == ncols_) {
    blocks_[0]->EvalAdjoint(result.data(), rhs.data());
    for (size_t i = 1; i < blocks_.size(); i++) blocks_[i]->EvalAdjointAdd(result.data(), rhs.data());
    return;
  }
  if (beta == 0 && col_plan_.size() == blocks_.size() && !blocks_.empty() && result.size() == ncols_) {
    for (size_t i = 0; i < blocks_.size(); i++) { if (col_plan_[i]) blocks_[i]->EvalAdjointAdd(result.data(), rhs.data()); else blocks_[i]->EvalAdjoint(result.data(), rhs.data()); }
    return;
  }
  ApplyBeta(result, beta, false);
  for (auto& b : blocks_) b->EvalAdjointAdd(result.data(), rhs.data());
}
template <typename T>
static double timed_eval(LinearOperator<T>* op, bool adjoint, std::vector<T>& result, const std::vector<T>& rhs) {
  static const int repeats = 5;                     // linearoperator.cu:178
  device_vector<T> d_rhs; d_rhs = rhs;
  device_vector<T> d_res(adjoint ? op->ncols() : op->nrows());
  CheckHip(prost_hip_stream_synchronize(CurrentStream()), "sync");
  const auto t0 = std::chrono::steady_clock::now();
  for (int i = 0; i < repeats; i++) {
    if (adjoint) op->EvalAdjoint(d_res, d_rhs); else op->Eval(d_res, d_rhs);
    CheckHip(prost_hip_stream_synchronize(CurrentStream()), "sync");
  }
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  d_res.copy_to(result);
  return ms / repeats;
}
template <typename T> double LinearOperator<T>::Eval(std::vector<T>& result, const std::vector<T>& rhs) { return timed_eval(this, false, result, rhs); }
template <typename T> double LinearOperator<T>::EvalAdjoint(std::vector<T>& result, const std::vector<T>& rhs) { return timed_eval(this, true, result, rhs); }

template <typename T>
T LinearOperator<T>::row_sum(size_t row, T alpha) const {
  T sum = 0;
  for (auto& b : blocks_) { if (row < b->row() || row >= b->row() + b->nrows()) continue; sum += b->row_sum(row - b->row(), alpha); }
  return sum;
}
template <typename T>
T LinearOperator<T>::col_sum(size_t col, T alpha) const {
  T sum = 0;
  for (auto& b : blocks_) { if (col < b->col() || col >= b->col() + b->ncols()) continue; sum += b->col_sum(col - b->col(), alpha); }
  return sum;
}
template <typename T>
void LinearOperator<T>::row_sums(std::vector<T>& out, T alpha) const {
  ParallelFor(out.size(), [&](size_t b, size_t e) { std::fill(out.begin() + b, out.begin() + e, (T)0); });
  for (auto& b : blocks_) { if (b->row() + b->nrows() <= out.size()) b->row_sums(out.data() + b->row(), alpha); }
}
template <typename T>
void LinearOperator<T>::col_sums(std::vector<T>& out, T alpha) const {
  ParallelFor(out.size(), [&](size_t b, size_t e) { std::fill(out.begin() + b, out.begin() + e, (T)0); });
  for (auto& b : blocks_) { if (b->col() + b->ncols() <= out.size()) b->col_sums(out.data() + b->col(), alpha); }
}
template <typename T>
size_t LinearOperator<T>::gpu_mem_amount() const { size_t m = 0; for (auto& b : blocks_) m += b->gpu_mem_amount(); return m; }
template class LinearOperator<float>;
template class LinearOperator<double>;

// ---- DualLinearOperator: -K^T (dual_linearoperator.cu:39-80) ----
static bool g_negate_quirk = false;
template <typename T> void DualLinearOperator<T>::SetReferenceNegateQuirk(bool on) { g_negate_quirk = on; }
template <typename T>
void DualLinearOperator<T>::Eval(device_vector<T>& result, const device_vector<T>& rhs, T beta) {
  this->ApplyBeta(result, beta, true);
  for (auto& b : child_->blocks_) b->EvalAdjointAdd(result.data(), rhs.data());
  CheckHip(negate(result.data(), result.size(), g_negate_quirk, CurrentStream()), "negate");
}
template <typename T>
void DualLinearOperator<T>::EvalAdjoint(device_vector<T>& result, const device_vector<T>& rhs, T beta) {
  this->ApplyBeta(result, beta, true);
  for (auto& b : child_->blocks_) b->EvalAdd(result.data(), rhs.data());
  CheckHip(negate(result.data(), result.size(), g_negate_quirk, CurrentStream()), "negate");
}
template class DualLinearOperator<float>;
template class DualLinearOperator<double>;

// ---- the operator as a block table ----
template <typename T>
bool DescribeOperatorTable(const LinearOperator<T>& linop, prost_hip_fused_op& op, const std::function<bool(const Block<T>&, const BlockDesc&)>& accept_sparse) {
  std::memset(&op, 0, sizeof(op));
  if (dynamic_cast<const DualLinearOperator<T>*>(&linop)) return false;
  const auto& blocks = linop.blocks();
  if (blocks.empty() || blocks.size() > (size_t)PROST_HIP_OP_MAX_BLOCKS) return false;
  for (const auto& b : blocks) {
    BlockDesc bd;
    if (!b->describe(bd)) return false;
    prost_hip_op_block& o = op.block[op.nblocks++];
    o.row = b->row(); o.col = b->col(); o.nrows = b->nrows(); o.ncols = b->ncols();
    if (bd.kind == BlockDesc::kSparse) {
      if (!accept_sparse(*b, bd)) return false;
      o.kind = PROST_OP_CSR;
      o.val = bd.val; o.ptr = bd.ptr; o.ind = bd.ind; o.val_t = bd.val_t; o.ptr_t = bd.ptr_t; o.ind_t = bd.ind_t;
      o.ids = bd.ids; o.pptr = bd.pptr; o.rel = bd.rel; o.pval = bd.pval; o.ids_t = bd.ids_t; o.pptr_t = bd.pptr_t; o.rel_t = bd.rel_t; o.pval_t = bd.pval_t;
      o.anchor = bd.anchor; o.anchor_t = bd.anchor_t;
    } else if ((bd.kind == BlockDesc::kGradient2D || bd.kind == BlockDesc::kGradient3D) && !bd.label_first) {
      o.kind = bd.kind == BlockDesc::kGradient2D ? PROST_OP_GRAD2D : PROST_OP_GRAD3D;
      o.nx = bd.nx; o.ny = bd.ny; o.L = bd.L;
    } else return false;
  }
  return true;
}
template bool DescribeOperatorTable<float>(const LinearOperator<float>&, prost_hip_fused_op&, const std::function<bool(const Block<float>&, const BlockDesc&)>&);
template bool DescribeOperatorTable<double>(const LinearOperator<double>&, prost_hip_fused_op&, const std::function<bool(const Block<double>&, const BlockDesc&)>&);

}  // namespace prost
