// prost/linop/blocks.hpp -- the in-tree blocks of the hot path
// (reference: include/prost/linop/block_{gradient2d,gradient3d,sparse,dense,dense_kron_id,id_kron_dense,diags,zero}.hpp).
#ifndef PROST_LINOP_BLOCKS_HPP_
#define PROST_LINOP_BLOCKS_HPP_
#include <mutex>

#include "prost/device_vector.hpp"
#include "prost/linop/block.hpp"
#include "prost/linop/conv2d.hpp"
#include "prost/linop/conv2d_strided.hpp"
#include "prost/linop/fanbeam2d.hpp"
#include "prost/linop/fft2d.hpp"
#include "prost/linop/hessian2d.hpp"
#include "prost/linop/radon2d.hpp"
#include "prost/linop/sample2d.hpp"
#include "prost/linop/sense2d.hpp"
#include "prost/linop/sym_gradient2d.hpp"
#include "prost/linop/tensor_gradient2d.hpp"
#include "prost/linop/nonlocal_gradient2d.hpp"
#include "prost/linop/wavelet2d.hpp"

namespace prost {

/// A block whose kernels take the direction and an accumulate flag: it implements ONE product, and the four evaluation entries of the
/// plugin contract (prost::Block<T>, block.hpp -- unchanged, plugins keep deriving from it) are written here once.
template <typename T>
class ProductBlock : public Block<T> {
 public:
  using Block<T>::Block;

 protected:
  /// res = K rhs, or K^T rhs (transpose); accumulate: res += ...
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate) = 0;
  void EvalLocalAdd(T* res, T*, const T* rhs, const T*) final { Product(res, rhs, false, true); }
  void EvalAdjointLocalAdd(T* res, T*, const T* rhs, const T*) final { Product(res, rhs, true, true); }
  void EvalLocal(T* res, T*, const T* rhs, const T*) final { Product(res, rhs, false, false); }
  void EvalAdjointLocal(T* res, T*, const T* rhs, const T*) final { Product(res, rhs, true, false); }
};

/// D = 2: forward differences with Neumann boundary, L channels (block_gradient2d.hpp / .cu:141-204); D = 3: as 2-D plus the label/z
/// difference with Dirichlet boundary at l = L-1 (block_gradient3d.cu:73-76).  Every row sums to 2 and every column to 2 D
/// (block_gradient2d.cu:154-163, block_gradient3d.cu:165-174).
template <typename T, int D>
class BlockGradient : public ProductBlock<T> {
 public:
  BlockGradient(size_t row, size_t col, size_t nx, size_t ny, size_t L, bool label_first = false)
      : ProductBlock<T>(row, col, nx * ny * L * D, nx * ny * L), nx_(nx), ny_(ny), L_(L), label_first_(label_first) {}
  virtual T row_sum(size_t, T) const { return 2; }
  virtual T col_sum(size_t, T) const { return 2 * D; }
  virtual bool uniform_sums(T, T, T& row, T& col) const { row = 2; col = 2 * D; return true; }
  virtual void row_sums(T* out, T alpha) const;
  virtual void col_sums(T* out, T alpha) const;
  virtual size_t gpu_mem_amount() const { return 0; }
  virtual bool describe(BlockDesc& d) const { d.kind = D == 2 ? BlockDesc::kGradient2D : BlockDesc::kGradient3D; d.nx = nx_; d.ny = ny_; d.L = L_; d.label_first = label_first_; return true; }

 protected:
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  size_t nx_, ny_, L_;
  bool label_first_;
};
template <typename T> using BlockGradient2D = BlockGradient<T, 2>;
template <typename T> using BlockGradient3D = BlockGradient<T, 3>;

/// K (side 0 of a block) or K^T (side 1) as a CSR matrix of `rows` rows with values of type V, on the host and -- between Upload() and
/// Clear() -- on the device
template <typename V>
struct CsrSide {
  size_t rows = 0;
  std::vector<int32_t> host_ind, host_ptr;
  std::vector<V> host_val;
  device_vector<int32_t> ind, ptr;
  device_vector<V> val;
  void Upload() { ind = host_ind; ptr = host_ptr; val = host_val; }
  void Clear() { ind.clear(); ptr.clear(); val.clear(); }
  template <typename T> T AbsPowSum(size_t row, T alpha) const;      ///< sum_j |K_row,j|^alpha
};

/// general sparse block; K as CSR and K^T as CSR (= the CSC arrays handed in) (block_sparse.hpp)
template <typename T>
class BlockSparse : public ProductBlock<T> {
 public:
  /// arrays in MATLAB CSC form: ptr = Jc (ncols+1), ind = Ir (nnz) (block_sparse.cu:34-68)
  static BlockSparse<T>* CreateFromCSC(size_t row, size_t col, int m, int n, int nnz, const std::vector<T>& val,
                                       const std::vector<int32_t>& ptr, const std::vector<int32_t>& ind);
  /// the same, taking the arrays over instead of copying them (a 4096^2 gradient handed over as a matrix: 0.8 GB)
  static BlockSparse<T>* CreateFromCSC(size_t row, size_t col, int m, int n, int nnz, std::vector<T>&& val, std::vector<int32_t>&& ptr,
                                       std::vector<int32_t>&& ind);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual void row_sums(T* out, T alpha) const;              ///< all rows at once, on all host cores (same sums as row_sum)
  virtual void col_sums(T* out, T alpha) const;
  virtual size_t gpu_mem_amount() const;
  /// MI355X addition (on by default): a matrix whose rows repeat a few (column - row, value) sequences -- a stencil written out as a
  /// sparse matrix -- is applied from one 16-bit pattern number per row + a small table instead of its CSR arrays; same sums, same order
  static void SetPatternCompression(bool on);
  static bool pattern_compression();
  /// which of K / K^T are applied from row patterns (after Initialize()), and how many patterns each has
  bool patterns_forward() const { return side_[0].pat.on; }
  bool patterns_adjoint() const { return side_[1].pat.on; }
  size_t pattern_count(bool adjoint) const { return side_[adjoint].pat.count; }
  /// the matrix IS spmat_gradient2d(nx, ny, L) (matlab/+prost/+test/private/spmat_gradient2d.m:7-14), entry for entry (Initialize())
  virtual bool stencil_shape(BlockDesc& d) const {
    if (!grad_nx_) return false;
    d.kind = BlockDesc::kGradient2D; d.nx = grad_nx_; d.ny = grad_ny_; d.L = grad_L_; d.label_first = false;
    return true;
  }
  static void SetStencilRecognition(bool on);
  virtual bool describe(BlockDesc& d) const;

 protected:
  BlockSparse(size_t row, size_t col, size_t nrows, size_t ncols) : ProductBlock<T>(row, col, nrows, ncols), nnz_(0) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);      ///< one pass either way (no separate zero fill)
  size_t nnz_;
  size_t grad_nx_ = 0, grad_ny_ = 0, grad_L_ = 0;      ///< non-zero: K == spmat_gradient2d(grad_nx_, grad_ny_, grad_L_)
  void DetectGradient2D();
  size_t pointwise_planes_ = 0;                        ///< non-zero: row i has its entries at columns i + c nrows, c < pointwise_planes_ (Initialize())
  void DetectPointwise();
  struct RowPatterns {
    bool on = false;
    size_t count = 0;
    device_vector<uint16_t> ids;              ///< pattern number of every row
    device_vector<int32_t> pptr, rel;         ///< entries pptr[id] .. pptr[id + 1] - 1 of the table: column - row ...
    device_vector<T> val;                     ///< ... and value
    device_vector<int32_t> anchor;            ///< anchored table (matrices between different geometries): offsets count from anchor[row]; empty: from the row number
  };
  /// a side that runs from row patterns keeps its CSR arrays on the host
  struct Side : CsrSide<T> { RowPatterns pat; };
  Side side_[2];                              ///< K and K^T
  void PatternProduct(const Side& s, T* r, const T* x, int acc);
};

/// kron(K, I_d) (id_first == false, block_sparse_kron_id.cu) or kron(I_d, K) (id_first == true,
/// block_id_kron_sparse.cu) for a small sparse K, without forming the product; values kept as float
template <typename T>
class BlockKronSparse : public ProductBlock<T> {
 public:
  static BlockKronSparse<T>* CreateFromCSC(bool id_first, size_t row, size_t col, size_t diaglength, int m, int n, int nnz,
                                           const std::vector<T>& val, const std::vector<int32_t>& ptr, const std::vector<int32_t>& ind);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual size_t gpu_mem_amount() const;

 protected:
  BlockKronSparse(size_t row, size_t col, size_t nrows, size_t ncols) : ProductBlock<T>(row, col, nrows, ncols) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);      ///< no fill pass in front of the product
  bool id_first_ = false;
  size_t diaglength_ = 0, mat_nnz_ = 0;
  CsrSide<float> side_[2];      ///< K (mat_nrows rows) and K^T (mat_ncols rows); each side's column count is the other's row count
};

/// general dense block, K column-major of type T (block_dense.hpp); the products are hand-written kernels instead of gemv calls and
/// repeat their result bit for bit from call to call
template <typename T>
class BlockDense : public ProductBlock<T> {
 public:
  static BlockDense<T>* CreateFromColFirstData(size_t row, size_t col, size_t nrows, size_t ncols, const std::vector<T>& data);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual size_t gpu_mem_amount() const;

 protected:
  BlockDense(size_t row, size_t col, size_t nrows, size_t ncols) : ProductBlock<T>(row, col, nrows, ncols) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  std::vector<T> host_data_;
  device_vector<T> data_;
  device_vector<double> workspace_;      ///< partial sums of a split product (prost_hip_dense_gemv_workspace_bytes)
};

/// kron(K, I_d) (id_first == false, block_dense_kron_id.cu) or kron(I_d, K) (id_first == true, block_id_kron_dense.cu) for a small
/// dense K, column-major, values of type T (the sparse Kronecker blocks keep float), without forming the product
template <typename T>
class BlockKronDense : public ProductBlock<T> {
 public:
  static BlockKronDense<T>* CreateFromColFirstData(bool id_first, size_t diaglength, size_t row, size_t col, size_t nrows, size_t ncols,
                                                   const std::vector<T>& data);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual size_t gpu_mem_amount() const;

 protected:
  BlockKronDense(size_t row, size_t col, size_t nrows, size_t ncols) : ProductBlock<T>(row, col, nrows, ncols) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  bool id_first_ = false;
  size_t diaglength_ = 0, mat_nrows_ = 0, mat_ncols_ = 0;
  std::vector<T> host_data_;
  device_vector<T> data_;
};

/// the coupling of the sublabel-accurate data term (Moellenhoff et al., CVPR 2016; the reference's CustomSources.cmake.example names
/// block_dataterm_sublabel and ships no source): L equidistant labels on [left, right], k = L - 1 intervals, N = nx ny pixels, domain
/// [u ; w] and range [r ; s] of 2 N k values each in planes of N (element (p, i) at i N + p), applied without a matrix.  Arithmetic:
/// prost/linop/dataterm_sublabel.hpp.  No describe(): the block runs on the generic paths.
template <typename T>
class BlockDatatermSublabel : public ProductBlock<T> {
 public:
  /// checks every argument (messages start with "BlockDatatermSublabel: "); declared_rows / declared_cols < 0: no size was declared
  static BlockDatatermSublabel<T>* Create(size_t row, size_t col, double nx, double ny, double L, double left, double right,
                                          double declared_rows = -1, double declared_cols = -1);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual void row_sums(T* out, T alpha) const;              ///< one constant per plane
  virtual void col_sums(T* out, T alpha) const;
  virtual size_t gpu_mem_amount() const { return gamma_.size() * sizeof(T); }
  size_t npixels() const { return npixels_; }
  size_t labels() const { return L_; }
  T delta() const { return delta_; }
  const std::vector<T>& gamma() const { return gamma_; }

 protected:
  BlockDatatermSublabel(size_t row, size_t col, size_t npixels, size_t L, double left, double right);
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  size_t npixels_, L_;
  T delta_;
  std::vector<T> gamma_;          ///< gamma_i = left + i delta, i < L - 1 (formed in double, rounded to T)
  device_vector<T> d_gamma_;
};

/// one small window applied at every pixel of L column-major image planes of ny x nx, zero padding, shape "full" / "same" / "valid",
/// without a matrix: the blur operator of a deblurring problem (the reference's example hands kron(speye(nc), convmtx2(..)) over as
/// a sparse matrix).  L my mx rows by L ny nx columns.  Arithmetic: prost/linop/conv2d.hpp.  No describe(): the block runs on the
/// generic paths.  Only O(taps) data is stored: one tap table per direction.
template <typename T>
class BlockConv2D : public ProductBlock<T> {
 public:
  /// checks every argument (messages start with "BlockConv2D: "); kernel: ky x kx, column-major; declared_rows / declared_cols < 0:
  /// no size was declared
  static BlockConv2D<T>* Create(size_t row, size_t col, double nx, double ny, double L, const std::vector<double>& kernel, size_t ky, size_t kx,
                                const std::string& shape, double declared_rows = -1, double declared_cols = -1);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual void row_sums(T* out, T alpha) const;              ///< O(rows + taps (ky + kx)): one table of rectangle sums per call
  virtual void col_sums(T* out, T alpha) const;
  virtual size_t gpu_mem_amount() const { return (words_[0].size() + words_[1].size()) * sizeof(int32_t); }
  size_t taps() const { return ntaps_; }

 protected:
  BlockConv2D(size_t row, size_t col, size_t nrows, size_t ncols) : ProductBlock<T>(row, col, nrows, ncols) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  conv2d::Geometry geometry_[2];           ///< the forward [0] and the adjoint [1] direction
  std::vector<T> window_[2];               ///< the window rounded to T, and flipped in both axes
  std::vector<int32_t> words_[2];          ///< the tap tables (conv2d::Tap<T> records) as they are uploaded
  size_t ntaps_ = 0;
  device_vector<int32_t> d_taps_[2];
};

/// blur, then keep every s-th pixel, K = S B, without a matrix: the operator of super-resolution, and its adjoint, the fractionally
/// strided convolution.  The window, the planes and the shape are those of BlockConv2D; stride (sy, sx), 1 .. 4 each, and phase
/// (py, px) pick the results that are kept.  L my mx rows by L ny nx columns.  Arithmetic, tile table and table layout:
/// prost/linop/conv2d_strided.hpp.  No describe(): the block runs on the generic paths.  Only O(taps) data is stored.
template <typename T>
class BlockConv2DStrided : public ProductBlock<T> {
 public:
  /// checks every argument (messages start with "BlockConv2DStrided: "); kernel: ky x kx, column-major; declared_rows /
  /// declared_cols < 0: no size was declared
  static BlockConv2DStrided<T>* Create(size_t row, size_t col, double nx, double ny, double L, const std::vector<double>& kernel, size_t ky, size_t kx,
                                       const std::string& shape, double sy, double sx, double py, double px, double declared_rows = -1, double declared_cols = -1);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual void row_sums(T* out, T alpha) const;              ///< one table of class sums per call, one look-up per pixel
  virtual void col_sums(T* out, T alpha) const;
  virtual size_t gpu_mem_amount() const { return (words_[0].size() + words_[1].size()) * sizeof(int32_t); }
  size_t taps() const { return ntaps_; }

 protected:
  BlockConv2DStrided(size_t row, size_t col, size_t nrows, size_t ncols) : ProductBlock<T>(row, col, nrows, ncols) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  conv2d_strided::Geometry geometry_[2];   ///< the forward [0] and the adjoint [1] direction
  std::vector<T> window_;                  ///< the window rounded to T
  std::vector<int32_t> words_[2];          ///< the tap tables (conv2d::Tap<T> records) as they are uploaded
  size_t ntaps_ = 0;
  device_vector<int32_t> d_taps_[2];
};

/// the parallel-beam projector of tomography (Joseph's method) and its exact transpose, without a matrix: L column-major planes of
/// ny x nx onto L sinograms of na angles x ndet bins.  L na ndet rows by L ny nx columns.  Geometry, per-angle table, arithmetic and the
/// candidate window of the adjoint: prost/linop/radon2d.hpp.  No describe(): the block runs on the generic paths.  Only the table,
/// five numbers per angle, is stored.
template <typename T>
class BlockRadon2D : public ProductBlock<T> {
 public:
  /// checks every argument (messages start with "BlockRadon2D: "); ndet < 0 (or NaN): the default detector length; declared_rows /
  /// declared_cols < 0: no size was declared
  static BlockRadon2D<T>* Create(size_t row, size_t col, double nx, double ny, double L, const std::vector<double>& angles, double ndet, double spacing, double shift,
                                 double declared_rows = -1, double declared_cols = -1);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual void row_sums(T* out, T alpha) const;              ///< one plane enumerated once on several host threads, then repeated for every plane
  virtual void col_sums(T* out, T alpha) const;
  virtual size_t gpu_mem_amount() const { return table_.size() * sizeof(T); }
  const radon2d::Geometry& geometry() const { return geometry_; }

 protected:
  BlockRadon2D(size_t row, size_t col, size_t nrows, size_t ncols) : ProductBlock<T>(row, col, nrows, ncols) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  radon2d::Geometry geometry_;
  std::vector<T> table_;                   ///< the per-angle table as it is uploaded
  device_vector<T> d_table_;
};

/// the fan-beam projector of tomography (a point source, a flat or an equiangular detector; Joseph's method) and its exact transpose,
/// without a matrix: L column-major planes of ny x nx onto L sinograms of na views x ndet bins.  L na ndet rows by L ny nx columns.
/// Geometry, tables, arithmetic and the candidate window of the adjoint: prost/linop/fanbeam2d.hpp.  No describe(): the block runs on
/// the generic paths.  Only the tables, five numbers per view, two per bin and ten more, are stored.
template <typename T>
class BlockFanbeam2D : public ProductBlock<T> {
 public:
  /// checks every argument (messages start with "BlockFanbeam2D: "); declared_rows / declared_cols < 0: no size was declared
  static BlockFanbeam2D<T>* Create(size_t row, size_t col, double nx, double ny, double L, const std::vector<double>& angles, double source_distance,
                                   double detector_distance, double ndet, double spacing, double shift, const std::string& detector, double declared_rows = -1,
                                   double declared_cols = -1);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual void row_sums(T* out, T alpha) const;              ///< one plane enumerated once on several host threads, then repeated for every plane
  virtual void col_sums(T* out, T alpha) const;
  virtual size_t gpu_mem_amount() const { return table_.size() * sizeof(T); }
  const fanbeam2d::Geometry& geometry() const { return geometry_; }

 protected:
  BlockFanbeam2D(size_t row, size_t col, size_t nrows, size_t ncols) : ProductBlock<T>(row, col, nrows, ncols) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  fanbeam2d::Geometry geometry_;
  std::vector<T> table_;                   ///< the three tables as they are uploaded
  device_vector<T> d_table_;
};

/// bilinear resampling of L column-major planes of ny x nx at M positions (a warp by a flow field, a rotation or zoom, scattered
/// samples; zero padding) and its exact transpose, without a matrix.  L M rows by L ny nx columns.  Arithmetic, order of operations and
/// the bucket tables of the adjoint: prost/linop/sample2d.hpp.  No describe(): the block runs on the generic paths.  Stored on the
/// device: the 2 M positions in T, M int32 sample indices sorted by cell and (ny + 1)(nx + 1) + 1 int32 cell offsets -- not O(1) per
/// row as BlockRadon2D, but about a quarter of the two sides of the sparse matrix it stands for.
template <typename T>
class BlockSample2D : public ProductBlock<T> {
 public:
  /// checks every argument (messages start with "BlockSample2D: "); declared_rows / declared_cols < 0: no size was declared
  static BlockSample2D<T>* Create(size_t row, size_t col, double nx, double ny, double L, const std::vector<double>& x, const std::vector<double>& y,
                                  double declared_rows = -1, double declared_cols = -1);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual void row_sums(T* out, T alpha) const;
  virtual void col_sums(T* out, T alpha) const;
  virtual size_t gpu_mem_amount() const { return (pos_x_.size() + pos_y_.size()) * sizeof(T) + (order_.size() + cell_start_.size()) * sizeof(int32_t); }
  const sample2d::Geometry& geometry() const { return geometry_; }

 protected:
  BlockSample2D(size_t row, size_t col, size_t nrows, size_t ncols) : ProductBlock<T>(row, col, nrows, ncols) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  sample2d::Geometry geometry_;
  std::vector<T> pos_x_, pos_y_;           ///< the positions rounded once to T
  std::vector<int32_t> order_, cell_start_;  ///< sample2d::MakeBuckets
  device_vector<T> d_pos_x_, d_pos_y_;
  device_vector<int32_t> d_order_, d_cell_start_;
};

/// the unitary 2-D discrete Fourier transform of L complex images of ny x nx (2 L real planes, real parts first) and its transpose, the
/// unitary inverse transform, without a matrix: the operator of k-space data terms (MRI).  2 L N rows by 2 L N columns, N = nx ny, nx
/// and ny powers of two up to 2048.  Arithmetic, order of operations, twiddle table and the closed-form sums: prost/linop/fft2d.hpp.
/// No describe(): the block runs on the generic paths.  Stored on the device: the table (2 max(nx, ny) values) and one work buffer of
/// 2 L N values between the two passes.
template <typename T>
class BlockFFT2D : public ProductBlock<T> {
 public:
  /// checks every argument (messages start with "BlockFFT2D: "); declared_rows / declared_cols < 0: no size was declared
  static BlockFFT2D<T>* Create(size_t row, size_t col, double nx, double ny, double L, double declared_rows = -1, double declared_cols = -1);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const { return row_sum(col, alpha); }      ///< the matrix is symmetric in (frequency, pixel)
  virtual void row_sums(T* out, T alpha) const;              ///< one table of at most 12 class sums per call, one look-up per row
  virtual void col_sums(T* out, T alpha) const { row_sums(out, alpha); }
  virtual size_t gpu_mem_amount() const { return (table_.size() + this->nrows()) * sizeof(T); }
  const fft2d::Geometry& geometry() const { return geometry_; }

 protected:
  BlockFFT2D(size_t row, size_t col, size_t nrows, size_t ncols) : ProductBlock<T>(row, col, nrows, ncols) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  fft2d::Geometry geometry_;
  std::vector<T> table_;                   ///< fft2d::MakeTable
  double sums1_[fft2d::kMaxLog2 + 1];      ///< fft2d::SumTable at alpha = 1, made at creation: what row-by-row callers of row_sum ask for
  device_vector<T> d_table_, d_work_;
};

/// the multi-coil Fourier operator of SENSE-type parallel MRI, K u = [ F (sigma_c . u) ]_c, and its transpose, without a matrix: L complex
/// images of ny x nx (the domain of BlockFFT2D with L images) onto L C k-space images (the range of BlockFFT2D with L C images, image
/// l C + c is coil c of image l), with C = 1 .. 64 complex sensitivity maps shared by the images.  2 L C N rows by 2 L N columns, N = nx ny.
/// Arithmetic, order of the coil sum, error bound and why the sums are bounds, not the matrix's sums: prost/linop/sense2d.hpp.  No
/// describe(): the block runs on the generic paths.  Stored on the device: the maps (2 C N values), BlockFFT2D's table and one work buffer
/// of 2 L C N values between the two passes.
template <typename T>
class BlockSense2D : public ProductBlock<T> {
 public:
  /// checks every argument (messages start with "BlockSense2D: "); maps: 2 C nx ny values, the C real planes first, then the C imaginary
  /// planes; declared_rows / declared_cols < 0: no size was declared
  static BlockSense2D<T>* Create(size_t row, size_t col, double nx, double ny, double L, double C, const std::vector<double>& maps, double declared_rows = -1,
                                 double declared_cols = -1);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;              ///< the bound Rbar_c of sense2d.hpp: a look-up while alpha stays the one asked last, else O(C N) once
  virtual T col_sum(size_t col, T alpha) const;              ///< the bound Cbar(p): O(C) per call
  virtual void row_sums(T* out, T alpha) const;              ///< C bounds, each added to the 2 L planes of its coil
  virtual void col_sums(T* out, T alpha) const;              ///< one pass over the pixels
  virtual size_t gpu_mem_amount() const { return (table_.size() + maps_.size() + this->nrows()) * sizeof(T); }
  const sense2d::Geometry& geometry() const { return geometry_; }

 protected:
  BlockSense2D(size_t row, size_t col, size_t nrows, size_t ncols) : ProductBlock<T>(row, col, nrows, ncols) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  sense2d::Geometry geometry_;
  std::vector<T> table_;                   ///< fft2d::MakeTable
  std::vector<T> maps_;                    ///< rounded once to T
  /// sense2d::RowBound of coil c: the C bounds of the alpha asked last are kept (alpha = 1 from creation), since row-by-row callers of
  /// row_sum ask every row for the same alpha and one bound costs a pass over a map
  double RowBoundOf(double alpha, size_t c) const;
  mutable std::mutex rows_lock_;
  mutable double rows_alpha_ = 1;
  mutable std::vector<double> rows_;
  device_vector<T> d_table_, d_maps_, d_work_;
};

/// the orthogonal, periodised, separable multi-level wavelet transform of L planes of ny x nx and its transpose, the inverse transform,
/// without a matrix: the operator of wavelet sparsity priors.  L N rows by L N columns, N = nx ny.  Arithmetic, order of operations,
/// limits and the sums: prost/linop/wavelet2d.hpp.  No describe(): the block runs on the generic paths.  Stored on the device: one work
/// buffer of wavelet2d::WorkSize values (5/16 L N in 2-D) for the low-low corners between the levels; the taps travel with each launch.
template <typename T>
class BlockWavelet2D : public ProductBlock<T> {
 public:
  /// checks every argument (messages start with "BlockWavelet2D: "); declared_rows / declared_cols < 0: no size was declared
  static BlockWavelet2D<T>* Create(size_t row, size_t col, double nx, double ny, double L, const std::vector<double>& taps, double levels,
                                   double declared_rows = -1, double declared_cols = -1);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual void row_sums(T* out, T alpha) const;
  virtual void col_sums(T* out, T alpha) const;
  virtual size_t gpu_mem_amount() const { return wavelet2d::WorkSize(geometry_) * sizeof(T); }
  const wavelet2d::Geometry& geometry() const { return geometry_; }

 protected:
  BlockWavelet2D(size_t row, size_t col, size_t nrows, size_t ncols) : ProductBlock<T>(row, col, nrows, ncols) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  void Tables(double alpha) const;         ///< the 1-D tables of both axes for this alpha, kept until another alpha is asked for
  wavelet2d::Geometry geometry_;
  std::vector<double> taps64_;             ///< the taps as given
  std::vector<T> taps_;                    ///< rounded once to T
  mutable double tables_alpha_ = -1;
  mutable wavelet2d::AxisSums tables_y_, tables_x_;
  device_vector<T> d_work_;
};

/// the symmetrised gradient of a vector field on L channels of an ny x nx grid, without a matrix: the second-order operator of TGV^2
/// (K = [grad -I ; 0 E]).  3 L N rows (exx, eyy, exy planes) by 2 L N columns (vx, vy planes, the range layout of gradient2d), backward
/// differences with the boundary handling of the divergence, the mixed rows weighted by w.  Arithmetic: prost/linop/sym_gradient2d.hpp.
/// No describe(): the block runs on the generic paths.  Nothing is stored on the device.
template <typename T>
class BlockSymGradient2D : public ProductBlock<T> {
 public:
  /// checks every argument (messages start with "BlockSymGradient2D: "); declared_rows / declared_cols < 0: no size was declared
  static BlockSymGradient2D<T>* Create(size_t row, size_t col, double nx, double ny, double L, double w, double declared_rows = -1, double declared_cols = -1);
  virtual void Initialize() {}
  virtual void Release() {}
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual void row_sums(T* out, T alpha) const;              ///< closed forms, one pass over the rows
  virtual void col_sums(T* out, T alpha) const;
  virtual size_t gpu_mem_amount() const { return 0; }

 protected:
  BlockSymGradient2D(size_t row, size_t col, size_t nx, size_t ny, size_t L, double w)
      : ProductBlock<T>(row, col, 3 * L * nx * ny, 2 * L * nx * ny), nx_(nx), ny_(ny), L_(L), w_(w) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  double WeightPower(T alpha) const { return sym_gradient2d::WeightPower((double)sym_gradient2d::RoundWeight<T>(w_), (double)alpha); }
  size_t nx_, ny_, L_;
  double w_;               ///< as given; the kernels and the sums round it to T once
};

/// K = T grad on L channels of an ny x nx grid, without a matrix: the gradient weighted per pixel by a scalar (mode 1, edge-weighted TV),
/// by one weight per axis (mode 2) or by a symmetric 2 x 2 tensor (mode 3, the diffusion tensor of anisotropic Huber-L1 and TGV).  2 L N
/// rows (gx, gy planes, the range layout of gradient2d) by L N columns.  Arithmetic, sums and error bound:
/// prost/linop/tensor_gradient2d.hpp.  No describe(): the block runs on the generic paths.  Stored on the device: the `mode` planes of
/// the tensor, N values each, shared by all channels.
template <typename T>
class BlockTensorGradient2D : public ProductBlock<T> {
 public:
  /// checks every argument (messages start with "BlockTensorGradient2D: "); tensor: mode planes of nx ny values one after the other;
  /// declared_rows / declared_cols < 0: no size was declared
  static BlockTensorGradient2D<T>* Create(size_t row, size_t col, double nx, double ny, double L, double mode, const std::vector<double>& tensor,
                                          double declared_rows = -1, double declared_cols = -1);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual void row_sums(T* out, T alpha) const;              ///< one pass over the pixels
  virtual void col_sums(T* out, T alpha) const;
  virtual size_t gpu_mem_amount() const { return tensor_.size() * sizeof(T); }

 protected:
  BlockTensorGradient2D(size_t row, size_t col, size_t nx, size_t ny, size_t L, int mode)
      : ProductBlock<T>(row, col, 2 * L * nx * ny, L * nx * ny), nx_(nx), ny_(ny), L_(L), mode_(mode) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  size_t nx_, ny_, L_;
  int mode_;
  std::vector<T> tensor_;          ///< rounded once to T
  device_vector<T> d_tensor_;
};

/// the nonlocal gradient (K u)_m[p] = w_m(p) (u[p + d_m] - u[p]) on L channels of an ny x nx grid, without a matrix: M displacements
/// inside a window of reach 15 and one weight plane per displacement, shared by all channels (nonlocal TV, nonlocal Huber / TV-L1).
/// M L N rows (plane (m, c) at (m L + c) N) by L N columns.  Arithmetic, sums and error bound: prost/linop/nonlocal_gradient2d.hpp.  No
/// describe(): the block runs on the generic paths.  Stored on the device: the M weight planes, N values each; the displacements
/// travel with every launch.
template <typename T>
class BlockNonlocalGradient2D : public ProductBlock<T> {
 public:
  /// checks every argument (messages start with "BlockNonlocalGradient2D: "); offsets: M pairs (dy, dx) one after the other; weights: M
  /// planes of nx ny values one after the other; declared_rows / declared_cols < 0: no size was declared
  static BlockNonlocalGradient2D<T>* Create(size_t row, size_t col, double nx, double ny, double L, const std::vector<double>& offsets,
                                            const std::vector<double>& weights, double declared_rows = -1, double declared_cols = -1);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual void row_sums(T* out, T alpha) const;              ///< one pass over the pixels
  virtual void col_sums(T* out, T alpha) const;
  virtual size_t gpu_mem_amount() const { return weights_.size() * sizeof(T); }

 protected:
  BlockNonlocalGradient2D(size_t row, size_t col, size_t nx, size_t ny, size_t L, int M)
      : ProductBlock<T>(row, col, (size_t)M * L * nx * ny, L * nx * ny), nx_(nx), ny_(ny), L_(L), M_(M) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  size_t nx_, ny_, L_;
  int M_;
  nonlocal_gradient2d::Offsets offsets_;
  std::vector<signed char> pairs_;  ///< (dy, dx) pairs as the entry points take them
  std::vector<T> weights_;          ///< rounded once to T
  device_vector<T> d_weights_;
};

/// the second-order differences H = E grad (u_xx, u_yy, u_xy) of L channels of an ny x nx grid, without a matrix and without the
/// intermediate field: the operator of TV^2 and of the Hessian-Schatten norms.  components = 3: 3 L N rows (hxx, hyy, hxy planes, the
/// range layout of sym_gradient2d); components = 4: 4 L N rows (hxx, hxy, hxy, hyy, the column-major symmetric 2 x 2 matrix); L N
/// columns.  The bits are those of gradient2d and sym_gradient2d chained.  Arithmetic, sums and error bound: prost/linop/hessian2d.hpp.
/// No describe(): the block runs on the generic paths.  Nothing is stored on the device.
template <typename T>
class BlockHessian2D : public ProductBlock<T> {
 public:
  /// checks every argument (messages start with "BlockHessian2D: "); declared_rows / declared_cols < 0: no size was declared
  static BlockHessian2D<T>* Create(size_t row, size_t col, double nx, double ny, double L, double w, double components, double declared_rows = -1,
                                   double declared_cols = -1);
  virtual void Initialize() {}
  virtual void Release() {}
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual void row_sums(T* out, T alpha) const;              ///< closed forms, one pass over the pixels
  virtual void col_sums(T* out, T alpha) const;
  virtual size_t gpu_mem_amount() const { return 0; }

 protected:
  BlockHessian2D(size_t row, size_t col, size_t nx, size_t ny, size_t L, double w, int components)
      : ProductBlock<T>(row, col, (size_t)components * L * nx * ny, L * nx * ny), nx_(nx), ny_(ny), L_(L), w_(w), components_(components) {}
  virtual void Product(T* res, const T* rhs, bool transpose, bool accumulate);
  double WeightPower(T alpha) const { return hessian2d::WeightPower((double)hessian2d::RoundWeight<T>(w_), (double)alpha); }
  size_t nx_, ny_, L_;
  double w_;               ///< as given; the kernels and the sums round it to T once
  int components_;
};

/// constant-coefficient multi-diagonal block; `identity` maps here (block_diags.hpp, identity.m:11-12)
template <typename T>
class BlockDiags : public Block<T> {
 public:
  BlockDiags(size_t row, size_t col, size_t nrows, size_t ncols, size_t ndiags, const std::vector<int64_t>& offsets,
             const std::vector<T>& factors);
  virtual void Initialize();
  virtual void Release();
  virtual T row_sum(size_t row, T alpha) const;
  virtual T col_sum(size_t col, T alpha) const;
  virtual size_t gpu_mem_amount() const { return ndiags_ * (sizeof(float) + sizeof(int64_t)); }
  /// reproduce the reference's adjoint launch grid sized from nrows (block_diags.cu:211)?
  /// default false: every column is written.
  static void SetReferenceGridQuirk(bool on);
  static bool ReferenceGridQuirk();

 protected:
  virtual void EvalLocalAdd(T*, T*, const T*, const T*);
  virtual void EvalAdjointLocalAdd(T*, T*, const T*, const T*);
  size_t ndiags_;
  std::vector<int64_t> offsets_;
  std::vector<float> factors_;      // float regardless of T (block_diags.cu:30,:108)
  device_vector<int64_t> d_offsets_;
  device_vector<float> d_factors_;
};

template <typename T>
class BlockZero : public Block<T> {
 public:
  BlockZero(size_t row, size_t col, size_t nrows, size_t ncols) : Block<T>(row, col, nrows, ncols) {}
  virtual T row_sum(size_t, T) const { return 0; }
  virtual T col_sum(size_t, T) const { return 0; }
  virtual size_t gpu_mem_amount() const { return 0; }

 protected:
  virtual void EvalLocalAdd(T*, T*, const T*, const T*) {}
  virtual void EvalAdjointLocalAdd(T*, T*, const T*, const T*) {}
};

}  // namespace prost
#endif
