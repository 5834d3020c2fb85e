// prost/prox/proxes.hpp -- in-tree proximal operators of the hot path (reference:
// prox_elem_operation.hpp/.inl + elemop/*, prox_moreau.hpp, prox_zero.hpp, prox_ind_epi_quad.hpp).
#ifndef PROST_PROX_PROXES_HPP_
#define PROST_PROX_PROXES_HPP_
#include <array>

#include "prost/prox/prox_separable_sum.hpp"

namespace prost {

/// The reference instantiates ProxElemOperation<T, ElemOperation1D|Norm2<T, Function1D*>> 176
/// times (prox_elem_operation.cu:44-256); here the elem operation and the scalar function are
/// run-time ids (PROST_OP_*, PROST_FN_* of prost_hip.h) dispatched wave-uniformly in one kernel.
/// (The reference's template itself -- ProxElemOperation<T, ELEM_OPERATION> for user-written
/// operations -- is prost/prox/prox_elem_operation.hpp.)
template <typename T>
class ProxElemDispatch : public ProxSeparableSum<T> {
 public:
  /// op: PROST_OP_1D (dim forced to 1, elem_operation_1d.hpp:30) or PROST_OP_NORM2
  ProxElemDispatch(int op, int fn, size_t index, size_t count, size_t dim, bool interleaved, bool diagsteps,
                    const std::array<std::vector<T>, 7>& coeffs);
  virtual void Initialize();      // uploads per-element coefficient vectors (prox_elem_operation.inl:200-222)
  virtual void Release();
  virtual size_t gpu_mem_amount() const;
  virtual bool describe(ProxDesc& d) const;
  int op() const { return op_; }
  int fn() const { return fn_; }
  /// prox of the conjugate (Moreau) of this elem operation in one fused pass; same ranges as EvalLocal
  void EvalMoreauLocal(T* res, const T* arg, const T* tau_diag, T tau, bool invert_tau);
  virtual bool supports_arg_source() const { return true; }
  virtual bool takes_step_record() const { return true; }
  /// the operator sources run the 16-bytes-per-lane kernel only: planar layout (or the 1-D operation), range and count on 16-byte boundaries
  virtual bool supports_op_source() const;
  virtual void EvalFromSource(device_vector<T>& result, const typename Prox<T>::ArgSource& src, const device_vector<T>& tau_diag, T tau, bool invert_tau = false) {
    EvalSourceLocal(false, result, src, tau_diag, tau, invert_tau);
  }
  /// moreau = true: the conjugate's prox from the source (used by ProxMoreau::EvalFromSource)
  void EvalSourceLocal(bool moreau, device_vector<T>& result, const typename Prox<T>::ArgSource& src, const device_vector<T>& tau_diag, T tau, bool invert_tau);

 protected:
  virtual void EvalLocal(T*, T*, const T*, const T*, const T*, const T*, T tau, bool invert_tau);
  void CoeffArgs(const T* (&ptrs)[7], double (&vals)[7]) const;
  int op_, fn_;
  std::array<std::vector<T>, 7> coeffs_;
  std::array<device_vector<T>, 7> d_coeffs_;
};

/// The spectral family: elem_operation:singular_nx2:* (a function of the two singular values of the n x 2 matrix a group holds,
/// dim = 2 n), elem_operation:eigen_2x2:* and elem_operation:eigen_3x3:* (a function of the eigenvalues of the symmetrised 2x2 / 3x3
/// matrix, dim 4 / 9), elem_operation:eigen_nxn:* (the same for a row-major n x n matrix, dim = n^2, n <= 32; from n = 6 on several lanes
/// share a matrix: prost_amd/csrc/kernels_prox_eigen_nxn.hip) and elem_operation:mass4 / mass5 / ind_comass4_ball / ind_comass5_ball (mass
/// norm of a 2-vector in R^4 / R^5, dim 6 / 10, and the projection onto the ball of its dual norm; coefficient 0 is the cost, the function
/// id is ignored; elem_operation_eigen_nxn.hpp, elem_operation_mass_norm.hpp).  Operation and function are run-time ids (PROST_SPECTRAL_*, PROST_FN_* / PROST_FN2D_* of prost_hip.h) of one
/// kernel family (prost_amd/csrc/kernels_prox_spectral.hip); the arithmetic is prost/prox/elemop/elem_operation_singular_nx2.hpp,
/// _eigen_2x2.hpp, _eigen_3x3.hpp.  A dimension the operation does not take throws at construction.  The kernel reads the step size
/// from device memory when asked to (Prox::StepView), so goldstein / boyd keep their device-resident rule on problems that use it.
template <typename T>
class ProxSpectral : public ProxSeparableSum<T> {
 public:
  ProxSpectral(int op, int fn, size_t index, size_t count, size_t dim, bool interleaved, bool diagsteps, const std::array<std::vector<T>, 7>& coeffs);
  static const char* OperationName(int op);
  virtual void Initialize();      // uploads per-group coefficient vectors
  virtual void Release();
  virtual size_t gpu_mem_amount() const;
  virtual bool takes_step_view() const { return true; }
  int op() const { return op_; }
  int fn() const { return fn_; }

 protected:
  virtual void EvalLocal(T*, T*, const T*, const T*, const T*, const T*, T tau, bool invert_tau);
  virtual void EvalLocalStepView(T*, T*, const T*, const T*, const T*, const T*, const typename Prox<T>::StepView& view, bool invert_tau);
  void Launch(T* res, const T* arg, const T* tau_diag, T tau, const T* step, const int* stop, bool invert_tau);
  int op_, fn_;
  std::array<std::vector<T>, 7> coeffs_;
  std::array<device_vector<T>, 7> d_coeffs_;
};

/// prox of the conjugate via Moreau's identity (prox_moreau.cu:98-134)
template <typename T>
class ProxMoreau : public Prox<T> {
 public:
  /// MI355X addition: a conjugated elem operation runs as ONE kernel (default on)
  static void SetFuseElemOperations(bool on);
  explicit ProxMoreau(shared_ptr<Prox<T>> conjugate) : Prox<T>(*conjugate), conjugate_(conjugate) {}
  virtual void Initialize();
  virtual void Release();
  virtual size_t gpu_mem_amount() const { return this->size_ * sizeof(T) + conjugate_->gpu_mem_amount(); }
  virtual void get_separable_structure(std::vector<std::tuple<size_t, size_t, size_t>>& sep) { conjugate_->get_separable_structure(sep); }
  virtual bool supports_arg_source() const;
  virtual bool takes_step_record() const { return supports_arg_source(); }
  /// true for a conjugated ProxIndEpiConjQuad1D: the inner prox does not depend on the step, the two scaling passes read it on the device
  virtual bool takes_step_view() const;
  virtual bool supports_op_source() const { return supports_arg_source() && conjugate_->supports_op_source(); }
  /// the wrapped operation's description with `moreau` set (a wrap of a wrap is not described)
  virtual bool describe(ProxDesc& d) const;
  virtual void EvalFromSource(device_vector<T>& result, const typename Prox<T>::ArgSource& src, const device_vector<T>& tau_diag, T tau, bool invert_tau = false);
  virtual void average_preconditioner(std::vector<T>& precond) { conjugate_->average_preconditioner(precond); }
  virtual bool average_uniform(T& value) const { return conjugate_->average_uniform(value); }

 protected:
  virtual void EvalLocal(T*, T*, const T*, const T*, const T*, const T*, T tau, bool invert_tau);
  virtual void EvalLocalStepView(T*, T*, const T*, const T*, const T*, const T*, const typename Prox<T>::StepView& view, bool invert_tau);
  shared_ptr<Prox<T>> conjugate_;
  device_vector<T> scaled_arg_;
};

/// identity (prox_zero.cu:37-48)
template <typename T>
class ProxZero : public Prox<T> {
 public:
  ProxZero(size_t index, size_t size) : Prox<T>(index, size, true) {}
  virtual size_t gpu_mem_amount() const { return 0; }
  virtual bool supports_arg_source() const { return true; }
  virtual bool takes_step_record() const { return true; }
  virtual bool supports_op_source() const { const size_t v = 16 / sizeof(T); return this->size_ % v == 0 && this->index_ % v == 0; }
  /// the identity prox of a source IS the argument pass, written straight into the result
  virtual void EvalFromSource(device_vector<T>& result, const typename Prox<T>::ArgSource& src, const device_vector<T>& tau_diag, T tau, bool invert_tau = false);

 protected:
  virtual void EvalLocal(T*, T*, const T*, const T*, const T*, const T*, T tau, bool invert_tau);
};

/// projection onto the epigraph of a |x|^2 + b^T x + c (prox_ind_epi_quad.cu:42-169)
template <typename T>
class ProxIndEpiQuad : public ProxSeparableSum<T> {
 public:
  ProxIndEpiQuad(size_t index, size_t count, size_t dim, bool interleaved, bool diagsteps, const std::vector<T>& a,
                 const std::vector<T>& b, const std::vector<T>& c)
      : ProxSeparableSum<T>(index, count, dim, interleaved, diagsteps), a_(a), b_(b), c_(c) {}
  virtual void Initialize();
  virtual void Release();
  virtual size_t gpu_mem_amount() const { return (a_.size() + b_.size() + c_.size()) * sizeof(T); }

 protected:
  virtual void EvalLocal(T*, T*, const T*, const T*, const T*, const T*, T tau, bool invert_tau);
  std::vector<T> a_, b_, c_;
  device_vector<T> d_a_, d_b_, d_c_;
};

/// elem_operation:ind_sum -- sum-to-one constraint per group (elem_operation_ind_sum.hpp:41-60)
template <typename T>
class ProxElemIndSum : public ProxSeparableSum<T> {
 public:
  ProxElemIndSum(size_t index, size_t count, size_t dim, bool interleaved, bool diagsteps)
      : ProxSeparableSum<T>(index, count, dim, interleaved, diagsteps) {}
  virtual size_t gpu_mem_amount() const { return 0; }

 protected:
  virtual void EvalLocal(T*, T*, const T*, const T*, const T*, const T*, T tau, bool invert_tau);
};

/// elem_operation:ind_simplex -- projection onto the unit simplex per group (elem_operation_ind_simplex.hpp:40-119)
template <typename T>
class ProxElemIndSimplex : public ProxSeparableSum<T> {
 public:
  ProxElemIndSimplex(size_t index, size_t count, size_t dim, bool interleaved, bool diagsteps)
      : ProxSeparableSum<T>(index, count, dim, interleaved, diagsteps) {}
  virtual void Initialize() { work_.resize(this->count_ * this->dim_); }
  virtual void Release() { work_.clear(); }
  virtual size_t gpu_mem_amount() const { return this->count_ * this->dim_ * sizeof(T); }

 protected:
  virtual void EvalLocal(T*, T*, const T*, const T*, const T*, const T*, T tau, bool invert_tau);
  device_vector<T> work_;      // sort workspace, planar like the data
};

/// h(x) = c f(ax - b) + dx + (e/2) x^2 around any inner prox (prox_transform.cu:99-221)
template <typename T>
class ProxTransform : public Prox<T> {
 public:
  ProxTransform(shared_ptr<Prox<T>> inner_fn, const std::vector<T>& a, const std::vector<T>& b, const std::vector<T>& c,
                const std::vector<T>& d, const std::vector<T>& e)
      : Prox<T>(*inner_fn), inner_fn_(inner_fn), host_{a, b, c, d, e} {}
  virtual void Initialize();
  virtual void Release();
  virtual size_t gpu_mem_amount() const;
  virtual void get_separable_structure(std::vector<std::tuple<size_t, size_t, size_t>>& sep) { inner_fn_->get_separable_structure(sep); }
  virtual void average_preconditioner(std::vector<T>& precond) { inner_fn_->average_preconditioner(precond); }
  virtual bool average_uniform(T& value) const { return inner_fn_->average_uniform(value); }

 protected:
  virtual void EvalLocal(T*, T*, const T*, const T*, const T*, const T*, T tau, bool invert_tau);
  shared_ptr<Prox<T>> inner_fn_;
  std::array<std::vector<T>, 5> host_;
  std::array<device_vector<T>, 5> dev_;
  device_vector<T> scaled_arg_, scaled_tau_;
};

/// composition with a permutation of the (local) variable order (prox_permute.cu:50-160)
template <typename T>
class ProxPermute : public Prox<T> {
 public:
  ProxPermute(shared_ptr<Prox<T>> base_prox, const std::vector<int32_t>& perm) : Prox<T>(*base_prox), base_prox_(base_prox), perm_host_(perm) {}
  virtual void Initialize();
  virtual void Release();
  virtual size_t gpu_mem_amount() const { return this->size_ * sizeof(T) + base_prox_->gpu_mem_amount(); }
  virtual void get_separable_structure(std::vector<std::tuple<size_t, size_t, size_t>>& sep) { base_prox_->get_separable_structure(sep); }
  virtual void average_preconditioner(std::vector<T>& precond) { base_prox_->average_preconditioner(precond); }
  virtual bool average_uniform(T& value) const { return base_prox_->average_uniform(value); }

 protected:
  virtual void EvalLocal(T*, T*, const T*, const T*, const T*, const T*, T tau, bool invert_tau);
  shared_ptr<Prox<T>> base_prox_;
  std::vector<int32_t> perm_host_;
  device_vector<int32_t> perm_;
  device_vector<T> permuted_arg_;
};

/// projection onto the halfspaces {x | <a, x> <= b} (prox_ind_halfspace.cu:31-153); planar layout always
template <typename T>
class ProxIndHalfspace : public ProxSeparableSum<T> {
 public:
  ProxIndHalfspace(size_t index, size_t count, size_t dim, bool interleaved, bool diagsteps, const std::vector<T>& a, const std::vector<T>& b)
      : ProxSeparableSum<T>(index, count, dim, interleaved, diagsteps), a_(a), b_(b) {}
  virtual void Initialize();
  virtual void Release() { d_a_.clear(); d_b_.clear(); }
  virtual size_t gpu_mem_amount() const { return (a_.size() + b_.size()) * sizeof(T); }

 protected:
  virtual void EvalLocal(T*, T*, const T*, const T*, const T*, const T*, T tau, bool invert_tau);
  std::vector<T> a_, b_;
  device_vector<T> d_a_, d_b_;
};

/// projection onto the second-order cone alpha ||x|| <= y, alpha == 1 only (prox_ind_soc.cu:30-124)
template <typename T>
class ProxIndSOC : public ProxSeparableSum<T> {
 public:
  ProxIndSOC(size_t index, size_t count, size_t dim, bool interleaved, bool diagsteps, T alpha)
      : ProxSeparableSum<T>(index, count, dim, interleaved, diagsteps), alpha_(alpha) {}
  virtual void Initialize();
  virtual size_t gpu_mem_amount() const { return 0; }

 protected:
  virtual void EvalLocal(T*, T*, const T*, const T*, const T*, const T*, T tau, bool invert_tau);
  T alpha_;
};

/// sum constraints over one or two index families, identity elsewhere (prox_ind_sum.cu:30-147)
template <typename T>
class ProxIndSum : public Prox<T> {
 public:
  ProxIndSum(size_t index, size_t size, size_t count, size_t dim, const std::vector<uint64_t>& inds, T sum)
      : Prox<T>(index, size, true), dim_(dim), dim_2_(0), count_(count), count_2_(0), inds_(inds), two_(false), sum_(sum), sum_2_(0) {}
  ProxIndSum(size_t index, size_t size, size_t count, size_t dim, const std::vector<uint64_t>& inds, T sum, size_t count2, size_t dim2,
             const std::vector<uint64_t>& inds2, T sum2)
      : Prox<T>(index, size, true), dim_(dim), dim_2_(dim2), count_(count), count_2_(count2), inds_(inds), inds_2_(inds2), two_(true),
        sum_(sum), sum_2_(sum2) {}
  virtual void Initialize();
  virtual void Release() { d_inds_.clear(); d_inds_2_.clear(); }
  virtual size_t gpu_mem_amount() const { return inds_.size() * sizeof(uint64_t); }

 protected:
  virtual void EvalLocal(T*, T*, const T*, const T*, const T*, const T*, T tau, bool invert_tau);
  size_t dim_, dim_2_, count_, count_2_;
  std::vector<uint64_t> inds_, inds_2_;
  device_vector<int64_t> d_inds_, d_inds_2_;
  bool two_;
  T sum_, sum_2_;
};

/// projection onto the range of a sparse m x n matrix A with full column rank: x = A (A'A)^-1 A' y (prox_ind_range.cu).  The reference
/// calls cuSPARSE and cuSOLVER (potrf at Initialize, potrs per evaluation); here the two products are prost_hip_csr_spmv_* on the stored
/// transpose and on A, and the dense solve is prost_amd/csrc/kernels_prox_range.hip: a blocked Cholesky factorisation at Initialize (a
/// pivot that is not positive throws there -- the reference ignores cuSOLVER's info), two blocked triangular sweeps per evaluation.
/// The prox of an indicator does not depend on the step: tau, tau_diag and invert_tau are ignored.
template <typename T>
class ProxIndRange : public Prox<T> {
 public:
  ProxIndRange(size_t index, size_t size) : Prox<T>(index, size, false), nrows_(0), ncols_(0), nnz_(0), ready_(false) {}
  /// A (m x n) in CSC, as the front end delivers it
  void setA(int m, int n, int nnz, const std::vector<T>& val, const std::vector<int32_t>& ptr, const std::vector<int32_t>& ind);
  /// AA = A'A, column-major; call after setA
  void setAA(int m, int n, const std::vector<T>& val);
  virtual void Initialize();
  virtual void Release();
  virtual size_t gpu_mem_amount() const;

 protected:
  virtual void EvalLocal(T*, T*, const T*, const T*, const T*, const T*, T tau, bool invert_tau);
  size_t nrows_, ncols_, nnz_;
  bool ready_;
  std::vector<T> host_val_, host_val_t_, host_AA_;
  std::vector<int32_t> host_ind_, host_ptr_, host_ind_t_, host_ptr_t_;
  device_vector<T> val_, val_t_, L_, U_, dinv_, temp_;
  device_vector<int32_t> ind_, ptr_, ind_t_, ptr_t_;
  device_vector<double> workspace_;      // (bytes of prost_hip_range_potrs_workspace_bytes_*, rounded up to doubles)
};

/// projection onto the epigraphs of max-affine functions, { (x, y) | y >= max_i <a_i, x> - b_i } per group of dim = d + 1 values
/// (x_1 .. x_d, y): the function behind prost.function.sum_ind_epi_polyhedral, which the reference's users add from outside its tree.
/// Group g owns the count_vec[g] constraints that start at index_vec[g] (0-based, counted in constraints; lists may be shared, the
/// starts need not be monotone); the d coefficients of one constraint are adjacent in a.  2 <= dim <= 4.  Every argument is checked
/// at construction (messages name the prox).  The kernel (prost_amd/csrc/kernels_prox_epi_polyhedral.hip, arithmetic in
/// prost/prox/epi_polyhedral.hpp) is a dual active-set projection with a hard step cap; fallback_count() reads back how many groups
/// reached it since Initialize.  The prox of an indicator does not depend on the step: tau, tau_diag and invert_tau are ignored.
template <typename T>
class ProxIndEpiPolyhedral : public ProxSeparableSum<T> {
 public:
  ProxIndEpiPolyhedral(size_t index, size_t count, size_t dim, bool interleaved, const std::vector<T>& a, const std::vector<T>& b,
                       const std::vector<double>& count_vec, const std::vector<double>& index_vec);
  virtual void Initialize();
  virtual void Release();
  virtual size_t gpu_mem_amount() const { return (a_.size() + b_.size()) * sizeof(T) + (cnt_.size() + idx_.size() + 1) * sizeof(int32_t); }
  size_t max_count() const { return max_count_; }
  /// groups that reached the step cap since Initialize (synchronous read-back)
  size_t fallback_count() const;

 protected:
  virtual void EvalLocal(T*, T*, const T*, const T*, const T*, const T*, T tau, bool invert_tau);
  std::vector<T> a_, b_;
  std::vector<int32_t> cnt_, idx_;
  size_t max_count_;
  bool ready_;
  device_vector<T> d_a_, d_b_;
  device_vector<int32_t> d_cnt_, d_idx_, d_fallback_;
};

/// projection onto the epigraphs of conjugate quadratic pieces, { (y, t) | t >= phi*(y) } per group of dim = 2 values (y, t), with
/// phi(x) = a x^2 + b x + c on [alpha, beta] and +inf elsewhere: the function behind prost.function.sum_ind_epi_conjquad_1d (the
/// sublabel-accurate relaxation with piecewise quadratic data terms), which the reference's users add from outside its tree.  Each
/// coefficient holds 1 or count values.  a >= 0, alpha <= beta, everything finite but alpha = -inf / beta = +inf with a > 0 (that ray
/// is absent); checked at construction (messages name the prox).  The kernel (prost_amd/csrc/kernels_prox_epi_conjquad.hip, arithmetic
/// in prost/prox/epi_conjquad.hpp) runs a Newton loop with a hard step cap in the arc region; fallback_count() reads back how many
/// groups reached it since Initialize.  The prox of an indicator does not depend on the step: tau, tau_diag and invert_tau are
/// ignored, and under a device-resident step-size rule (Prox::StepView) only the stop word is read.
template <typename T>
class ProxIndEpiConjQuad1D : public ProxSeparableSum<T> {
 public:
  ProxIndEpiConjQuad1D(size_t index, size_t size, size_t count, bool interleaved, const std::array<std::vector<T>, 5>& coeffs);
  virtual void Initialize();
  virtual void Release();
  virtual size_t gpu_mem_amount() const;
  virtual bool takes_step_view() const { return true; }
  /// groups that reached the step cap since Initialize (synchronous read-back)
  size_t fallback_count() const;

 protected:
  virtual void EvalLocal(T*, T*, const T*, const T*, const T*, const T*, T tau, bool invert_tau);
  virtual void EvalLocalStepView(T*, T*, const T*, const T*, const T*, const T*, const typename Prox<T>::StepView& view, bool invert_tau);
  void Launch(T* res, const T* arg, const int* stop);
  std::array<std::vector<T>, 5> coeffs_;       // a, b, c, alpha, beta
  std::array<device_vector<T>, 5> d_coeffs_;
  device_vector<int32_t> d_fallback_;
  bool ready_;
};

}  // namespace prost
#endif
