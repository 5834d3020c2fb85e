// prox.cpp -- proximal operators of the prost host library (calls prost_hip.h only).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>
#include <sstream>

#include "hipapi.hpp"
#include "prost/prox/proxes.hpp"

namespace prost {

template <typename T>
void Prox<T>::Eval(device_vector<T>& result, const device_vector<T>& arg, const device_vector<T>& tau_diag, T tau, bool invert_tau) {
  EvalLocal(result.data() + index_, result.data() + index_ + size_, arg.data() + index_, arg.data() + index_ + size_,
            tau_diag.data() + index_, tau_diag.data() + index_ + size_, tau, invert_tau);
}
template <typename T>
void Prox<T>::EvalWithStepView(device_vector<T>& result, const device_vector<T>& arg, const device_vector<T>& tau_diag, const StepView& view, bool invert_tau) {
  EvalLocalStepView(result.data() + index_, result.data() + index_ + size_, arg.data() + index_, arg.data() + index_ + size_,
                    tau_diag.data() + index_, tau_diag.data() + index_ + size_, view, invert_tau);
}
template <typename T>
double Prox<T>::Eval(std::vector<T>& result, const std::vector<T>& arg, const std::vector<T>& tau_diag, T tau) {
  device_vector<T> d_arg; d_arg = arg;
  device_vector<T> d_tau; d_tau = tau_diag;
  device_vector<T> d_res(arg.size());
  CheckHip(prost_hip_stream_synchronize(CurrentStream()), "sync");
  const auto t0 = std::chrono::steady_clock::now();
  Eval(d_res, d_arg, d_tau, tau);
  CheckHip(prost_hip_stream_synchronize(CurrentStream()), "sync");
  const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  CheckHip(prost_hip_check_last_error(), "prox kernel");
  d_res.copy_to(result);
  return ms;
}
template class Prox<float>;
template class Prox<double>;

// ---- elementwise 1d / norm2 ----
template <typename T>
ProxElemDispatch<T>::ProxElemDispatch(int op, int fn, size_t index, size_t count, size_t dim, bool interleaved, bool diagsteps,
                                        const std::array<std::vector<T>, 7>& coeffs)
    : ProxSeparableSum<T>(index, count, op == PROST_OP_1D ? 1 : dim, interleaved, diagsteps), op_(op), fn_(fn), coeffs_(coeffs) {
  for (int i = 0; i < 7; i++)
    if (coeffs_[i].empty()) throw Exception("Empty vector passed.");
}
template <typename T>
void ProxElemDispatch<T>::Initialize() {
  for (int i = 0; i < 7; i++)
    if (coeffs_[i].size() > 1) {
      if (coeffs_[i].size() < this->count_) throw Exception("Size of coefficients should be either 1 or count.");
      d_coeffs_[i] = coeffs_[i];
    }
}
template <typename T> void ProxElemDispatch<T>::Release() { for (int i = 0; i < 7; i++) d_coeffs_[i].clear(); }
template <typename T>
size_t ProxElemDispatch<T>::gpu_mem_amount() const {
  size_t mem = 0;
  for (int i = 0; i < 7; i++) if (coeffs_[i].size() > 1) mem += this->count_ * sizeof(T);
  return mem;
}
template <typename T>
bool ProxElemDispatch<T>::describe(ProxDesc& d) const {
  d.kind = op_ == PROST_OP_1D ? ProxDesc::kElem1D : ProxDesc::kElemNorm2;
  d.fn = fn_; d.count = this->count_; d.dim = this->dim_; d.interleaved = this->interleaved_;
  for (int i = 0; i < 7; i++) {
    if (coeffs_[i].size() > 1) {
      if (d_coeffs_[i].size() != coeffs_[i].size()) return false;     // not initialised yet
      d.coeff_ptr[i] = d_coeffs_[i].data(); d.coeff_val[i] = 0;
    } else { d.coeff_ptr[i] = nullptr; d.coeff_val[i] = (double)coeffs_[i][0]; }
  }
  return true;
}
/// device pointer (per-element coefficient) or scalar value of each of the seven coefficients, as the kernels take them
template <typename T>
void ProxElemDispatch<T>::CoeffArgs(const T* (&ptrs)[7], double (&vals)[7]) const {
  for (int i = 0; i < 7; i++) {
    if (coeffs_[i].size() > 1) {
      if (d_coeffs_[i].size() != coeffs_[i].size()) throw Exception("ProxElemOperation used before Initialize().");
      ptrs[i] = d_coeffs_[i].data(); vals[i] = 0;
    } else { ptrs[i] = nullptr; vals[i] = (double)coeffs_[i][0]; }
  }
}
template <typename T>
void ProxElemDispatch<T>::EvalLocal(T* res, T*, const T* arg, const T*, const T* tau_diag, const T*, T tau, bool invert_tau) {
  const T* ptrs[7]; double vals[7];
  CoeffArgs(ptrs, vals);
  CheckHip(Api<T>::prox_elem(op_, fn_, res, arg, tau_diag, (double)tau, invert_tau ? 1 : 0, this->count_, this->dim_,
                             this->interleaved_ ? 1 : 0, ptrs, vals, CurrentStream()), "prox_elem");
}
/// the device-side argument description of a prox that covers [index, index + size) of its variable (prost_hip_arg_spec)
template <typename T>
static void FillArgSpec(prost_hip_arg_spec& a, const typename Prox<T>::ArgSource& src, size_t index, size_t size) {
  (void)size;
  a.mode = src.mode;
  for (int k = 0; k < 4; k++) a.v[k] = src.v[k] ? src.v[k] + index : nullptr;
  a.s[0] = (double)src.s[0]; a.s[1] = (double)src.s[1];
  a.op = src.op; a.op_rows = src.op_rows; a.op_cols = src.op_cols; a.base = index;
  a.w[0] = src.w[0]; a.w[1] = src.w[1];                        // WHOLE vectors: the operator indexes them
  a.kty_out = src.kty_out ? src.kty_out + index : nullptr;
  a.use[0] = src.use[0]; a.use[1] = src.use[1];
  a.res_ws = src.res_ws; a.res_slot = src.res_slot ? *src.res_slot : 0; a.res_slots_max = src.res_slots_max;
}
/// workgroups (= partial slots) the 16-bytes-per-lane kernel launches for `count` element groups under the cap of the source
template <typename T>
static unsigned ResSlotsOfLaunch(const typename Prox<T>::ArgSource& src, size_t count) {
  const size_t v = 16 / sizeof(T), lanes = count / v;
  size_t g = (lanes + 255) / 256;
  if (g < 1) g = 1;
  if (g > (size_t)1 << 20) g = (size_t)1 << 20;
  return (unsigned)std::min<size_t>(g, src.res_slots_max);
}
template <typename T>
void ProxElemDispatch<T>::EvalMoreauLocal(T* res, const T* arg, const T* tau_diag, T tau, bool invert_tau) {
  const T* ptrs[7]; double vals[7];
  CoeffArgs(ptrs, vals);
  CheckHip(Api<T>::prox_elem_moreau(op_, fn_, res, arg, tau_diag, (double)tau, invert_tau ? 1 : 0, this->count_, this->dim_,
                                    this->interleaved_ ? 1 : 0, ptrs, vals, CurrentStream()), "prox_elem_moreau");
}
template <typename T>
void ProxElemDispatch<T>::EvalSourceLocal(bool moreau, device_vector<T>& result, const typename Prox<T>::ArgSource& src,
                                           const device_vector<T>& tau_diag, T tau, bool invert_tau) {
  const T* ptrs[7]; double vals[7];
  CoeffArgs(ptrs, vals);
  prost_hip_arg_spec a;
  FillArgSpec<T>(a, src, this->index_, this->size_);
  CheckHip(Api<T>::prox_elem_arg(op_, fn_, moreau ? 1 : 0, result.data() + this->index_, &a, tau_diag.data() + this->index_, (double)tau,
                                 invert_tau ? 1 : 0, this->count_, this->dim_, this->interleaved_ ? 1 : 0, ptrs, vals, CurrentStream()), "prox_elem_arg");
  if (src.res_ws && src.res_slot) *src.res_slot += ResSlotsOfLaunch<T>(src, this->count_);
}
template <typename T>
bool ProxElemDispatch<T>::supports_op_source() const {
  const size_t v = 16 / sizeof(T);
  const bool planar = op_ == PROST_OP_1D || !this->interleaved_ || this->dim_ == 1;
  return planar && this->count_ % v == 0 && this->index_ % v == 0;
}
template class ProxElemDispatch<float>;
template class ProxElemDispatch<double>;

// ---- spectral: singular_nx2 / eigen_2x2 / eigen_3x3 / eigen_nxn / mass4 / mass5 / ind_comass4_ball / ind_comass5_ball ----
template <typename T>
const char* ProxSpectral<T>::OperationName(int op) {
  switch (op) {
    case PROST_SPECTRAL_SINGULAR_NX2: return "singular_nx2";
    case PROST_SPECTRAL_EIGEN_2X2: return "eigen_2x2";
    case PROST_SPECTRAL_EIGEN_3X3: return "eigen_3x3";
    case PROST_SPECTRAL_EIGEN_NXN: return "eigen_nxn";
    case PROST_SPECTRAL_MASS4: return "mass4";
    case PROST_SPECTRAL_IND_COMASS4_BALL: return "ind_comass4_ball";
    case PROST_SPECTRAL_MASS5: return "mass5";
    case PROST_SPECTRAL_IND_COMASS5_BALL: return "ind_comass5_ball";
  }
  return "spectral";
}
template <typename T>
ProxSpectral<T>::ProxSpectral(int op, int fn, size_t index, size_t count, size_t dim, bool interleaved, bool diagsteps,
                              const std::array<std::vector<T>, 7>& coeffs)
    : ProxSeparableSum<T>(index, count, dim, interleaved, diagsteps), op_(op), fn_(fn), coeffs_(coeffs) {
  std::stringstream ss;
  if (op == PROST_SPECTRAL_SINGULAR_NX2 && (dim == 0 || dim % 2 != 0)) ss << "singular_nx2: dim = " << dim << ", but a group is an n x 2 matrix: dim has to be even.";
  else if (op == PROST_SPECTRAL_EIGEN_2X2 && dim != 4) ss << "eigen_2x2: dim = " << dim << ", but a group is a 2 x 2 matrix: dim has to be 4.";
  else if (op == PROST_SPECTRAL_EIGEN_3X3 && dim != 9) ss << "eigen_3x3: dim = " << dim << ", but a group is a 3 x 3 matrix: dim has to be 9.";
  else if (op == PROST_SPECTRAL_EIGEN_NXN) {
    size_t n = 0;                                      // dim comes from the description: at most 32 steps whatever it is
    for (size_t k = 1; k <= 32 && n == 0; k++)
      if (k * k == dim) n = k;
    if (n == 0) ss << "eigen_nxn: dim = " << dim << ", but a group is an n x n matrix with 1 <= n <= 32: dim has to be one of 1, 4, 9, .., 1024.";
  } else if ((op == PROST_SPECTRAL_MASS4 || op == PROST_SPECTRAL_IND_COMASS4_BALL) && dim != 6)
    ss << OperationName(op) << ": Wrong dimension in mass norm prox: dim = " << dim << ", but a 2-vector in R^4 has 6 components.";
  else if ((op == PROST_SPECTRAL_MASS5 || op == PROST_SPECTRAL_IND_COMASS5_BALL) && dim != 10)
    ss << OperationName(op) << ": Wrong dimension in mass norm prox: dim = " << dim << ", but a 2-vector in R^5 has 10 components.";
  else if (op < PROST_SPECTRAL_SINGULAR_NX2 || op > PROST_SPECTRAL_IND_COMASS5_BALL) ss << "spectral prox: unknown operation id " << op << ".";
  if (!ss.str().empty()) throw Exception(ss.str());
  for (int i = 0; i < 7; i++)
    if (coeffs_[i].empty()) throw Exception(std::string(OperationName(op)) + ": empty coefficient vector passed.");
}
template <typename T>
void ProxSpectral<T>::Initialize() {
  for (int i = 0; i < 7; i++)
    if (coeffs_[i].size() > 1) {
      if (coeffs_[i].size() < this->count_) throw Exception(std::string(OperationName(op_)) + ": size of coefficients should be either 1 or count.");
      d_coeffs_[i] = coeffs_[i];
    }
}
template <typename T> void ProxSpectral<T>::Release() { for (int i = 0; i < 7; i++) d_coeffs_[i].clear(); }
template <typename T>
size_t ProxSpectral<T>::gpu_mem_amount() const {
  size_t mem = 0;
  for (int i = 0; i < 7; i++) if (coeffs_[i].size() > 1) mem += this->count_ * sizeof(T);
  return mem;
}
template <typename T>
void ProxSpectral<T>::Launch(T* res, const T* arg, const T* tau_diag, T tau, const T* step, const int* stop, bool invert_tau) {
  const T* ptrs[7]; double vals[7];
  for (int i = 0; i < 7; i++) {
    if (coeffs_[i].size() > 1) {
      if (d_coeffs_[i].size() != coeffs_[i].size()) throw Exception(std::string(OperationName(op_)) + ": prox used before Initialize().");
      ptrs[i] = d_coeffs_[i].data(); vals[i] = 0;
    } else { ptrs[i] = nullptr; vals[i] = (double)coeffs_[i][0]; }
  }
  CheckHip(Api<T>::prox_spectral(op_, fn_, res, arg, tau_diag, (double)tau, step, stop, invert_tau ? 1 : 0, this->count_, this->dim_,
                                 this->interleaved_ ? 1 : 0, ptrs, vals, CurrentStream()), "prox_spectral");
}
template <typename T>
void ProxSpectral<T>::EvalLocal(T* res, T*, const T* arg, const T*, const T* tau_diag, const T*, T tau, bool invert_tau) {
  Launch(res, arg, tau_diag, tau, nullptr, nullptr, invert_tau);
}
template <typename T>
void ProxSpectral<T>::EvalLocalStepView(T* res, T*, const T* arg, const T*, const T* tau_diag, const T*, const typename Prox<T>::StepView& view, bool invert_tau) {
  Launch(res, arg, tau_diag, (T)0, view.step, view.stop, invert_tau);
}
template class ProxSpectral<float>;
template class ProxSpectral<double>;

// ---- Moreau ----
template <typename T> void ProxMoreau<T>::Initialize() { scaled_arg_.resize(this->size_); conjugate_->Initialize(); }
template <typename T> void ProxMoreau<T>::Release() { conjugate_->Release(); scaled_arg_.clear(); }
static bool g_moreau_fuse = true;
template <typename T> void ProxMoreau<T>::SetFuseElemOperations(bool on) { g_moreau_fuse = on; }
template <typename T>
void ProxMoreau<T>::EvalLocal(T* res, T* res_end, const T* arg, const T* arg_end, const T* tau_diag, const T* tau_end, T tau, bool invert_tau) {
  const size_t n = this->size_;
  if (g_moreau_fuse && res != arg) {
    if (auto* e = dynamic_cast<ProxElemDispatch<T>*>(conjugate_.get())) {        // pre-scale, elem operation and post-scale in one kernel
      e->EvalMoreauLocal(res, arg, tau_diag, tau, invert_tau);
      return;
    }
  }
  CheckHip(Api<T>::moreau_prescale(scaled_arg_.data(), arg, tau_diag, (double)tau, invert_tau ? 1 : 0, n, CurrentStream()), "moreau_prescale");
  conjugate_->EvalLocal(res, res_end, scaled_arg_.data(), scaled_arg_.data() + n, tau_diag, tau_end, tau, !invert_tau);
  CheckHip(Api<T>::moreau_postscale(res, arg, tau_diag, (double)tau, invert_tau ? 1 : 0, n, CurrentStream()), "moreau_postscale");
  (void)arg_end;
}
template <typename T>
bool ProxMoreau<T>::takes_step_view() const { return dynamic_cast<ProxIndEpiConjQuad1D<T>*>(conjugate_.get()) != nullptr; }
template <typename T>
void ProxMoreau<T>::EvalLocalStepView(T* res, T* res_end, const T* arg, const T*, const T* tau_diag, const T* tau_end, const typename Prox<T>::StepView& view, bool invert_tau) {
  if (!takes_step_view()) throw Exception("ProxMoreau: only a conjugated prox that does not depend on the step takes it from the device.");
  const size_t n = this->size_;
  CheckHip(Api<T>::moreau_prescale_view(scaled_arg_.data(), arg, tau_diag, view.step, view.stop, invert_tau ? 1 : 0, n, CurrentStream()), "moreau_prescale_view");
  conjugate_->EvalLocalStepView(res, res_end, scaled_arg_.data(), scaled_arg_.data() + n, tau_diag, tau_end, view, !invert_tau);
  CheckHip(Api<T>::moreau_postscale_view(res, arg, tau_diag, view.step, view.stop, invert_tau ? 1 : 0, n, CurrentStream()), "moreau_postscale_view");
}
template <typename T>
bool ProxMoreau<T>::describe(ProxDesc& d) const {
  if (!conjugate_->describe(d) || d.moreau) return false;
  d.moreau = true;
  return true;
}
template <typename T>
bool ProxMoreau<T>::supports_arg_source() const { return g_moreau_fuse && dynamic_cast<ProxElemDispatch<T>*>(conjugate_.get()) != nullptr; }
template <typename T>
void ProxMoreau<T>::EvalFromSource(device_vector<T>& result, const typename Prox<T>::ArgSource& src, const device_vector<T>& tau_diag, T tau, bool invert_tau) {
  auto* e = dynamic_cast<ProxElemDispatch<T>*>(conjugate_.get());
  if (!e) throw Exception("ProxMoreau: only a conjugated elem operation evaluates from an argument source.");
  e->EvalSourceLocal(true, result, src, tau_diag, tau, invert_tau);
}
template class ProxMoreau<float>;
template class ProxMoreau<double>;

// ---- zero ----
template <typename T>
void ProxZero<T>::EvalFromSource(device_vector<T>& result, const typename Prox<T>::ArgSource& src, const device_vector<T>&, T, bool) {
  const size_t i = this->index_;
  void* s = CurrentStream();
  const bool sums = src.res_ws != nullptr && (src.mode == PROST_ARG_PDHG_PRIMAL || src.mode == PROST_ARG_PDHG_DUAL);
  if (src.mode == PROST_ARG_PDHG_PRIMAL && !sums)
    CheckHip(Api<T>::pdhg_primal_arg(result.data() + i, src.v[0] + i, src.v[1] + i, src.v[2] + i, (double)src.s[0], this->size_, s), "primal_arg");
  else if (src.mode == PROST_ARG_PDHG_DUAL && !sums)
    CheckHip(Api<T>::pdhg_dual_arg(result.data() + i, src.v[0] + i, src.v[1] + i, src.v[2] + i, src.v[3] + i, (double)src.s[0], (double)src.s[1], this->size_, s), "dual_arg");
  else if (sums || src.mode == PROST_ARG_PDHG_PRIMAL_OP || src.mode == PROST_ARG_PDHG_DUAL_OP) {
    // the identity as the 1-D operation of the zero function with a = c = 1, b = d = e = 0: ((1 (arg - 0 tau)) / 1 - 0 + 0) / 1 = arg, exactly
    // (elem_operation_1d.hpp:45-58) -- the launch that forms the argument from the operator writes it straight into the result
    prost_hip_arg_spec a;
    FillArgSpec<T>(a, src, i, this->size_);
    const T* ptrs[7] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    const double vals[7] = {1, 0, 1, 0, 0, 0, 0};
    CheckHip(Api<T>::prox_elem_arg(PROST_OP_1D, PROST_FN_ZERO, 0, result.data() + i, &a, src.v[1] + i, (double)src.s[0], 0, this->size_, 1, 0, ptrs, vals, s), "prox_elem_arg");
    if (src.res_ws && src.res_slot) *src.res_slot += ResSlotsOfLaunch<T>(src, this->size_);
  }
  else throw Exception("ProxZero: unknown argument source.");
}
template <typename T>
void ProxZero<T>::EvalLocal(T* res, T*, const T* arg, const T*, const T*, const T*, T, bool) {
  if (res != arg) CheckHip(prost_hip_memcpy_d2d(res, arg, this->size_ * sizeof(T), CurrentStream()), "memcpy_d2d");
}
template class ProxZero<float>;
template class ProxZero<double>;

// ---- epigraph of a quadratic ----
template <typename T>
void ProxIndEpiQuad<T>::Initialize() {
  if (a_.size() != this->count_ && a_.size() != 1) throw Exception("Wrong input: Coefficient a has to have dimension count or 1!");
  for (T& a : a_) if (a <= 0) throw Exception("Wrong input: Coefficient a must be greater 0!");
  if (b_.size() != this->count_ * (this->dim_ - 1)) throw Exception("Wrong input: Coefficient b has to have dimension count*(dim-1)!");
  if (c_.size() != this->count_ && c_.size() != 1) throw Exception("Wrong input: Coefficient c has to have dimension count or 1!");
  d_a_ = a_; d_b_ = b_; d_c_ = c_;
}
template <typename T> void ProxIndEpiQuad<T>::Release() { d_a_.clear(); d_b_.clear(); d_c_.clear(); }
template <typename T>
void ProxIndEpiQuad<T>::EvalLocal(T* res, T*, const T* arg, const T*, const T*, const T*, T, bool) {
  if (d_b_.size() != b_.size()) throw Exception("ProxIndEpiQuad used before Initialize().");
  CheckHip(Api<T>::prox_epi_quad(res, arg, this->count_, this->dim_, a_.size() != 1 ? d_a_.data() : nullptr, (double)a_[0], d_b_.data(),
                                 c_.size() != 1 ? d_c_.data() : nullptr, (double)c_[0], CurrentStream()), "prox_epi_quad");
}
template class ProxIndEpiQuad<float>;
template class ProxIndEpiQuad<double>;

// ---- elem_operation:ind_sum ----
template <typename T>
void ProxElemIndSum<T>::EvalLocal(T* res, T*, const T* arg, const T*, const T*, const T*, T, bool) {
  CheckHip(Api<T>::prox_elem_ind_sum(res, arg, this->count_, this->dim_, this->interleaved_ ? 1 : 0, CurrentStream()), "prox_elem_ind_sum");
}
template class ProxElemIndSum<float>;
template class ProxElemIndSum<double>;

// ---- elem_operation:ind_simplex ----
template <typename T>
void ProxElemIndSimplex<T>::EvalLocal(T* res, T*, const T* arg, const T*, const T*, const T*, T, bool) {
  if (work_.size() != this->count_ * this->dim_) throw Exception("ProxElemIndSimplex used before Initialize().");
  CheckHip(Api<T>::prox_elem_ind_simplex(res, arg, work_.data(), this->count_, this->dim_, this->interleaved_ ? 1 : 0, CurrentStream()), "prox_elem_ind_simplex");
}
template class ProxElemIndSimplex<float>;
template class ProxElemIndSimplex<double>;

// ---- transform ----
template <typename T>
void ProxTransform<T>::Initialize() {
  for (T& a : host_[0])
    if (a == 0) throw Exception("ProxTransform: Vector 'a' isn't allowed to contain zero element. (Division by zero)");
  for (int k = 0; k < 5; k++) {
    if (host_[k].empty()) throw Exception("Empty vector passed.");
    if (host_[k].size() > 1) {
      if (host_[k].size() < this->size_) throw Exception("Size of coefficients should be either 1 or count.");
      dev_[k] = host_[k];
    }
  }
  scaled_arg_.resize(this->size_);
  scaled_tau_.resize(this->size_);
  inner_fn_->Initialize();
}
template <typename T>
void ProxTransform<T>::Release() {
  inner_fn_->Release();
  for (int k = 0; k < 5; k++) dev_[k].clear();
  scaled_arg_.clear(); scaled_tau_.clear();
}
template <typename T>
size_t ProxTransform<T>::gpu_mem_amount() const {
  size_t mem = inner_fn_->gpu_mem_amount() + 2 * this->size_ * sizeof(T);
  for (int k = 0; k < 5; k++) if (host_[k].size() > 1) mem += host_[k].size() * sizeof(T);
  return mem;
}
template <typename T>
void ProxTransform<T>::EvalLocal(T* res, T* res_end, const T* arg, const T*, const T* tau_diag, const T*, T tau, bool invert_tau) {
  const size_t n = this->size_;
  if (scaled_arg_.size() != n) throw Exception("ProxTransform used before Initialize().");
  const T* ptrs[5]; double vals[5];
  for (int k = 0; k < 5; k++) {
    ptrs[k] = host_[k].size() > 1 ? dev_[k].data() : nullptr;
    vals[k] = (double)host_[k][0];
  }
  void* s = CurrentStream();
  CheckHip(Api<T>::transform_prescale(scaled_arg_.data(), scaled_tau_.data(), arg, tau_diag, ptrs, vals, (double)tau, invert_tau ? 1 : 0, n, s), "transform_prescale");
  // the inner prox sees local ranges: its own index is not applied (prox_transform.cu:202-210)
  inner_fn_->EvalLocal(res, res_end, scaled_arg_.data(), scaled_arg_.data() + n, scaled_tau_.data(), scaled_tau_.data() + n, (T)1, false);
  CheckHip(Api<T>::transform_postscale(res, ptrs[0], vals[0], ptrs[1], vals[1], n, s), "transform_postscale");
}
template class ProxTransform<float>;
template class ProxTransform<double>;

// ---- permute ----
template <typename T>
void ProxPermute<T>::Initialize() {
  permuted_arg_.resize(this->size_);
  perm_ = perm_host_;
  if (perm_host_.size() != base_prox_->size()) {
    std::stringstream ss;
    ss << "Permutation vector has wrong size (" << perm_host_.size() << ") instead of " << base_prox_->size() << ".";
    throw Exception(ss.str());
  }
  for (int32_t v : perm_host_)      // the reference does not check; an out-of-range entry would read / write out of bounds
    if (v < 0 || (size_t)v >= perm_host_.size()) throw Exception("Permutation vector has an entry outside [0, size).");
  base_prox_->Initialize();
}
template <typename T> void ProxPermute<T>::Release() { base_prox_->Release(); perm_.clear(); permuted_arg_.clear(); }
template <typename T>
void ProxPermute<T>::EvalLocal(T* res, T* res_end, const T* arg, const T*, const T* tau_diag, const T* tau_end, T tau, bool invert_tau) {
  const size_t n = perm_host_.size();
  if (permuted_arg_.size() != this->size_) throw Exception("ProxPermute used before Initialize().");
  void* s = CurrentStream();
  // permuted argument into `res`, prox of it into permuted_arg_, scattered back into `res`; tau_diag is
  // NOT permuted (prox_permute.cu:113-143)
  CheckHip(Api<T>::permute(res, arg, perm_.data(), n, 0, s), "permute");
  base_prox_->EvalLocal(permuted_arg_.data(), permuted_arg_.data() + n, res, res_end, tau_diag, tau_end, tau, invert_tau);
  CheckHip(Api<T>::permute(res, permuted_arg_.data(), perm_.data(), n, 1, s), "permute");
}
template class ProxPermute<float>;
template class ProxPermute<double>;

// ---- halfspace ----
template <typename T>
void ProxIndHalfspace<T>::Initialize() {
  if (a_.size() != this->count_ * this->dim_ && a_.size() != this->dim_) throw Exception("Wrong input: Coefficient a has to have dimension count*dim or dim!");
  if (b_.size() != this->count_ && b_.size() != 1) throw Exception("Wrong input: Coefficient b has to have dimension count or 1!");
  d_a_ = a_; d_b_ = b_;
}
template <typename T>
void ProxIndHalfspace<T>::EvalLocal(T* res, T*, const T* arg, const T*, const T*, const T*, T, bool) {
  if (d_a_.size() != a_.size()) throw Exception("ProxIndHalfspace used before Initialize().");
  CheckHip(Api<T>::prox_ind_halfspace(res, arg, this->count_, this->dim_, d_a_.data(), a_.size(), d_b_.data(), b_.size(), CurrentStream()), "prox_ind_halfspace");
}
template class ProxIndHalfspace<float>;
template class ProxIndHalfspace<double>;

// ---- second-order cone ----
template <typename T>
void ProxIndSOC<T>::Initialize() {
  if (alpha_ != 1) throw Exception("ProxIndSOC: Only alpha = 1 implemented right now.");
  if (this->dim_ < 1) throw Exception("ProxIndSOC: dim must be at least 1.");
}
template <typename T>
void ProxIndSOC<T>::EvalLocal(T* res, T*, const T* arg, const T*, const T*, const T*, T, bool) {
  CheckHip(Api<T>::prox_ind_soc(res, arg, this->count_, this->dim_, CurrentStream()), "prox_ind_soc");
}
template class ProxIndSOC<float>;
template class ProxIndSOC<double>;

// ---- index-family sum constraints ----
template <typename T>
void ProxIndSum<T>::Initialize() {
  if (count_ * dim_ != inds_.size()) throw Exception("ProxIndSum: dimensions dont fit");
  if (two_ && count_2_ * dim_2_ != inds_2_.size()) throw Exception("ProxIndSum: dimensions dont fit");
  for (uint64_t v : inds_) if (v >= this->size_) throw Exception("ProxIndSum: index outside the prox range.");   // unchecked in the reference
  for (uint64_t v : inds_2_) if (v >= this->size_) throw Exception("ProxIndSum: index outside the prox range.");
  d_inds_ = std::vector<int64_t>(inds_.begin(), inds_.end());
  if (two_) d_inds_2_ = std::vector<int64_t>(inds_2_.begin(), inds_2_.end());
}
template <typename T>
void ProxIndSum<T>::EvalLocal(T* res, T*, const T* arg, const T*, const T* tau_diag, const T*, T tau, bool invert_tau) {
  if (d_inds_.size() != inds_.size()) throw Exception("ProxIndSum used before Initialize().");
  void* s = CurrentStream();
  if (res != arg) CheckHip(prost_hip_memcpy_d2d(res, arg, this->size_ * sizeof(T), s), "memcpy_d2d");       // "zero prox on other indices" :119
  CheckHip(Api<T>::prox_ind_sum(res, arg, tau_diag, reinterpret_cast<const uint64_t*>(d_inds_.data()), count_, dim_, (double)sum_, (double)tau,
                                invert_tau ? 1 : 0, s), "prox_ind_sum");
  if (two_)
    CheckHip(Api<T>::prox_ind_sum(res, arg, tau_diag, reinterpret_cast<const uint64_t*>(d_inds_2_.data()), count_2_, dim_2_, (double)sum_2_,
                                  (double)tau, invert_tau ? 1 : 0, s), "prox_ind_sum");
}
template class ProxIndSum<float>;
template class ProxIndSum<double>;

// ---- range of a sparse matrix ----
template <typename T>
void ProxIndRange<T>::setA(int m, int n, int nnz, const std::vector<T>& val, const std::vector<int32_t>& ptr, const std::vector<int32_t>& ind) {
  if (m < 0 || n < 0 || nnz < 0 || ptr.size() != (size_t)n + 1 || val.size() < (size_t)nnz || ind.size() < (size_t)nnz)
    throw Exception("ProxIndRange: the CSC arrays of 'A' do not fit its dimensions.");
  if (ptr[0] != 0 || ptr[n] != nnz) throw Exception("ProxIndRange: the CSC arrays of 'A' do not fit its dimensions.");
  for (int c = 0; c < n; c++)
    if (ptr[c + 1] < ptr[c]) throw Exception("ProxIndRange: the column starts of 'A' decrease.");
  for (int k = 0; k < nnz; k++)                      // unchecked in the reference; a row index outside A would read out of bounds on the device
    if (ind[k] < 0 || ind[k] >= m) throw Exception("ProxIndRange: 'A' has a row index outside [0, rows).");
  nrows_ = m; ncols_ = n; nnz_ = nnz;
  // the CSC arrays of A are the CSR arrays of A'; A itself in CSR comes from one transposition (as BlockSparse::CreateFromCSC)
  host_ind_t_ = ind; host_ptr_t_ = ptr; host_val_t_ = val;
  host_ind_.assign(nnz_, 0); host_val_.assign(nnz_, (T)0); host_ptr_.assign(nrows_ + 1, 0);
  csr2csc<T>(n, m, nnz, host_val_t_.data(), host_ind_t_.data(), host_ptr_t_.data(), host_val_.data(), host_ind_.data(), host_ptr_.data());
}
template <typename T>
void ProxIndRange<T>::setAA(int m, int n, const std::vector<T>& val) {
  if (m != n) throw Exception("ProxIndRange: Matrix 'AA' must be square!");
  if ((size_t)m != ncols_) throw Exception("ProxIndRange: Matrix 'AA' must fit dimension of 'A'!");
  if (val.size() != (size_t)m * (size_t)n) throw Exception("ProxIndRange: the values of 'AA' do not fit its dimensions.");
  host_AA_ = val;
}
template <typename T>
void ProxIndRange<T>::Initialize() {
  const size_t n = ncols_;
  if (n < 1 || host_AA_.size() != n * n) throw Exception("ProxIndRange: 'A' and 'AA' have to be set before Initialize().");
  size_t solve_ws = 0;
  if (prost_hip_range_potrs_plan(n, dtype_id<T>(), nullptr, nullptr, nullptr, nullptr, &solve_ws) != 0)
    throw Exception("ProxIndRange: 'AA' is n x n with n * n >= 2^31: too large for the dense solve.");
  ready_ = false;
  val_ = host_val_; ind_ = host_ind_; ptr_ = host_ptr_;
  val_t_ = host_val_t_; ind_t_ = host_ind_t_; ptr_t_ = host_ptr_t_;
  L_ = host_AA_;
  U_.resize(n * n);
  dinv_.resize(prost_hip_range_dinv_elements(n));
  temp_.resize(n);
  device_vector<double> setup_ws((Api<T>::range_potrf_workspace_bytes(n) + sizeof(double) - 1) / sizeof(double));
  device_vector<int32_t> status(1);
  void* s = CurrentStream();
  CheckHip(Api<T>::range_potrf(L_.data(), U_.data(), dinv_.data(), setup_ws.data(), reinterpret_cast<int*>(status.data()), n, s), "range_potrf");
  std::vector<int32_t> info;
  status.copy_to(info);                              // synchronous: the one read-back of the set-up
  CheckHip(prost_hip_check_last_error(), "range_potrf kernels");
  if (info[0] >= 0) {
    Release();
    std::stringstream ss;
    ss << "ProxIndRange: matrix 'AA' is not positive definite (pivot " << info[0] << ").";
    throw Exception(ss.str());
  }
  workspace_.resize((solve_ws + sizeof(double) - 1) / sizeof(double));
  ready_ = true;
}
template <typename T>
void ProxIndRange<T>::Release() {
  ready_ = false;
  val_.clear(); ind_.clear(); ptr_.clear(); val_t_.clear(); ind_t_.clear(); ptr_t_.clear();
  L_.clear(); U_.clear(); dinv_.clear(); temp_.clear(); workspace_.clear();
}
template <typename T>
size_t ProxIndRange<T>::gpu_mem_amount() const {
  const size_t n = ncols_;
  size_t solve_ws = 0;
  if (n >= 1) prost_hip_range_potrs_plan(n, dtype_id<T>(), nullptr, nullptr, nullptr, nullptr, &solve_ws);
  // A and A' in CSR, L and U, the inverted diagonal blocks, the n-vector between the products and the workspace of the solve
  return 2 * nnz_ * (sizeof(T) + sizeof(int32_t)) + (nrows_ + 1 + n + 1) * sizeof(int32_t) + (2 * n * n + prost_hip_range_dinv_elements(n) + n) * sizeof(T) + solve_ws;
}
template <typename T>
void ProxIndRange<T>::EvalLocal(T* res, T*, const T* arg, const T*, const T*, const T*, T, bool) {
  if (!ready_) throw Exception("ProxIndRange used before Initialize().");
  void* s = CurrentStream();
  // t = A' y consumes the argument before anything is written: res may be arg
  CheckHip(Api<T>::csr_spmv(temp_.data(), arg, ncols_, nnz_, val_t_.data(), ptr_t_.data(), ind_t_.data(), s), "csr_spmv");
  CheckHip(Api<T>::range_potrs(temp_.data(), L_.data(), U_.data(), dinv_.data(), workspace_.data(), ncols_, 0, s), "range_potrs");
  CheckHip(Api<T>::csr_spmv(res, temp_.data(), nrows_, nnz_, val_.data(), ptr_.data(), ind_.data(), s), "csr_spmv");
}
template class ProxIndRange<float>;
template class ProxIndRange<double>;

// ---- epigraph of a max-affine function ----
template <typename T>
ProxIndEpiPolyhedral<T>::ProxIndEpiPolyhedral(size_t index, size_t count, size_t dim, bool interleaved, const std::vector<T>& a, const std::vector<T>& b,
                                              const std::vector<double>& count_vec, const std::vector<double>& index_vec)
    : ProxSeparableSum<T>(index, count, dim, interleaved, false), a_(a), b_(b), max_count_(0), ready_(false) {
  const size_t lim = (size_t)1 << 31;
  if (dim < 2 || dim > 4) {
    std::stringstream ss;
    ss << "ProxIndEpiPolyhedral: dim = " << dim << " is not supported, dim has to be between 2 and 4.";
    throw Exception(ss.str());
  }
  if (count_vec.size() != count || index_vec.size() != count) {
    std::stringstream ss;
    ss << "ProxIndEpiPolyhedral: count_vec and index_vec need one entry per group (count = " << count << ", got " << count_vec.size() << " and " << index_vec.size() << ").";
    throw Exception(ss.str());
  }
  if (a.size() != b.size() * (dim - 1)) {
    std::stringstream ss;
    ss << "ProxIndEpiPolyhedral: a has " << a.size() << " entries, expected len(b) * (dim - 1) = " << b.size() * (dim - 1) << ".";
    throw Exception(ss.str());
  }
  if (count >= lim || b.size() >= lim || a.size() >= lim) throw Exception("ProxIndEpiPolyhedral: the number of groups, of constraints and of coefficients each have to stay below 2^31.");
  cnt_.resize(count); idx_.resize(count);
  for (size_t g = 0; g < count; g++) {
    const double c = count_vec[g], s = index_vec[g];
    if (!(c >= 0) || !(s >= 0) || c != std::floor(c) || s != std::floor(s) || c >= (double)lim || s >= (double)lim) {
      std::stringstream ss;
      ss << "ProxIndEpiPolyhedral: count_vec and index_vec have to hold non-negative integers below 2^31 (group " << g << ").";
      throw Exception(ss.str());
    }
    if ((size_t)c + (size_t)s > b.size()) {
      std::stringstream ss;
      ss << "ProxIndEpiPolyhedral: group " << g << " names constraints " << (size_t)s << " .. " << (size_t)s + (size_t)c << ", but there are only " << b.size() << ".";
      throw Exception(ss.str());
    }
    cnt_[g] = (int32_t)c; idx_[g] = (int32_t)s;
    if ((size_t)c > max_count_) max_count_ = (size_t)c;
  }
}
template <typename T>
void ProxIndEpiPolyhedral<T>::Initialize() {
  ready_ = false;
  d_a_ = a_; d_b_ = b_; d_cnt_ = cnt_; d_idx_ = idx_;
  d_fallback_.resize(1);
  ready_ = true;
}
template <typename T>
void ProxIndEpiPolyhedral<T>::Release() {
  ready_ = false;
  d_a_.clear(); d_b_.clear(); d_cnt_.clear(); d_idx_.clear(); d_fallback_.clear();
}
template <typename T>
size_t ProxIndEpiPolyhedral<T>::fallback_count() const {
  if (!ready_) return 0;
  std::vector<int32_t> v;
  d_fallback_.copy_to(v);
  return (size_t)(uint32_t)v[0];
}
template <typename T>
void ProxIndEpiPolyhedral<T>::EvalLocal(T* res, T*, const T* arg, const T*, const T*, const T*, T, bool) {
  if (!ready_) throw Exception("ProxIndEpiPolyhedral used before Initialize().");
  CheckHip(Api<T>::prox_ind_epi_polyhedral(res, arg, this->count_, this->dim_, this->interleaved_ ? 1 : 0, d_a_.data(), d_b_.data(), d_cnt_.data(), d_idx_.data(),
                                           max_count_, reinterpret_cast<unsigned*>(d_fallback_.data()), CurrentStream()),
           "prox_ind_epi_polyhedral");
}
template class ProxIndEpiPolyhedral<float>;
template class ProxIndEpiPolyhedral<double>;

// ---- epigraph of the conjugate of a quadratic piece ----
template <typename T>
ProxIndEpiConjQuad1D<T>::ProxIndEpiConjQuad1D(size_t index, size_t size, size_t count, bool interleaved, const std::array<std::vector<T>, 5>& coeffs)
    : ProxSeparableSum<T>(index, count, 2, interleaved, false), coeffs_(coeffs), ready_(false) {
  static const char* const names[5] = {"a", "b", "c", "alpha", "beta"};
  if (size != 2 * count) {
    std::stringstream ss;
    ss << "ProxIndEpiConjQuad1D: size = " << size << " is not 2 * count = 2 * " << count << ".";
    throw Exception(ss.str());
  }
  for (int i = 0; i < 5; i++)
    if (coeffs_[i].size() != 1 && coeffs_[i].size() != count) {
      std::stringstream ss;
      ss << "ProxIndEpiConjQuad1D: coefficient " << names[i] << " has " << coeffs_[i].size() << " entries, expected 1 or count = " << count << ".";
      throw Exception(ss.str());
    }
  auto at = [this](int i, size_t g) { return coeffs_[i].size() == 1 ? coeffs_[i][0] : coeffs_[i][g]; };
  size_t groups = 1;
  for (int i = 0; i < 5; i++) groups = std::max(groups, coeffs_[i].size());
  for (size_t g = 0; g < groups; g++) {
    const T a = at(0, g), b = at(1, g), c = at(2, g), alpha = at(3, g), beta = at(4, g);
    std::stringstream ss;
    if (!std::isfinite(a) || !std::isfinite(b) || !std::isfinite(c)) ss << "a, b and c have to be finite";
    else if (std::isnan(alpha) || std::isnan(beta) || alpha == std::numeric_limits<T>::infinity() || beta == -std::numeric_limits<T>::infinity())
      ss << "alpha has to be finite or -inf and beta finite or +inf";
    else if (a < 0) ss << "a = " << a << " is negative, the piece has to be convex";
    else if (alpha > beta) ss << "alpha = " << alpha << " is above beta = " << beta;
    else if (a == 0 && (std::isinf(alpha) || std::isinf(beta))) ss << "a = 0 needs finite alpha and beta";
    if (!ss.str().empty()) {
      std::stringstream msg;
      msg << "ProxIndEpiConjQuad1D: " << ss.str() << " (group " << g << ").";
      throw Exception(msg.str());
    }
  }
}
template <typename T>
void ProxIndEpiConjQuad1D<T>::Initialize() {
  ready_ = false;
  for (int i = 0; i < 5; i++)
    if (coeffs_[i].size() > 1) d_coeffs_[i] = coeffs_[i];
  d_fallback_.resize(1);
  ready_ = true;
}
template <typename T>
void ProxIndEpiConjQuad1D<T>::Release() {
  ready_ = false;
  for (int i = 0; i < 5; i++) d_coeffs_[i].clear();
  d_fallback_.clear();
}
template <typename T>
size_t ProxIndEpiConjQuad1D<T>::gpu_mem_amount() const {
  size_t mem = sizeof(int32_t);
  for (int i = 0; i < 5; i++) if (coeffs_[i].size() > 1) mem += coeffs_[i].size() * sizeof(T);
  return mem;
}
template <typename T>
size_t ProxIndEpiConjQuad1D<T>::fallback_count() const {
  if (!ready_) return 0;
  std::vector<int32_t> v;
  d_fallback_.copy_to(v);
  return (size_t)(uint32_t)v[0];
}
template <typename T>
void ProxIndEpiConjQuad1D<T>::Launch(T* res, const T* arg, const int* stop) {
  if (!ready_) throw Exception("ProxIndEpiConjQuad1D used before Initialize().");
  const T* ptr[5]; double val[5];
  for (int i = 0; i < 5; i++) {
    const bool vec = coeffs_[i].size() > 1;
    ptr[i] = vec ? d_coeffs_[i].data() : nullptr; val[i] = vec ? 0.0 : (double)coeffs_[i][0];
  }
  CheckHip(Api<T>::prox_ind_epi_conjquad_1d(res, arg, this->count_, this->interleaved_ ? 1 : 0, ptr[0], val[0], ptr[1], val[1], ptr[2], val[2], ptr[3], val[3],
                                            ptr[4], val[4], reinterpret_cast<unsigned*>(d_fallback_.data()), stop, CurrentStream()),
           "prox_ind_epi_conjquad_1d");
}
template <typename T>
void ProxIndEpiConjQuad1D<T>::EvalLocal(T* res, T*, const T* arg, const T*, const T*, const T*, T, bool) { Launch(res, arg, nullptr); }
template <typename T>
void ProxIndEpiConjQuad1D<T>::EvalLocalStepView(T* res, T*, const T* arg, const T*, const T*, const T*, const typename Prox<T>::StepView& view, bool) {
  Launch(res, arg, view.stop);
}
template class ProxIndEpiConjQuad1D<float>;
template class ProxIndEpiConjQuad1D<double>;

}  // namespace prost
