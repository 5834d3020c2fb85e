// prost/backend/backend_admm.hpp -- graph-projection ADMM with a CGLS inner solve
// (reference backend_admm.hpp:36-112, src/backend/backend_admm.cu, include/prost/cgls.hpp).
#ifndef PROST_BACKEND_ADMM_HPP_
#define PROST_BACKEND_ADMM_HPP_
#include "prost/backend/backend.hpp"
#include "prost_hip.h"

namespace prost {

template <typename T>
class BackendADMM : public Backend<T> {
 public:
  struct Options {
    double rho0;
    double alpha;            ///< over-relaxation
    double cg_tol_pow, cg_tol_min, cg_tol_max;
    int cg_max_iter;
    int residual_iter;
    T arb_delta, arb_tau, arb_gamma;
    bool cg_graph;           ///< replay the CG rounds of a solve from one captured HIP graph (needs device_cg); off by default:
                             ///< measured 10-25 % SLOWER than the direct launches on ROCm 7.2
    bool fused_rounds;       ///< CG rounds of four launches with the operator applied inside them (needs device_cg and an operator of
                             ///< CSR / gradient blocks); false: the staged rounds with LinearOperator::Eval between the stages
    bool pixel_rounds;       ///< CG rounds of TWO launches for operators [D ; gradient2d] with D coupling the channels of one pixel (needs
                             ///< fused_rounds); false: the four-launch rounds
    bool device_cg;          ///< fused passes + CG scalars resident on the device (default); false = the reference's launch sequence, one blocking nrm2 per scalar
    Options() : rho0(1), alpha(1.7), cg_tol_pow(1.3), cg_tol_min(1e-5), cg_tol_max(1e-8), cg_max_iter(10), residual_iter(1),
                arb_delta(1.05), arb_tau(0.8), arb_gamma(1.01), cg_graph(false), fused_rounds(true), pixel_rounds(true), device_cg(true) {}
  };
  explicit BackendADMM(const Options& opts) : opts_(opts) {}
  virtual ~BackendADMM();

  virtual void Initialize();
  virtual void PerformIteration();
  virtual void Release();
  virtual void current_solution(std::vector<T>& primal, std::vector<T>& dual);
  virtual void current_solution(std::vector<T>& primal_x, std::vector<T>& primal_z, std::vector<T>& dual_y, std::vector<T>& dual_w);
  virtual size_t gpu_mem_amount() const;
  /// "admm:pixel-op": CG rounds of two launches (operators [D ; gradient2d], D pixel-diagonal or any sparse block with one row per
  /// pixel, e.g. a warp matrix); "admm:fused-op": CG rounds of four launches with the
  /// operator inside the stage kernels; "admm:generic": staged rounds
  virtual std::string path() const { return cg_mode_ == kCgPixel ? "admm:pixel-op" : cg_mode_ == kCgFused4 ? "admm:fused-op" : "admm:generic"; }
  T rho() const { return rho_; }
  size_t iteration() const { return iteration_; }
  virtual void KernelTimes(std::vector<typename Backend<T>::KernelTime>& out);
  int last_cg_iterations();                 ///< iterations taken by the most recent CGLS solve (reads the device record)

 private:
  /// How the CGLS solve of an outer iteration runs: decided ONCE, in Initialize(), from the options and the operator
  enum CgMode {
    kCgHost,      ///< device_cg = false: the reference's sequence, one launch per functor and one blocking nrm2 per scalar
    kCgStaged,    ///< CG scalars on the device, LinearOperator::Eval between the stages (any operator)
    kCgGraph,     ///< the staged rounds, captured once into a HIP graph and replayed with one host call per solve (cg_graph)
    kCgFused4,    ///< rounds of four launches with the operator inside (operators of CSR / gradient blocks)
    kCgPixel      ///< rounds of two launches (operators [D ; gradient2d], D with one row per pixel)
  };
  bool OperatorInside() const { return cg_mode_ == kCgFused4 || cg_mode_ == kCgPixel; }
  static constexpr size_t kEventsPerSample = 8, kMaxSamples = 512;       ///< (begin, end) of up to four kernels; the pixel rounds use the first four events
  int KernelsPerRound() const { return cg_mode_ == kCgPixel ? 2 : 4; }

  /// y := alpha op(Sigma^(1/2) K Tau^(1/2)) x + beta y   (GemvPrecondK, backend_admm.cu:199-272)
  void Gemv(char op, T alpha, const device_vector<T>& x, T beta, device_vector<T>& y);
  double Nrm2(const device_vector<T>& v, size_t n);
  int Cgls(const device_vector<T>& b, device_vector<T>& x, double shift, double tol, int maxit, device_vector<T>& p,
           device_vector<T>& q, device_vector<T>& r, device_vector<T>& s, int& iterations);   // cgls.hpp:222-371
  double CgTolerance() const;               ///< tolerance of this outer iteration's solve (backend_admm.cu:408-410)
  /// the same solve on the device: b = z_dual_, x = x_proj_, p = x_half_, q = z_half_, r = z_proj_, s = x_dual_, shift 1, cg_max_iter rounds
  void CglsDevice(double tol);
  void LaunchRound(const prost_hip_cgls_desc& d, int k, void* const* events);
  void ReplayRounds(const prost_hip_cgls_desc& d, int maxit);
  void* const* TakeSampleEvents();
  bool DescribePixelOperator();
  void OuterStage(int which, const prost_hip_admm_desc& d);
  void PerformIterationFused();
  void PerformIterationUnfused();
  void FinishResiduals(double primal_residual, double primal_var_norm, double dual_residual, double dual_var_norm);
  void GetDual(device_vector<T>& out, const device_vector<T>& half, const device_vector<T>& proj, const device_vector<T>& dual,
               const device_vector<T>& scaling, T expo, size_t n);

  Options opts_;
  CgMode cg_mode_ = kCgHost;
  device_vector<T> x_half_, z_half_, x_proj_, z_proj_, x_dual_, z_dual_, temp1_, temp2_, temp3_, tmp_n_, tmp_m_;
  double* scal_dev_ = nullptr;
  double* scal_host_ = nullptr;
  void* workspace_ = nullptr;
  void* cg_state_ = nullptr;          ///< device records of the CG scalars (prost_hip_cgls_state_bytes each): one per round + the initial one
  void* cg_workspace_ = nullptr;      ///< per-workgroup partial sums of the fused stages (prost_hip_cgls_workspace_bytes)
  int* cg_done_host_ = nullptr;       ///< pinned word the device stores the solve's epoch to when the stopping test fires
  void* cg_stream_ = nullptr;         ///< kCgGraph: stream the captured CG rounds are replayed on
  void* cg_graph_ = nullptr;          ///< kCgGraph: executable HIP graph of cg_max_iter rounds
  void* cg_ev_[2] = {nullptr, nullptr};
  int cg_epoch_ = 0;
  bool cg_iters_valid_ = true;
  prost_hip_fused_op fused_op_ = {};  ///< kCgFused4, kCgPixel: the operator as a table of CSR / gradient blocks
  prost_hip_pixel_op pixel_op_ = {};  ///< kCgPixel: the operator as [D ; gradient2d], with the second buffers for p and r
  device_vector<T> cg_p_alt_, cg_r_alt_;
  int cg_result_index_ = 0;           ///< record that holds the result of the most recent device solve
  std::vector<void*> ev_;             ///< event pool, kEventsPerSample per sampled round
  size_t ev_used_ = 0, solves_ = 0, rounds_launched_ = 0;
  T rho_ = 0, delta_ = 0;
  int arb_u_ = 0, arb_l_ = 0;
  size_t iteration_ = 0;
  int last_cg_iters_ = 0;
  std::vector<shared_ptr<Prox<T>>> prox_g_, prox_f_;
};

}  // namespace prost
#endif
