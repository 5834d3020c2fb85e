// kernels_prox_moreau_view.hip -- the two scaling passes of ProxMoreau (prox_moreau.cu:29-61) with the step size read on the device:
// inside a batch of iterations whose step-size rule runs on the device (Prox::StepView) the host does not know tau when it enqueues
// the passes.  Same arithmetic as prost_hip_moreau_prescale_* / _postscale_* (kernels_prox.hip) with tau = *step_dev; a non-zero
// *stop_dev (the rule's stopping test has fired) makes both return without writing.  Used in front of and behind a conjugated prox
// that does not depend on the step itself (ProxIndEpiConjQuad1D), so that goldstein / boyd keep their device-resident rule.
#include "common.hpp"

namespace prost_hip {

template <class T, bool POST>
__global__ void __launch_bounds__(kBlock) moreau_scale_view_kernel(T* out, const T* arg, const T* __restrict__ tau_diag,
                                                                  const T* __restrict__ step, const int* __restrict__ stop, bool inv, size_t n) {
  if (*stop) return;
  const T tau = *step;
  const size_t stride = (size_t)gridDim.x * kBlock;
  for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += stride) {
    const T a = arg[i], td = tau_diag[i];
    if (POST) { const T r = out[i]; out[i] = inv ? a - r / (tau * td) : a - tau * td * r; }
    else out[i] = inv ? a * (tau * td) : a / (tau * td);
  }
}

template <class T, bool POST>
static int launch_moreau_scale_view(T* out, const T* arg, const T* tau_diag, const T* step, const int* stop, int inv, size_t n, void* stream) {
  if (n == 0) return 0;
  if (!out || !arg || !tau_diag || !step || !stop) { set_error("moreau scaling with a device step: null pointer"); return 1; }
  hipStream_t s = as_stream(stream);
  PH_LAUNCH((moreau_scale_view_kernel<T, POST>), dim3(grid_for(n)), dim3(kBlock), 0, s, out, arg, tau_diag, step, stop, inv != 0, n);
  PH_LAUNCH_END("moreau scaling kernel (device step)");
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {
int prost_hip_moreau_prescale_view_f32(float* o, const float* a, const float* td, const float* step_dev, const int* stop_dev, int inv, size_t n, void* s) {
  return launch_moreau_scale_view<float, false>(o, a, td, step_dev, stop_dev, inv, n, s);
}
int prost_hip_moreau_prescale_view_f64(double* o, const double* a, const double* td, const double* step_dev, const int* stop_dev, int inv, size_t n, void* s) {
  return launch_moreau_scale_view<double, false>(o, a, td, step_dev, stop_dev, inv, n, s);
}
int prost_hip_moreau_postscale_view_f32(float* r, const float* a, const float* td, const float* step_dev, const int* stop_dev, int inv, size_t n, void* s) {
  return launch_moreau_scale_view<float, true>(r, a, td, step_dev, stop_dev, inv, n, s);
}
int prost_hip_moreau_postscale_view_f64(double* r, const double* a, const double* td, const double* step_dev, const int* stop_dev, int inv, size_t n, void* s) {
  return launch_moreau_scale_view<double, true>(r, a, td, step_dev, stop_dev, inv, n, s);
}
}  // extern "C"
