// CPU harness for the LAUNCH PLAN of the fused PDHG paths (tests/test_pdhg_launch_trace.py).  The host sources of the solver are
// compiled into this translation unit as they are; the kernel C ABI (include/prost_hip.h) is replaced by a recording mock, as in
// slab_schedule_harness.cpp.  Nothing is computed: every mocked launch appends one line to a trace -- entry point, iterations per
// launch, every pointer argument as the ORDINAL of the allocation it points into (prost_hip_malloc / _host_alloc number them in the
// order they are made; "-" is null), the step sizes of every iteration of the launch (%a), the use_* flags, whether sums / rule / a
// stored intermediate iterate are asked for and the iteration number passed.  Host waits, event operations, all-reduces and D2H
// copies leave a line too.  The residual sums a launch "computes" are a fixed function of the iteration number, chosen so that both
// branches of goldstein's and of boyd's rule fire within a run and (on request) the stopping test holds from some iteration on.
// The trace is a function of the host code's decisions alone -- which kernel, on which buffers, with which step sizes -- so two
// versions of backend_pdhg.cpp that print the same traces sequence the same launches.  Only the public interface is used.
//
//   pdhg_launch_trace_harness --list          names of all scenarios
//   pdhg_launch_trace_harness all             every scenario, each behind a line "@ <name>"
//   pdhg_launch_trace_harness <name> ...      the named scenarios
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include <execinfo.h>
#include <signal.h>
#include <unistd.h>

#include "prost_hip.h"

// ---- what the mock answers and how a scenario is driven -------------------------------------------------------------------------
struct MockConfig {
  int iteration_supported = 0, iteration2_profitable = 0, iterationk_max = 0, iteration3d = 0, iteration3d_pw = 0, iteration3d_x2 = 0, mc = 0, mc_x2 = 0;
  int host_transport = 0;
  int residual_iter = 1;
  long long converged_from = -1;          // the sums of residual iterations >= this one satisfy the stopping test (-1: never)
};
static MockConfig g_cfg;
static std::vector<std::string> g_log;
static void logf(const char* fmt, ...) {
  char buf[1024];
  va_list ap; va_start(ap, fmt); vsnprintf(buf, sizeof(buf), fmt, ap); va_end(ap);
  g_log.push_back(buf);
}
// allocations in the order they were made; a pointer prints as the ordinal of the allocation that holds it (+ byte offset)
struct Allocation { size_t bytes; int ordinal; };
static std::map<uintptr_t, Allocation> g_allocs;
static std::map<const void*, int> g_events;
static int g_next_ordinal = 0, g_next_event = 0;
static void* allocate(size_t bytes) {
  void* p = calloc(bytes ? bytes : 1, 1);
  g_allocs[(uintptr_t)p] = {bytes ? bytes : 1, g_next_ordinal++};
  return p;
}
static void release(void* p) { g_allocs.erase((uintptr_t)p); free(p); }
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
static std::string E(const void* e) { auto it = g_events.find(e); return it == g_events.end() ? "e?" : "e" + std::to_string(it->second); }
static const char* S(const void* stream) { return stream == (void*)0x10 ? "side" : "main"; }
static std::string D(const prost_hip_fused_desc* d) {
  char buf[96];
  snprintf(buf, sizeof(buf), "desc[arith%d masked%d a=%s b=%s]", d->arith, d->g_b_masked, P(d->g_coeff_ptr[0]).c_str(), P(d->g_coeff_ptr[1]).c_str());
  return buf;
}
static std::string Steps(const double* t, const double* s, const double* th, int g) {
  std::string out;
  char buf[128];
  for (int i = 0; i < g; i++) { snprintf(buf, sizeof(buf), "%s(%a %a %a)", i ? " " : "", t[i], s[i], th[i]); out += buf; }
  return out;
}
static unsigned long long current_iteration();          // BackendPDHG::iteration() of the running scenario (defined below)

// the four sums of residual iteration `it`: residual norms 1000 / 1 by turns (three phases: primal large, dual large, both large)
static void mock_sums_primal(unsigned long long it, double* out2) {
  const int phase = (int)((it / (unsigned long long)g_cfg.residual_iter) % 3);
  const bool done = g_cfg.converged_from >= 0 && (long long)it >= g_cfg.converged_from;
  out2[0] = done || phase == 1 ? 1.0 : 1e6; out2[1] = 4.0 + (double)(it % 5);
}
static void mock_sums_dual(unsigned long long it, double* out2) {
  const int phase = (int)((it / (unsigned long long)g_cfg.residual_iter) % 3);
  const bool done = g_cfg.converged_from >= 0 && (long long)it >= g_cfg.converged_from;
  out2[0] = done || phase == 0 ? 1.0 : 1e6; out2[1] = 9.0 + (double)(it % 7);
}
static void mock_sums(unsigned long long it, double* out4) { mock_sums_primal(it, out4); mock_sums_dual(it, out4 + 2); }

// ---- the rule kernels' state (kernels_pdhg_rule.hip), evaluated in float like BackendPDHG<float>::ResolveResiduals
static prost_hip_pdhg_rule_state g_rule;
static prost_hip_pdhg_rule_opts g_rule_opts;
static int g_rule_stop_on_convergence = 0;
static void evaluate(unsigned long long it, const double* sums, prost_hip_pdhg_rule_state* mirror) {
  if (g_rule.stopped) return;
  g_rule.prev_tau = g_rule.tau; g_rule.prev_sigma = g_rule.sigma; g_rule.prev_theta = g_rule.theta;
  g_rule.evaluations++; g_rule.last_iteration = it;
  for (int i = 0; i < 4; i++) g_rule.sums[i] = sums[i];
  const float pres = std::sqrt((float)sums[0]), pvar = std::sqrt((float)sums[1]), dres = std::sqrt((float)sums[2]), dvar = std::sqrt((float)sums[3]);
  const float eps_p = (float)(g_rule_opts.sqrt_rows * g_rule_opts.tol_abs_primal + g_rule_opts.tol_rel_primal * pvar);
  const float eps_d = (float)(g_rule_opts.sqrt_cols * g_rule_opts.tol_abs_dual + g_rule_opts.tol_rel_dual * dvar);
  g_rule.primal_res = pres; g_rule.primal_var = pvar; g_rule.dual_res = dres; g_rule.dual_var = dvar; g_rule.eps_primal = eps_p; g_rule.eps_dual = eps_d;
  float tau = (float)g_rule.tau, sigma = (float)g_rule.sigma, alpha = (float)g_rule.arg_alpha;
  if (g_rule_opts.variant == PROST_PDHG_RULE_GOLDSTEIN) {
    const float scale = eps_d / eps_p, delta = (float)g_rule_opts.arg_delta, nu = (float)g_rule_opts.arg_nu;
    if (dres > scale * pres * delta) { tau = tau / (1 - alpha); sigma = sigma * (1 - alpha); alpha = alpha * nu; }
    if (dres < scale * pres / delta) { tau = tau * (1 - alpha); sigma = sigma / (1 - alpha); alpha = alpha * nu; }
  } else if (g_rule_opts.variant == PROST_PDHG_RULE_BOYD) {
    const float delta = (float)g_rule_opts.arb_delta, at = (float)g_rule_opts.arb_tau;
    if (dres < eps_d && at * it > g_rule.arb_l) { tau /= delta; sigma *= delta; g_rule.arb_u = (long long)it; }
    else if (pres < eps_p && at * it > g_rule.arb_u) { tau *= delta; sigma /= delta; g_rule.arb_l = (long long)it; }
  }
  g_rule.tau = tau; g_rule.sigma = sigma; g_rule.arg_alpha = alpha;
  if (g_rule_stop_on_convergence && pres < eps_p && dres < eps_d) { g_rule.stopped = 1; g_rule.stop_iteration = it; }
  if (mirror) *mirror = g_rule;
}

// ---- the launches: one line each --------------------------------------------------------------------------------------------------
// single-iteration kernels (prost_hip_fused_iteration, _mc, 3d and their _rec forms)
static int single(const char* name, const prost_hip_fused_desc* d, const void* xn, const void* yn, const void* x, const void* y, const void* yp, const double* steps,
                  const void* record, int u0, int u1, int u2, int cols, double* res, const void* ws, int apply_rule, unsigned long long it,
                  prost_hip_pdhg_rule_state* mirror) {
  char st[128] = "";
  if (steps) snprintf(st, sizeof(st), " steps=(%a %a %a)", steps[0], steps[1], steps[2]);
  char rc[160] = "";
  if (record) snprintf(rc, sizeof(rc), " rec=%s rule=%d k=%llu mirror=%s", P(record).c_str(), apply_rule, it, P(mirror).c_str());
  logf("%s x1 %s out=%s,%s in=%s,%s yprev=%s%s%s use=%d%d%d cols=%d sums=%s ws=%s", name, D(d).c_str(), P(xn).c_str(), P(yn).c_str(), P(x).c_str(), P(y).c_str(),
       P(yp).c_str(), st, rc, u0, u1, u2, cols, P(res).c_str(), P(ws).c_str());
  if (record && g_rule.stopped) return 0;
  if (res) { mock_sums(record ? it : current_iteration(), res); if (record && apply_rule) evaluate(it, res, mirror); }
  return 0;
}
// multi-iteration kernels (prost_hip_fused_iteration2, _mc_x2, 3d_x2, iterationk and their _rec forms)
static int multi(const char* name, const prost_hip_fused_desc* d, int g, const void* xo, const void* yo, const void* x, const void* y, const void* xm, const void* ym,
                 const double* tau, const double* sigma, const double* theta, const void* record, int cols, double* res, const void* ws, int apply_rule,
                 unsigned long long it, prost_hip_pdhg_rule_state* mirror) {
  char rc[160] = "";
  if (record) snprintf(rc, sizeof(rc), " rec=%s rule=%d k=%llu mirror=%s", P(record).c_str(), apply_rule, it, P(mirror).c_str());
  logf("%s x%d %s out=%s,%s in=%s,%s mid=%s,%s%s%s%s cols=%d sums=%s ws=%s", name, g, D(d).c_str(), P(xo).c_str(), P(yo).c_str(), P(x).c_str(), P(y).c_str(), P(xm).c_str(),
       P(ym).c_str(), tau ? " steps=" : "", tau ? Steps(tau, sigma, theta, g).c_str() : "", rc, cols, P(res).c_str(), P(ws).c_str());
  if (record && g_rule.stopped) return 0;
  if (res) { mock_sums(record ? it : current_iteration(), res); if (record && apply_rule) evaluate(it, res, mirror); }
  return 0;
}

extern "C" {
const char* prost_hip_last_error(void) { return ""; }
int prost_hip_check_last_error(void) { return 0; }
int prost_hip_malloc(void** p, size_t bytes) { *p = allocate(bytes); return 0; }
int prost_hip_free(void* p) { release(p); return 0; }
int prost_hip_host_alloc(void** p, size_t bytes) { *p = allocate(bytes); return 0; }
int prost_hip_host_free(void* p) { release(p); return 0; }
int prost_hip_memcpy_h2d(void* d, const void* s, size_t n, void*) { memcpy(d, s, n); return 0; }
int prost_hip_memcpy_d2h(void* d, const void* s, size_t n, void* stream) { memcpy(d, s, n); logf("d2h %zu bytes from %s (%s)", n, P(s).c_str(), S(stream)); return 0; }
int prost_hip_memcpy_d2d(void* d, const void* s, size_t n, void*) { memmove(d, s, n); return 0; }
int prost_hip_memset(void* d, int v, size_t n, void*) { memset(d, v, n); return 0; }
int prost_hip_stream_create(void** s) { *s = (void*)0x10; return 0; }
int prost_hip_stream_destroy(void*) { return 0; }
int prost_hip_stream_synchronize(void* s) { logf("HOST WAIT stream %s", S(s)); return 0; }
int prost_hip_device_synchronize(void) { logf("HOST WAIT device"); return 0; }
int prost_hip_event_create(void** e) { *e = malloc(1); g_events[*e] = g_next_event++; return 0; }
int prost_hip_event_create_timing(void** e) { *e = malloc(1); g_events[*e] = g_next_event++; return 0; }
int prost_hip_event_destroy(void* e) { g_events.erase(e); free(e); return 0; }
int prost_hip_event_record(void* e, void* s) { logf("event_record %s (%s)", E(e).c_str(), S(s)); return 0; }
int prost_hip_event_synchronize(void* e) { logf("HOST WAIT event %s", E(e).c_str()); return 0; }
int prost_hip_stream_wait_event(void* s, void* e) { logf("stream_wait %s for %s", S(s), E(e).c_str()); return 0; }
int prost_hip_next_launch_events(void*, void*) { return 0; }
int prost_hip_event_elapsed_ms(void*, void*, float* ms) { *ms = 1; return 0; }
size_t prost_hip_reduce_workspace_bytes(void) { return 1 << 12; }
size_t prost_hip_pdhg_rule_record_bytes(void) { return 512; }
int prost_hip_pdhg_record_view(const void* rec, int, const void** tau, const void** sigma, const void** theta, const int** stop) {
  if (tau) *tau = rec; if (sigma) *sigma = (char*)rec + 8; if (theta) *theta = (char*)rec + 16; if (stop) *stop = (const int*)((char*)rec + 24);
  return 0;
}
int prost_hip_mem_info(size_t* f, size_t* t) { *f = *t = (size_t)1 << 34; return 0; }
int prost_hip_get_device(int* d) { *d = 0; return 0; }
int prost_hip_fill_f32(float* p, double v, size_t n, void*) { for (size_t i = 0; i < n; i++) p[i] = (float)v; return 0; }
int prost_hip_scale_f32(float*, size_t, double, void*) { return 0; }
int prost_hip_comm_is_host(void*) { return g_cfg.host_transport; }
int prost_hip_mask_merge_f32(float* bm, const float* a, const float* b, double, size_t, unsigned long long*, void*) {
  logf("mask_merge out=%s a=%s b=%s", P(bm).c_str(), P(a).c_str(), P(b).c_str()); return 0;      // (the counter stays 0: a binary mask)
}
// ---- what Initialize() asks about a description
static int gray(const prost_hip_fused_desc* d) { return !d->is3d && d->L <= 2; }
int prost_hip_fused_supported(const prost_hip_fused_desc*, int) { return 1; }
int prost_hip_fused_iteration_supported(const prost_hip_fused_desc* d, int) { return g_cfg.iteration_supported && gray(d); }
int prost_hip_fused_iteration2_supported(const prost_hip_fused_desc* d, int) { return g_cfg.iteration2_profitable && !d->is3d && d->L == 1; }
int prost_hip_fused_iteration2_profitable(const prost_hip_fused_desc* d, int) { return g_cfg.iteration2_profitable && !d->is3d && d->L == 1; }
int prost_hip_fused_iteration2_chunk_cols(const prost_hip_fused_desc*, int, int res) { return res ? 17 : 18; }
int prost_hip_fused_iteration2_arith(const prost_hip_fused_desc* d, int) { return d->arith; }
int prost_hip_fused_iterationk_max(const prost_hip_fused_desc*, int) { return g_cfg.iterationk_max; }
int prost_hip_fused_iterationk_chunk_cols(const prost_hip_fused_desc*, int, int k, int res) { return 20 + 2 * k + res; }
int prost_hip_fused_iteration3d_supported(const prost_hip_fused_desc* d, int) { return g_cfg.iteration3d && d->is3d; }
int prost_hip_fused_iteration3d_pw_supported(const prost_hip_fused_desc* d, int) { return g_cfg.iteration3d_pw && d->is3d; }
int prost_hip_fused_iteration3d_x2_supported(const prost_hip_fused_desc* d, int) { return g_cfg.iteration3d_x2 && d->is3d; }
int prost_hip_fused_iteration3d_x2_arith(const prost_hip_fused_desc* d, int) { return d->arith; }
int prost_hip_fused_iteration3d_x2_chunk_cols(const prost_hip_fused_desc*, int, int res) { return res ? 11 : 12; }
int prost_hip_fused_iteration_mc_supported(const prost_hip_fused_desc* d, int) { return g_cfg.mc && !d->is3d && d->L >= 3 && d->L <= 4; }
int prost_hip_fused_iteration_mc_x2_supported(const prost_hip_fused_desc* d, int) { return g_cfg.mc_x2 && !d->is3d && d->L >= 2 && d->L <= 4; }
int prost_hip_fused_iteration_mc_x2_profitable(const prost_hip_fused_desc* d, int) { return g_cfg.mc_x2 && !d->is3d && d->L >= 2 && d->L <= 4; }
int prost_hip_fused_iteration_mc_x2_arith(const prost_hip_fused_desc* d, int) { return d->arith; }
int prost_hip_fused_iteration_mc_x2_chunk_cols(const prost_hip_fused_desc*, int, int res) { return res ? 7 : 8; }
// ---- the operator products of a read-out (ConstraintVariables)
int prost_hip_grad2d_fwd_f32(float* r, const float* x, size_t, size_t, size_t, int, int acc, void*) { logf("grad2d_fwd out=%s in=%s acc=%d", P(r).c_str(), P(x).c_str(), acc); return 0; }
int prost_hip_grad2d_adj_f32(float* r, const float* x, size_t, size_t, size_t, int, int acc, void*) { logf("grad2d_adj out=%s in=%s acc=%d", P(r).c_str(), P(x).c_str(), acc); return 0; }
int prost_hip_grad3d_fwd_f32(float* r, const float* x, size_t, size_t, size_t, int, int acc, void*) { logf("grad3d_fwd out=%s in=%s acc=%d", P(r).c_str(), P(x).c_str(), acc); return 0; }
int prost_hip_grad3d_adj_f32(float* r, const float* x, size_t, size_t, size_t, int, int acc, void*) { logf("grad3d_adj out=%s in=%s acc=%d", P(r).c_str(), P(x).c_str(), acc); return 0; }
int prost_hip_pdhg_w_variable_f32(float* w, const float* xp, const float* x, const float*, const float* ktyp, double tau, size_t, void*) {
  logf("w_variable out=%s xprev=%s x=%s ktyprev=%s tau=%a", P(w).c_str(), P(xp).c_str(), P(x).c_str(), P(ktyp).c_str(), tau); return 0;
}
int prost_hip_pdhg_z_variable_f32(float* z, const float* yp, const float* y, const float*, const float* kx, const float* kxp, double sigma, double theta, size_t, void*) {
  logf("z_variable out=%s yprev=%s y=%s kx=%s kxprev=%s sigma=%a theta=%a", P(z).c_str(), P(yp).c_str(), P(y).c_str(), P(kx).c_str(), P(kxp).c_str(), sigma, theta); return 0;
}
// ---- the two passes
int prost_hip_fused_primal_f32(const prost_hip_fused_desc* d, float* xn, const float* x, const float* y, const float* yp, double tau, int use_kty, int use_kty_prev, double* res,
                               void* ws, void*) {
  logf("fused_primal %s out=%s x=%s y=%s yprev=%s tau=%a use=%d%d sums=%s ws=%s", D(d).c_str(), P(xn).c_str(), P(x).c_str(), P(y).c_str(), P(yp).c_str(), tau, use_kty,
       use_kty_prev, P(res).c_str(), P(ws).c_str());
  if (res) mock_sums_dual(current_iteration(), res);
  return 0;
}
int prost_hip_fused_dual_f32(const prost_hip_fused_desc* d, float* yn, const float* y, const float* xn, const float* xo, double sigma, double theta, int use_kx_prev, double* res,
                             void* ws, void*) {
  logf("fused_dual %s out=%s y=%s xnew=%s xold=%s sigma=%a theta=%a use=%d sums=%s ws=%s", D(d).c_str(), P(yn).c_str(), P(y).c_str(), P(xn).c_str(), P(xo).c_str(), sigma, theta,
       use_kx_prev, P(res).c_str(), P(ws).c_str());
  if (res) mock_sums_primal(current_iteration(), res);
  return 0;
}
// ---- one kernel per iteration
#define SINGLE(NAME)                                                                                                                                                      \
  int prost_hip_##NAME##_f32(const prost_hip_fused_desc* d, float* xn, float* yn, const float* x, const float* y, const float* yp, double tau, double sigma, double theta, \
                             int u0, int u1, int u2, int cols, double* res, void* ws, void*) {                                                                            \
    const double st[3] = {tau, sigma, theta};                                                                                                                             \
    return single(#NAME, d, xn, yn, x, y, yp, st, nullptr, u0, u1, u2, cols, res, ws, 0, 0, nullptr);                                                                     \
  }                                                                                                                                                                       \
  int prost_hip_##NAME##_rec_f32(const prost_hip_fused_desc* d, float* xn, float* yn, const float* x, const float* y, const float* yp, void* rec, int u0, int u1, int u2,  \
                                 int cols, double* res, void* ws, int apply_rule, unsigned long long it, prost_hip_pdhg_rule_state* mirror, void*) {                      \
    return single(#NAME "_rec", d, xn, yn, x, y, yp, nullptr, rec, u0, u1, u2, cols, res, ws, apply_rule, it, mirror);                                                    \
  }
SINGLE(fused_iteration)
SINGLE(fused_iteration_mc)
SINGLE(fused_iteration3d)
#undef SINGLE
int prost_hip_fused_iteration3d_pw_f32(const prost_hip_fused_desc* d, float* xn, float* yn, const float* x, const float* y, double tau, double sigma, double theta, int u0, int u1,
                                       int cols, int waves, void*) {
  const double st[3] = {tau, sigma, theta};
  return single("fused_iteration3d_pw", d, xn, yn, x, y, nullptr, st, nullptr, u0, u1, waves, cols, nullptr, nullptr, 0, 0, nullptr);
}
int prost_hip_fused_iteration3d_pw_rec_f32(const prost_hip_fused_desc* d, float* xn, float* yn, const float* x, const float* y, void* rec, int u0, int u1, int cols, int waves, void*) {
  logf("fused_iteration3d_pw_rec x1 %s out=%s,%s in=%s,%s rec=%s use=%d%d cols=%d waves=%d", D(d).c_str(), P(xn).c_str(), P(yn).c_str(), P(x).c_str(), P(y).c_str(), P(rec).c_str(),
       u0, u1, cols, waves);
  return 0;
}
// ---- several iterations per launch
#define PAIR(NAME)                                                                                                                                                       \
  int prost_hip_##NAME##_f32(const prost_hip_fused_desc* d, float* xo, float* yo, const float* x, const float* y, const double* tau, const double* sigma,                 \
                             const double* theta, int cols, double* res, void* ws, void*) {                                                                              \
    return multi(#NAME, d, 2, xo, yo, x, y, nullptr, nullptr, tau, sigma, theta, nullptr, cols, res, ws, 0, 0, nullptr);                                                 \
  }                                                                                                                                                                      \
  int prost_hip_##NAME##_rec_f32(const prost_hip_fused_desc* d, float* xo, float* yo, const float* x, const float* y, void* rec, int cols, double* res, void* ws,         \
                                 int apply_rule, unsigned long long it, prost_hip_pdhg_rule_state* mirror, void*) {                                                      \
    return multi(#NAME "_rec", d, 2, xo, yo, x, y, nullptr, nullptr, nullptr, nullptr, nullptr, rec, cols, res, ws, apply_rule, it, mirror);                             \
  }
PAIR(fused_iteration_mc_x2)
PAIR(fused_iteration3d_x2)
#undef PAIR
int prost_hip_fused_iteration2_f32(const prost_hip_fused_desc* d, float* xo, float* yo, const float* x, const float* y, float* xm, float* ym, const double* tau, const double* sigma,
                                   const double* theta, int cols, double* res, void* ws, void*) {
  return multi("fused_iteration2", d, 2, xo, yo, x, y, xm, ym, tau, sigma, theta, nullptr, cols, res, ws, 0, 0, nullptr);
}
int prost_hip_fused_iteration2_rec_f32(const prost_hip_fused_desc* d, float* xo, float* yo, const float* x, const float* y, float* xm, float* ym, void* rec, int cols, double* res,
                                       void* ws, int apply_rule, unsigned long long it, prost_hip_pdhg_rule_state* mirror, void*) {
  return multi("fused_iteration2_rec", d, 2, xo, yo, x, y, xm, ym, nullptr, nullptr, nullptr, rec, cols, res, ws, apply_rule, it, mirror);
}
int prost_hip_fused_iterationk_f32(const prost_hip_fused_desc* d, int k, float* xo, float* yo, const float* x, const float* y, const double* tau, const double* sigma,
                                   const double* theta, int cols, double* res, void* ws, void*) {
  return multi("fused_iterationk", d, k, xo, yo, x, y, nullptr, nullptr, tau, sigma, theta, nullptr, cols, res, ws, 0, 0, nullptr);
}
int prost_hip_fused_iterationk_rec_f32(const prost_hip_fused_desc* d, int k, float* xo, float* yo, const float* x, const float* y, void* rec, int cols, double* res, void* ws,
                                       int apply_rule, unsigned long long it, prost_hip_pdhg_rule_state* mirror, void*) {
  return multi("fused_iterationk_rec", d, k, xo, yo, x, y, nullptr, nullptr, nullptr, nullptr, nullptr, rec, cols, res, ws, apply_rule, it, mirror);
}
// ---- rule begin / apply, all-reduce
int prost_hip_pdhg_rule_begin_f32(void* rec, const prost_hip_pdhg_rule_opts* o, const prost_hip_fused_desc* d, double tau, double sigma, double theta, double alpha, int l, int u,
                                  int stop_on_convergence, prost_hip_pdhg_rule_state* mirror, void*) {
  memset(&g_rule, 0, sizeof(g_rule));
  g_rule_opts = *o; g_rule_stop_on_convergence = stop_on_convergence;
  g_rule.tau = g_rule.prev_tau = tau; g_rule.sigma = g_rule.prev_sigma = sigma; g_rule.theta = g_rule.prev_theta = theta; g_rule.arg_alpha = alpha; g_rule.arb_l = l; g_rule.arb_u = u;
  if (mirror) *mirror = g_rule;
  logf("rule_begin rec=%s variant=%d %s steps=(%a %a %a) alpha=%a l=%d u=%d stop_on_convergence=%d mirror=%s", P(rec).c_str(), o->variant, D(d).c_str(), tau, sigma, theta, alpha, l,
       u, stop_on_convergence, P(mirror).c_str());
  return 0;
}
int prost_hip_pdhg_rule_apply_f32(void* rec, const double* sums, unsigned long long it, prost_hip_pdhg_rule_state* mirror, void*) {
  logf("rule_apply rec=%s sums=%s k=%llu mirror=%s", P(rec).c_str(), P(sums).c_str(), it, P(mirror).c_str());
  evaluate(it, sums, mirror);
  return 0;
}
int prost_hip_allreduce_sum_f64(void*, double* buf, size_t n, void* s) { logf("allreduce %zu of %s (%s)", n, P(buf).c_str(), S(s)); return 0; }
}  // extern "C"

#include "../../prost_amd/csrc/host/common.cpp"
#include "../../prost_amd/csrc/host/linop.cpp"
#include "../../prost_amd/csrc/host/prox.cpp"
#include "../../prost_amd/csrc/host/problem.cpp"
#include "../../prost_amd/csrc/host/backend_pdhg.cpp"
#include "../../prost_amd/csrc/host/solver.cpp"

using namespace prost;
typedef BackendPDHG<float> PDHG;

static PDHG* g_backend = nullptr;
static unsigned long long current_iteration() { return g_backend ? (unsigned long long)g_backend->iteration() : 0; }

// a call through an entry point this mock does not define jumps to address 0: say where from (build with -rdynamic)
static void on_segv(int) {
  void* frames[32];
  const int n = backtrace(frames, 32);
  const char msg[] = "pdhg_launch_trace_harness: call of an entry point the mock does not define (or a crash); backtrace:\n";
  if (write(2, msg, sizeof(msg) - 1) < 0) _exit(3);
  backtrace_symbols_fd(frames, n, 2);
  _exit(3);
}

// ---- scenarios -----------------------------------------------------------------------------------------------------------------
struct Family {
  const char* name;
  int is3d; size_t L;
  MockConfig mock;                       // (the _supported answers; the rest is filled per scenario)
  bool allow_single, allow_pair;
  int arithmetic, group_max;
  bool masked;
};
static MockConfig Mock(int it, int it2, int kmax, int d3, int pw, int d3x2, int mc, int mcx2) {
  MockConfig m; m.iteration_supported = it; m.iteration2_profitable = it2; m.iterationk_max = kmax; m.iteration3d = d3; m.iteration3d_pw = pw; m.iteration3d_x2 = d3x2; m.mc = mc; m.mc_x2 = mcx2;
  return m;
}
static const Family kFamilies[] = {
    {"twopass", 0, 1, Mock(1, 1, 6, 0, 0, 0, 0, 0), false, true, PROST_HIP_ARITH_EXACT, 0, false},
    {"single", 0, 1, Mock(1, 1, 6, 0, 0, 0, 0, 0), true, false, PROST_HIP_ARITH_EXACT, 0, false},
    {"pair", 0, 1, Mock(1, 1, 0, 0, 0, 0, 0, 0), true, true, PROST_HIP_ARITH_EXACT, 0, false},
    {"group3", 0, 1, Mock(1, 1, 6, 0, 0, 0, 0, 0), true, true, PROST_HIP_ARITH_EXACT, 3, false},
    {"group4", 0, 1, Mock(1, 1, 6, 0, 0, 0, 0, 0), true, true, PROST_HIP_ARITH_EXACT, 4, false},
    {"fmad", 0, 1, Mock(1, 1, 6, 0, 0, 0, 0, 0), true, true, PROST_HIP_ARITH_FMAD, 0, false},
    {"mc3", 0, 3, Mock(1, 1, 6, 0, 0, 0, 1, 1), true, true, PROST_HIP_ARITH_EXACT, 0, false},
    {"mc3pair", 0, 3, Mock(1, 1, 6, 0, 0, 0, 0, 1), true, true, PROST_HIP_ARITH_EXACT, 0, false},
    {"vol", 1, 2, Mock(1, 1, 6, 1, 0, 1, 0, 0), true, true, PROST_HIP_ARITH_EXACT, 0, false},
    {"volpw", 1, 3, Mock(1, 1, 6, 1, 1, 1, 0, 0), true, true, PROST_HIP_ARITH_EXACT, 0, false},
    {"volpair", 1, 4, Mock(1, 1, 6, 1, 1, 1, 0, 0), true, true, PROST_HIP_ARITH_EXACT, 0, false},
    {"l2", 0, 2, Mock(1, 1, 6, 0, 0, 0, 1, 1), true, true, PROST_HIP_ARITH_EXACT, 0, false},
    // (below: a reduced set of rules / periods / drivers)
    {"mask", 0, 1, Mock(1, 1, 0, 0, 0, 0, 0, 0), true, true, PROST_HIP_ARITH_EXACT, 0, true},
    {"volpaironly", 1, 4, Mock(1, 1, 6, 0, 0, 1, 0, 0), true, true, PROST_HIP_ARITH_EXACT, 0, false},
    {"mc3fmad", 0, 3, Mock(1, 1, 6, 0, 0, 0, 1, 1), true, true, PROST_HIP_ARITH_FMAD, 0, false},
    {"volpairfmad", 1, 4, Mock(1, 1, 6, 1, 1, 1, 0, 0), true, true, PROST_HIP_ARITH_FMAD, 0, false},
};
static const int kFullFamilies = 12;
static const char* kRules[] = {"alg1", "alg2", "goldstein", "boyd"};
static const int kPeriods[] = {1, 2, 3, 7, 10};
static const char* kDrivers[] = {"solve", "iterate", "poll", "stop"};
static const char* kComms[] = {"", "comm", "commnospec", "nospec", "slab", "slabhost"};

struct Scenario { int family, rule, period, driver, comm; };
static std::string Name(const Scenario& s) {
  std::string n = std::string(kFamilies[s.family].name) + "." + kRules[s.rule] + "." + kDrivers[s.driver];
  if (s.comm) n += std::string(".") + kComms[s.comm];
  return n + ".r" + std::to_string(s.period);
}
static std::vector<Scenario> AllScenarios() {
  std::vector<Scenario> all;
  const int nfam = (int)(sizeof(kFamilies) / sizeof(kFamilies[0]));
  for (int f = 0; f < nfam; f++)
    for (int r = 0; r < 4; r++)
      for (int d = 0; d < 4; d++)
        for (int p = 0; p < 5; p++) {
          if (d == 3 && kPeriods[p] != 2 && kPeriods[p] != 3) continue;                 // the stopping run: one even and one odd period
          if (f >= kFullFamilies && (d == 2 || (kPeriods[p] != 2 && kPeriods[p] != 7))) continue;
          all.push_back({f, r, kPeriods[p], d, 0});
        }
  // with a communicator (plain: the sums are all-reduced; slabs: owned columns and the halo exchange hook on either transport), with and
  // without the speculative launch
  const int comm_fam[] = {1, 2, 5, 6};                  // single, pair, fmad (groups), mc3
  for (int f : comm_fam)
    for (int r = 0; r < 4; r++)
      for (int c = 1; c <= 5; c++)
        for (int p : {3, 10}) {
          if ((c == 2 || c == 3) && r >= 2) continue;                                   // speculation: alg1 / alg2 only
          if (c >= 4 && f >= 5) continue;                                               // slabs: the gray-value kernels
          all.push_back({f, r, p, c >= 4 ? 1 : 0, c});
          if (c >= 4) all.push_back({f, r, p, 3, c});
        }
  for (int r = 0; r < 4; r++) for (int p : {1, 10}) all.push_back({2, r, p, 0, 5});          // pairs on the host-callback transport, read-outs between launches
  return all;
}

static void Run(const Scenario& sc) {
  const Family& fam = kFamilies[sc.family];
  g_log.clear(); g_allocs.clear(); g_events.clear(); g_next_ordinal = g_next_event = 0;
  g_cfg = fam.mock;
  g_cfg.residual_iter = sc.period;
  g_cfg.host_transport = sc.comm == 5;
  g_cfg.converged_from = sc.driver == 3 ? 37 : -1;
  const bool slab = sc.comm >= 4, comm = sc.comm == 1 || sc.comm == 2 || slab;
  const size_t nx = slab ? 24 : 8, ny = 8, pixels = nx * ny, n = pixels * fam.L, m = fam.is3d ? 3 * n : 2 * n;
  auto problem = std::make_shared<Problem<float>>();
  problem->SetDimensions(m, n);
  problem->SetScalingAlpha(1);
  if (fam.is3d) problem->AddBlock(std::make_shared<BlockGradient3D<float>>(0, 0, nx, ny, fam.L, false));
  else problem->AddBlock(std::make_shared<BlockGradient2D<float>>(0, 0, nx, ny, fam.L, false));
  std::array<std::vector<float>, 7> cg = {{{1.f}, std::vector<float>(n, 0.5f), {10.f}, {0.f}, {0.f}, {0.f}, {0.f}}};
  if (fam.masked) { cg[0] = std::vector<float>(n, 1.f); cg[0][3] = 0.f; }
  std::array<std::vector<float>, 7> cf = {{{1.f}, {1.f}, {1.f}, {0.f}, {0.f}, {0.f}, {0.f}}};
  problem->AddProx_g(std::make_shared<ProxElemDispatch<float>>(PROST_OP_1D, PROST_FN_SQUARE, 0, n, 1, false, true, cg));
  problem->AddProx_fstar(std::make_shared<ProxElemDispatch<float>>(PROST_OP_NORM2, PROST_FN_IND_LEQ0, 0, fam.is3d ? n : pixels, fam.is3d ? 3 : 2 * fam.L, false, false, cf));
  PDHG::Options bo;
  const PDHG::StepsizeVariant variants[] = {PDHG::kPDHGStepsAlg1, PDHG::kPDHGStepsAlg2, PDHG::kPDHGStepsResidualGoldstein, PDHG::kPDHGStepsResidualBoyd};
  bo.stepsize_variant = variants[sc.rule]; bo.residual_iter = sc.period; bo.scale_steps_operator = false;
  bo.alg2_gamma = 0.35f; bo.tau0 = 0.25; bo.sigma0 = 0.5;
  bo.allow_single_kernel = fam.allow_single; bo.allow_pair_kernel = fam.allow_pair;
  bo.arithmetic = fam.arithmetic; bo.group_max = fam.group_max;
  bo.allow_speculation = !(sc.comm == 2 || sc.comm == 3);
  auto backend = std::make_shared<PDHG>(bo);
  if (comm) backend->SetCommunicator((void*)0x1, 2 * m, 2 * n);
  if (slab) backend->SetOwnedColumns(4, nx - 4);
  backend->EnableKernelTiming(true, 4);
  Solver<float> solver(problem, backend);
  Solver<float>::Options so;
  so.tol_rel_primal = so.tol_rel_dual = 0; so.tol_abs_primal = so.tol_abs_dual = 1;      // eps = sqrt(rows), sqrt(cols): between the mock's residual norms 1 and 1000
  int polls = 0, exchanges = 0;
  const char* result = "";
  try {
    switch (sc.driver) {
      case 0: so.max_iters = 61; so.num_cback_calls = 7; break;
      case 1: so.max_iters = 1 << 20; so.num_cback_calls = 0; break;
      case 2: so.max_iters = 45; so.num_cback_calls = 0; break;
      default: so.max_iters = 80; so.num_cback_calls = 0; break;
    }
    solver.SetOptions(so);
    solver.Initialize();
    g_backend = backend.get();
    logf("-- initialized: path %s device_rules %d single_kernel %d sharded_path %d fused_channels %zu arithmetic %d group_max %d", backend->path().c_str(), (int)backend->device_rules(),
         (int)backend->single_kernel(), (int)backend->sharded_path(), backend->fused_channels(), backend->arithmetic(), backend->group_max());
    if (slab) backend->SetExchangeHook([&]() { exchanges++; logf("HALO EXCHANGE"); }, 6, 0);
    if (sc.driver == 0) {
      solver.SetIntermCallback([&](int it, const std::vector<float>&, const std::vector<float>&) { logf("-- callback at %d", it); return false; });
      result = solver.Solve() == Solver<float>::kStoppedMaxIters ? "max_iters" : "other";
    } else if (sc.driver == 1) {
      const int budgets[] = {1, 2, 3, 5, 247, 1, 2, 3, 5, 250};
      for (int b : budgets) { solver.Iterate(b); logf("-- budget %d done: iteration %zu", b, backend->iteration()); }
    } else if (sc.driver == 2) {
      solver.SetStoppingCallback([&]() { polls++; logf("-- poll %d at %zu", polls, backend->iteration()); return polls == 27; });
      result = solver.Solve() == Solver<float>::kStoppedUser ? "user" : "other";
    } else {
      const Solver<float>::ConvergenceResult r = solver.Solve();
      result = r == Solver<float>::kConverged ? "converged" : r == Solver<float>::kStoppedMaxIters ? "max_iters" : "user";
    }
    logf("-- end: result %s iteration %zu steps=(%a %a %a) pair_launches %zu speculative %zu adopted %zu device_rule_batches %zu exchanges %d since_exchange %zu path %s", result,
         backend->iteration(), (double)backend->tau(), (double)backend->sigma(), (double)backend->theta(), backend->pair_launches(), backend->speculative_launches(),
         backend->speculative_adopted(), backend->device_rule_batches(), exchanges, backend->since_exchange(), backend->path().c_str());
    logf("-- residuals %a %a %a %a", (double)backend->primal_residual(), (double)backend->dual_residual(), (double)backend->primal_var_norm(), (double)backend->dual_var_norm());
    std::vector<Backend<float>::KernelTime> times;
    backend->KernelTimes(times);
    for (const auto& t : times) logf("-- kernel %s sampled %zu launches %zu iterations %d cols %d", t.name.c_str(), t.sampled, t.launches, t.iterations_per_launch, t.chunk_cols);
    float *x, *y, *xp, *yp;
    backend->device_iterates(x, y, xp, yp);
    logf("-- iterates x=%s y=%s xprev=%s yprev=%s", P(x).c_str(), P(y).c_str(), P(xp).c_str(), P(yp).c_str());
  } catch (const std::exception& e) {
    logf("-- EXCEPTION %s", e.what());
  }
  g_backend = nullptr;
  solver.Release();
  std::printf("@ %s\n", Name(sc).c_str());
  for (const std::string& l : g_log) std::printf("%s\n", l.c_str());
}

int main(int argc, char** argv) {
  signal(SIGSEGV, on_segv);
  const std::vector<Scenario> all = AllScenarios();
  if (argc < 2 || !strcmp(argv[1], "--list")) { for (const Scenario& s : all) std::printf("%s\n", Name(s).c_str()); return 0; }
  for (int a = 1; a < argc; a++) {
    bool found = false;
    for (const Scenario& s : all) if (!strcmp(argv[a], "all") || Name(s) == argv[a]) { Run(s); found = true; }
    if (!found) { std::fprintf(stderr, "no scenario %s\n", argv[a]); return 2; }
  }
  return 0;
}
