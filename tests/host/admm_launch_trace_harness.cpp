// CPU harness for what BackendADMM LAUNCHES (tests/test_admm_launch_trace.py), the counterpart of pdhg_launch_trace_harness.cpp and
// written to its conventions: the host sources of the solver are compiled into this translation unit as they are, the kernel C ABI
// (include/prost_hip.h) is a recording mock, nothing is computed.  Every mocked launch appends one line to a trace -- entry point,
// stage / round number, every pointer argument as the ORDINAL of the allocation it points into (+ byte offset; "-" is null, "?" is
// memory the mock did not hand out), every scalar as %a -- and so do host waits, D2H and D2D copies, event operations, stream capture,
// graph launches and all-reduces.  What the "device" answers is a fixed function of the iteration and round number:
//   * the stop word: on round `stop_round` of every second device solve the mock stores the descriptor's epoch to host_done;
//   * the norms of the host-driven CGLS: per outer iteration, by turns, |s| < eps at the start, the tolerance met on round 2, maxit
//     reached, and dlt <= 0 on round 0 followed by the tolerance on round 1;
//   * the four residual norms: by turns both large, dual small, primal small, both large -- both branches of the rho adaptation fire
//     within a run, and there are stretches without a rescale.
// The trace is a function of the host code's decisions alone, so two versions of backend_admm.cpp that print the same traces
// sequence the same launches.  Only the public interface is used.
//
//   admm_launch_trace_harness --list          names of all scenarios
//   admm_launch_trace_harness all             every scenario, each behind a line "@ <name>"
//   admm_launch_trace_harness <name> ...      the named scenarios
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <tuple>
#include <vector>

#include <execinfo.h>
#include <signal.h>
#include <unistd.h>

#include "prost_hip.h"

// ---- what the mock answers ----------------------------------------------------------------------------------------------------------
struct MockConfig {
  int fused_op_supported = 1, pixel_op_supported = 1;
  int stop_round = -1;                    // the stop word is stored on this round of every second device solve (-1: never)
};
static MockConfig g_cfg;
static int g_solves = 0;                  // device solves begun (INIT_X / cgls_init_fused)
static int g_staged_round = 0;            // STEP_S stages since the last INIT_X
static int g_host_iteration = 0;          // iterations of the host-driven sequence begun (PROST_ADMM_TEMP1 launches)
static int g_nrm2_calls = 0;              // nrm2 calls since the phase began
static bool g_nrm2_residuals = false;     // phase: false = inside Cgls, true = the residual norms
static int g_residual_evals = 0;
static std::vector<std::string> g_log;
static void logf(const char* fmt, ...) {
  char buf[4096];
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
static std::string E(const void* e) { if (!e) return "-"; auto it = g_events.find(e); return it == g_events.end() ? "e?" : "e" + std::to_string(it->second); }
static const char* S(const void* stream) { return stream == (void*)0x10 ? "side" : "main"; }
#define PS(x) P(x).c_str()

static std::string Cg(const prost_hip_cgls_desc* d) {
  char buf[512];
  snprintf(buf, sizeof(buf), "cg[state=%s ws=%s b=%s x=%s p=%s q=%s r=%s s=%s t=%s sigma=%s tau=%s m=%llu n=%llu shift=%a tol=%a done=%s epoch=%d]", PS(d->state), PS(d->workspace),
           PS(d->b), PS(d->x), PS(d->p), PS(d->q), PS(d->r), PS(d->s), PS(d->t), PS(d->sigma), PS(d->tau), (unsigned long long)d->m, (unsigned long long)d->n, d->shift, d->tol,
           PS(d->host_done), d->epoch);
  return buf;
}
static std::string Admm(const prost_hip_admm_desc* d) {
  char buf[512];
  snprintf(buf, sizeof(buf), "admm[ws=%s x=%s,%s,%s z=%s,%s,%s temp=%s,%s,%s kx=%s kty=%s sigma=%s tau=%s m=%llu n=%llu alpha=%a rho=%a out4=%s]", PS(d->workspace), PS(d->x_half),
           PS(d->x_proj), PS(d->x_dual), PS(d->z_half), PS(d->z_proj), PS(d->z_dual), PS(d->temp1), PS(d->temp2), PS(d->temp3), PS(d->kx), PS(d->kty), PS(d->sigma), PS(d->tau),
           (unsigned long long)d->m, (unsigned long long)d->n, d->alpha, d->rho, PS(d->out4));
  return buf;
}
// every field of the blocks in use
static std::string Op(const prost_hip_fused_op* op) {
  std::string out = "op[" + std::to_string(op->nblocks);
  char buf[640];
  for (int i = 0; i < op->nblocks && i < PROST_HIP_OP_MAX_BLOCKS; i++) {
    const prost_hip_op_block& o = op->block[i];
    snprintf(buf, sizeof(buf), " {kind=%d at=%llu,%llu size=%llux%llu grid=%llu,%llu,%llu csr=%s,%s,%s csr_t=%s,%s,%s pat=%s,%s,%s,%s pat_t=%s,%s,%s,%s anchor=%s,%s}", o.kind,
             (unsigned long long)o.row, (unsigned long long)o.col, (unsigned long long)o.nrows, (unsigned long long)o.ncols, (unsigned long long)o.nx, (unsigned long long)o.ny,
             (unsigned long long)o.L, PS(o.val), PS(o.ptr), PS(o.ind), PS(o.val_t), PS(o.ptr_t), PS(o.ind_t), PS(o.ids), PS(o.pptr), PS(o.rel), PS(o.pval), PS(o.ids_t), PS(o.pptr_t), PS(o.rel_t),
             PS(o.pval_t), PS(o.anchor), PS(o.anchor_t));
    out += buf;
  }
  return out + "]";
}
static std::string OpShort(const prost_hip_fused_op* op) {
  std::string out = "op[" + std::to_string(op->nblocks) + ":";
  for (int i = 0; i < op->nblocks && i < PROST_HIP_OP_MAX_BLOCKS; i++) out += " " + std::to_string(op->block[i].kind);
  return out + "]";
}
static std::string Pix(const prost_hip_pixel_op* o) {
  char buf[640];
  snprintf(buf, sizeof(buf), "pix[%llux%llu L=%d has_d=%d d_first=%d d_row=%llu g_row=%llu w=%s alt=%s,%s sigma_grad=%a d_csr=%d d=%s,%s,%s dt=%s,%s,%s]", (unsigned long long)o->nx,
           (unsigned long long)o->ny, o->L, o->has_d, o->d_first, (unsigned long long)o->d_row, (unsigned long long)o->g_row, PS(o->w), PS(o->p_alt), PS(o->r_alt), o->sigma_grad, o->d_csr,
           PS(o->d_val), PS(o->d_ptr), PS(o->d_ind), PS(o->dt_val), PS(o->dt_ptr), PS(o->dt_ind));
  return buf;
}

// the four residual norms of residual evaluation e: {primal residual, primal variable norm, dual residual, dual variable norm}
static void mock_residuals(int e, double* out4) {
  const int phase = e % 4;
  out4[0] = phase == 2 ? 1.0 : 1000.0; out4[1] = 4.0 + (double)(e % 5);
  out4[2] = phase == 1 ? 1.0 : 1000.0; out4[3] = 9.0 + (double)(e % 7);
}
// the norms Cgls reads, call c of outer iteration `it` (see the head of this file)
static double mock_cg_norm(int it, int c) {
  const int mode = it % 4;
  if (c < 3) return mode == 0 ? 0.0 : 1.0;                       // |x|, |s|, |x| before the first round
  const int j = (c - 3) / 4, which = (c - 3) % 4;                // |p|, |q|, |s|, |x| of round j
  if (which == 3) return 1.0;
  if (which == 2) return (mode == 1 && j >= 2) || (mode == 3 && j >= 1) ? 0x1p-40 : 0.5;
  return mode == 3 && j == 0 ? 0.0 : 1.0;
}
static void stop_word(const prost_hip_cgls_desc* d, int round) {
  if (g_cfg.stop_round == round && g_solves % 2 == 0 && d->host_done) { *d->host_done = d->epoch; logf("   (device: stop word := %d)", d->epoch); }
}

extern "C" {
const char* prost_hip_last_error(void) { return ""; }
int prost_hip_check_last_error(void) { return 0; }
int prost_hip_malloc(void** p, size_t bytes) { *p = allocate(bytes); return 0; }
int prost_hip_free(void* p) { release(p); return 0; }
int prost_hip_host_alloc(void** p, size_t bytes) { *p = allocate(bytes); return 0; }
int prost_hip_host_free(void* p) { release(p); return 0; }
int prost_hip_memcpy_h2d(void* d, const void* s, size_t n, void*) { memcpy(d, s, n); return 0; }
int prost_hip_memcpy_d2h(void* d, const void* s, size_t n, void* stream) { memcpy(d, s, n); logf("d2h %zu bytes from %s (%s)", n, PS(s), S(stream)); return 0; }
int prost_hip_memcpy_d2d(void* d, const void* s, size_t n, void* stream) { memmove(d, s, n); logf("d2d %zu bytes %s <- %s (%s)", n, PS(d), PS(s), S(stream)); return 0; }
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
int prost_hip_event_elapsed_ms(void* a, void* b, float* ms) { logf("event_elapsed %s .. %s", E(a).c_str(), E(b).c_str()); *ms = 1; return 0; }
int prost_hip_stream_begin_capture(void* s) { logf("begin_capture (%s)", S(s)); return 0; }
int prost_hip_stream_end_capture(void* s, void** graph) { *graph = malloc(1); logf("end_capture (%s)", S(s)); return 0; }
int prost_hip_graph_launch(void*, void* s) { logf("graph_launch (%s)", S(s)); return 0; }
int prost_hip_graph_destroy(void* g) { free(g); return 0; }
size_t prost_hip_reduce_workspace_bytes(void) { return 1 << 12; }
size_t prost_hip_cgls_state_bytes(void) { return 128; }
size_t prost_hip_cgls_workspace_bytes(void) { return 1 << 12; }
int prost_hip_mem_info(size_t* f, size_t* t) { *f = *t = (size_t)1 << 34; return 0; }
int prost_hip_get_device(int* d) { *d = 0; return 0; }
int prost_hip_fill_f32(float* p, double v, size_t n, void*) { for (size_t i = 0; i < n; i++) p[i] = (float)v; return 0; }
int prost_hip_allreduce_sum_f64(void*, double* buf, size_t n, void* s) { logf("allreduce %zu of %s (%s)", n, PS(buf), S(s)); return 0; }

// ---- the products and proxes of the staged and the host-driven sequence
int prost_hip_scale_f32(float* x, size_t n, double beta, void* s) { logf("scale %s n=%zu beta=%a (%s)", PS(x), n, beta, S(s)); return 0; }
int prost_hip_negate_f32(float* x, size_t n, void* s) { logf("negate %s n=%zu (%s)", PS(x), n, S(s)); return 0; }
int prost_hip_grad2d_fwd_f32(float* r, const float* x, size_t, size_t, size_t, int lf, int acc, void* s) { logf("grad2d_fwd out=%s in=%s label_first=%d acc=%d (%s)", PS(r), PS(x), lf, acc, S(s)); return 0; }
int prost_hip_grad2d_adj_f32(float* r, const float* x, size_t, size_t, size_t, int lf, int acc, void* s) { logf("grad2d_adj out=%s in=%s label_first=%d acc=%d (%s)", PS(r), PS(x), lf, acc, S(s)); return 0; }
int prost_hip_csr_spmv_f32(float* r, const float* x, size_t rows, size_t nnz, const float* v, const int32_t* p, const int32_t* i, void* s) {
  logf("csr_spmv out=%s in=%s rows=%zu nnz=%zu csr=%s,%s,%s (%s)", PS(r), PS(x), rows, nnz, PS(v), PS(p), PS(i), S(s)); return 0;
}
int prost_hip_csr_spmv_acc_f32(float* r, const float* x, size_t rows, size_t nnz, const float* v, const int32_t* p, const int32_t* i, void* s) {
  logf("csr_spmv_acc out=%s in=%s rows=%zu nnz=%zu csr=%s,%s,%s (%s)", PS(r), PS(x), rows, nnz, PS(v), PS(p), PS(i), S(s)); return 0;
}
int prost_hip_diags_fwd_f32(float* r, const float* x, size_t, size_t, size_t nd, const int64_t* o, const float* f, void* s) { logf("diags_fwd out=%s in=%s ndiags=%zu tab=%s,%s (%s)", PS(r), PS(x), nd, PS(o), PS(f), S(s)); return 0; }
int prost_hip_diags_adj_f32(float* r, const float* x, size_t, size_t, size_t nd, const int64_t* o, const float* f, int, void* s) { logf("diags_adj out=%s in=%s ndiags=%zu tab=%s,%s (%s)", PS(r), PS(x), nd, PS(o), PS(f), S(s)); return 0; }
int prost_hip_prox_elem_f32(int op, int fn, float* res, const float* arg, const float* td, double tau, int inv, size_t count, size_t dim, int il, const float* const*, const double*, void* s) {
  logf("prox_elem op=%d fn=%d out=%s arg=%s tau_diag=%s tau=%a invert=%d count=%zu dim=%zu interleaved=%d (%s)", op, fn, PS(res), PS(arg), PS(td), tau, inv, count, dim, il, S(s)); return 0;
}
int prost_hip_prox_elem_moreau_f32(int op, int fn, float* res, const float* arg, const float* td, double tau, int inv, size_t count, size_t dim, int il, const float* const*, const double*, void* s) {
  logf("prox_elem_moreau op=%d fn=%d out=%s arg=%s tau_diag=%s tau=%a invert=%d count=%zu dim=%zu interleaved=%d (%s)", op, fn, PS(res), PS(arg), PS(td), tau, inv, count, dim, il, S(s)); return 0;
}

// ---- the host-driven sequence: one launch per functor, one blocking copy per norm
int prost_hip_admm_elem_f32(int op, float* o, const float* a, const float* b, const float* c, const float* d, double alpha, double beta, size_t n, void* s) {
  if (op == PROST_ADMM_TEMP1) { g_host_iteration++; g_nrm2_calls = 0; g_nrm2_residuals = false; }
  if (op == PROST_ADMM_XPROJ) { g_nrm2_calls = 0; g_nrm2_residuals = true; }
  logf("admm_elem op=%d out=%s a=%s b=%s c=%s d=%s alpha=%a beta=%a n=%zu (%s)", op, PS(o), PS(a), PS(b), PS(c), PS(d), alpha, beta, n, S(s)); return 0;
}
int prost_hip_nrm2_f32(double* out, const float* x, size_t n, void* ws, void* s) {
  double v;
  if (g_nrm2_residuals) {
    double r[4]; mock_residuals(g_residual_evals, r);
    const int order[4] = {0, 1, 3, 2};                           // the sequence asks for the dual variable norm before the dual residual
    v = r[order[g_nrm2_calls % 4]];
    if (++g_nrm2_calls % 4 == 0) g_residual_evals++;
  } else {
    v = mock_cg_norm(g_host_iteration - 1, g_nrm2_calls++);
  }
  out[0] = v; out[1] = 0;
  logf("nrm2 out=%s x=%s n=%zu ws=%s (%s) -> %a", PS(out), PS(x), n, PS(ws), S(s), v); return 0;
}
int prost_hip_axpy_f32(float* y, const float* x, double alpha, size_t n, void* s) { logf("axpy y=%s x=%s alpha=%a n=%zu (%s)", PS(y), PS(x), alpha, n, S(s)); return 0; }

// ---- the device-resident solves
int prost_hip_cgls_stage_f32(int stage, const prost_hip_cgls_desc* d, void* s) {
  logf("cgls_stage %d %s (%s)", stage, Cg(d).c_str(), S(s));
  if (stage == PROST_CGLS_INIT_X) { g_solves++; g_staged_round = 0; }
  if (stage == PROST_CGLS_STEP_S) stop_word(d, g_staged_round++);
  return 0;
}
int prost_hip_cgls_result_at(const void* state, int index, prost_hip_cgls_result_t* out, void* s) {
  logf("cgls_result_at state=%s index=%d (%s)", PS(state), index, S(s));
  memset(out, 0, sizeof(*out)); out->iterations = 100 + index;
  return 0;
}
int prost_hip_fused_op_supported(const prost_hip_fused_op* op, uint64_t m, uint64_t n) {
  logf("fused_op_supported? %s m=%llu n=%llu -> %d", Op(op).c_str(), (unsigned long long)m, (unsigned long long)n, g_cfg.fused_op_supported); return g_cfg.fused_op_supported;
}
int prost_hip_pixel_op_supported(const prost_hip_pixel_op* op, uint64_t m, uint64_t n, int dtype) {
  logf("pixel_op_supported? %s m=%llu n=%llu dtype=%d -> %d", Pix(op).c_str(), (unsigned long long)m, (unsigned long long)n, dtype, g_cfg.pixel_op_supported); return g_cfg.pixel_op_supported;
}
int prost_hip_cgls_init_fused_f32(const prost_hip_cgls_desc* d, const prost_hip_fused_op* op, void* s) {
  g_solves++;
  logf("cgls_init_fused %s %s (%s)", Cg(d).c_str(), Op(op).c_str(), S(s)); return 0;
}
int prost_hip_cgls_round_f32(const prost_hip_cgls_desc* d, const prost_hip_fused_op* op, int round, void* s) {
  logf("cgls_round %d %s %s (%s)", round, Cg(d).c_str(), OpShort(op).c_str(), S(s)); stop_word(d, round); return 0;
}
int prost_hip_cgls_round_timed_f32(const prost_hip_cgls_desc* d, const prost_hip_fused_op* op, int round, void* const* ev, void* s) {
  std::string e;
  for (int i = 0; i < 8; i++) e += (i ? "," : "") + E(ev[i]);
  logf("cgls_round_timed %d %s %s events=%s (%s)", round, Cg(d).c_str(), OpShort(op).c_str(), e.c_str(), S(s)); stop_word(d, round); return 0;
}
int prost_hip_cgls_pixel_round_f32(const prost_hip_cgls_desc* d, const prost_hip_pixel_op* op, int round, void* s) {
  logf("cgls_pixel_round %d %s %s (%s)", round, Cg(d).c_str(), Pix(op).c_str(), S(s)); stop_word(d, round); return 0;
}
int prost_hip_cgls_pixel_round_timed_f32(const prost_hip_cgls_desc* d, const prost_hip_pixel_op* op, int round, void* const* ev, void* s) {
  std::string e;
  for (int i = 0; i < 4; i++) e += (i ? "," : "") + E(ev[i]);
  logf("cgls_pixel_round_timed %d %s %s events=%s (%s)", round, Cg(d).c_str(), Pix(op).c_str(), e.c_str(), S(s)); stop_word(d, round); return 0;
}
int prost_hip_cgls_pixel_close_f32(const prost_hip_cgls_desc* d, const prost_hip_pixel_op* op, int last, void* s) {
  logf("cgls_pixel_close %d %s %s (%s)", last, Cg(d).c_str(), Pix(op).c_str(), S(s)); return 0;
}
int prost_hip_admm_stage_f32(int stage, const prost_hip_admm_desc* d, void* s) {
  logf("admm_stage %d %s (%s)", stage, Admm(d).c_str(), S(s));
  if (stage == PROST_ADMM_STAGE_RES_X) mock_residuals(g_residual_evals++, d->out4);
  return 0;
}
int prost_hip_admm_fused_stage_f32(int stage, const prost_hip_admm_desc* d, const prost_hip_fused_op* op, void* s) {
  logf("admm_fused_stage %d %s %s (%s)", stage, Admm(d).c_str(), OpShort(op).c_str(), S(s));
  if (stage == PROST_ADMM_FUSED_RES) mock_residuals(g_residual_evals++, d->out4);
  return 0;
}
}  // extern "C"

#include "../../prost_amd/csrc/host/common.cpp"
#include "../../prost_amd/csrc/host/linop.cpp"
#include "../../prost_amd/csrc/host/prox.cpp"
#include "../../prost_amd/csrc/host/problem.cpp"
#include "../../prost_amd/csrc/host/backend_admm.cpp"
#include "../../prost_amd/csrc/host/solver.cpp"

using namespace prost;
typedef BackendADMM<float> ADMM;

// a call through an entry point this mock does not define jumps to address 0: say where from (addresses only: the build cannot
// export its symbols, the undefined entry points would then have to resolve at start-up; resolve them with addr2line)
static void on_segv(int) {
  void* frames[32];
  const int n = backtrace(frames, 32);
  const char msg[] = "admm_launch_trace_harness: call of an entry point the mock does not define (or a crash); backtrace:\n";
  if (write(2, msg, sizeof(msg) - 1) < 0) _exit(3);
  backtrace_symbols_fd(frames, n, 2);
  _exit(3);
}

// ---- operators ------------------------------------------------------------------------------------------------------------------
static const size_t kNx = 6, kNy = 5, kPix = kNx * kNy;
typedef std::vector<std::tuple<int, int, float>> Triplets;      // (row, column, value)
static std::shared_ptr<Block<float>> Sparse(size_t row, size_t col, int m, int n, Triplets t) {
  std::sort(t.begin(), t.end(), [](const std::tuple<int, int, float>& a, const std::tuple<int, int, float>& b) {
    return std::make_pair(std::get<1>(a), std::get<0>(a)) < std::make_pair(std::get<1>(b), std::get<0>(b));
  });
  std::vector<float> val; std::vector<int32_t> ptr(n + 1, 0), ind;
  for (const auto& e : t) { ptr[std::get<1>(e) + 1]++; ind.push_back(std::get<0>(e)); val.push_back(std::get<2>(e)); }
  for (int c = 0; c < n; c++) ptr[c + 1] += ptr[c];
  return std::shared_ptr<Block<float>>(BlockSparse<float>::CreateFromCSC(row, col, m, n, (int)t.size(), val, ptr, ind));
}
// D couples the L channels of one pixel: row i has its entries at columns i + c pixels
static Triplets Pointwise(size_t rows, size_t L) {
  Triplets t;
  for (size_t i = 0; i < rows; i++) for (size_t c = 0; c < L; c++) t.emplace_back((int)i, (int)(i + c * rows), 1.f + 0.25f * (float)((i + c) % 3));
  return t;
}
// one row per pixel that gathers at ANOTHER pixel: channel 0 of the next pixel and channel 1 of its own (columns >= `cols` are left out)
static Triplets Warp(size_t rows, size_t cols) {
  Triplets t;
  for (size_t i = 0; i < rows; i++) {
    t.emplace_back((int)i, (int)((i + 1) % kPix), 0.5f);
    if (kPix + i < cols) t.emplace_back((int)i, (int)(kPix + i), -1.5f);
  }
  return t;
}
static std::shared_ptr<Block<float>> Grad(size_t row, size_t col, size_t L, bool label_first = false) { return std::make_shared<BlockGradient2D<float>>(row, col, kNx, kNy, L, label_first); }

enum Shape { kDiagFirst, kDiagSecond, kCsrFirst, kCsrSecond, kGradOnly,
             // the shapes DescribeOperator turns away
             kManyBlocks, kNoDescribe, kCsrRow, kCsrCol, kLabelFirst, kThreeBlocks, kGradOffset, kFourChannels, kDRows, kDCols, kPlanes };
static void BuildOperator(Problem<float>& p, Shape shape, size_t& m, size_t& n) {
  const size_t L = shape == kFourChannels ? 4 : 2, g = 2 * L * kPix;
  n = L * kPix;
  switch (shape) {
    case kDiagFirst: p.AddBlock(Sparse(0, 0, kPix, n, Pointwise(kPix, L))); p.AddBlock(Grad(kPix, 0, L)); m = kPix + g; break;
    case kDiagSecond: p.AddBlock(Grad(0, 0, L)); p.AddBlock(Sparse(g, 0, kPix, n, Pointwise(kPix, L))); m = kPix + g; break;
    case kCsrFirst: p.AddBlock(Sparse(0, 0, kPix, n, Warp(kPix, n))); p.AddBlock(Grad(kPix, 0, L)); m = kPix + g; break;
    case kCsrSecond: p.AddBlock(Grad(0, 0, L)); p.AddBlock(Sparse(g, 0, kPix, n, Warp(kPix, n))); m = kPix + g; break;
    case kGradOnly: case kFourChannels: p.AddBlock(Grad(0, 0, L)); m = g; break;
    case kLabelFirst: p.AddBlock(Grad(0, 0, L, true)); m = g; break;
    case kManyBlocks: for (size_t i = 0; i < 5; i++) p.AddBlock(Sparse(i * kPix, 0, kPix, n, Pointwise(kPix, L))); m = 5 * kPix; break;
    case kNoDescribe: p.AddBlock(std::make_shared<BlockDiags<float>>(0, 0, n, n, 1, std::vector<int64_t>{0}, std::vector<float>{1.f})); p.AddBlock(Grad(n, 0, L)); m = n + g; break;
    case kCsrRow: { Triplets t; for (int c = 0; c < 7; c++) t.emplace_back(0, 3 * c, 1.f); p.AddBlock(Sparse(0, 0, 1, n, t)); p.AddBlock(Grad(1, 0, L)); m = 1 + g; break; }
    case kCsrCol: { Triplets t; for (int r = 0; r < 7; r++) t.emplace_back(r, 0, 1.f); p.AddBlock(Sparse(0, 0, 7, 1, t)); p.AddBlock(Grad(7, 0, L)); m = 7 + g; break; }
    case kThreeBlocks: p.AddBlock(Sparse(0, 0, kPix, n, Pointwise(kPix, L))); p.AddBlock(Grad(kPix, 0, L)); p.AddBlock(Sparse(kPix + g, 0, kPix, n, Pointwise(kPix, L))); m = 2 * kPix + g; break;
    case kGradOffset: { Triplets t; for (int i = 0; i < 4; i++) t.emplace_back(i, i, 2.f); p.AddBlock(Sparse(0, 0, 4, 4, t)); p.AddBlock(Grad(4, 4, L)); m = 4 + g; n += 4; break; }
    case kDRows: p.AddBlock(Sparse(0, 0, kPix - 1, n, Warp(kPix - 1, n))); p.AddBlock(Grad(kPix - 1, 0, L)); m = kPix - 1 + g; break;
    case kDCols: p.AddBlock(Sparse(0, 0, kPix, n - 1, Warp(kPix, n - 1))); p.AddBlock(Grad(kPix, 0, L)); m = kPix + g; break;
    case kPlanes: p.AddBlock(Sparse(0, 0, kPix, kPix, Pointwise(kPix, 1))); p.AddBlock(Grad(kPix, 0, L)); m = kPix + g; break;
  }
}

// ---- scenarios -----------------------------------------------------------------------------------------------------------------
enum Variant { kBase, kProxZero, kMoreau, kComm };
struct Scenario {
  std::string name;
  Shape shape = kDiagFirst;
  bool device_cg = true, fused_rounds = true, pixel_rounds = true, cg_graph = false;
  int cg_max_iter = 10, residual_iter = 1, stop_round = -1, sample_every = 0, iterations = 12;
  Variant variant = kBase;
  bool dual = false, custom_sigma = false;
  int fused_op_supported = 1, pixel_op_supported = 1;
};
struct Mode { const char* name; Shape shape; bool device_cg, fused_rounds, pixel_rounds, cg_graph; };
static const Mode kModes[] = {
    {"host", kDiagFirst, false, true, true, false},
    {"staged", kDiagFirst, true, false, true, false},
    {"graph", kDiagFirst, true, true, true, true},
    {"fused4", kDiagFirst, true, true, false, false},
    {"pixdiag1", kDiagFirst, true, true, true, false},
    {"pixdiag2", kDiagSecond, true, true, true, false},
    {"pixcsr1", kCsrFirst, true, true, true, false},
    {"pixcsr2", kCsrSecond, true, true, true, false},
    {"pixgrad", kGradOnly, true, true, true, false},
};
static const char* kVariants[] = {"base", "proxzero", "moreau", "comm"};
static Scenario Make(const Mode& mo, Variant v, int maxit, int stop, int every, int period) {
  Scenario s;
  s.shape = mo.shape; s.device_cg = mo.device_cg; s.fused_rounds = mo.fused_rounds; s.pixel_rounds = mo.pixel_rounds; s.cg_graph = mo.cg_graph;
  s.variant = v; s.cg_max_iter = maxit; s.stop_round = stop; s.sample_every = every; s.residual_iter = period;
  char buf[128];
  snprintf(buf, sizeof(buf), "%s.%s.m%d.s%s.t%d.r%d", mo.name, kVariants[v], maxit, stop < 0 ? "no" : std::to_string(stop).c_str(), every, period);
  s.name = buf;
  return s;
}
static Scenario Reject(const char* name, Shape shape) { Scenario s; s.name = std::string("reject.") + name + ".r1"; s.shape = shape; s.iterations = 1; s.cg_max_iter = 2; return s; }
static std::vector<Scenario> AllScenarios() {
  std::vector<Scenario> all;
  for (const Mode& mo : kModes) {
    const bool device = mo.device_cg, rounds_timed = device && mo.fused_rounds && !mo.cg_graph;
    for (int maxit : {0, 1, 10})
      for (int stop : {-1, 0, 3}) {
        if (stop >= 0 && (!device || stop >= maxit)) continue;               // no stop word without a device solve / beyond the last round
        for (int every : {0, 1, 3}) {
          if (every && !rounds_timed && !(every == 1 && maxit == 10 && stop < 0)) continue;      // (one timed run of the modes that sample nothing)
          for (int period : {1, 3}) all.push_back(Make(mo, kBase, maxit, stop, every, period));
        }
      }
    for (Variant v : {kProxZero, kMoreau, kComm})
      for (int maxit : {1, 10})
        for (int period : {1, 3}) all.push_back(Make(mo, v, maxit, device && maxit > 3 ? 3 : -1, rounds_timed ? 3 : 0, period));
  }
  // every way DescribeOperator turns an operator away: path() and the first outer iteration
  { Scenario s = Reject("dual", kDiagFirst); s.dual = true; all.push_back(s); }
  all.push_back(Reject("manyblocks", kManyBlocks));
  all.push_back(Reject("nodescribe", kNoDescribe));
  all.push_back(Reject("csrrow", kCsrRow));
  all.push_back(Reject("csrcol", kCsrCol));
  all.push_back(Reject("labelfirst", kLabelFirst));
  { Scenario s = Reject("fusedunsupported", kDiagFirst); s.fused_op_supported = 0; all.push_back(s); }
  { Scenario s = Reject("pixeloff", kDiagFirst); s.pixel_rounds = false; all.push_back(s); }
  all.push_back(Reject("threeblocks", kThreeBlocks));
  all.push_back(Reject("gradoffset", kGradOffset));
  all.push_back(Reject("fourchannels", kFourChannels));
  all.push_back(Reject("drows", kDRows));
  all.push_back(Reject("dcols", kDCols));
  all.push_back(Reject("planes", kPlanes));
  { Scenario s = Reject("sigma", kGradOnly); s.custom_sigma = true; all.push_back(s); }
  { Scenario s = Reject("pixelunsupported", kDiagFirst); s.pixel_op_supported = 0; all.push_back(s); }
  return all;
}

static void Run(const Scenario& sc) {
  g_log.clear(); g_allocs.clear(); g_events.clear(); g_next_ordinal = g_next_event = 0;
  g_solves = g_staged_round = g_host_iteration = g_nrm2_calls = g_residual_evals = 0; g_nrm2_residuals = false;
  g_cfg = MockConfig();
  g_cfg.fused_op_supported = sc.fused_op_supported; g_cfg.pixel_op_supported = sc.pixel_op_supported; g_cfg.stop_round = sc.stop_round;
  auto problem = std::make_shared<Problem<float>>();
  size_t m = 0, n = 0;
  BuildOperator(*problem, sc.shape, m, n);
  problem->SetDimensions(m, n);
  if (sc.custom_sigma) {
    std::vector<float> left(m, 1.f), right(n, 1.f);
    left[m / 2] = 2.f;
    problem->SetScalingCustom(left, right);
  } else problem->SetScalingAlpha(1);
  const std::array<std::vector<float>, 7> cg = {{{1.f}, std::vector<float>(n, 0.5f), {10.f}, {0.f}, {0.f}, {0.f}, {0.f}}};
  const std::array<std::vector<float>, 7> cf = {{{1.f}, {1.f}, {1.f}, {0.f}, {0.f}, {0.f}, {0.f}}};
  auto g = std::make_shared<ProxElemDispatch<float>>(PROST_OP_1D, PROST_FN_SQUARE, 0, n, 1, false, true, cg);
  auto f = std::make_shared<ProxElemDispatch<float>>(PROST_OP_1D, PROST_FN_IND_LEQ0, 0, m, 1, false, true, cf);
  if (sc.variant == kMoreau) { problem->AddProx_gstar(g); problem->AddProx_fstar(f); }
  else {
    if (sc.variant == kProxZero) problem->AddProx_g(std::make_shared<ProxZero<float>>(0, n)); else problem->AddProx_g(g);
    problem->AddProx_f(f);
  }
  ADMM::Options bo;
  bo.device_cg = sc.device_cg; bo.fused_rounds = sc.fused_rounds; bo.pixel_rounds = sc.pixel_rounds; bo.cg_graph = sc.cg_graph;
  bo.cg_max_iter = sc.cg_max_iter; bo.residual_iter = sc.residual_iter;
  auto backend = std::make_shared<ADMM>(bo);
  if (sc.variant == kComm) backend->SetCommunicator((void*)0x1, 2 * m, 2 * n);
  if (sc.sample_every) backend->EnableKernelTiming(true, sc.sample_every);
  Solver<float> solver(problem, backend);
  Solver<float>::Options so;
  so.tol_rel_primal = so.tol_rel_dual = 0; so.tol_abs_primal = so.tol_abs_dual = 1;      // eps = sqrt(rows), sqrt(cols): between the mock's residual norms 1 and 1000
  so.max_iters = sc.iterations; so.num_cback_calls = 0; so.solve_dual_problem = sc.dual;
  try {
    solver.SetOptions(so);
    solver.Initialize();
    logf("-- initialized: path %s gpu_mem %zu", backend->path().c_str(), backend->gpu_mem_amount());
    for (int i = 0; i < sc.iterations; i++) {
      solver.Iterate(1);
      const int cg_iterations = backend->last_cg_iterations();
      logf("-- iteration %zu done: cg_iterations %d rho %a residuals %a %a %a %a", backend->iteration(), cg_iterations, (double)backend->rho(), (double)backend->primal_residual(),
           (double)backend->dual_residual(), (double)backend->primal_var_norm(), (double)backend->dual_var_norm());
    }
    std::vector<Backend<float>::KernelTime> times;
    backend->KernelTimes(times);
    for (const auto& t : times) logf("-- kernel %s avg %a sampled %zu launches %zu", t.name.c_str(), t.avg_ms, t.sampled, t.launches);
    std::vector<float> a, b, c, d;
    logf("-- current_solution(primal, dual)");
    backend->current_solution(a, b);
    logf("-- sizes %zu %zu; current_solution(x, z, y, w)", a.size(), b.size());
    backend->current_solution(a, b, c, d);
    logf("-- sizes %zu %zu %zu %zu; path %s gpu_mem %zu", a.size(), b.size(), c.size(), d.size(), backend->path().c_str(), backend->gpu_mem_amount());
  } catch (const std::exception& e) {
    logf("-- EXCEPTION %s", e.what());
  }
  solver.Release();
  std::printf("@ %s\n", sc.name.c_str());
  for (const std::string& l : g_log) std::printf("%s\n", l.c_str());
}

int main(int argc, char** argv) {
  signal(SIGSEGV, on_segv);
  const std::vector<Scenario> all = AllScenarios();
  if (argc < 2 || !strcmp(argv[1], "--list")) { for (const Scenario& s : all) std::printf("%s\n", s.name.c_str()); return 0; }
  for (int a = 1; a < argc; a++) {
    bool found = false;
    for (const Scenario& s : all) if (!strcmp(argv[a], "all") || s.name == argv[a]) { Run(s); found = true; }
    if (!found) { std::fprintf(stderr, "no scenario %s\n", argv[a]); return 2; }
  }
  return 0;
}
