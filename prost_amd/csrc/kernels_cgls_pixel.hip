// kernels_cgls_pixel.hip -- the CG rounds of TWO launches for operators [D ; gradient2d] (prost_hip_cgls_pixel_round_*); records,
// workspace regions and arithmetic as in kernels_cgls.hip, whose cgls_init_fused writes record 0.
#include <limits>

#include "elementwise.hpp"
#include "fused_op.hpp"
#include "cgls_common.hpp"

namespace prost_hip {

// ---- pixel-ordered CG rounds: TWO launches per round (round 5) ------------------------------------------------------------
// For operators K = [D ; grad2d(nx, ny, L)] -- D couples the L channels of ONE pixel (row i of D has its L entries at columns
// i + c nx ny: the warp matrix [diag(Ix) diag(Iy)] of the TV-L1 flow shape, BASELINE config 4), D optional -- a thread that owns
// 4 consecutive pixels of an image column (2 in fp64) owns every row and every column of K that belongs to them: the D row, the
// 2 L gradient rows, the L primal entries.  What a stage needs from NEIGHBOURING pixels (the forward differences of the updated
// p at the right / lower neighbour, the backward differences of the updated r at the left / upper neighbour) it recomputes
// from the neighbour's operands instead of waiting for another thread to publish it -- the loads are cache hits -- so the
// vector updates of a round fold into the operator stages:
//   launch A (PQ):   beta, stopping test from the partials of the previous round ; p = beta p + s ; q = sqrt(Sigma) K sqrt(Tau) p ;
//                    |p|^2, |q|^2                                   [STEP_P2 + OP_FWD<FwdQ>;  t = sqrt(Tau) p is never stored]
//   launch B (XRS):  alpha ; x += alpha p ; r -= alpha q ; s = sqrt(Tau) (-shift x / sqrt(Tau) + K^T sqrt(Sigma) r) ;
//                    |x|^2, |s|^2                                   [STEP_XR2 + OP_ADJ<AdjS>; t = sqrt(Sigma) r is never stored]
// p and r are written to a second buffer each (a neighbour may still read the old values): round j reads p from P[(j-1) % 2]
// and leaves it in P[j % 2], reads r from R[j % 2] and leaves it in R[(j+1) % 2].  Per element every value is formed by the
// expressions of the four-launch round above in the same order (csr_rows / op_fwd_rows / op_adj_cols / the epilogues / StepXR /
// StepP), the sums are order-independent (reduce.hpp): x, p, q, r, s and every CG scalar are bit-identical to the four-launch
// round and to the staged round.  Per pixel and round (L = 2): A reads p, s, tau (6), D's values (2), sigma (5), writes p, q (7);
// B reads r, q (10), D's sigma (1), x, p, tau (6), D's values (2), writes r, x, s (9); A: sigma on D's rows only (1 instead of 5):
// 44 values instead of ~80.  (Sigma on the gradient rows is ONE number: the caller checks it.)
// D_CSR (round 6, prost_hip_pixel_op.d_csr): D is ANY sparse block with one row per pixel (a warp matrix: row i gathers the channels at
// pixels displaced from i).  The owner of pixel i still owns D's row i (launch A) and the L columns of D^T at i (launch B); the operand
// of an entry belongs to ANOTHER pixel and is recomputed from that pixel's stored operands like the stencil neighbours are -- three
// gathered values per entry instead of one, t never stored (csr_rows_formed below).
template <class T> struct PixArgs {
  unsigned nx, ny;                     // image; ny % VEC == 0
  size_t npx;                          // nx ny
  size_t d_row, g_row;                 // first row of the D block / of the gradient block
  const T* w;                          // D's values, row-major: w[i L + c] (the CSR value array of the block); nullptr-free when HAS_D
  // D_CSR (round 6): D is ANY CSR block of nx ny rows over the L nx ny primal entries (a warp matrix that gathers at displaced pixels):
  // its CSR arrays for the rows, those of D^T for the columns
  const T* d_val; const int32_t* d_ptr; const int32_t* d_ind;
  const T* dt_val; const int32_t* dt_ptr; const int32_t* dt_ind;
  const T* sigma; const T* tau;          // sigma: read on D's rows only
  T sig_g;                               // Sigma on the gradient rows: ONE value (a gradient block's row sums are constant, block_gradient2d.cu:154-158)
  T* x; const T* p_in; T* p_out; T* s; T* q; const T* r_in; T* r_out;
  T negshift;
  unsigned tiles;                      // workgroups
};
struct PixGeom { size_t px0; unsigned x, y0; bool active; };
template <int VEC>
__device__ __forceinline__ PixGeom pix_geom(unsigned tiles, unsigned ny, size_t npx) {
  // XCD-aware tile order: workgroup b runs on XCD b % 8 (round-robin dispatch); each XCD takes a contiguous range of tiles, so
  // the neighbouring image columns a tile re-reads were fetched by the same XCD's L2 a moment ago
  unsigned t = blockIdx.x;
  if ((tiles & 7u) == 0) t = (blockIdx.x & 7u) * (tiles >> 3) + (blockIdx.x >> 3);
  PixGeom g;
  g.px0 = ((size_t)t * kBlock + threadIdx.x) * VEC;
  g.active = g.px0 < npx;
  const size_t c = g.active ? g.px0 : 0;
  g.x = (unsigned)(c / ny); g.y0 = (unsigned)(c - (size_t)g.x * ny);
  return g;
}

// sum[j] = sum_k val[k] f(ind[k]) over the CSR rows row0 .. row0 + V - 1 of this lane, entries in order (csr_rows of fused_op.hpp with the
// operand FORMED per entry: the vector the four-launch round would have stored is recomputed from its operands at the gathered position).
// `whole` (wave-uniform: the wavefront's 64 V rows from wave0 on all exist): the lanes take the rows TRANSPOSED -- lane, lane + 64, ... --
// so that neighbouring lanes read neighbouring row starts, entries and (for a warp) neighbouring gathered operands, and the sums are
// shuffled back to the lanes that own the rows (csr_contrib's scheme).  Taking a lane's own V rows instead costs 4-8 cache lines per
// lane and load: the first version of these instances ran launch A in 107 us at 1024^2 against 48 us for the two launches it replaces.
template <class T, int V, class F>
__device__ __forceinline__ void csr_rows_formed(const T* __restrict__ val, const int32_t* __restrict__ ptr, const int32_t* __restrict__ ind, size_t row0, size_t wave0,
                                                bool whole, F f, T (&sum)[V]) {
  const unsigned lane = threadIdx.x & (kWave - 1);
  size_t r[V];
#pragma unroll
  for (int j = 0; j < V; j++) r[j] = whole ? wave0 + (size_t)j * kWave + lane : row0 + j;
  int32_t b[V], e[V], len = 0;
#pragma unroll
  for (int j = 0; j < V; j++) { b[j] = ptr[r[j]]; e[j] = ptr[r[j] + 1]; }
  T acc[V];
#pragma unroll
  for (int j = 0; j < V; j++) { acc[j] = 0; len = e[j] - b[j] > len ? e[j] - b[j] : len; }
  for (int32_t st = 0; st < len; st++) {
#pragma unroll
    for (int j = 0; j < V; j++) {
      const int32_t k = b[j] + st;
      if (k < e[j]) acc[j] += val[k] * f((size_t)ind[k]);
    }
  }
  if (V > 1 && whole) wave_untranspose<T, V>(acc, sum, lane);
  else {
#pragma unroll
    for (int j = 0; j < V; j++) sum[j] = acc[j];
  }
}

template <class T, int L, bool HAS_D, bool D_FIRST, bool FIRST, bool D_CSR = false>
__global__ void __launch_bounds__(kBlock, (L <= 2 ? 4 : 2)) cg_pixel_pq_kernel(PixArgs<T> a, const CgState* prev, CgState* cur, double* ws, RoundScalars sc) {
  constexpr int V = VecOf<T>::N;
  if (FIRST ? cur->done != 0 : prev->done != 0) {
    if (!FIRST && blockIdx.x == 0 && threadIdx.x == 0) *cur = *prev;
    return;
  }
  const PixGeom g = pix_geom<V>(a.tiles, a.ny, a.npx);
  const unsigned nx = a.nx, ny = a.ny;
  const bool right = g.active && g.x + 1 < nx, below = g.active && g.y0 + V < ny;
  // operands requested before the fold: none of them depends on beta
  T pc[L][V], sv[L][V], tc[L][V], pr[L][V], sr[L][V], tr[L][V], pb[L], sb_[L], tb[L];
#pragma unroll
  for (int c = 0; c < L; c++) {
#pragma unroll
    for (int j = 0; j < V; j++) { pc[c][j] = 0; sv[c][j] = 0; tc[c][j] = 1; pr[c][j] = 0; sr[c][j] = 0; tr[c][j] = 1; }
    pb[c] = 0; sb_[c] = 0; tb[c] = 1;
    const size_t e = (size_t)c * a.npx + g.px0;
    if (g.active) { ldv<T, V>(a.p_in + e, pc[c]); ldv<T, V>(a.tau + e, tc[c]); if (!FIRST) ldv<T, V>(a.s + e, sv[c]); }
    if (right) { ldv<T, V>(a.p_in + e + ny, pr[c]); ldv<T, V>(a.tau + e + ny, tr[c]); if (!FIRST) ldv<T, V>(a.s + e + ny, sr[c]); }
    if (below) { pb[c] = a.p_in[e + V]; tb[c] = a.tau[e + V]; if (!FIRST) sb_[c] = a.s[e + V]; }
  }
  T wv[HAS_D && !D_CSR ? V * L : 1], sgd[V];
  if (g.active && HAS_D) {
    if constexpr (!D_CSR) {
#pragma unroll
      for (int k = 0; k < L; k++) ldv<T, V>(a.w + g.px0 * L + (size_t)k * V, *reinterpret_cast<T(*)[V]>(&wv[k * V]));
    }
    ldv<T, V>(a.sigma + a.d_row + g.px0, sgd);
  }
  const T sqg = t_sqrt(a.sig_g);                       // sqrt(Sigma) of every gradient row
  T beta = 0;
  if (!FIRST) {
    // STEP_P2's head: beta and the stopping test from |s|^2, |x|^2 of the previous round (cgls.hpp:326-360); workgroup 0 records
    double s0, s1;
    fold_dd2(region(ws, kRegionS), sc.g_a, 2, region(ws, kRegionX), sc.g_b, 2, s0, s1);
    const double norms = sqrt(s0), gamma = norms * norms, normx = sqrt(s1);
    beta = (T)(gamma / prev->gamma);
    const bool done = (norms <= prev->norms0 * prev->tol) || (normx * prev->tol >= 1.);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      const int indefinite = cur->indefinite;          // written by the previous round's launch B
      CgState r = *prev;
      r.indefinite = indefinite;
      r.norms = norms; r.gamma = gamma; r.beta = (double)beta; r.normx = normx;
      r.xmax = prev->xmax > normx ? prev->xmax : normx;
      if (done) {
        r.done = 1;
        if (sc.host_done) __hip_atomic_store(sc.host_done, prev->epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
      } else {
        r.k = prev->k + 1;
      }
      *cur = r;
    }
    if (done) return;                                  // (the four-launch round still updates p here; nobody reads it afterwards)
  }
  dd_t sq{0.0, 0.0}, sp{0.0, 0.0};
  if (g.active) {
    // STEP_P: p = beta p + s ; t = sqrt(Tau) p -- own pixels (stored), right and lower neighbours (recomputed, not stored)
    T t0[L][V], t_r[L][V], t_b[L];
#pragma unroll
    for (int c = 0; c < L; c++) {
#pragma unroll
      for (int j = 0; j < V; j++) {
        if (!FIRST) { pc[c][j] = beta * pc[c][j] + sv[c][j]; pr[c][j] = beta * pr[c][j] + sr[c][j]; }
        t0[c][j] = t_sqrt(tc[c][j]) * pc[c][j];
        t_r[c][j] = t_sqrt(tr[c][j]) * pr[c][j];
        dd_acc(sp, (double)pc[c][j] * (double)pc[c][j]);
      }
      if (!FIRST) pb[c] = beta * pb[c] + sb_[c];
      t_b[c] = t_sqrt(tb[c]) * pb[c];
      if (!FIRST) stv<T, V>(a.p_out + (size_t)c * a.npx + g.px0, pc[c]);
    }
    // OP_FWD<FwdQ>: the D row (csr_rows: entries in order), then the gradient rows (op_fwd_rows), each scaled by EpiFwdQ
    if (HAS_D) {
      T qd[V], dsum[V];
      if constexpr (D_CSR) {
        // t = sqrt(Tau) p at the gathered primal entry, p updated as above (STEP_P's expressions; the stored p of that entry is written by its owner)
        const size_t wave0 = ((size_t)(g.px0 / V) - (threadIdx.x & (kWave - 1))) * V;          // first pixel of the wavefront
        csr_rows_formed<T, V>(a.d_val, a.d_ptr, a.d_ind, g.px0, wave0, wave0 + (size_t)kWave * V <= a.npx, [&](size_t col) {
          T pv = a.p_in[col];
          if (!FIRST) pv = beta * pv + a.s[col];
          return t_sqrt(a.tau[col]) * pv;
        }, dsum);
      }
#pragma unroll
      for (int j = 0; j < V; j++) {
        T sum = 0;
        if constexpr (D_CSR) sum = dsum[j];
        else {
#pragma unroll
          for (int c = 0; c < L; c++) sum += wv[j * L + c] * t0[c][j];
        }
        T kv = 0;
        kv = kv + sum;
        qd[j] = (T)1 * t_sqrt(sgd[j]) * kv;
        dd_acc(sq, (double)qd[j] * (double)qd[j]);
      }
      stv<T, V>(a.q + a.d_row + g.px0, qd);
    }
#pragma unroll
    for (int c = 0; c < L; c++) {
      T qx[V], qy[V];
#pragma unroll
      for (int j = 0; j < V; j++) {
        const T gx = g.x < nx - 1 ? t_r[c][j] - t0[c][j] : (T)0;
        const T dn = j + 1 < V ? t0[c][(j + 1) % V] : t_b[c];
        const T gy = g.y0 + j < ny - 1 ? dn - t0[c][j] : (T)0;
        T kx = 0, ky = 0;
        kx = kx + gx; ky = ky + gy;
        qx[j] = (T)1 * sqg * kx;
        qy[j] = (T)1 * sqg * ky;
        dd_acc(sq, (double)qx[j] * (double)qx[j]);
        dd_acc(sq, (double)qy[j] * (double)qy[j]);
      }
      stv<T, V>(a.q + a.g_row + (size_t)c * a.npx + g.px0, qx);
      stv<T, V>(a.q + a.g_row + (size_t)(L + c) * a.npx + g.px0, qy);
    }
  }
  block_dd_store1(sq, region(ws, kRegionQ), blockIdx.x);
  block_dd_store1(sp, region(ws, kRegionP), blockIdx.x);
}

template <class T, int L, bool HAS_D, bool D_FIRST, bool D_CSR = false>
__global__ void __launch_bounds__(kBlock, (L <= 2 ? 4 : 2)) cg_pixel_xrs_kernel(PixArgs<T> a, const CgState* cur, CgState* nxt, double* ws, RoundScalars sc) {
  constexpr int V = VecOf<T>::N;
  if (cur->done) return;
  const PixGeom g = pix_geom<V>(a.tiles, a.ny, a.npx);
  const unsigned nx = a.nx, ny = a.ny;
  const bool left = g.active && g.x > 0, above = g.active && g.y0 > 0;
  // operands requested before the fold (none depends on alpha): own rows of r, q, sigma; the d/dx rows of the left neighbour
  // column; the d/dy row of the pixel above; x, p, tau, D's values
  T rd[V], qd[V], gd[V];
  T rx[L][V], qx[L][V], ry[L][V], qy[L][V], rl[L][V], ql[L][V], ra[L], qa[L];
  T xv[L][V], pv[L][V], tv[L][V];
  T wv[HAS_D && !D_CSR ? V * L : 1];
#pragma unroll
  for (int j = 0; j < V; j++) { rd[j] = 0; qd[j] = 0; gd[j] = 1; }
#pragma unroll
  for (int c = 0; c < L; c++) {
#pragma unroll
    for (int j = 0; j < V; j++) { rl[c][j] = 0; ql[c][j] = 0; }
    ra[c] = 0; qa[c] = 0;
  }
  if (g.active) {
    if (HAS_D) {
      const size_t e = a.d_row + g.px0;
      ldv<T, V>(a.r_in + e, rd); ldv<T, V>(a.q + e, qd); ldv<T, V>(a.sigma + e, gd);
      if constexpr (!D_CSR) {
#pragma unroll
        for (int k = 0; k < L; k++) ldv<T, V>(a.w + g.px0 * L + (size_t)k * V, *reinterpret_cast<T(*)[V]>(&wv[k * V]));
      }
    }
#pragma unroll
    for (int c = 0; c < L; c++) {
      const size_t ex = a.g_row + (size_t)c * a.npx + g.px0, ey = a.g_row + (size_t)(L + c) * a.npx + g.px0;
      ldv<T, V>(a.r_in + ex, rx[c]); ldv<T, V>(a.q + ex, qx[c]);
      ldv<T, V>(a.r_in + ey, ry[c]); ldv<T, V>(a.q + ey, qy[c]);
      if (left) { ldv<T, V>(a.r_in + ex - ny, rl[c]); ldv<T, V>(a.q + ex - ny, ql[c]); }
      if (above) { ra[c] = a.r_in[ey - 1]; qa[c] = a.q[ey - 1]; }
    }
  }
  // STEP_XR2's head: alpha from |q|^2, |p|^2 (cgls.hpp:297-310)
  double s0, s1;
  fold_dd2(region(ws, kRegionQ), sc.g_a, 2, region(ws, kRegionP), sc.g_b, 2, s0, s1);
  const double normq = sqrt(s0), normp = sqrt(s1);
  double dlt = normq * normq + sc.shift * normp * normp;
  const int indefinite = dlt <= 0. ? 1 : 0;
  if (dlt == 0.) dlt = sc.eps;
  const T alpha = (T)(cur->gamma / dlt), neg_alpha = (T)(-cur->gamma / dlt);
  if (blockIdx.x == 0 && threadIdx.x == 0) nxt->indefinite = cur->indefinite | indefinite;
  dd_t sx{0.0, 0.0}, ss{0.0, 0.0};
  const T sqg = t_sqrt(a.sig_g);                       // sqrt(Sigma) of every gradient row
  if (g.active) {
    // second batch of operands (behind the fold's barriers: they arrive while r and t are formed; all at once would not fit 128 registers)
#pragma unroll
    for (int c = 0; c < L; c++) {
      const size_t en = (size_t)c * a.npx + g.px0;
      ldv<T, V>(a.x + en, xv[c]); ldv<T, V>(a.p_in + en, pv[c]); ldv<T, V>(a.tau + en, tv[c]);
    }
    // STEP_XR (m): r = -alpha q + r ; t = sqrt(Sigma) r -- own rows (stored), neighbour rows (recomputed, not stored)
    T td[V];
    if (HAS_D) {
#pragma unroll
      for (int j = 0; j < V; j++) { rd[j] = neg_alpha * qd[j] + rd[j]; td[j] = t_sqrt(gd[j]) * rd[j]; }
      stv<T, V>(a.r_out + a.d_row + g.px0, rd);
    }
#pragma unroll
    for (int c = 0; c < L; c++) {
      T tx[V], ty[V], tl[V];
#pragma unroll
      for (int j = 0; j < V; j++) {
        rx[c][j] = neg_alpha * qx[c][j] + rx[c][j]; tx[j] = sqg * rx[c][j];
        ry[c][j] = neg_alpha * qy[c][j] + ry[c][j]; ty[j] = sqg * ry[c][j];
        rl[c][j] = neg_alpha * ql[c][j] + rl[c][j]; tl[j] = sqg * rl[c][j];
      }
      ra[c] = neg_alpha * qa[c] + ra[c];
      const T t_above = sqg * ra[c];
      stv<T, V>(a.r_out + a.g_row + (size_t)c * a.npx + g.px0, rx[c]);
      stv<T, V>(a.r_out + a.g_row + (size_t)(L + c) * a.npx + g.px0, ry[c]);
      // STEP_XR (n): x = alpha p + x ; OP_ADJ<AdjS>: v = s0 ; + D^T t ; - div t (blocks in operator order) ; s = 1 sqrt(Tau) v
      T so[V], dcol[V];
      if constexpr (HAS_D && D_CSR) {
        // t = sqrt(Sigma) r at the gathered D row, r updated as above (STEP_XR's expressions; the stored r of that row is written by its owner)
        const size_t wave0 = ((size_t)(g.px0 / V) - (threadIdx.x & (kWave - 1))) * V;          // first pixel of the wavefront
        csr_rows_formed<T, V>(a.dt_val, a.dt_ptr, a.dt_ind, (size_t)c * a.npx + g.px0, (size_t)c * a.npx + wave0, wave0 + (size_t)kWave * V <= a.npx, [&](size_t row) {
          const size_t e = a.d_row + row;
          return t_sqrt(a.sigma[e]) * (neg_alpha * a.q[e] + a.r_in[e]);
        }, dcol);
      }
#pragma unroll
      for (int j = 0; j < V; j++) {
        xv[c][j] = alpha * pv[c][j] + xv[c][j];
        dd_acc(sx, (double)xv[c][j] * (double)xv[c][j]);
        const T sq = t_sqrt(tv[c][j]);
        T v = (a.negshift / ((T)1 * sq)) * xv[c][j];
        T dsum = 0;
        if constexpr (HAS_D && D_CSR) dsum = dcol[j];
        else if (HAS_D) dsum += wv[j * L + c] * td[j];
        T divy = g.y0 + j < ny - 1 ? ty[j] : (T)0;
        if (g.y0 + j > 0) divy -= j > 0 ? ty[(j + V - 1) % V] : t_above;
        T divx = g.x < nx - 1 ? tx[j] : (T)0;
        if (g.x > 0) divx -= tl[j];
        const T sdiv = divx + divy;
        if (HAS_D && D_FIRST) { v = v + dsum; v = v - sdiv; }
        else if (HAS_D) { v = v - sdiv; v = v + dsum; }
        else v = v - sdiv;
        so[j] = (T)1 * sq * v;
        dd_acc(ss, (double)so[j] * (double)so[j]);
      }
      stv<T, V>(a.x + (size_t)c * a.npx + g.px0, xv[c]);
      stv<T, V>(a.s + (size_t)c * a.npx + g.px0, so);
    }
  }
  block_dd_store1(sx, region(ws, kRegionX), blockIdx.x);
  block_dd_store1(ss, region(ws, kRegionS), blockIdx.x);
}

// the closing evaluation of a solve whose last queued round was round `last`: beta / stopping test of that round -> record last + 1
// (what launch A of round last + 1 would record), so that the result record (iterations, flags, norms) is that of the other paths
template <class T>
__global__ void __launch_bounds__(kBlock) cg_pixel_close_kernel(const CgState* prev, CgState* cur, double* ws, RoundScalars sc) {
  if (prev->done) { if (threadIdx.x == 0) *cur = *prev; return; }
  double s0, s1;
  fold_dd2(region(ws, kRegionS), sc.g_a, 2, region(ws, kRegionX), sc.g_b, 2, s0, s1);
  if (threadIdx.x != 0) return;
  const double norms = sqrt(s0), gamma = norms * norms, normx = sqrt(s1);
  CgState r = *prev;
  r.indefinite = cur->indefinite;
  r.norms = norms; r.gamma = gamma; r.beta = (double)(T)(gamma / prev->gamma); r.normx = normx;
  r.xmax = prev->xmax > normx ? prev->xmax : normx;
  if ((norms <= prev->norms0 * prev->tol) || (normx * prev->tol >= 1.)) {
    r.done = 1;
    if (sc.host_done) __hip_atomic_store(sc.host_done, prev->epoch, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  } else {
    r.k = prev->k + 1;
  }
  *cur = r;
}

static bool pixel_op_ok(const prost_hip_pixel_op* op, uint64_t m, uint64_t n, unsigned V) {
  if (!op || op->nx == 0 || op->ny == 0 || op->L < 1 || op->L > 3) return false;
  const uint64_t npx = op->nx * op->ny;
  if (op->ny % V || npx >= ((uint64_t)1 << 31)) return false;
  // one workgroup per tile of kBlock x V pixels writes a partial into the reduction workspace (cgls_pixel_round): images beyond
  // kReduceBlocks tiles (8.4 M pixels in fp32, 4.2 M in fp64 -- 4096^2) are refused HERE, so that BackendADMM::DescribeOperator falls
  // back to the four-launch rounds (whose fold grids are capped) instead of picking a path whose every solve then fails
  if ((npx / V + kBlock - 1) / kBlock > (uint64_t)kReduceBlocks) return false;
  if (n != (uint64_t)op->L * npx) return false;
  if (op->d_csr && (!op->has_d || !op->d_val || !op->d_ptr || !op->d_ind || !op->dt_val || !op->dt_ptr || !op->dt_ind)) return false;
  if (op->has_d) {
    if ((!op->d_csr && !op->w) || m != npx + 2 * (uint64_t)op->L * npx) return false;
    const bool d_first = op->d_row == 0 && op->g_row == npx, g_first = op->g_row == 0 && op->d_row == 2 * (uint64_t)op->L * npx;
    if (!d_first && !g_first) return false;
  } else if (m != 2 * (uint64_t)op->L * npx || op->g_row != 0) {
    return false;
  }
  return true;
}

template <class T>
static int cgls_pixel_round(const prost_hip_cgls_desc* d, const prost_hip_pixel_op* op, int round, int close, void* stream, void* const* ev4) {
  constexpr int V = VecOf<T>::N;
  if (!d || !d->state || !d->workspace) { set_error("cgls_pixel_round: state and workspace are required"); return 1; }
  if (round < 0) { set_error("cgls_pixel_round: negative round"); return 1; }
  if (!pixel_op_ok(op, d->m, d->n, V) || !op->p_alt || !op->r_alt) { set_error("cgls_pixel_round: unsupported operator description (prost_hip_pixel_op_supported)"); return 1; }
  T* P[2] = {static_cast<T*>(d->p), static_cast<T*>(op->p_alt)};
  T* R[2] = {static_cast<T*>(d->r), static_cast<T*>(op->r_alt)};
  for (const void* ptr : {(const void*)d->x, (const void*)d->q, (const void*)d->s, (const void*)d->sigma, (const void*)d->tau, op->d_csr ? (const void*)d->x : (const void*)op->w,
      (const void*)P[0], (const void*)P[1], (const void*)R[0], (const void*)R[1]})
    if (!aligned16(ptr)) { set_error("cgls_pixel_round: operands must be 16-byte aligned"); return 1; }
  hipStream_t st = as_stream(stream);
  const size_t npx = (size_t)(op->nx * op->ny);
  const unsigned tiles = (unsigned)((npx / V + kBlock - 1) / kBlock);
  if (tiles > (unsigned)kReduceBlocks) { set_error("cgls_pixel_round: image too large for the reduction workspace"); return 1; }
  // the partial sums of round 0's |p|^2 and of the solve's first |s|^2 come from the kernels of prost_hip_cgls_init_fused, whose grids
  // are what cgls_round computes for them; afterwards every region is written by `tiles` workgroups
  CgState* rec = static_cast<CgState*>(d->state);
  double* ws = static_cast<double*>(d->workspace);
  const double eps = (double)std::numeric_limits<T>::epsilon();
  PixArgs<T> a;
  a.nx = (unsigned)op->nx; a.ny = (unsigned)op->ny; a.npx = npx; a.d_row = (size_t)op->d_row; a.g_row = (size_t)op->g_row;
  a.w = static_cast<const T*>(op->w); a.sigma = static_cast<const T*>(d->sigma); a.tau = static_cast<const T*>(d->tau);
  a.d_val = static_cast<const T*>(op->d_val); a.d_ptr = op->d_ptr; a.d_ind = op->d_ind;
  a.dt_val = static_cast<const T*>(op->dt_val); a.dt_ptr = op->dt_ptr; a.dt_ind = op->dt_ind;
  const bool d_csr = op->has_d != 0 && op->d_csr != 0;
  a.x = static_cast<T*>(d->x); a.s = static_cast<T*>(d->s); a.q = static_cast<T*>(d->q);
  a.negshift = (T)(-d->shift); a.tiles = tiles; a.sig_g = (T)op->sigma_grad;
  const bool has_d = op->has_d != 0, d_first = has_d && op->d_first != 0;
  const int L = op->L;
  auto mark = [&](int k) { if (ev4 && ev4[2 * k] && ev4[2 * k + 1]) { g_launch_ev_start = (hipEvent_t)ev4[2 * k]; g_launch_ev_stop = (hipEvent_t)ev4[2 * k + 1]; } };
  if (close) {
    const RoundScalars sc{d->shift, eps, tiles, tiles, d->host_done};
    if (round < 1) { set_error("cgls_pixel_close: no round to close"); return 1; }
    PH_LAUNCH((cg_pixel_close_kernel<T>), dim3(1), dim3(kBlock), 0, st, rec + round - 1, rec + round, ws, sc);
    PH_LAUNCH_END("cgls pixel close");
  }
  // launch A of round j: beta / stopping test of round j - 1 -> record j ; p ; q
  a.p_in = round == 0 ? P[0] : P[(round - 1) & 1]; a.p_out = P[round & 1];
  a.r_in = R[round & 1]; a.r_out = R[(round + 1) & 1];
  const RoundScalars sa{d->shift, eps, tiles, tiles, d->host_done};
  mark(0);
#define PIX_A(LL, HD, DF, FI, DC) PH_LAUNCH((cg_pixel_pq_kernel<T, LL, HD, DF, FI, DC>), dim3(tiles), dim3(kBlock), 0, st, a, round == 0 ? rec : rec + round - 1, rec + round, ws, sa)
#define PIX_A_D(LL, FI) do { if (!has_d) PIX_A(LL, false, false, FI, false); else if (d_csr) { if (d_first) PIX_A(LL, true, true, FI, true); else PIX_A(LL, true, false, FI, true); } \
                             else if (d_first) PIX_A(LL, true, true, FI, false); else PIX_A(LL, true, false, FI, false); } while (0)
#define PIX_A_L(LL) do { if (round == 0) PIX_A_D(LL, true); else PIX_A_D(LL, false); } while (0)
  if (L == 1) PIX_A_L(1); else if (L == 2) PIX_A_L(2); else PIX_A_L(3);
#undef PIX_A_L
#undef PIX_A_D
#undef PIX_A
  // launch B of round j: alpha ; x, r ; s
  a.p_in = P[round & 1];
  const RoundScalars sb{d->shift, eps, tiles, tiles, nullptr};
  mark(1);
#define PIX_B(LL, HD, DF, DC) PH_LAUNCH((cg_pixel_xrs_kernel<T, LL, HD, DF, DC>), dim3(tiles), dim3(kBlock), 0, st, a, rec + round, rec + round + 1, ws, sb)
#define PIX_B_L(LL) do { if (!has_d) PIX_B(LL, false, false, false); else if (d_csr) { if (d_first) PIX_B(LL, true, true, true); else PIX_B(LL, true, false, true); } \
                         else if (d_first) PIX_B(LL, true, true, false); else PIX_B(LL, true, false, false); } while (0)
  if (L == 1) PIX_B_L(1); else if (L == 2) PIX_B_L(2); else PIX_B_L(3);
#undef PIX_B_L
#undef PIX_B
  PH_LAUNCH_END("cgls pixel round");
}

}  // namespace prost_hip

using namespace prost_hip;

extern "C" {

int prost_hip_pixel_op_supported(const prost_hip_pixel_op* op, uint64_t m, uint64_t n, int dtype) { return pixel_op_ok(op, m, n, dtype == 0 ? 4u : 2u) ? 1 : 0; }
int prost_hip_cgls_pixel_round_f32(const prost_hip_cgls_desc* d, const prost_hip_pixel_op* op, int round, void* stream) { return cgls_pixel_round<float>(d, op, round, 0, stream, nullptr); }
int prost_hip_cgls_pixel_round_f64(const prost_hip_cgls_desc* d, const prost_hip_pixel_op* op, int round, void* stream) { return cgls_pixel_round<double>(d, op, round, 0, stream, nullptr); }
int prost_hip_cgls_pixel_round_timed_f32(const prost_hip_cgls_desc* d, const prost_hip_pixel_op* op, int round, void* const* ev4,
    void* stream) { return cgls_pixel_round<float>(d, op, round, 0, stream, ev4); }
int prost_hip_cgls_pixel_round_timed_f64(const prost_hip_cgls_desc* d, const prost_hip_pixel_op* op, int round, void* const* ev4,
    void* stream) { return cgls_pixel_round<double>(d, op, round, 0, stream, ev4); }
int prost_hip_cgls_pixel_close_f32(const prost_hip_cgls_desc* d, const prost_hip_pixel_op* op, int last_round,
    void* stream) { return cgls_pixel_round<float>(d, op, last_round + 1, 1, stream, nullptr); }
int prost_hip_cgls_pixel_close_f64(const prost_hip_cgls_desc* d, const prost_hip_pixel_op* op, int last_round,
    void* stream) { return cgls_pixel_round<double>(d, op, last_round + 1, 1, stream, nullptr); }

}  // extern "C"
