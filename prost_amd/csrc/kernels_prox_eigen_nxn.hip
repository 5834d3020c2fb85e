// kernels_prox_eigen_nxn.hip -- elem_operation:eigen_nxn:* for 6 <= n <= 32: several lanes per matrix, A and V^T in LDS.
//
// One matrix per lane (the reference's form, and the functor ElemOperationEigenNxN) needs 2 n^2 doubles of private memory per lane,
// which is scratch memory on gfx950.  Here a group of L lanes (16, 32 or 64: eigen_coop_plan, prox_spectral.hpp) owns one matrix, a
// 256-lane workgroup holds 256 / L of them, and A and V^T sit in LDS as m x m doubles each for both data types, m = n rounded up to
// even (an odd n plays with a bye: row and column n of A stay zero, so that plane's rotation is the identity -- no predicates).
// The arithmetic is the lane-count-agnostic part of spectral_common.hpp: JacobiAngle, RoundRobinPair, JacobiBlock, JacobiConverged,
// SpectralProx1D -- the same rounds EigenNxNApply runs on one lane.
//
// A round of a sweep (m - 1 rounds, m / 2 disjoint pairs each):
//   1. lane k < m / 2 computes the rotation (c, s) of pair k from three entries of A; it stays in that lane's registers;
//   2. work items (k, l): the 2x2 block of A with rows in pair k and columns in pair l becomes J_k^T B J_l (JacobiBlock); the block
//      (k, k) gets exact zeros next to its diagonal.  Work items (k, j): rows p_k, q_k of V^T, element j, are rotated.  Items are
//      strided over the L lanes, every item reads and writes entries no other item touches, and (c, s) of pairs k and l are read
//      across lanes (ds_bpermute), not through LDS: at n = 32 the four matrices fill the 64 KiB.
//   3. one wave-level synchronisation: a matrix belongs to the lanes of ONE wavefront (L <= 64), LDS operations of a wavefront
//      complete in order, so the rounds need no workgroup barrier -- only the compiler has to be kept from moving LDS accesses
//      across the round boundary (wave_lds_sync).
// LDS banks: inside the rounds and in the recomposition, items consecutive in a lane group walk ALONG rows of A and V^T (V is kept
// transposed for that; in item (k, l) the lanes vary l, i.e. the column; the recomposition reads V^T[k][i], one address per i, and
// V^T[k][j], consecutive j), so the rows are not padded -- at n = 32 a padded row would not fit four matrices into 64 KiB anyway.
// Not conflict-free: the one-off symmetrisation reads V^T by columns (32-way at n = 32), block items with equal l and different k
// meet 2-way per 32-lane half at m = 32, and the planar load writes LDS with a stride of one matrix across consecutive lanes
// (16-way at n = 8).  Padding for n < 32 is left for when the kernel is tuned.
//
// Barriers and termination: the stop-word exit is grid-uniform and precedes the first barrier; after it no lane returns early.  A
// matrix index >= count is a zero matrix that takes part in everything and is never stored.  The workgroup barriers stand around
// the load and in front of the store only, outside every loop.  Every loop with a cross-lane read inside has a trip count that
// depends on (n, L) only and is the same in all 256 lanes; lanes without an item are predicated inside.  The sweep loop is a `for`
// up to kJacobiSweepsNxN whose early exit is a wavefront-uniform vote (__all) over the convergence tests of the wavefront's matrices:
// NaN or Inf input runs the capped number of sweeps and ends.  (A workgroup-wide vote -- __syncthreads_and -- brings 256 bytes of
// LDS of its own, which the four 32 x 32 matrices of a workgroup leave no room for, and nothing in a sweep crosses a wavefront.)
//
// Loads and stores: interleaved -- a workgroup's matrices are one contiguous run, moved in 16-byte accesses per lane where the run is
// 16-byte aligned; planar -- consecutive lanes take consecutive groups of the same component.  Only tau_diag[first component] and one
// coefficient set per group are read.
#include "prox_spectral.hpp"
#include "prost/prox/elemop/spectral_common.hpp"

namespace prost_hip {

namespace el = prost::elemop;

/// item index -> (major, minor) = (it / d, it % d) advanced by `step` items without a division
struct ItemWalk {
  int major, minor, dmaj, dmin, d;
  __device__ __forceinline__ ItemWalk(int first, int step, int d_) : major(first / d_), minor(first % d_), dmaj(step / d_), dmin(step % d_), d(d_) {}
  __device__ __forceinline__ void next() {
    major += dmaj; minor += dmin;
    if (minor >= d) { minor -= d; major++; }
  }
};

/// orders the LDS accesses of a wavefront's lanes around it (hardware: in order already; this binds the compiler)
__device__ __forceinline__ void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <class T, bool INTERLEAVED>
__global__ void __launch_bounds__(kBlock) eigen_nxn_coop_kernel(SpectralArgs<T> p, int n, int lanes_log2) {
  extern __shared__ double lds[];              // per matrix: A (m x m), then V^T (m x m)
  T tau_scal;
  if (!spectral_step(p, tau_scal)) return;     // the same in every lane of the grid, before the first barrier
  const int L = 1 << lanes_log2, M = kBlock >> lanes_log2;
  const int tid = (int)threadIdx.x, lane = tid & (L - 1), mat = tid >> lanes_log2;
  const int m = n + (n & 1), mm = m * m, nn = n * n, half = m / 2;
  const size_t g0 = (size_t)blockIdx.x * M, g = g0 + mat;
  const bool live = g < p.count;
  const int valid_mats = p.count - g0 < (size_t)M ? (int)(p.count - g0) : M;
  double* const A = lds + (size_t)mat * 2 * mm;
  double* const Vt = A + mm;
  constexpr int V = 16 / (int)sizeof(T);

  // ---- load: raw values into the V^T slots (zero elsewhere), then A = (M + M^T) / 2 and V^T = I ----
  for (int e = lane; e < mm; e += L) Vt[e] = 0.;
  __syncthreads();
  if constexpr (INTERLEAVED) {
    const T* hbm = p.arg + g0 * nn;
    const bool wide = (reinterpret_cast<uintptr_t>(hbm) & 15u) == 0;
    const int valid = valid_mats * nn;
    for (int i = tid * V; i < valid; i += kBlock * V) {
      T vals[V];
      if (wide && i + V <= valid) {
        const SpPack<T, V> pk = *reinterpret_cast<const SpPack<T, V>*>(hbm + i);
#pragma unroll
        for (int j = 0; j < V; j++) vals[j] = pk.v[j];
      } else {
#pragma unroll
        for (int j = 0; j < V; j++) vals[j] = i + j < valid ? hbm[i + j] : (T)0;
      }
#pragma unroll
      for (int j = 0; j < V; j++) {
        const int e = i + j;
        if (e < valid) {
          const int mt = e / nn, rem = e - mt * nn, r = rem / n, c = rem - r * n;
          lds[(size_t)mt * 2 * mm + mm + r * m + c] = (double)vals[j];
        }
      }
    }
  } else {
    const int mats_log2 = 8 - lanes_log2;
    for (int e = tid; e < M * nn; e += kBlock) {
      const int ml = e & (M - 1), comp = e >> mats_log2;
      if (ml < valid_mats) {
        const int r = comp / n, c = comp - r * n;
        lds[(size_t)ml * 2 * mm + mm + r * m + c] = (double)p.arg[g0 + ml + p.count * comp];
      }
    }
  }
  __syncthreads();
  for (int e = lane; e < mm; e += L) {
    const int i = e / m, j = e - i * m;
    A[e] = (Vt[e] + Vt[j * m + i]) / 2.;
  }
  __syncthreads();
  for (int e = lane; e < mm; e += L) {
    const int i = e / m, j = e - i * m;
    Vt[e] = i == j ? 1. : 0.;
  }

  // ---- sweeps ----
  const int hh = half * half, hm = half * m;
  const int nit_a = (hh + L - 1) >> lanes_log2, nit_v = (hm + L - 1) >> lanes_log2;
  const int diag_first = lane % (m + 1), diag_step = L % (m + 1);
  const ItemWalk wa0(lane, L, half), wv0(lane, L, m);
  for (int sweep = 0; sweep < el::kJacobiSweepsNxN; sweep++) {
    wave_lds_sync();                           // V^T = I (first sweep) / the last round's writes are visible
    double off = 0., diag = 0.;
    for (int e = lane, d = diag_first; e < mm; e += L) {
      const double x = fabs(A[e]);
      if (d == 0) diag += x; else off += x;
      d += diag_step;
      if (d >= m + 1) d -= m + 1;
    }
    for (int o = 1; o < L; o <<= 1) {          // butterfly inside the lane group: every lane ends with the same sums
      off += __shfl_xor(off, o);
      diag += __shfl_xor(diag, o);
    }
    if (__all(el::JacobiConverged(diag, off) ? 1 : 0)) break;                  // wavefront-uniform
    for (int round = 0; round < m - 1; round++) {
      double c = 1., s = 0.;
      if (lane < half) {
        int pp, qq;
        double t;
        el::RoundRobinPair(m, round, lane, pp, qq);
        el::JacobiAngle(A[pp * m + pp], A[qq * m + qq], A[pp * m + qq], c, s, t);
      }
      ItemWalk wa = wa0;
      for (int it = 0; it < nit_a; it++, wa.next()) {
        const bool act = wa.major < half;
        const int k = act ? wa.major : 0, l = wa.minor;
        const double ck = __shfl(c, k, L), sk = __shfl(s, k, L), cl = __shfl(c, l, L), sl = __shfl(s, l, L);
        if (act) {
          int pk, qk, pl, ql;
          el::RoundRobinPair(m, round, k, pk, qk);
          el::RoundRobinPair(m, round, l, pl, ql);
          double x00 = A[pk * m + pl], x01 = A[pk * m + ql], x10 = A[qk * m + pl], x11 = A[qk * m + ql];
          el::JacobiBlock(ck, sk, cl, sl, x00, x01, x10, x11);
          if (k == l) x01 = x10 = 0.;          // the annihilated pair: exact zeros
          A[pk * m + pl] = x00; A[pk * m + ql] = x01; A[qk * m + pl] = x10; A[qk * m + ql] = x11;
        }
      }
      ItemWalk wv = wv0;
      for (int it = 0; it < nit_v; it++, wv.next()) {
        const bool act = wv.major < half;
        const int k = act ? wv.major : 0, j = wv.minor;
        const double ck = __shfl(c, k, L), sk = __shfl(s, k, L);
        if (act) {
          int pk, qk;
          el::RoundRobinPair(m, round, k, pk, qk);
          const double x = Vt[pk * m + j], y = Vt[qk * m + j];
          Vt[pk * m + j] = ck * x - sk * y;
          Vt[qk * m + j] = sk * x + ck * y;
        }
      }
      wave_lds_sync();
    }
  }

  // ---- scalar prox of the eigenvalues: lane k < n holds p_k ----
  double pval = 0.;
  if (lane < n) {
    T c[7];
#pragma unroll
    for (int k = 0; k < 7; k++) c[k] = live && p.cp[k] != nullptr ? p.cp[k][g] : p.cv[k];
    const T td = live ? p.tau_diag[INTERLEAVED ? g * nn : g] : (T)1;
    double l1[1] = {A[lane * m + lane]};
    el::SpectralProx1D(l1, el::SpectralStep(tau_scal, td, p.invert_tau), el::SpectralCoeffs<T>(c), RtFun1D{p.fn});
    pval = l1[0];
  }
  wave_lds_sync();                             // every diagonal entry is read before A is overwritten

  // ---- R = V diag(p) V^T into the A slots ----
  {
    const int nit_r = (nn + L - 1) >> lanes_log2;
    ItemWalk wr(lane, L, n);
    for (int it = 0; it < nit_r; it++, wr.next()) {
      const bool act = wr.major < n;
      const int i = act ? wr.major : 0, j = wr.minor;
      double acc = 0.;
      for (int k = 0; k < n; k++) acc += Vt[k * m + i] * Vt[k * m + j] * __shfl(pval, k, L);
      if (act) A[i * m + j] = acc;
    }
  }
  __syncthreads();

  // ---- store ----
  if constexpr (INTERLEAVED) {
    T* hbm = p.res + g0 * nn;
    const bool wide = (reinterpret_cast<uintptr_t>(hbm) & 15u) == 0;
    const int valid = valid_mats * nn;
    for (int i = tid * V; i < valid; i += kBlock * V) {
      SpPack<T, V> pk;
#pragma unroll
      for (int j = 0; j < V; j++) {
        const int e = i + j < valid ? i + j : valid - 1;
        const int mt = e / nn, rem = e - mt * nn, r = rem / n, c = rem - r * n;
        pk.v[j] = (T)lds[(size_t)mt * 2 * mm + r * m + c];
      }
      if (wide && i + V <= valid) *reinterpret_cast<SpPack<T, V>*>(hbm + i) = pk;
      else {
#pragma unroll
        for (int j = 0; j < V; j++)
          if (i + j < valid) hbm[i + j] = pk.v[j];
      }
    }
  } else {
    const int mats_log2 = 8 - lanes_log2;
    for (int e = tid; e < M * nn; e += kBlock) {
      const int ml = e & (M - 1), comp = e >> mats_log2;
      if (ml < valid_mats) {
        const int r = comp / n, c = comp - r * n;
        p.res[g0 + ml + p.count * comp] = (T)lds[(size_t)ml * 2 * mm + r * m + c];
      }
    }
  }
}

template <class T>
int launch_eigen_nxn_coop(const SpectralArgs<T>& p, int n, bool interleaved, hipStream_t s) {
  if (n < kEigenCoopMinN || n > el::kEigenNxNMax) { set_error("prox_spectral: eigen_nxn cooperative kernel takes 6 <= n <= 32"); return 1; }
  const EigenCoopPlan g = eigen_coop_plan(n);
  const size_t blocks = (p.count + g.matrices - 1) / g.matrices;
  if (blocks > 0x7FFFFFFFu) { set_error("prox_spectral: too many groups for one launch"); return 1; }
  int lanes_log2 = 0;
  while ((1 << lanes_log2) < g.lanes) lanes_log2++;
  if (interleaved) PH_LAUNCH((eigen_nxn_coop_kernel<T, true>), dim3((unsigned)blocks), dim3(kBlock), g.lds_bytes, s, p, n, lanes_log2);
  else PH_LAUNCH((eigen_nxn_coop_kernel<T, false>), dim3((unsigned)blocks), dim3(kBlock), g.lds_bytes, s, p, n, lanes_log2);
  PH_LAUNCH_END("prox_spectral eigen_nxn kernel");
}
template int launch_eigen_nxn_coop<float>(const SpectralArgs<float>&, int, bool, hipStream_t);
template int launch_eigen_nxn_coop<double>(const SpectralArgs<double>&, int, bool, hipStream_t);

}  // namespace prost_hip
