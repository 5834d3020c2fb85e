// kernels_fused_iterk_lw.hip -- K PDHG iterations per launch with ONE LEVEL PER WAVEFRONT (exact class, plain launches, K = 3 and 4).
// The pipeline, its single-wave instances and the host side: kernels_fused_iterk.hip.  A file of its own because it is built with
// flags of its own (Makefile: the stages are written on register pairs by hand, and the SLP vectoriser's second guess costs 0.7 %).
#include "iterk_common.hpp"

namespace prost_hip {

// The single-wave exact instances (fused_iter2d_xk_kernel, kernels_fused_iterk.hip) hold all 2K stages in one wavefront's registers: 166 / 203 VGPRs at K = 3 / 4 leave 3 / 2
// wavefronts per SIMD, too few to keep the VALU issuing (a lone wave issues every ~5 cycles), so their exact arithmetic -- 16-20 us
// of VALU work per iteration at 4096^2 -- lies open on top of the memory time.  Here a workgroup is K wavefronts on one (strip,
// chunk), wave l carries level l (the stage pair P_l, D_l of that kernel's `step`, same expressions, same operands: the bits are those of
// the single-wave instance, the pair kernel and the oracle) and hands each finished column to wave l + 1 through LDS.  A wave holds
// the state of ONE iteration, so four waves per SIMD stay resident and the arithmetic of the K iterations runs on all four SIMDs,
// while the launch still reads x, y, b once and writes x, y once per K iterations.  Index rules: iterk_levelwave.hpp.
//
// Synchronisation: per step one s_waitcnt lgkmcnt(0) + s_barrier (a raw barrier: wave 1's LDS-DMA batches stay in flight across
// it).  A wave reads link slot (t - 1) & 1 and writes slot t & 1, so the only writer of a slot and its only reader are always
// separated by a barrier in both directions.  Every wave of a workgroup runs lw_steps() steps whatever its level, rows or columns;
// the only return (rec->stop) is uniform and lies in front of the first barrier.
// Loads: wave 1 alone issues the input ring (R columns, the batch of column p + R - 1 in front of the wait for column p) and reads
// it; it stores nothing, so its vmcnt counts load batches only.  Wave K alone stores.
// Ring depth R (lw_ring_depth): three slots, except K = 4 with per-pixel b, which runs two: (6 + 2) x 4 KiB = 32 KiB per workgroup.  With
// two slots one batch is in flight while a column is computed: the batch of column p + 1 goes into the slot of column p - 1, whose
// ds_read_b128 were waited for (lgkmcnt(0)) one barrier ago.  That is 1.4 % of a launch faster than three slots at the same chunk
// length.  Five such workgroups fit a CU (the launch bounds allow it, the hardware places them), but a grid cut for five per CU is
// slower than one cut for four, so the chunk rule does not use it (docs/rounds/r31.md).  PROST_ITERK_LW_RING=3 keeps three slots.
//
// Placement (measured, docs/rounds/r26.md): workgroups b, b + 256, b + 512, b + 768 share a CU, and the hardware starts each of them
// on the next SIMD, so with level = wave + 1 every SIMD already holds one wave of each level: the levels' idle steps (2 (l - 1) at the
// start, 2 (K - l) at the end), wave 1's loads and wave K's stores are spread over the four SIMDs.  Rotating the levels by b / 256
// undoes exactly that (one level per SIMD) and costs 5.7 % of a launch at 4096^2, so the assignment stays as it is.
// PLACE (tools/iterk_levelwave_probe.py only): lane 0 of every wave records where it ran, after its last step, in place[b K + wave].
template <int K, int GFN, bool BPTR, int R = kLevelWaveRing, bool PLACE = false>
__global__ void __launch_bounds__(K * kWave, lw_groups_per_cu(R))
    fused_iter2d_xkw_kernel(float* __restrict__ x_out, float* __restrict__ y_out, const float* __restrict__ x, const float* __restrict__ y,
                            FusedArgs<float> a, const StepsK<K> sp, const PdhgRecord<float>* __restrict__ rec, unsigned* __restrict__ place) {
  static_assert(K >= 2 && K <= 4, "one halo lane per side: K <= 4");
  static_assert(R == 2 || R == 3, "the counted waits of wave 1 are written for two and three slots");
  constexpr int VEC = 4, H = 1;
  typedef float T;
  typedef native_f4 V4;
  if (rec && rec->stop) return;
  const int lvl = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / kWave)) + 1;      // 1 .. K, wave-uniform
  LevelStep P = sp.s[0];
  static_for<1, K>([&](auto L) { if (lvl - 1 == decltype(L)::value) P = sp.s[decltype(L)::value]; });
  if (rec) {                       // device-resident step sizes: the same for every iteration of the launch
    P.tauT = rec->p.tau * a.Tval; P.rD = (float)rec->p.ug.sq.rD; P.step = rec->p.ug.step; P.sigS = rec->p.sigma * a.Sval;
    P.theta = rec->p.theta; P.opt = 1 + rec->p.theta; P.sq = rec->p.ug.sq;
  }
  const idx_t nx = (idx_t)a.nx, ny = (idx_t)a.ny;
  const int lane = threadIdx.x & (kWave - 1);
  const unsigned total = gridDim.x, chunks = a.chunks;
  const unsigned xcd = blockIdx.x % 8u, q8 = blockIdx.x / 8u;          // XCD-aware tile order (kernels_fused_iter.hip)
  const unsigned tile = xcd * (total / 8u) + (xcd < total % 8u ? xcd : total % 8u) + q8;
  const unsigned strip = a.strips ? tile % a.strips : tile / chunks, chunk = a.strips ? tile / a.strips : tile % chunks;
  const idx_t row0 = (idx_t)strip * kLevelWaveRows + ((idx_t)lane - H) * VEC;
  const bool active = row0 >= 0 && row0 < ny;
  const bool owner = active && lane >= H && lane < kWave - H;
  const idx_t xa = (idx_t)chunk * a.cols_per_block;
  const idx_t xb = xa + a.cols_per_block < nx ? xa + a.cols_per_block : nx;
  const size_t N = (size_t)nx * (size_t)ny;
  constexpr int NB = 3 + (BPTR ? 1 : 0);
  constexpr int kSlot = NB * 1024;                 // one column: planes y_1, y_2, x (, b) of 64 lanes x 16 bytes
  // [ring: R slots][link 1: 2 slots] .. [link K - 1: 2 slots]; link l is written by wave l and read by wave l + 1
  __shared__ __attribute__((aligned(16))) char lds[lw_lds_bytes(K, NB, R)];
  const T* const y2base = y + N;
  T* const y2out = y_out + N;
  const T* const bptr = BPTR ? a.g_ptr[1] : nullptr;
  const T bval = a.g_val[1], bq = a.f_val[1];
  const bool tiny_is_zero = a.f_val[1] >= (T)kTinyIsZeroRadius;     // device_math.hpp: norm2_leq0_fast
  auto off_of = [&](idx_t c) { return ((unsigned)c * (unsigned)ny + (unsigned)row0) * (unsigned)sizeof(T); };
  const unsigned lds_base = (unsigned)(uintptr_t)((__attribute__((address_space(3))) char*)lds);
  const unsigned lane_addr = lds_base + (unsigned)lane * 16u;
  auto ring_issue = [&](idx_t k) {
    if (active) {
      const unsigned o = off_of(k);
      char* slot = lds + lw_ring_slot(k, R) * kSlot;
      __builtin_amdgcn_global_load_lds((glb_void_k*)(reinterpret_cast<const char*>(y) + o), (lds_void_k*)(slot), 16, 0, ITERK_LOAD_AUX);
      __builtin_amdgcn_global_load_lds((glb_void_k*)(reinterpret_cast<const char*>(y2base) + o), (lds_void_k*)(slot + 1024), 16, 0, ITERK_LOAD_AUX);
      __builtin_amdgcn_global_load_lds((glb_void_k*)(reinterpret_cast<const char*>(x) + o), (lds_void_k*)(slot + 2048), 16, 0, ITERK_LOAD_AUX);
      if (BPTR) __builtin_amdgcn_global_load_lds((glb_void_k*)(reinterpret_cast<const char*>(bptr) + o), (lds_void_k*)(slot + 3072), 16, 0, ITERK_LOAD_AUX);
    }
  };
  V4 n0 = {}, n1 = {}, n2 = {}, n3 = {};           // the column a step receives: y_1, y_2, x, b of the level below
  auto column_read = [&](unsigned slot_off) {       // four ds_read_b128, waited for by column_wait
    const unsigned addr = lane_addr + slot_off;
    asm volatile("ds_read_b128 %0, %1" : "=v"(n0) : "v"(addr) : "memory");
    asm volatile("ds_read_b128 %0, %1 offset:1024" : "=v"(n1) : "v"(addr) : "memory");
    asm volatile("ds_read_b128 %0, %1 offset:2048" : "=v"(n2) : "v"(addr) : "memory");
    if (BPTR) asm volatile("ds_read_b128 %0, %1 offset:3072" : "=v"(n3) : "v"(addr) : "memory");
  };
  auto column_wait = [&]() { asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(n0), "+v"(n1), "+v"(n2), "+v"(n3)::"memory"); };
  // Register layout: a column of four rows is TWO aligned pairs, rows (0, 1) and (2, 3) -- the halves of the 128-bit vector the ring
  // and link reads deliver and the link writes and stores take.  The stages below compute on these pairs (v_pk_add_f32 /
  // v_pk_mul_f32 on whole pairs wherever both rows run the same operation on operands of the same rows), so no element is moved
  // between a read, the arithmetic and a write.  Left to itself the SLP vectoriser packs the scalar lambdas of the single-wave kernel
  // too, but into pairs of its own choosing (row 1 of one array with row 3 of another) that it assembles with two v_mov_b32
  // per operand: 44 of that step's 243 VALU instructions were such copies (docs/rounds/r28.md).
  // The file is built with packed fp32 instructions switched off (Makefile): a pair operation is then two plain instructions on the
  // halves of the pair, in place -- the layout and the absence of copies are what the pairs are for, the v_pk_* forms cost VALU time
  // (docs/rounds/r31.md).
  typedef native_f2 V2;
  auto quad = [](const V2 (&v)[2]) { return __builtin_shufflevector(v[0], v[1], 0, 1, 2, 3); };
  auto column_write = [&](unsigned slot_off, const V2 (&v0)[2], const V2 (&v1)[2], const V2 (&v2)[2], const V2 (&v3)[2]) {
    const unsigned addr = lane_addr + slot_off;
    const V4 w0 = quad(v0), w1 = quad(v1), w2 = quad(v2), w3 = quad(v3);
    asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(w0) : "memory");
    asm volatile("ds_write_b128 %0, %1 offset:1024" ::"v"(addr), "v"(w1) : "memory");
    asm volatile("ds_write_b128 %0, %1 offset:2048" ::"v"(addr), "v"(w2) : "memory");
    if (BPTR) asm volatile("ds_write_b128 %0, %1 offset:3072" ::"v"(addr), "v"(w3) : "memory");
  };
  auto store_column = [&](T* base, unsigned byte_off, const V2 (&v)[2]) {
    V4* const dst = reinterpret_cast<V4*>(reinterpret_cast<char*>(base) + byte_off);
    if (ITERK_NT) __builtin_nontemporal_store(quad(v), dst);
    else *dst = quad(v);
  };

  // the state of ONE level: x^(l-1), y^(l-1), b and x^l at the columns p - 1 and p (which index holds which alternates: `stage`)
  V2 XP[2][2], YP[2][2][2], BP[2][2], XN[2][2];
#pragma unroll
  for (int s = 0; s < 2; s++)
#pragma unroll
    for (int h = 0; h < 2; h++) { XP[s][h] = V2{}; YP[s][0][h] = V2{}; YP[s][1][h] = V2{}; BP[s][h] = V2{}; XN[s][h] = V2{}; }
  // the step sizes of this wave's level as pairs: broadcast once, outside the step loop
  const V2 tauT2 = {P.tauT, P.tauT}, sigS2 = {P.sigS, P.sigS}, opt2 = {P.opt, P.opt}, theta2 = {P.theta, P.theta}, zero2 = {};
  // rows 2h, 2h + 1 of v where the conditions hold, 0 elsewhere (the boundary instance's selects; the select-free one passes v through)
  auto keep = [](bool c0, bool c1, V2 v) { return V2{c0 ? v[0] : (T)0, c1 ? v[1] : (T)0}; };

  // primal step at column c: x^l = prox_g(x^(l-1) - tau T K^T y^(l-1)) -- the EXACT forms of the single-wave kernel's `primal`, expression for
  // expression and operand for operand.  The divergence's vertical difference takes row j - 1: written as four scalar subtractions
  // straight into the halves of the pairs (one DPP shift for the row above the lane's first), never as a shifted pair built by copies.
  auto primal = [&](auto inner, idx_t c, const V2 (&y1c)[2], const V2 (&y2c)[2], const V2 (&y1p)[2], const V2 (&xin)[2], const V2 (&bc)[2], V2 (&xn)[2]) {
    constexpr bool I = decltype(inner)::value;
    const T up = lane_up(y2c[1][1]);            // lane 0: no source, its first row is halo
    const bool cn = I || c < nx - 1, cp = I || c > 0;
    V2 parg[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const idx_t row = row0 + 2 * h;
      const bool n0_ = I || row < ny - 1, n1_ = I || row + 1 < ny - 1, p0_ = I || row > 0, p1_ = I || row + 1 > 0;
      const T upj = h == 0 ? up : y2c[0][1];
      const V2 divy = {(n0_ ? y2c[h][0] : (T)0) - (p0_ ? upj : (T)0), (n1_ ? y2c[h][1] : (T)0) - (p1_ ? y2c[h][0] : (T)0)};
      const V2 divx = (I ? y1c[h] : keep(cn, cn, y1c[h])) - (I ? y1p[h] : keep(cp, cp, y1p[h]));
      const V2 sdiv = divx + divy;
      const V2 kty = zero2 - sdiv;
      const V2 arg = xin[h] - tauT2 * kty;
      parg[h] = arg - bc[h];
    }
    V2 r[2];
    if (GFN == PROST_FN_SQUARE) div_to_float_exact_vec<2>(parg, P.sq, r);
    else {
#pragma unroll
      for (int h = 0; h < 2; h++) r[h] = V2{f1d_apply<T, GFN>(GFN, parg[h][0], P.step, a.g_val[5], a.g_val[6]), f1d_apply<T, GFN>(GFN, parg[h][1], P.step, a.g_val[5], a.g_val[6])};
    }
#pragma unroll
    for (int h = 0; h < 2; h++) xn[h] = r[h] + bc[h];
  };
  // dual step at column c: y^l = prox_f*(y^(l-1) + sigma S K ((1 + theta) x^l - theta x^(l-1))) -- the EXACT forms of the single-wave kernel's `dual`.
  // The vertical differences take row j + 1: scalar subtractions into pair halves again, one DPP shift per array.
  auto dual = [&](auto inner, idx_t c, const V2 (&xn_c)[2], const V2 (&xn_n)[2], const V2 (&xo_c)[2], const V2 (&xo_n)[2], const V2 (&y1c)[2],
                  const V2 (&y2c)[2], V2 (&o1)[2], V2 (&o2)[2]) {
    constexpr bool I = decltype(inner)::value;
    const bool has_next = I || c + 1 < nx;
    const T bel_n = lane_down(xn_c[0][0]);            // lane 63: no source, its last row is halo
    const T bel_o = lane_down(xo_c[0][0]);
    V2 av[2][2], nv[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
      const idx_t row = row0 + 2 * h;
      const bool r0_ = I || row < ny - 1, r1_ = I || row + 1 < ny - 1;
      const T below_n = h == 0 ? xn_c[1][0] : bel_n, below_o = h == 0 ? xo_c[1][0] : bel_o;
      const V2 kx1 = keep(has_next, has_next, xn_n[h] - xn_c[h]);
      const V2 kx2 = {r0_ ? xn_c[h][1] - xn_c[h][0] : (T)0, r1_ ? below_n - xn_c[h][1] : (T)0};
      const V2 kp1 = keep(has_next, has_next, xo_n[h] - xo_c[h]);
      const V2 kp2 = {r0_ ? xo_c[h][1] - xo_c[h][0] : (T)0, r1_ ? below_o - xo_c[h][1] : (T)0};
      const V2 arg1 = y1c[h] + sigS2 * (opt2 * kx1 - theta2 * kp1);
      const V2 arg2 = y2c[h] + sigS2 * (opt2 * kx2 - theta2 * kp2);
      V2 norm = zero2;
      norm += arg1 * arg1;
      norm += arg2 * arg2;
      av[0][h] = arg1; av[1][h] = arg2; nv[h] = norm;
    }
    V2 out[2][2];
    norm2_leq0_fast<2, 2>(nv, av, bq, tiny_is_zero, out);
#pragma unroll
    for (int h = 0; h < 2; h++) { o1[h] = out[0][h]; o2[h] = out[1][h]; }
  };

  // ---- prologue: zero the LDS (lanes outside the image never receive data, links before their first write), start the ring ----
  if (lvl == 1 && active && xa - K >= 0) {          // y_1^0 at column xa - K: the left neighbour of P_1's first column
    const V4 v = *reinterpret_cast<const V4*>(reinterpret_cast<const char*>(y) + off_of(xa - K));
    YP[1][0][0] = v.lo; YP[1][0][1] = v.hi;
  }
  {
    V4* z = reinterpret_cast<V4*>(lds);
    const V4 zero = {};
    for (int i = threadIdx.x; i < lw_lds_bytes(K, NB, R) / 16; i += K * kWave) z[i] = zero;
  }
  asm volatile("s_waitcnt vmcnt(0)" : "+v"(YP[1][0][0]), "+v"(YP[1][0][1])::"memory");
  __syncthreads();
  const idx_t p0 = lw_col(K, xa, 1, 0);
  if (lvl == 1) {
#pragma unroll
    for (int r = 0; r < R - 1; r++) if (lw_loaded(K, xa, xb, nx, p0 + r)) ring_issue(p0 + r);
  }
  // every lane active and no lane on the first / last image row: the whole strip is interior
  const bool strip_inner = (idx_t)strip * kLevelWaveRows - H * VEC >= 1 && (idx_t)strip * kLevelWaveRows + (idx_t)(kWave - H) * VEC < ny - 1;
  const unsigned link_in = (unsigned)(R + 2 * (lvl - 2)) * kSlot, link_out = (unsigned)(R + 2 * (lvl - 1)) * kSlot;      // (wave 1 has no link_in, wave K no link_out)

  // nw: the index the state arrays keep column p at in this step, 1 - nw: column p - 1.  The two alternate from step to step (the loop
  // below is unrolled by two), so no register is copied to shift the pipeline by a column.
  auto stage = [&](auto inner, auto parity, idx_t p) {
    constexpr int nw = decltype(parity)::value, od = 1 - nw;
    const idx_t q = p - 1;
    if (lw_p_active(K, xa, xb, nx, lvl, p)) primal(inner, p, YP[nw][0], YP[nw][1], YP[od][0], XP[nw], BP[nw], XN[nw]);
    else {          // (as if the pipeline had shifted: the column keeps the value of the one before it)
      XN[nw][0] = XN[od][0]; XN[nw][1] = XN[od][1];
    }
    if (lvl == K && owner && lw_stores_x(xa, xb, p)) store_column(x_out, off_of(p), XN[nw]);
    V2 o1[2] = {}, o2[2] = {};
    if (lw_d_active(K, xa, xb, nx, lvl, q)) {
      dual(inner, q, XN[od], XN[nw], XP[od], XP[nw], YP[od][0], YP[od][1], o1, o2);
      if (lvl == K && owner && lw_stores_y(xa, xb, q)) { store_column(y_out, off_of(q), o1); store_column(y2out, off_of(q), o2); }
    }
    if (lvl < K) column_write(link_out + (unsigned)nw * kSlot, o1, o2, XN[od], BP[od]);      // column q of level lvl into slot lw_slot_written(t)
  };
  auto step = [&](auto parity, int t) {
    constexpr int nw = decltype(parity)::value;
    static_assert(lw_slot_written(nw) == nw && lw_slot_read(nw) == 1 - nw, "the link slot of a step is its parity");
    const idx_t p = lw_col(K, xa, lvl, t);
    n0 = V4{}; n1 = V4{}; n2 = V4{}; n3 = V4{};
    if (lvl == 1) {
      // the batch of column p + R - 1 goes into the slot of column p - 1, read (and waited for) in the previous step
      if (lw_loaded(K, xa, xb, nx, p + R - 1)) ring_issue(p + R - 1);
      if (lw_loaded(K, xa, xb, nx, p)) {
        // batches issued behind column p's (lw_ring_wait): those of p + 1 .. p + R - 1 that exist (the loaded columns are one range)
        //   R = 3:  p + 2 loaded: 2 batches   else p + 1 loaded: 1 batch   else none
        //   R = 2:                            p + 1 loaded: 1 batch        else none
        if (R == 3 && lw_loaded(K, xa, xb, nx, p + 2)) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * NB) : "memory");
        else if (lw_loaded(K, xa, xb, nx, p + 1)) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NB) : "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        column_read((unsigned)lw_ring_slot(p, R) * kSlot);
      }
    } else if (t >= 1) {
      column_read(link_in + (unsigned)(1 - nw) * kSlot);
    }
    column_wait();
    YP[nw][0][0] = n0.lo; YP[nw][0][1] = n0.hi; YP[nw][1][0] = n1.lo; YP[nw][1][1] = n1.hi; XP[nw][0] = n2.lo; XP[nw][1] = n2.hi;
    BP[nw][0] = BPTR ? n3.lo : V2{bval, bval}; BP[nw][1] = BPTR ? n3.hi : V2{bval, bval};
    // every stencil of both stages strictly inside the image: the select-free instance
    if (strip_inner && p >= 2 && p < nx - 1) stage(std::true_type(), parity, p);
    else stage(std::false_type(), parity, p);
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
  };
  const int steps = lw_steps(K, xa, xb);
  for (int t = 0; t < steps; t += 2) {
    step(int_c<0>(), t);
    if (t + 1 < steps) step(int_c<1>(), t + 1);
  }
  if constexpr (PLACE) {          // HW_ID[15:0]: wave, SIMD, pipe, CU, SH, SE; XCC_ID[3:0] above them
    const unsigned hw = __builtin_amdgcn_s_getreg((16 - 1) << 11 | 4), xcc = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 20);
    if (lane == 0) place[(size_t)blockIdx.x * K + (lvl - 1)] = hw | xcc << 16;
  }
}

// ring: the depth of the input ring, lw_ring_depth(K, b_per_pixel) or kLevelWaveRing (the instances built)
template <int K>
int launch_iterk_levelwave(int g_fn, bool b_per_pixel, int ring, dim3 grid, hipStream_t s, float* x_out, float* y_out, const float* x, const float* y,
                           const FusedArgs<float>& a, const StepsK<K>& sp, const PdhgRecord<float>* rec, unsigned* place) {
  const dim3 blockw(K * kWave);
  if (ring != kLevelWaveRing && ring != lw_ring_depth(K, b_per_pixel)) { set_error("fused K-iteration launch (level per wavefront): no instance with that ring depth"); return 1; }
#define GOWR(G, BP, RD) PH_LAUNCH((fused_iter2d_xkw_kernel<K, G, BP, RD>), grid, blockw, 0, s, x_out, y_out, x, y, a, sp, rec, nullptr)
#define GOW(G, BP) do { if (ring == kLevelWaveRing) GOWR(G, BP, kLevelWaveRing); else GOWR(G, BP, lw_ring_depth(K, BP)); } while (0)
  if constexpr (K == 4) {
    if (place) {          // the instance that ships: the ring depth of the headline launch
      if (ring != lw_ring_depth(4, true)) { set_error("fused K-iteration launch: the placement record exists for the default ring depth"); return 1; }
      PH_LAUNCH((fused_iter2d_xkw_kernel<4, PROST_FN_SQUARE, true, lw_ring_depth(4, true), true>), grid, blockw, 0, s, x_out, y_out, x, y, a, sp, rec, place);
      hipError_t e_ = hipGetLastError();
      return e_ != hipSuccess ? fail(e_, "fused K-iteration kernel (level per wavefront, placement record)") : 0;
    }
  }
  if (g_fn == PROST_FN_SQUARE) { if (b_per_pixel) GOW(PROST_FN_SQUARE, true); else GOW(PROST_FN_SQUARE, false); }
  else { if (b_per_pixel) GOW(PROST_FN_ABS, true); else GOW(PROST_FN_ABS, false); }
#undef GOW
#undef GOWR
  { hipError_t e_ = hipGetLastError(); if (e_ != hipSuccess) return fail(e_, "fused K-iteration kernel (level per wavefront)"); }
  return 0;
}
template int launch_iterk_levelwave<3>(int, bool, int, dim3, hipStream_t, float*, float*, const float*, const float*, const FusedArgs<float>&, const StepsK<3>&,
                                       const PdhgRecord<float>*, unsigned*);
template int launch_iterk_levelwave<4>(int, bool, int, dim3, hipStream_t, float*, float*, const float*, const float*, const FusedArgs<float>&, const StepsK<4>&,
                                       const PdhgRecord<float>*, unsigned*);

}  // namespace prost_hip
