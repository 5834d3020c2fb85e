// iterk_levelwave.hpp -- index rules of the level-per-wavefront K-iteration kernel (fused_iter2d_xkw_kernel, kernels_fused_iterk_lw.hip).
//
// Plain C++ (host and device): the kernel, the launcher and tests/host/iterk_levelwave_harness.cpp follow this one definition.
//
// A workgroup is K wavefronts on one (strip, chunk); the chunk owns the columns [xa, xb).  Wave l = 1 .. K carries level l of the
// pipeline of fused_iter2d_xk_kernel: in step t it runs
//     P_l : x^l at column p = lw_col(K, xa, l, t)        (needs x^(l-1), y^(l-1), b there and y_1^(l-1) one column to the left)
//     D_l : y^l at column q = p - 1                      (needs y^(l-1) there, x^l and x^(l-1) at q and p)
// and then hands column q of (y_1^l, y_2^l, x^l, b) to wave l + 1 through LDS slot lw_slot_written(t) of link l.  Wave l + 1 reads that
// slot in step t + 1 (lw_slot_read(t + 1)), where it is its column p: every level runs two columns -- one step -- behind the one before
// it, so whatever a wave reads was written before the barrier that ended the previous step.  One barrier per step, the same number
// of steps (lw_steps) for every wave of the workgroup: the bounds depend on the chunk only.
// Level 0 is the loaded iterate: wave 1 takes column p from the input ring instead of a link; wave K stores x^K at p and y^K at q.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PH_LW_HD __host__ __device__
#else
#define PH_LW_HD
#endif

namespace prost_hip {

constexpr int kLevelWaveRows = 248;        // rows a workgroup owns: 62 lanes x 4 rows, one halo lane per side (K <= 4)
constexpr int kLevelWaveRing = 3;          // slots of the input ring (columns in flight ahead of wave 1)

// steps (and barriers) of a chunk of xb - xa columns: the last one is D_K at column xb - 1
PH_LW_HD constexpr int lw_steps(int K, int xa, int xb) { return (xb - xa) + 3 * K - 2; }

// the column of P_l in step t (D_l: one less)
PH_LW_HD constexpr int lw_col(int K, int xa, int l, int t) { return xa - K + 1 + t - 2 * (l - 1); }

// the columns of level l a chunk needs: x^l on [xa - (K - l), xb + (K - l)], y^l on [xa - (K - l), xb + (K - l) - 1], inside the image
PH_LW_HD constexpr bool lw_p_active(int K, int xa, int xb, int nx, int l, int p) { return p >= 0 && p >= xa - (K - l) && p < nx && p <= xb + (K - l); }
PH_LW_HD constexpr bool lw_d_active(int K, int xa, int xb, int nx, int l, int q) { return q >= 0 && q >= xa - (K - l) && q < nx && q <= xb + (K - l) - 1; }

// columns of the iterate (level 0) a chunk loads through the ring; y_1^0 at column xa - K goes into registers directly
PH_LW_HD constexpr bool lw_loaded(int K, int xa, int xb, int nx, int k) { return k >= 0 && k < nx && k >= xa - K + 1 && k <= xb + K - 1; }
PH_LW_HD constexpr int lw_ring_slot(int k) { return (int)((unsigned)(k + 4 * kLevelWaveRing) % (unsigned)kLevelWaveRing); }      // k >= -K > -4 R
// The same ring with R slots (R = 2: the K = 4 per-pixel-b instances, whose workgroup then holds 32 KiB and five fit a CU).  Wave 1
// keeps R - 1 batches in flight: the prologue issues the columns p0 .. p0 + R - 2, the step of column p issues column p + R - 1 into
// the slot of column p - 1 -- read, and waited for, one barrier ago -- and then waits for column p with lw_ring_wait() batches behind it.
PH_LW_HD constexpr int lw_ring_slot(int k, int R) { return (int)((unsigned)(k + 4 * R) % (unsigned)R); }      // k >= -K >= -4 >= -4 R + 4
// batches issued behind column p's when its step waits: the columns p + 1 .. p + R - 1 that are loaded (the loaded columns are one range)
PH_LW_HD constexpr int lw_ring_wait(int K, int xa, int xb, int nx, int p, int R) {
  int n = 0;
  for (int r = 1; r < R; r++) n += lw_loaded(K, xa, xb, nx, p + r) ? 1 : 0;
  return n;
}

// link slots: a wave writes lw_slot_written(t) at the end of step t and reads lw_slot_read(t) at its start (t >= 1; step 0 reads nothing)
PH_LW_HD constexpr int lw_slot_written(int t) { return t & 1; }
PH_LW_HD constexpr int lw_slot_read(int t) { return (t - 1) & 1; }

// wave K: the owned columns it stores in a step
PH_LW_HD constexpr bool lw_stores_x(int xa, int xb, int p) { return p >= xa && p < xb; }
PH_LW_HD constexpr bool lw_stores_y(int xa, int xb, int q) { return q >= xa && q < xb; }

// bytes of LDS per workgroup: (K - 1) links x 2 slots + the ring, planes of 1 KiB (y_1, y_2, x and, per pixel, b)
PH_LW_HD constexpr int lw_lds_bytes(int K, int planes) { return (2 * (K - 1) + kLevelWaveRing) * planes * 1024; }
PH_LW_HD constexpr int lw_lds_bytes(int K, int planes, int R) { return (2 * (K - 1) + R) * planes * 1024; }
// the ring depth of an instance and the workgroups of it a CU can hold -- the kernel's launch bounds (160 KiB of LDS; the register
// budget of the instances allows five wavefronts per SIMD): K = 4 with per-pixel b runs two slots, 32 KiB, five per CU; every other
// instance keeps three slots.  The chunk rule below counts four per CU for all of them: a grid cut for five is slower.
PH_LW_HD constexpr int lw_ring_depth(int K, bool b_per_pixel) { return K == 4 && b_per_pixel ? 2 : kLevelWaveRing; }
PH_LW_HD constexpr int lw_groups_per_cu(int R) { return R == 2 ? 5 : 4; }
constexpr int kLevelWaveCUs = 256;          // slots of a round: kLevelWaveCUs x the workgroups per CU the rule counts (4: 1024)

// the shortest chunk in [lo, hi] whose workgroups (strips x chunks) all run in one round of `slots` resident workgroups; hi where
// none does (such images run several rounds whatever the length).  A chunk of c columns runs c + 3K - 2 steps: shorter is cheaper.
constexpr int lw_one_round_cols(long long nx, long long strips, long long slots = 1024, int lo = 6, int hi = 72) {
  for (int c = lo; c <= hi; c++)
    if (strips * ((nx + c - 1) / c) <= slots) return c;
  return hi;
}

}  // namespace prost_hip
