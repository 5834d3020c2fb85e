// pdhg_pair_plan.hpp -- the launch plan of the exact-class gray-value PDHG path (pair kernel, optionally with groups of four).
//
// Plain C++: BackendPDHG::NextLaunch calls it, tests/host/pdhg_pair_plan_harness.cpp checks it without a GPU.
#pragma once

#include <cstddef>

namespace prost {

/// backend_pdhg.cu:389
inline bool pdhg_is_residual_iteration(size_t k, size_t residual_iter) { return k == 0 || (k % residual_iter) == 0; }

enum PdhgPairPlanMode {
  kPairPlanPairs = 0,        ///< singles and pairs
  kPairPlanFours = 1         ///< ... and one launch of four iterations wherever two plain pairs would follow one another
};

/// `count` iterations in one launch; `residuals`: the last of them is a residual iteration (its sums are formed in the kernel);
/// `store_mid`: a pair that also stores the iterate in between; `group`: a launch of the K-iteration kernel
struct PdhgLaunch { int count; bool residuals, store_mid; bool group = false; };

/// What runs at iteration k when `room` iterations may run unobserved.
/// Pairs: two iterations share a launch whenever k >= 2 is not a residual iteration (iterations 0 and 1 run with zeroed K^T y / K x
/// vectors; a residual iteration as the FIRST of a launch would need y^(k-1)).  If the second is a residual iteration its sums are
/// formed in the kernel; a pair whose successor k + 2 is a residual iteration -- it streams y^(k+1) as y_prev -- stores the iterate
/// in between.
/// Fours: where that plan would launch two PLAIN pairs in a row -- none of k .. k + 4 is a residual iteration, so neither pair
/// carries sums or stores its middle iterate -- and the room allows it, the four iterations run in one launch.  A group therefore
/// never contains a residual iteration and never directly precedes one; everything else is the pair plan unchanged.
/// The first residual period (k < residual_iter) keeps the pair plan: it starts with the two single launches and is never the
/// steady state, a solve of a handful of iterations launches exactly what it launched before, and the launch kinds of the first
/// twelve iterations of the headline problem are pinned by tests/test_gpu_fullsize.py.
inline PdhgLaunch pdhg_pair_plan(size_t k, int room, size_t residual_iter, int mode) {
  const bool res_k = pdhg_is_residual_iteration(k, residual_iter);
  if (room < 2 || k < 2 || res_k) return PdhgLaunch{1, res_k, false, false};
  if (mode == kPairPlanFours && room >= 4 && k >= residual_iter) {
    bool plain = true;
    for (size_t i = 1; i <= 4; i++) plain = plain && !pdhg_is_residual_iteration(k + i, residual_iter);
    if (plain) return PdhgLaunch{4, false, false, true};
  }
  return PdhgLaunch{2, pdhg_is_residual_iteration(k + 1, residual_iter), pdhg_is_residual_iteration(k + 2, residual_iter), false};
}

}  // namespace prost
