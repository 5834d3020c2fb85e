// iterk_levelwave_harness.cpp -- CPU checks of the index rules of the level-per-wavefront K-iteration kernel
// (prost_amd/csrc/iterk_levelwave.hpp) and of the pair plan with launches of four (include/prost/backend/pdhg_pair_plan.hpp).
// Stand-alone: exits 0 and prints "ok <checks>" or prints the first violated rule and exits 1.
//
// usage: iterk_levelwave_harness index K cols nx      simulates every chunk of an image of nx columns, step by step
//        iterk_levelwave_harness plan                 periods 1, 2, 3, 7, 10, budgets 1 .. 12
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "iterk_levelwave.hpp"
#include "prost/backend/pdhg_pair_plan.hpp"

using namespace prost_hip;

static long checks = 0;
#define REQUIRE(cond, ...)                                             \
  do {                                                                 \
    checks++;                                                          \
    if (!(cond)) { std::printf("VIOLATED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } \
  } while (0)

struct Slot { int col = -1, step = -1; bool read = true; };

static void check_chunk(int K, int xa, int xb, int nx) {
  const int steps = lw_steps(K, xa, xb), R = kLevelWaveRing;
  // which columns of x^l / y^l hold the true iterate (computed from true operands); level 0: what the chunk loads
  std::vector<std::set<int>> X(K + 1), Y(K + 1);
  for (int k = -2 * K; k <= nx + 2 * K; k++) if (lw_loaded(K, xa, xb, nx, k)) { X[0].insert(k); Y[0].insert(k); }
  if (xa - K >= 0) Y[0].insert(xa - K);          // y_1^0 of the column left of the first one, read directly
  std::vector<Slot> ring(R);
  std::vector<std::vector<Slot>> link(K + 1, std::vector<Slot>(2));          // link[l]: written by level l, read by level l + 1
  std::vector<int> barriers(K + 1, 0), held(K + 1, -1000);                    // held[l]: the column wave l received last (its p)
  std::vector<int> xstores(nx, 0), ystores(nx, 0);
  const int p0 = lw_col(K, xa, 1, 0);
  for (int r = 0; r < R - 1; r++) if (lw_loaded(K, xa, xb, nx, p0 + r)) ring[lw_ring_slot(p0 + r)] = Slot{p0 + r, -1, false};
  for (int t = 0; t < steps; t++) {
    // reads first: everything a wave reads in step t was written before the barrier that ended step t - 1
    for (int l = 1; l <= K; l++) {
      const int p = lw_col(K, xa, l, t);
      REQUIRE(l == 1 || p == lw_col(K, xa, l - 1, t) - 2, "level %d runs two columns behind level %d", l, l - 1);
      if (l == 1) {
        if (lw_loaded(K, xa, xb, nx, p + R - 1)) {      // the batch issued in this step overwrites the slot of column p - 1
          Slot& s = ring[lw_ring_slot(p + R - 1)];
          REQUIRE(s.read, "ring slot of column %d overwritten at step %d before it was read", s.col, t);
          REQUIRE(lw_ring_slot(p + R - 1) != lw_ring_slot(p), "the batch of step %d lands in the slot read in this step", t);
          s = Slot{p + R - 1, t, false};
        }
        if (lw_loaded(K, xa, xb, nx, p)) {
          Slot& s = ring[lw_ring_slot(p)];
          REQUIRE(s.col == p && s.step < t, "ring: step %d wants column %d, the slot holds %d issued at %d", t, p, s.col, s.step);
          s.read = true;
        }
      } else if (t >= 1) {
        Slot& s = link[l - 1][lw_slot_read(t)];
        REQUIRE(lw_slot_read(t) != lw_slot_written(t), "step %d reads the slot it writes", t);
        if (s.step != -1) {
          REQUIRE(s.step == t - 1 && s.col == p, "link %d: step %d wants column %d, the slot holds %d written at %d", l - 1, t, p, s.col, s.step);
          s.read = true;
        }
      }
      held[l] = p;
    }
    // the stages, then the hand-off
    for (int l = 1; l <= K; l++) {
      const int p = held[l], q = p - 1;
      if (lw_p_active(K, xa, xb, nx, l, p)) {
        REQUIRE(X[l - 1].count(p) && Y[l - 1].count(p) && (p == 0 || Y[l - 1].count(p - 1)), "P_%d at column %d reads a column level %d never computed (chunk %d..%d)", l, p, l - 1, xa, xb);
        REQUIRE(!X[l].count(p), "P_%d computes column %d twice", l, p);
        X[l].insert(p);
        if (l == K && lw_stores_x(xa, xb, p)) xstores[p]++;
      }
      if (lw_d_active(K, xa, xb, nx, l, q)) {
        REQUIRE(Y[l - 1].count(q) && X[l].count(q) && X[l - 1].count(q) && (q + 1 >= nx || (X[l].count(q + 1) && X[l - 1].count(q + 1))),
                "D_%d at column %d reads a column that was never computed (chunk %d..%d)", l, q, xa, xb);
        REQUIRE(!Y[l].count(q), "D_%d computes column %d twice", l, q);
        Y[l].insert(q);
        if (l == K && lw_stores_y(xa, xb, q)) ystores[q]++;
      }
      if (l < K) {
        Slot& s = link[l][lw_slot_written(t)];
        REQUIRE(s.read || s.step + 1 >= steps, "link %d: column %d (step %d) overwritten at step %d before level %d read it", l, s.col, s.step, t, l + 1);
        s = Slot{q, t, false};
      }
      barriers[l]++;
    }
  }
  for (int l = 1; l <= K; l++) REQUIRE(barriers[l] == steps && barriers[l] == barriers[1], "wave %d meets %d barriers, wave 1 %d", l, barriers[l], barriers[1]);
  for (int c = 0; c < nx; c++) {
    const int want = c >= xa && c < xb ? 1 : 0;
    REQUIRE(xstores[c] == want && ystores[c] == want, "column %d of chunk %d..%d: %d x stores, %d y stores", c, xa, xb, xstores[c], ystores[c]);
  }
  // the levels cover what the next one needs and no more than the header says
  for (int l = 1; l <= K; l++)
    for (int c = 0; c < nx; c++) REQUIRE((X[l].count(c) != 0) == (c >= xa - (K - l) && c <= xb + (K - l)), "x^%d at column %d", l, c);
}

static int run_index(int K, int cols, int nx) {
  REQUIRE(K >= 2 && K <= 4 && cols >= 1 && nx >= 1, "arguments");
  REQUIRE(lw_lds_bytes(K, 4) <= 40 * 1024, "LDS budget: four workgroups per CU");
  for (int xa = 0; xa < nx; xa += cols) check_chunk(K, xa, xa + cols < nx ? xa + cols : nx, nx);
  std::printf("ok %ld\n", checks);
  return 0;
}

// the pair plan as BackendPDHG::NextLaunch stated it before launches of four existed
static prost::PdhgLaunch old_pair_plan(size_t k, int room, size_t ri) {
  const bool res = prost::pdhg_is_residual_iteration(k, ri);
  if (room < 2 || k < 2 || res) return prost::PdhgLaunch{1, res, false, false};
  return prost::PdhgLaunch{2, prost::pdhg_is_residual_iteration(k + 1, ri), prost::pdhg_is_residual_iteration(k + 2, ri), false};
}

static int run_plan() {
  using namespace prost;
  const size_t periods[] = {1, 2, 3, 7, 10};
  for (size_t ri : periods)
    for (int budget = 1; budget <= 12; budget++)
      for (int mode : {kPairPlanPairs, kPairPlanFours}) {
        size_t k = 0; long fours = 0;
        std::vector<int> covered(200, 0);
        while (k < 150) {
          // a caller with `budget` iterations to run calls the plan with what is left of it, launch after launch
          for (int room = budget; room > 0;) {
            const PdhgLaunch l = pdhg_pair_plan(k, room, ri, mode), o = old_pair_plan(k, room, ri);
            REQUIRE(l.count >= 1 && l.count <= room, "period %zu budget %d: launch of %d with room %d", ri, budget, l.count, room);
            if (mode == kPairPlanPairs || !l.group)
              REQUIRE(l.count == o.count && l.residuals == o.residuals && l.store_mid == o.store_mid && !l.group, "period %zu k %zu room %d: not the pair plan", ri, k, room);
            if (l.group) {
              fours++;
              REQUIRE(l.count == 4 && !l.residuals && !l.store_mid, "a group is four plain iterations");
              REQUIRE(k >= ri, "period %zu: a group at %zu, inside the first residual period", ri, k);
              for (size_t i = 0; i <= 4; i++) REQUIRE(!pdhg_is_residual_iteration(k + i, ri), "period %zu: the group at %zu contains or directly precedes the residual iteration %zu", ri, k, k + i);
              const PdhgLaunch a = old_pair_plan(k, room, ri), b = old_pair_plan(k + 2, room - 2, ri);
              REQUIRE(a.count == 2 && b.count == 2 && !a.residuals && !a.store_mid && !b.residuals && !b.store_mid, "a group replaces two plain pairs");
            } else if (mode == kPairPlanFours && room >= 4 && k >= ri) {
              const PdhgLaunch a = old_pair_plan(k, room, ri), b = old_pair_plan(k + 2, room - 2, ri);
              REQUIRE(!(a.count == 2 && b.count == 2 && !a.residuals && !a.store_mid && !b.residuals && !b.store_mid), "period %zu k %zu: two plain pairs left as they are", ri, k);
            }
            REQUIRE(l.residuals == pdhg_is_residual_iteration(k + l.count - 1, ri) || l.count == 4, "the residual flag is that of the last iteration");
            for (int i = 0; i < l.count; i++) covered[k + i]++;
            k += (size_t)l.count; room -= l.count;
          }
        }
        for (size_t i = 0; i < k; i++) REQUIRE(covered[i] == 1, "period %zu budget %d: iteration %zu covered %d times", ri, budget, i, covered[i]);
        if (mode == kPairPlanFours && ri >= 7 && budget >= 4) REQUIRE(fours > 0, "period %zu budget %d: no launch of four", ri, budget);
        if (mode == kPairPlanPairs || ri < 5 || budget < 4) REQUIRE(fours == 0, "period %zu budget %d mode %d: %ld launches of four", ri, budget, mode, fours);
      }
  std::printf("ok %ld\n", checks);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 5 && !std::strcmp(argv[1], "index")) return run_index(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]));
  if (argc == 2 && !std::strcmp(argv[1], "plan")) return run_plan();
  std::fprintf(stderr, "usage: %s index K cols nx | plan\n", argv[0]);
  return 2;
}
