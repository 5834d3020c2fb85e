// iterk_levelwave_ring_harness.cpp -- CPU checks of the input ring of the level-per-wavefront K-iteration kernel at a ring depth
// given as a parameter (lw_ring_slot(k, R), lw_ring_wait, lw_lds_bytes(K, planes, R): prost_amd/csrc/iterk_levelwave.hpp) and of the
// chunk rule at five workgroups per CU.  Stand-alone: exits 0 and prints "ok <checks>" or prints the first violated rule and exits 1.
//
// usage: iterk_levelwave_ring_harness ring R K cols nx      wave 1 of every chunk of an image of nx columns, step by step
//        iterk_levelwave_ring_harness geom                  LDS bytes, workgroups per CU, chunk lengths at 1280 slots
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "iterk_levelwave.hpp"

using namespace prost_hip;

static long checks = 0;
#define REQUIRE(cond, ...)                                             \
  do {                                                                 \
    checks++;                                                          \
    if (!(cond)) { std::printf("VIOLATED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } \
  } while (0)

// a ring slot: the column it holds, the step its batch was issued in (-1: the prologue), the step it was read in (-2: not yet)
struct Slot { int col = -1000, issued = -2, read_at = -2; bool filled = false; };

// Wave 1 as the kernel runs it: the prologue issues R - 1 batches; the step of column p issues the batch of p + R - 1, waits until at
// most lw_ring_wait() batches are outstanding (loads return in order) and reads the slot of p.
static void check_chunk(int R, int K, int xa, int xb, int nx) {
  const int steps = lw_steps(K, xa, xb);
  std::vector<Slot> ring(R);
  std::vector<int> order;                       // the columns in the order their batches were issued
  std::vector<int> reads(nx + 2 * K + 2, 0);    // reads of column k at index k + K
  auto issue = [&](int k, int t) {
    const int s = lw_ring_slot(k, R);
    REQUIRE(s >= 0 && s < R, "R %d: slot %d of column %d", R, s, k);
    Slot& sl = ring[s];
    REQUIRE(!sl.filled || sl.read_at >= -1, "R %d chunk %d..%d: the batch of column %d (step %d) overwrites column %d, never read", R, xa, xb, k, t, sl.col);
    REQUIRE(!sl.filled || sl.read_at < t, "R %d chunk %d..%d: the batch of column %d lands at step %d in a slot read at step %d", R, xa, xb, k, t, sl.read_at);
    sl = Slot{k, t, -2, true};
    order.push_back(k);
  };
  const int p0 = lw_col(K, xa, 1, 0);
  for (int r = 0; r < R - 1; r++) if (lw_loaded(K, xa, xb, nx, p0 + r)) issue(p0 + r, -1);
  for (int t = 0; t < steps; t++) {
    const int p = lw_col(K, xa, 1, t);
    if (lw_loaded(K, xa, xb, nx, p + R - 1)) {
      REQUIRE(lw_ring_slot(p + R - 1, R) != lw_ring_slot(p, R), "R %d: the batch of step %d lands in the slot read in this step", R, t);
      REQUIRE(lw_ring_slot(p + R - 1, R) == lw_ring_slot(p - 1, R), "R %d: the batch of step %d goes into the slot of the column read one step ago", R, t);
      issue(p + R - 1, t);
    }
    if (lw_loaded(K, xa, xb, nx, p)) {
      size_t at = 0;
      while (at < order.size() && order[at] != p) at++;
      REQUIRE(at < order.size(), "R %d chunk %d..%d: step %d reads column %d, whose batch was never issued", R, xa, xb, t, p);
      const int behind = (int)(order.size() - 1 - at), wait = lw_ring_wait(K, xa, xb, nx, p, R);
      REQUIRE(wait == behind, "R %d chunk %d..%d nx %d: step %d waits for %d batches behind column %d, %d were issued", R, xa, xb, nx, t, wait, p, behind);
      REQUIRE(wait >= 0 && wait <= R - 1, "R %d: a wait of %d batches", R, wait);
      Slot& sl = ring[lw_ring_slot(p, R)];
      REQUIRE(sl.filled && sl.col == p && sl.issued < t, "R %d chunk %d..%d: step %d wants column %d, the slot holds %d issued at %d", R, xa, xb, t, p, sl.col, sl.issued);
      REQUIRE(sl.read_at == -2, "R %d: column %d read twice", R, p);
      sl.read_at = t;
      reads[p + K]++;
    }
  }
  for (int k = -K; k <= nx + K; k++) {
    const bool inside = k >= 0 && k < nx;
    REQUIRE(!lw_loaded(K, xa, xb, nx, k) || inside, "column %d outside the image is loaded", k);
    REQUIRE(reads[k + K] == (lw_loaded(K, xa, xb, nx, k) ? 1 : 0), "R %d chunk %d..%d nx %d: column %d read %d times", R, xa, xb, nx, k, reads[k + K]);
  }
  int loaded = 0;
  for (int k = 0; k < nx; k++) loaded += lw_loaded(K, xa, xb, nx, k) ? 1 : 0;
  REQUIRE((int)order.size() == loaded, "R %d chunk %d..%d: %d batches for %d loaded columns", R, xa, xb, (int)order.size(), loaded);
}

static int run_ring(int R, int K, int cols, int nx) {
  REQUIRE((R == 2 || R == 3) && K >= 2 && K <= 4 && cols >= 1 && nx >= 1, "arguments");
  for (int k = -K; k < 3 * R; k++) REQUIRE(lw_ring_slot(k + 1, R) == (lw_ring_slot(k, R) + 1) % R, "R %d: the slots of the columns %d, %d do not follow each other", R, k, k + 1);
  if (R == kLevelWaveRing) for (int k = -K; k < 200; k++) REQUIRE(lw_ring_slot(k, R) == lw_ring_slot(k), "the three-slot ring is the one without a depth argument");
  for (int xa = 0; xa < nx; xa += cols) check_chunk(R, K, xa, xa + cols < nx ? xa + cols : nx, nx);
  std::printf("ok %ld\n", checks);
  return 0;
}

static long long strips_of(long long ny) { return (ny + kLevelWaveRows - 1) / kLevelWaveRows; }
static long long grid_of(long long nx, long long strips, int c) { return strips * ((nx + c - 1) / c); }

static int run_geom() {
  constexpr int kLdsPerCU = 160 * 1024;
  for (int K = 2; K <= 4; K++)
    for (int planes = 3; planes <= 4; planes++) {
      REQUIRE(lw_lds_bytes(K, planes, kLevelWaveRing) == lw_lds_bytes(K, planes), "K %d: the three-slot bytes are those without a depth argument", K);
      REQUIRE(lw_lds_bytes(K, planes, 3) - lw_lds_bytes(K, planes, 2) == planes * 1024, "K %d: a ring slot is one column of %d planes", K, planes);
    }
  REQUIRE(lw_ring_depth(4, true) == 2, "K = 4 with per-pixel b runs the two-slot ring");
  REQUIRE(lw_ring_depth(4, false) == 3 && lw_ring_depth(3, true) == 3 && lw_ring_depth(3, false) == 3, "every other instance keeps three slots");
  REQUIRE(lw_lds_bytes(4, 4, lw_ring_depth(4, true)) == 32768, "K = 4, per-pixel b: %d bytes", lw_lds_bytes(4, 4, 2));
  REQUIRE(lw_lds_bytes(4, 4) == 36864, "the three-slot instance: %d bytes", lw_lds_bytes(4, 4));
  REQUIRE(kLdsPerCU / lw_lds_bytes(4, 4, 2) == 5 && lw_groups_per_cu(2) == 5, "five workgroups of 32 KiB per CU");
  REQUIRE(kLdsPerCU / lw_lds_bytes(4, 4, 3) == 4 && lw_groups_per_cu(3) == 4, "four workgroups of 36 KiB per CU");
  const long long slots = (long long)kLevelWaveCUs * lw_groups_per_cu(2);
  REQUIRE(slots == 1280, "%lld slots", slots);
  const struct { int n, cols; long long groups; } want[] = {{4096, 55, 1275}, {3072, 32, 1248}, {2048, 15, 1233}, {1024, 6, 855}};
  for (const auto& w : want) {
    const int c = lw_one_round_cols(w.n, strips_of(w.n), slots);
    REQUIRE(c == w.cols, "%d^2 at 1280 slots: %d columns", w.n, c);
    REQUIRE(grid_of(w.n, strips_of(w.n), c) == w.groups, "%d^2: %lld workgroups", w.n, grid_of(w.n, strips_of(w.n), c));
    REQUIRE(c == 6 || grid_of(w.n, strips_of(w.n), c - 1) > slots, "%d^2: %d columns fit as well", w.n, c - 1);
  }
  REQUIRE(lw_one_round_cols(8192, strips_of(8192), slots) == 72 && grid_of(8192, strips_of(8192), 72) > slots, "8192^2 runs several rounds at 72 columns");
  // the defaults are untouched: the round of four per CU
  REQUIRE(lw_one_round_cols(4096, strips_of(4096)) == 69 && lw_one_round_cols(2048, strips_of(2048)) == 19, "the default rule");
  static_assert(lw_one_round_cols(4096, 17, 1280) == 55, "usable in constant expressions");
  static_assert(lw_ring_wait(4, 0, 55, 4096, 10, 2) == 1 && lw_ring_wait(4, 0, 55, 4096, 10, 3) == 2, "usable in constant expressions");
  std::printf("ok %ld\n", checks);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 6 && !std::strcmp(argv[1], "ring")) return run_ring(std::atoi(argv[2]), std::atoi(argv[3]), std::atoi(argv[4]), std::atoi(argv[5]));
  if (argc == 2 && !std::strcmp(argv[1], "geom")) return run_geom();
  std::fprintf(stderr, "usage: %s ring R K cols nx | geom\n", argv[0]);
  return 2;
}
