// iterk_levelwave_rot_harness.cpp -- CPU checks of the one-round chunk rule of the level-per-wavefront K-iteration kernel
// (lw_one_round_cols, prost_amd/csrc/iterk_levelwave.hpp).  Stand-alone: exits 0 and prints "ok <checks>" or prints the first violated
// rule and exits 1.  (The level rotation this file was planned to cover as well was measured and not built: docs/rounds/r26.md.)
//
// usage: iterk_levelwave_rot_harness cols
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>

#include "iterk_levelwave.hpp"

using namespace prost_hip;

static long checks = 0;
#define REQUIRE(cond, ...)                                             \
  do {                                                                 \
    checks++;                                                          \
    if (!(cond)) { std::printf("VIOLATED %s: ", #cond); std::printf(__VA_ARGS__); std::printf("\n"); std::exit(1); } \
  } while (0)

static long long strips_of(long long ny) { return (ny + kLevelWaveRows - 1) / kLevelWaveRows; }
static long long grid_of(long long nx, long long strips, int c) { return strips * ((nx + c - 1) / c); }

static void check_rule(long long nx, long long strips, long long slots, int lo, int hi) {
  const int c = lw_one_round_cols(nx, strips, slots, lo, hi);
  REQUIRE(c >= lo && c <= hi, "nx %lld strips %lld slots %lld [%d, %d]: %d outside the range", nx, strips, slots, lo, hi, c);
  bool any = false;
  for (int k = lo; k <= hi; k++) any = any || grid_of(nx, strips, k) <= slots;
  if (!any) { REQUIRE(c == hi, "nx %lld strips %lld: nothing fits, %d instead of %d", nx, strips, c, hi); return; }
  REQUIRE(grid_of(nx, strips, c) <= slots, "nx %lld strips %lld: %d columns give %lld workgroups, more than %lld", nx, strips, c, grid_of(nx, strips, c), slots);
  REQUIRE(c == lo || grid_of(nx, strips, c - 1) > slots, "nx %lld strips %lld: %d columns fit as well as %d", nx, strips, c - 1, c);
  for (int k = lo; k < c; k++) REQUIRE(grid_of(nx, strips, k) > slots, "nx %lld strips %lld: the shorter chunk %d fits", nx, strips, k);
}

static int run_cols() {
  // the defaults (1024 slots, 6 .. 72) over widths and heights around the sizes in use, and other slots / ranges
  for (long long nx = 8; nx <= 9000; nx += (nx < 300 ? 1 : 37))
    for (long long ny : {8LL, 248LL, 252LL, 500LL, 1024LL, 2048LL, 3072LL, 4096LL, 8192LL}) {
      const long long strips = strips_of(ny);
      check_rule(nx, strips, 1024, 6, 72);
      REQUIRE(lw_one_round_cols(nx, strips) == lw_one_round_cols(nx, strips, 1024, 6, 72), "the defaults are 1024 slots, 6 .. 72 columns");
    }
  for (long long slots : {1LL, 4LL, 255LL, 256LL, 1000LL, 2048LL})
    for (long long nx : {8LL, 9LL, 37LL, 150LL, 1000LL, 4096LL})
      for (long long strips : {1LL, 2LL, 3LL, 17LL, 34LL}) {
        check_rule(nx, strips, slots, 6, 72);
        check_rule(nx, strips, slots, 1, 5);
        check_rule(nx, strips, slots, 72, 72);
      }
  // the sizes of the benchmark family, strips from kLevelWaveRows
  REQUIRE(strips_of(4096) == 17, "4096 rows are 17 strips");
  REQUIRE(lw_one_round_cols(4096, strips_of(4096)) == 69, "4096^2: %d", lw_one_round_cols(4096, strips_of(4096)));
  REQUIRE(grid_of(4096, strips_of(4096), 69) == 1020, "4096^2: %lld workgroups", grid_of(4096, strips_of(4096), 69));
  REQUIRE(lw_one_round_cols(3072, strips_of(3072)) == 40, "3072^2: %d", lw_one_round_cols(3072, strips_of(3072)));
  REQUIRE(lw_one_round_cols(2048, strips_of(2048)) == 19, "2048^2: %d", lw_one_round_cols(2048, strips_of(2048)));
  REQUIRE(lw_one_round_cols(1024, strips_of(1024)) == 6, "1024^2: %d", lw_one_round_cols(1024, strips_of(1024)));
  REQUIRE(lw_one_round_cols(8192, strips_of(8192)) == 72, "8192^2: %d", lw_one_round_cols(8192, strips_of(8192)));
  REQUIRE(grid_of(8192, strips_of(8192), 72) > 1024, "8192^2 runs several rounds at 72 columns");
  static_assert(lw_one_round_cols(4096, 17) == 69, "usable in constant expressions");
  std::printf("ok %ld\n", checks);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 2 && !std::strcmp(argv[1], "cols")) return run_cols();
  std::fprintf(stderr, "usage: %s cols\n", argv[0]);
  return 2;
}
