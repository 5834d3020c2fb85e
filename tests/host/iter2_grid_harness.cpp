// iter2_grid_harness.cpp -- prints the wave grid of the two-iterations kernel (prost_amd/csrc/iter2_grid.hpp) without a GPU.
//
//   iter2_grid_harness NX NY COLS PAIR
// prints "blocks B waves W" and then one line per wavefront: "block wave strip xa xb" -- the wave owns the columns [xa, xb) of
// row strip `strip` (62 x 4 rows, fp32); xa >= xb: it owns nothing.  The launcher (kernels_fused_iter2.hip: run_iter2) forms the
// same grid from the same header: strips x chunks workgroups of one wave, or strips x ceil(chunks / 2) workgroups of two.
#include <cstdio>
#include <cstdlib>

#include "iter2_grid.hpp"

int main(int argc, char** argv) {
  if (argc != 5) { std::fprintf(stderr, "usage: %s NX NY COLS PAIR\n", argv[0]); return 2; }
  const int nx = std::atoi(argv[1]), ny = std::atoi(argv[2]), cols = std::atoi(argv[3]);
  const bool pair = std::atoi(argv[4]) != 0;
  if (nx < 1 || ny < 1 || cols < 1) return 2;
  const unsigned strips = (unsigned)((ny + 62 * 4 - 1) / (62 * 4)), chunks = (unsigned)((nx + cols - 1) / cols);
  const unsigned blocks = prost_hip::iter2_blocks(strips, chunks, pair), waves = pair ? 2u : 1u;
  std::printf("blocks %u waves %u\n", blocks, waves);
  for (unsigned b = 0; b < blocks; b++)
    for (unsigned w = 0; w < waves; w++) {
      const prost_hip::Iter2Span s = prost_hip::iter2_span(b, blocks, w, chunks, cols, nx, pair);
      std::printf("%u %u %u %d %d\n", b, w, s.strip, s.xa, s.xb);
    }
  return 0;
}
