// iter2_grid.hpp -- which columns a wavefront of the two-iterations kernel (kernels_fused_iter2.hip) owns.
//
// Plain C++ (host and device): the kernel and the launcher read the grid from here, and tests/host/iter2_grid_harness.cpp
// prints it without a GPU.
//
// An image is cut into row strips (62 x VEC rows each) and every strip into `chunks` column chunks of `cols` columns.
//   unpaired: one workgroup = one wavefront = one chunk, marching left to right.
//   paired  : one workgroup = two wavefronts = the chunks 2m and 2m+1 of a strip.  Wave 0 marches LEFT over chunk 2m starting at
//             the seam between the two, wave 1 marches RIGHT over chunk 2m+1 starting there.  With an odd chunk count the last
//             pair's wave 1 owns nothing (xa >= xb); it still takes part in the workgroup's barriers.
// Workgroups are numbered XCD-aware (kernels_fused_iter.hip): block b runs on XCD b % 8, and every XCD gets a contiguous range of
// tiles, so the chunks of a strip -- and both halves of a pair, which are one workgroup -- share an L2.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PH_ITER2_HD __host__ __device__
#else
#define PH_ITER2_HD
#endif

namespace prost_hip {

struct Iter2Span {
  unsigned strip;   // row strip of the wavefront
  int xa, xb;       // it owns the columns [xa, xb); xa >= xb: none (second wave of an odd last pair)
};

PH_ITER2_HD inline unsigned iter2_groups_per_strip(unsigned chunks, bool pair) { return pair ? (chunks + 1u) / 2u : chunks; }

PH_ITER2_HD inline unsigned iter2_blocks(unsigned strips, unsigned chunks, bool pair) { return strips * iter2_groups_per_strip(chunks, pair); }

PH_ITER2_HD inline unsigned iter2_tile_of(unsigned block, unsigned blocks) {
  const unsigned xcd = block % 8u, q = block / 8u;
  return xcd * (blocks / 8u) + (xcd < blocks % 8u ? xcd : blocks % 8u) + q;
}

// wave: 0 / 1 inside a paired workgroup (0: marches left, 1: marches right), ignored otherwise
PH_ITER2_HD inline Iter2Span iter2_span(unsigned block, unsigned blocks, unsigned wave, unsigned chunks, int cols, int nx, bool pair) {
  const unsigned per_strip = iter2_groups_per_strip(chunks, pair);
  const unsigned tile = iter2_tile_of(block, blocks);
  const unsigned g = tile % per_strip;
  const unsigned chunk = pair ? 2u * g + wave : g;
  Iter2Span s;
  s.strip = tile / per_strip;
  s.xa = chunk < chunks ? (int)chunk * cols : nx;
  s.xb = s.xa + cols < nx ? s.xa + cols : nx;
  return s;
}

}  // namespace prost_hip
