// prost/prox/potrs_blocks.hpp -- the per-block arithmetic of the blocked Cholesky factorisation and of the two triangular sweeps
// behind ProxIndRange (x = A (A'A)^-1 A' y).  Host and device templates: prost_amd/csrc/kernels_prox_range.hip calls them with one
// lane per row (or per matrix entry), tests/host/potrs_blocks_harness.cpp runs the same functions in plain loops under the
// sanitizers.  No function here allocates, synchronises or knows about lanes: the caller decides who runs which row, and puts a
// barrier wherever a comment below says "after every row has finished".
//
// Matrices are column-major.  The factor is blocked by kNB columns.  Block column k of the factorisation:
//   1. diagonal block: CholPivot / CholScaleRow / CholUpdateRow column by column (right-looking, unblocked), then its inverse in
//      place (TrtiDiag / TrtiRow, the column order of LAPACK's trti2);
//   2. panel: the rows below the block times the transposed inverse (PanelEntry) -- a product, not a substitution;
//   3. trailing update: every entry of the lower triangle to the right loses the dot product of two panel rows (TrailingDot).
// A sweep solves with the inverted diagonal blocks: z_k = Dinv_k r_k (BlockRow: four partial sums of kGroup columns each, added in
// the fixed order of Combine4), then every remaining row i loses M[i, block k] z_k (the same BlockRow).  The forward sweep walks
// L downwards; the backward sweep walks U = L' upwards, so both read a column of their matrix along consecutive rows.
#ifndef PROST_PROX_POTRS_BLOCKS_HPP_
#define PROST_PROX_POTRS_BLOCKS_HPP_
#include <cmath>
#include <cstddef>

#if defined(__HIPCC__)
#define PROST_POTRS_HD __host__ __device__ __forceinline__
#else
#define PROST_POTRS_HD inline
#endif

namespace prost {
namespace potrs {

constexpr int kNB = 64;                    ///< block size of the factorisation and of both sweeps
constexpr int kGroups = 4;                 ///< partial sums per row of a block step
constexpr int kGroup = kNB / kGroups;      ///< columns per partial sum

/// blocks of kNB that cover n
PROST_POTRS_HD size_t NumBlocks(size_t n) { return (n + kNB - 1) / kNB; }

// ---- diagonal block: D is nb x nb, lower triangle, leading dimension ld ----
/// column j, first: the pivot.  false (D untouched) for a pivot that is not a positive finite number.
template <class F>
PROST_POTRS_HD bool CholPivot(F* D, int ld, int j) {
  const F p = D[j + (size_t)j * ld];
  if (!(p > (F)0) || !(p - p == (F)0)) return false;      // (Inf - Inf and NaN - NaN are NaN)
  D[j + (size_t)j * ld] = std::sqrt(p);
  return true;
}
/// column j, then, row r > j (after the pivot is stored)
template <class F>
PROST_POTRS_HD void CholScaleRow(F* D, int ld, int j, int r) { D[r + (size_t)j * ld] = D[r + (size_t)j * ld] / D[j + (size_t)j * ld]; }
/// column j, last, row r > j (after every row has been scaled): the row's entries right of column j lose their share of column j
template <class F>
PROST_POTRS_HD void CholUpdateRow(F* D, int ld, int j, int r) {
  const F l = D[r + (size_t)j * ld];
  for (int c = j + 1; c <= r; c++) D[r + (size_t)c * ld] -= l * D[c + (size_t)j * ld];
}
/// inverse in place, column j = nb - 1 .. 0.  First every row r > j computes TrtiRow (reads column j and the inverted columns right of
/// it), then -- after every row has finished -- the values are stored to D[r, j] and D[j, j] becomes TrtiDiag.
template <class F>
PROST_POTRS_HD F TrtiDiag(const F* D, int ld, int j) { return (F)1 / D[j + (size_t)j * ld]; }
template <class F>
PROST_POTRS_HD F TrtiRow(const F* D, int ld, int j, int r) {
  F acc = 0;
  for (int c = j + 1; c <= r; c++) acc += D[r + (size_t)c * ld] * D[c + (size_t)j * ld];
  return -(acc * TrtiDiag(D, ld, j));
}

// ---- panel: row `row` of W below the diagonal block whose first column is col0; Dinv = the inverted block (leading dimension ldd) ----
/// entry c of the row: sum_{j <= c} W[row, col0 + j] Dinv[c, j].  It overwrites W[row, col0 + c], so a row goes c = nb - 1 .. 0.
template <class F>
PROST_POTRS_HD F PanelEntry(const F* W, size_t ld, size_t row, size_t col0, const F* Dinv, int ldd, int c) {
  F acc = 0;
  for (int j = 0; j <= c; j++) acc += W[row + (col0 + j) * ld] * Dinv[c + (size_t)j * ldd];
  return acc;
}

// ---- trailing update: W[row, col] -= TrailingDot for col0 + nb <= col <= row ----
template <class F>
PROST_POTRS_HD F TrailingDot(const F* W, size_t ld, size_t row, size_t col, size_t col0, int nb) {
  F acc = 0;
  for (int j = 0; j < nb; j++) acc += W[row + (col0 + j) * ld] * W[col + (col0 + j) * ld];
  return acc;
}

// ---- sweeps ----
/// partial sum `group` of sum_j M[row, col0 + j] z[j]: columns group * kGroup .. + kGroup - 1, below nb, in ascending order
template <class T>
PROST_POTRS_HD T BlockRow(const T* M, size_t ld, size_t row, size_t col0, int group, int nb, const T* z) {
  const int j1 = (group + 1) * kGroup < nb ? (group + 1) * kGroup : nb;
  T acc = 0;
  for (int j = group * kGroup; j < j1; j++) acc += M[row + (col0 + j) * ld] * z[j];
  return acc;
}
template <class T>
PROST_POTRS_HD T Combine4(T p0, T p1, T p2, T p3) { return ((p0 + p1) + p2) + p3; }

}  // namespace potrs
}  // namespace prost
#endif
