// window_pieces.hpp -- the output arrays of a window call (fmskf_tick_many_loglik,
// fmskf_tick_many_em, fmskf_tick_many_trace) as a table of pieces, and the plan of their device mirror.  Host only,
// nothing from HIP (tests/native/piece_table.cpp builds it with a plain C++ compiler); api_ctx.hpp
// includes it and runs the copies.
//
// Host arrays are mirrored on the device at the caller's pitch, so the kernel takes one pitch
// whatever the memory; only the `cols` elements of each row cross PCIe, either way.
#pragma once
#include <cstddef>
#include <cstdint>

namespace fmskf {

// a * b, or false when no allocation could hold it
inline bool bytes_fit(uint64_t a, uint64_t b, uint64_t *out) {
  if (b && a > (uint64_t)SIZE_MAX / b) return false;
  *out = a * b;
  return true;
}

// One output array: `rows` rows of `cols` elements of `elem` bytes, `step` elements apart (the
// same on both sides); null when the caller does not want it.  off: its place in the mirror.
struct Piece {
  void *user;
  uint64_t elem, rows, cols, step;
  uint64_t off = 0;
  uint64_t row_bytes() const { return cols * elem; }
  uint64_t step_bytes() const { return step * elem; }
};

// 256-byte-aligned offsets for the pieces the caller wants, the mirror's size in *bytes; false
// when no allocation could hold it
inline bool plan_pieces(Piece *pc, int count, uint64_t *bytes) {
  uint64_t total = 0;
  for (int k = 0; k < count; k++) {
    if (!pc[k].user) continue;
    pc[k].off = total;
    uint64_t b;
    if (!bytes_fit(pc[k].step, pc[k].rows, &b) || !bytes_fit(b, pc[k].elem, &b)) return false;
    if (b > (uint64_t)SIZE_MAX - 255) return false;
    b = (b + 255) & ~(uint64_t)255;
    if (b > (uint64_t)SIZE_MAX - total) return false;
    total += b;
  }
  *bytes = total;
  return true;
}

// the piece tables of the calls: n robots, `pitch` elements between the rows of the multi-row
// planes; a plain [N] plane and the total are one row
inline void loglik_pieces(Piece (&pc)[6], uint64_t n, uint64_t pitch, void *n_meas, void *nis_sum, void *logdet_sum,
                          void *innov_sum, void *innov_outer, void *total) {
  pc[0] = {n_meas, 4, 1, n, n};
  pc[1] = {nis_sum, 8, 1, n, n};
  pc[2] = {logdet_sum, 8, 1, n, n};
  pc[3] = {innov_sum, 8, 4, n, pitch};
  pc[4] = {innov_outer, 8, 10, n, pitch};
  pc[5] = {total, 8, 1, 4, 4};
}
inline void em_pieces(Piece (&pc)[4], uint64_t n, uint64_t pitch, void *n_meas, void *sq, void *sr, void *total) {
  pc[0] = {n_meas, 4, 1, n, n};
  pc[1] = {sq, 8, 21, n, pitch};
  pc[2] = {sr, 8, 10, n, pitch};
  pc[3] = {total, 8, 1, 34, 34};  // FMSKF_EM_TOTAL_LEN
}
// fmskf_tick_many_trace: n_ticks rows of the three per-tick planes, `rows` (n_ticks / every) state
// rows of 6 and 21 planes each, every row `pitch` elements from the next
inline void trace_pieces(Piece (&pc)[5], uint64_t n, uint64_t pitch, uint64_t n_ticks, uint64_t rows, void *nis,
                         void *status, void *applied, void *x, void *P) {
  pc[0] = {nis, 4, n_ticks, n, pitch};
  pc[1] = {status, 1, n_ticks, n, pitch};
  pc[2] = {applied, 1, n_ticks, n, pitch};
  pc[3] = {x, 4, 6 * rows, n, pitch};
  pc[4] = {P, 4, 21 * rows, n, pitch};
}

}  // namespace fmskf
