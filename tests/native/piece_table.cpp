// piece_table.cpp -- the piece tables of fmskf_tick_many_loglik and fmskf_tick_many_em and the plan
// of their device mirror, as csrc/window_pieces.hpp states them: a stand-alone host program built
// from that header alone (tests/test_pieces_cpu.py).  One query per line on stdin,
//   <loglik|em> <N> <pitch, 0 for N> <mask of the null pointers, bit k = piece k>
// one answer line each: the mirror's bytes, then per piece "off row_bytes step_bytes rows" ("-" for
// a null piece), or ENOMEM when no allocation could hold the mirror.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../roboken-fmskf-robot-controller_amd/csrc/window_pieces.hpp"

using namespace fmskf;

int main() {
  char call[16];
  uint64_t n, pitch;
  unsigned null_mask;
  static char user;  // any non-null address: the plan never follows it
  while (scanf("%15s %" SCNu64 " %" SCNu64 " %u", call, &n, &pitch, &null_mask) == 4) {
    auto p = [&](int k) -> void * { return (null_mask >> k) & 1u ? nullptr : &user; };
    if (!pitch) pitch = n;
    Piece pc[6];
    int count;
    if (!strcmp(call, "loglik")) {
      loglik_pieces(pc, n, pitch, p(0), p(1), p(2), p(3), p(4), p(5));
      count = 6;
    } else {
      Piece e[4];
      em_pieces(e, n, pitch, p(0), p(1), p(2), p(3));
      for (int k = 0; k < 4; k++) pc[k] = e[k];
      count = 4;
    }
    uint64_t bytes;
    if (!plan_pieces(pc, count, &bytes)) {
      puts("ENOMEM");
      continue;
    }
    printf("%" PRIu64, bytes);
    for (int k = 0; k < count; k++) {
      if (pc[k].user) printf(" | %" PRIu64 " %" PRIu64 " %" PRIu64 " %" PRIu64, pc[k].off, pc[k].row_bytes(), pc[k].step_bytes(), pc[k].rows);
      else printf(" | -");
    }
    puts("");
  }
  return 0;
}
