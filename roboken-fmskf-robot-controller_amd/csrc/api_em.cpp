// api_em.cpp -- the EM sufficient statistics for Q and R of a replayed window of KF6 ticks:
// fmskf_tick_many_em (its own argument checks, the smoother's workspace, the piece table of its
// outputs, the smoother's forward launch and the launches of kernels_em.hip; the front end of the
// window calls is api_ctx.hpp's) and the host M-step fmskf_em_mstep.
#include <cmath>

#include "api_ctx.hpp"

using namespace fmskf;
using namespace fmskf::capi;

namespace {

constexpr size_t kTotal = FMSKF_EM_TOTAL_LEN;

}  // namespace

extern "C" {

int fmskf_tick_many_em(fmskf_handle h, const fmskf_tick_inputs *in, uint32_t n_ticks, uint64_t tick_stride,
                       const fmskf_em_out *out) {
  return guarded([&] {
    check_handle(h);
    check_window_model(h, "smoothing is");
    const uint64_t n = h->s.n;
    if (!out) fail(FMSKF_EINVAL, "null EM output");
    if (!out->n_meas && !out->sq && !out->sr && !out->total) fail(FMSKF_EINVAL, "every EM output pointer is null");
    if (out->flags & ~(uint32_t)FMSKF_EM_ACCUMULATE) fail(FMSKF_EINVAL, "unknown FMSKF_EM_* flags");
    // the kernels store device outputs with 4- and 8-byte accesses
    const uintptr_t d = (uintptr_t)out->sq | (uintptr_t)out->sr | (uintptr_t)out->total;
    const bool misaligned = (d & 7u) || ((uintptr_t)out->n_meas & 3u);
    window_call(h, "fmskf_tick_many_em", "EM", out->mem, out->pitch, misaligned, in, n_ticks, tick_stride,
                [&](const TickIn &t) {
      const bool host = out->mem == FMSKF_MEM_HOST, accumulate = (out->flags & FMSKF_EM_ACCUMULATE) != 0;
      const uint64_t pitch = out->pitch ? out->pitch : n;
      const SmoothHist hist = smooth_hist(h, n_ticks);
      EmOut eo{out->n_meas, out->sq, out->sr, pitch,
               out->total ? ensure_partial(h, &h->em_partial, kTotal, "EM") : nullptr, accumulate ? 1u : 0u};
      double *total = out->total;
      Piece pc[4];
      em_pieces(pc, n, pitch, out->n_meas, out->sq, out->sr, out->total);
      if (host) {
        char *stg = stage_pieces(h, pc, 4, "EM");
        eo.n_meas = piece_at<uint32_t>(stg, pc[0]);
        eo.sq = piece_at<double>(stg, pc[1]);
        eo.sr = piece_at<double>(stg, pc[2]);
        total = piece_at<double>(stg, pc[3]);
      }
      // a pending asynchronous ensemble event: its fold runs stand-alone, as ahead of fmskf_tick_many
      ens_flush(h);
      if (host && accumulate) pieces_in(h, pc, 4, "EM");
      const bool libm = h->cfg.trig == FMSKF_TRIG_LIBM;
      timed_passes(h, [&] {
        launch_check(launch_kf6_smooth_fwd(h->s, t, h->kf6, libm, hist, h->stream), "EM forward launch");
      }, [&] {
        launch_check(launch_kf6_em_bwd(h->s, t, h->kf6, libm, hist, eo, total, h->stream), "EM backward launch");
      });
      if (host) pieces_out(h, pc, 4, "EM");
    });
  });
}

int fmskf_em_mstep(const double *total, double *q, double *r) {
  return guarded([&] {
    if (!total || !q || !r) fail(FMSKF_EINVAL, "null argument");
    for (size_t k = 0; k < kTotal; k++)
      if (!std::isfinite(total[k])) fail(FMSKF_EINVAL, "non-finite EM total");
    if (!(total[0] > 0.0) || !(total[1] > 0.0)) fail(FMSKF_EINVAL, "EM total without transitions or measurements");
    for (int k = 0; k < 21; k++) q[k] = total[3 + k] / total[0];
    for (int k = 0; k < 10; k++) r[k] = total[24 + k] / total[1];
  });
}

}  // extern "C"
