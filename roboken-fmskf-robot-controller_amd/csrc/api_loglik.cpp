// api_loglik.cpp -- the innovation log-likelihood of a replayed window of KF6 ticks:
// fmskf_tick_many_loglik (its own argument checks, the piece table of its outputs, the launches of
// kernels_loglik.hip; the front end of the window calls is api_ctx.hpp's).
#include "api_ctx.hpp"

using namespace fmskf;
using namespace fmskf::capi;

extern "C" {

int fmskf_tick_many_loglik(fmskf_handle h, const fmskf_tick_inputs *in, uint32_t n_ticks, uint64_t tick_stride,
                           const fmskf_loglik_out *out) {
  return guarded([&] {
    check_handle(h);
    check_window_model(h, "the innovation log-likelihood is");
    const uint64_t n = h->s.n;
    if (!out) fail(FMSKF_EINVAL, "null log-likelihood output");
    if (!out->n_meas && !out->nis_sum && !out->logdet_sum && !out->innov_sum && !out->innov_outer && !out->total)
      fail(FMSKF_EINVAL, "every log-likelihood output pointer is null");
    if (out->flags & ~(uint32_t)FMSKF_LL_ACCUMULATE) fail(FMSKF_EINVAL, "unknown FMSKF_LL_* flags");
    // the kernels store device outputs with 4- and 8-byte accesses
    const uintptr_t d = (uintptr_t)out->nis_sum | (uintptr_t)out->logdet_sum | (uintptr_t)out->innov_sum |
                        (uintptr_t)out->innov_outer | (uintptr_t)out->total;
    const bool misaligned = (d & 7u) || ((uintptr_t)out->n_meas & 3u);
    window_call(h, "fmskf_tick_many_loglik", "log-likelihood", out->mem, out->pitch, misaligned, in, n_ticks,
                tick_stride, [&](const TickIn &t) {
      const bool host = out->mem == FMSKF_MEM_HOST, accumulate = (out->flags & FMSKF_LL_ACCUMULATE) != 0;
      const uint64_t pitch = out->pitch ? out->pitch : n;
      LoglikOut lo{out->n_meas, out->nis_sum, out->logdet_sum, out->innov_sum, out->innov_outer, pitch,
                   out->total ? ensure_partial(h, &h->loglik_partial, 4, "log-likelihood") : nullptr,
                   accumulate ? 1u : 0u};
      double *total = out->total;
      Piece pc[6];
      loglik_pieces(pc, n, pitch, out->n_meas, out->nis_sum, out->logdet_sum, out->innov_sum, out->innov_outer,
                    out->total);
      if (host) {
        char *stg = stage_pieces(h, pc, 6, "log-likelihood");
        lo.n_meas = piece_at<uint32_t>(stg, pc[0]);
        lo.nis_sum = piece_at<double>(stg, pc[1]);
        lo.logdet_sum = piece_at<double>(stg, pc[2]);
        lo.innov_sum = piece_at<double>(stg, pc[3]);
        lo.innov_outer = piece_at<double>(stg, pc[4]);
        total = piece_at<double>(stg, pc[5]);
      }
      // a pending asynchronous ensemble event: its fold runs stand-alone, as ahead of fmskf_tick_many
      ens_flush(h);
      if (host && accumulate) pieces_in(h, pc, 6, "log-likelihood");
      h->time_begin();
      launch_check(launch_kf6_loglik(h->s, t, h->kf6, h->cfg.trig == FMSKF_TRIG_LIBM, lo, total, h->stream),
                   "log-likelihood launch");
      h->time_end();
      if (host) pieces_out(h, pc, 6, "log-likelihood");
    });
  });
}

}  // extern "C"
