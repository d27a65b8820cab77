// api_trace.cpp -- the per-tick trace of a replayed window of KF6 ticks: fmskf_tick_many_trace
// (its own model and argument checks, the piece table of its outputs, the launch of
// kernels_trace.hip; the front end of the window calls is api_ctx.hpp's).
#include "api_ctx.hpp"

using namespace fmskf;
using namespace fmskf::capi;

namespace {

// KF6 with the plain state, gated or not: check_window_model without its gate refusal, which the
// other window calls keep
void check_trace_model(const fmskf_ctx *h) {
  if (h->cfg.model != FMSKF_MODEL_KF6) fail(FMSKF_ENOTSUP, "the per-tick trace is for KF6");
  if (h->cfg.flags & FMSKF_CFG_COMP_POS) fail(FMSKF_ENOTSUP, "the per-tick trace is for KF6 without FMSKF_CFG_COMP_POS");
}

}  // namespace

extern "C" {

int fmskf_tick_many_trace(fmskf_handle h, const fmskf_tick_inputs *in, uint32_t n_ticks, uint64_t tick_stride,
                          const fmskf_trace_out *out) {
  return guarded([&] {
    check_handle(h);
    check_trace_model(h);
    const uint64_t n = h->s.n;
    if (!out) fail(FMSKF_EINVAL, "null trace output");
    if (!out->nis && !out->status && !out->applied && !out->x && !out->P)
      fail(FMSKF_EINVAL, "every trace output pointer is null");
    if (out->reserved || out->reserved2) fail(FMSKF_EINVAL, "fmskf_trace_out.reserved and reserved2 must be 0");
    const bool state_rows = out->x || out->P;
    if (state_rows && (out->every == 0 || out->every > n_ticks))
      fail(FMSKF_EINVAL, "fmskf_trace_out.every must be 1 .. n_ticks when x or P is given");
    // the kernel stores the float planes with 4-byte accesses, the byte planes byte by byte
    const bool misaligned = (((uintptr_t)out->nis | (uintptr_t)out->x | (uintptr_t)out->P) & 3u) != 0;
    window_call(h, "fmskf_tick_many_trace", "trace", out->mem, out->pitch, misaligned, in, n_ticks, tick_stride,
                [&](const TickIn &t) {
      const bool host = out->mem == FMSKF_MEM_HOST;
      const uint64_t pitch = out->pitch ? out->pitch : n;
      TraceOut to{out->nis, out->status, out->applied, out->x, out->P, pitch, state_rows ? out->every : 0u};
      Piece pc[5];
      trace_pieces(pc, n, pitch, n_ticks, state_rows ? n_ticks / out->every : 0u, out->nis, out->status, out->applied,
                   out->x, out->P);
      if (host) {
        char *stg = stage_pieces(h, pc, 5, "trace");
        to.nis = piece_at<float>(stg, pc[0]);
        to.status = piece_at<uint8_t>(stg, pc[1]);
        to.applied = piece_at<uint8_t>(stg, pc[2]);
        to.x = piece_at<float>(stg, pc[3]);
        to.P = piece_at<float>(stg, pc[4]);
      }
      // a pending asynchronous ensemble event: its fold runs stand-alone, as ahead of fmskf_tick_many
      ens_flush(h);
      h->time_begin();
      launch_check(launch_kf6_trace(h->s, t, h->kf6, h->gate_on ? &h->gate : nullptr,
                                    h->cfg.trig == FMSKF_TRIG_LIBM, to, h->stream), "trace launch");
      h->time_end();
      if (host) pieces_out(h, pc, 5, "trace");
    });
  });
}

}  // extern "C"
