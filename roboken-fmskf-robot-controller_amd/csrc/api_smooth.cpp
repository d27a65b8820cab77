// api_smooth.cpp -- fixed-interval smoothing of a replayed window of KF6 ticks:
// fmskf_tick_many_smooth (its own argument checks, the workspace, staging of host outputs, the two
// launches of kernels_smooth.hip; the front end of the window calls is api_ctx.hpp's),
// fmskf_smooth_workspace_bytes and fmskf_smooth_reserve.
#include "api_ctx.hpp"

using namespace fmskf;
using namespace fmskf::capi;

namespace {

// the history of one tick in elements: x, then P, each tiled like the state (SmoothHist)
struct Slice {
  uint64_t sx, sp;
};
Slice slice_of(const fmskf_ctx *h) {
  const uint64_t W = tile_w<float>(), tiles = (h->s.n + W - 1) / W;
  return {tiles * 6 * W, tiles * 21 * W};
}
// tick t's slice starts t * (sx + sp) elements into the workspace: the x tiles, then the P tiles
SmoothHist hist_of(const fmskf_ctx *h) {
  const Slice s = slice_of(h);
  return {(float *)h->smooth_ws, (float *)h->smooth_ws + s.sx, s.sx + s.sp, s.sx + s.sp};
}
uint64_t workspace_bytes(const fmskf_ctx *h, uint32_t n_ticks) {
  const Slice s = slice_of(h);
  return bytes_mul((s.sx + s.sp) * sizeof(float), n_ticks, "smoothing window");
}

void free_workspace(fmskf_ctx *h) {
  if (!h->smooth_ws) return;
  hip_check(hipStreamSynchronize(h->stream), "hipStreamSynchronize");
  (void)hipFree(h->smooth_ws);
  h->smooth_ws = nullptr;
  h->smooth_ws_bytes = 0;
}
// grow-only; a failed allocation leaves no workspace and no stale capacity
void ensure_workspace(fmskf_ctx *h, uint64_t bytes) {
  if (bytes <= h->smooth_ws_bytes) return;
  free_workspace(h);
  const hipError_t e = hipMalloc(&h->smooth_ws, bytes);
  if (e != hipSuccess) {
    h->smooth_ws = nullptr;
    (void)hipGetLastError();  // the next launch check must not see this allocation's error
    fail(FMSKF_ENOMEM, std::string("smoothing workspace hipMalloc: ") + hipGetErrorString(e));
  }
  h->smooth_ws_bytes = bytes;
}

}  // namespace

SmoothHist fmskf::capi::smooth_hist(fmskf_ctx *h, uint32_t n_ticks) {
  ensure_workspace(h, workspace_bytes(h, n_ticks));
  return hist_of(h);
}

extern "C" {

int fmskf_smooth_workspace_bytes(fmskf_handle h, uint32_t n_ticks, uint64_t *bytes) {
  return guarded([&] {
    check_handle(h);
    check_window_model(h, "smoothing is");
    if (!bytes) fail(FMSKF_EINVAL, "null bytes");
    *bytes = workspace_bytes(h, n_ticks);
  });
}

int fmskf_smooth_reserve(fmskf_handle h, uint32_t n_ticks) {
  return guarded([&] {
    check_handle(h);
    check_window_model(h, "smoothing is");
    if (h->capturing) fail(FMSKF_EINVAL, "the smoothing workspace cannot change inside a graph capture");
    DeviceGuard g(h->cfg.device);
    if (n_ticks == 0) free_workspace(h);
    else ensure_workspace(h, workspace_bytes(h, n_ticks));
  });
}

int fmskf_tick_many_smooth(fmskf_handle h, const fmskf_tick_inputs *in, uint32_t n_ticks,
                           uint64_t tick_stride, const fmskf_smooth_out *out) {
  return guarded([&] {
    check_handle(h);
    check_window_model(h, "smoothing is");
    const uint64_t n = h->s.n;
    if (!out || !out->x) fail(FMSKF_EINVAL, "null smoothing output");
    if (out->reserved) fail(FMSKF_EINVAL, "fmskf_smooth_out.reserved must be 0");
    window_call(h, "fmskf_tick_many_smooth", "smoothing", out->mem, out->pitch, false, in, n_ticks, tick_stride,
                [&](const TickIn &t) {
      const bool host = out->mem == FMSKF_MEM_HOST;
      const uint64_t pitch = out->pitch ? out->pitch : n;
      const SmoothHist hist = smooth_hist(h, n_ticks);
      const uint64_t xrow = bytes_mul(6 * n * sizeof(float), n_ticks, "smoothing window"),
                     prow = bytes_mul(21 * n * sizeof(float), n_ticks, "smoothing window");
      SmoothOut so{out->x, out->P, pitch};
      // Dense [T][rows][N] on the device, copied out row by row at the caller's pitch: not a piece
      // table (window_pieces.hpp), whose mirror has the caller's pitch on both sides
      if (host) {
        if (out->P && xrow > (uint64_t)SIZE_MAX - prow) fail(FMSKF_ENOMEM, "smoothing window too large");
        char *stg = (char *)h->out_for(xrow + (out->P ? prow : 0));
        so = SmoothOut{(float *)stg, out->P ? (float *)(stg + xrow) : nullptr, n};
      }
      // a pending asynchronous ensemble event: its fold runs stand-alone, as ahead of fmskf_tick_many
      ens_flush(h);
      const bool libm = h->cfg.trig == FMSKF_TRIG_LIBM;
      timed_passes(h, [&] {
        launch_check(launch_kf6_smooth_fwd(h->s, t, h->kf6, libm, hist, h->stream), "smoothing forward launch");
      }, [&] {
        launch_check(launch_kf6_smooth_bwd(h->s, t, h->kf6, libm, hist, so, h->stream), "smoothing backward launch");
      });
      if (host) {
        const size_t row = (size_t)n * sizeof(float), dp = (size_t)pitch * sizeof(float);
        hip_check(hipMemcpy2DAsync(out->x, dp, so.x, row, row, (size_t)6 * n_ticks, hipMemcpyDeviceToHost, h->stream),
                  "smoothed x D2H");
        if (out->P)
          hip_check(hipMemcpy2DAsync(out->P, dp, so.P, row, row, (size_t)21 * n_ticks, hipMemcpyDeviceToHost, h->stream),
                    "smoothed P D2H");
        finish_out(h, out->mem);
      }
    });
  });
}

}  // extern "C"
