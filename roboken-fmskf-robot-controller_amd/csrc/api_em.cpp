// api_em.cpp -- the EM sufficient statistics for Q and R of a replayed window of KF6 ticks:
// fmskf_tick_many_em (argument checks, the smoother's workspace, the scratch of block partials,
// staging of host outputs, the smoother's forward launch and the launches of kernels_em.hip) and
// the host M-step fmskf_em_mstep.
#include <cmath>

#include "api_ctx.hpp"

using namespace fmskf;
using namespace fmskf::capi;

namespace {

constexpr size_t kTotal = FMSKF_EM_TOTAL_LEN;

// a * b bytes, or FMSKF_ENOMEM when no allocation could hold it
uint64_t bytes_mul(uint64_t a, uint64_t b) {
  if (b && a > (uint64_t)SIZE_MAX / b) fail(FMSKF_ENOMEM, "EM output staging too large");
  return a * b;
}

// the blocks' partial totals [34][grid]: allocated on the first call that asks for the total, freed
// with the handle (N is fixed, so it never grows)
double *ensure_partial(fmskf_ctx *h) {
  if (!h->em_partial) {
    const size_t blocks = (size_t)((h->s.n + kBlock - 1) / kBlock);
    const hipError_t e = hipMalloc((void **)&h->em_partial, kTotal * blocks * sizeof(double));
    if (e != hipSuccess) {
      h->em_partial = nullptr;
      (void)hipGetLastError();  // the next launch check must not see this allocation's error
      fail(FMSKF_ENOMEM, std::string("EM scratch hipMalloc: ") + hipGetErrorString(e));
    }
  }
  return h->em_partial;
}

// one output array of the call (api_loglik.cpp Piece): host arrays are mirrored on the device at
// the caller's pitch, and only the n elements of each row cross PCIe
struct Piece {
  void *user;
  size_t elem, rows, off;
};

}  // namespace

extern "C" {

int fmskf_tick_many_em(fmskf_handle h, const fmskf_tick_inputs *in, uint32_t n_ticks, uint64_t tick_stride,
                       const fmskf_em_out *out) {
  return guarded([&] {
    check_handle(h);
    check_smooth_model(h);
    const uint64_t n = h->s.n;
    if (!out) fail(FMSKF_EINVAL, "null EM output");
    if (!out->n_meas && !out->sq && !out->sr && !out->total) fail(FMSKF_EINVAL, "every EM output pointer is null");
    if (out->flags & ~(uint32_t)FMSKF_EM_ACCUMULATE) fail(FMSKF_EINVAL, "unknown FMSKF_EM_* flags");
    if (out->mem != FMSKF_MEM_HOST && out->mem != FMSKF_MEM_DEVICE) fail(FMSKF_EINVAL, "bad mem flag");
    if (out->pitch && out->pitch < n) fail(FMSKF_EINVAL, "EM output pitch < N");
    if (n_ticks == 0) fail(FMSKF_EINVAL, "n_ticks == 0");
    const bool host = out->mem == FMSKF_MEM_HOST;
    if (!host) {  // the kernels store them with 4- and 8-byte accesses
      const uintptr_t d = (uintptr_t)out->sq | (uintptr_t)out->sr | (uintptr_t)out->total;
      if ((d & 7u) || ((uintptr_t)out->n_meas & 3u)) fail(FMSKF_EINVAL, "misaligned EM device output");
    }
    if (h->capturing) fail(FMSKF_EINVAL, "fmskf_tick_many_em cannot be captured");
    DeviceGuard g(h->cfg.device);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (h->stream && hipStreamIsCapturing(h->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
      fail(FMSKF_EINVAL, "fmskf_tick_many_em cannot be captured");
    // the input forms and checks of fmskf_tick_many; host inputs are staged, nothing is launched
    TickIn t = resolve_inputs(h, in, true, true, n_ticks, tick_stride);
    // every allocation before the first launch: a failure leaves the state as it was
    const uint64_t pitch = out->pitch ? out->pitch : n;
    const bool accumulate = (out->flags & FMSKF_EM_ACCUMULATE) != 0;
    const SmoothHist hist = smooth_hist(h, n_ticks);
    EmOut eo{out->n_meas, out->sq, out->sr, pitch, out->total ? ensure_partial(h) : nullptr, accumulate ? 1u : 0u};
    double *total = out->total;
    Piece pc[4] = {{out->n_meas, 4, 1, 0}, {out->sq, 8, 21, 0}, {out->sr, 8, 10, 0}, {out->total, 8, 1, 0}};
    if (host) {
      uint64_t bytes = 0;
      for (int k = 0; k < 4; k++) {
        if (!pc[k].user) continue;
        pc[k].off = bytes;
        const uint64_t cols = k == 3 ? kTotal : pc[k].rows > 1 ? pitch : n;
        const uint64_t b = (bytes_mul(bytes_mul(cols, pc[k].rows), pc[k].elem) + 255) & ~(uint64_t)255;
        if (b > (uint64_t)SIZE_MAX - bytes) fail(FMSKF_ENOMEM, "EM output staging too large");
        bytes += b;
      }
      char *stg = (char *)h->out_for(bytes);
      auto at = [&](int k) { return pc[k].user ? stg + pc[k].off : nullptr; };
      eo.n_meas = (uint32_t *)at(0);
      eo.sq = (double *)at(1);
      eo.sr = (double *)at(2);
      total = (double *)at(3);
    }
    // the row of piece k: its bytes, and the bytes between rows (the same on both sides)
    auto row = [&](int k) { return (size_t)(k == 3 ? kTotal : n) * pc[k].elem; };
    auto step = [&](int k) { return (size_t)(pc[k].rows > 1 ? pitch : k == 3 ? kTotal : n) * pc[k].elem; };
    // a pending asynchronous ensemble event: its fold runs stand-alone, as ahead of fmskf_tick_many
    ens_flush(h);
    if (host && accumulate) {  // the caller's values, staged in
      char *stg = (char *)h->oscratch;
      for (int k = 0; k < 4; k++)
        if (pc[k].user)
          hip_check(hipMemcpy2DAsync(stg + pc[k].off, step(k), pc[k].user, step(k), row(k), pc[k].rows,
                                     hipMemcpyHostToDevice, h->stream), "EM outputs H2D");
    }
    const bool libm = h->cfg.trig == FMSKF_TRIG_LIBM;
    const int only = smooth_timed_pass();
    if (only != 2) h->time_begin();
    launch_check(launch_kf6_smooth_fwd(h->s, t, h->kf6, libm, hist, h->stream), "EM forward launch");
    if (only == 1) h->time_end();
    if (only == 2) h->time_begin();
    launch_check(launch_kf6_em_bwd(h->s, t, h->kf6, libm, hist, eo, total, h->stream), "EM backward launch");
    if (only != 1) h->time_end();
    if (host) {
      char *stg = (char *)h->oscratch;
      for (int k = 0; k < 4; k++)
        if (pc[k].user)
          hip_check(hipMemcpy2DAsync(pc[k].user, step(k), stg + pc[k].off, step(k), row(k), pc[k].rows,
                                     hipMemcpyDeviceToHost, h->stream), "EM outputs D2H");
      finish_out(h, out->mem);
    }
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
