// api_loglik.cpp -- the innovation log-likelihood of a replayed window of KF6 ticks:
// fmskf_tick_many_loglik (argument checks, the scratch of block partials, staging of host
// outputs, the launches of kernels_loglik.hip).
#include "api_ctx.hpp"

using namespace fmskf;
using namespace fmskf::capi;

namespace {

// plain ungated KF6, the smoother's exclusions: a gate's rejected ticks would have to leave the
// sums, and the compensated positions have their own update
void check_loglik_model(const fmskf_ctx *h) {
  if (h->cfg.model != FMSKF_MODEL_KF6) fail(FMSKF_ENOTSUP, "the innovation log-likelihood is for KF6");
  if (h->cfg.flags & FMSKF_CFG_COMP_POS)
    fail(FMSKF_ENOTSUP, "the innovation log-likelihood is for KF6 without FMSKF_CFG_COMP_POS");
  if (h->gate_on) fail(FMSKF_ENOTSUP, "the innovation log-likelihood is for a KF6 handle without a gate (fmskf_set_gate)");
}

// a * b bytes, or FMSKF_ENOMEM when no allocation could hold it
uint64_t bytes_mul(uint64_t a, uint64_t b) {
  if (b && a > (uint64_t)SIZE_MAX / b) fail(FMSKF_ENOMEM, "log-likelihood output staging too large");
  return a * b;
}

// the blocks' partial totals [4][grid]: allocated on the first call that asks for the total, freed
// with the handle (N is fixed, so it never grows)
double *ensure_partial(fmskf_ctx *h) {
  if (!h->loglik_partial) {
    const size_t blocks = (size_t)((h->s.n + kBlock - 1) / kBlock);
    const hipError_t e = hipMalloc((void **)&h->loglik_partial, 4 * blocks * sizeof(double));
    if (e != hipSuccess) {
      h->loglik_partial = nullptr;
      (void)hipGetLastError();  // the next launch check must not see this allocation's error
      fail(FMSKF_ENOMEM, std::string("log-likelihood scratch hipMalloc: ") + hipGetErrorString(e));
    }
  }
  return h->loglik_partial;
}

// One output array of the call: `rows` rows of n elements of `elem` bytes, `pitch` elements
// apart.  Host arrays are mirrored on the device at the caller's pitch, so the kernel takes one
// pitch whatever the memory; only the n elements of each row cross PCIe, either way.
struct Piece {
  void *user;
  size_t elem, rows, off;
};

}  // namespace

extern "C" {

int fmskf_tick_many_loglik(fmskf_handle h, const fmskf_tick_inputs *in, uint32_t n_ticks, uint64_t tick_stride,
                           const fmskf_loglik_out *out) {
  return guarded([&] {
    check_handle(h);
    check_loglik_model(h);
    const uint64_t n = h->s.n;
    if (!out) fail(FMSKF_EINVAL, "null log-likelihood output");
    if (!out->n_meas && !out->nis_sum && !out->logdet_sum && !out->innov_sum && !out->innov_outer && !out->total)
      fail(FMSKF_EINVAL, "every log-likelihood output pointer is null");
    if (out->flags & ~(uint32_t)FMSKF_LL_ACCUMULATE) fail(FMSKF_EINVAL, "unknown FMSKF_LL_* flags");
    if (out->mem != FMSKF_MEM_HOST && out->mem != FMSKF_MEM_DEVICE) fail(FMSKF_EINVAL, "bad mem flag");
    if (out->pitch && out->pitch < n) fail(FMSKF_EINVAL, "log-likelihood output pitch < N");
    if (n_ticks == 0) fail(FMSKF_EINVAL, "n_ticks == 0");
    const bool host = out->mem == FMSKF_MEM_HOST;
    if (!host) {  // the kernels store them with 4- and 8-byte accesses
      const uintptr_t d = (uintptr_t)out->nis_sum | (uintptr_t)out->logdet_sum | (uintptr_t)out->innov_sum |
                          (uintptr_t)out->innov_outer | (uintptr_t)out->total;
      if ((d & 7u) || ((uintptr_t)out->n_meas & 3u)) fail(FMSKF_EINVAL, "misaligned log-likelihood device output");
    }
    if (h->capturing) fail(FMSKF_EINVAL, "fmskf_tick_many_loglik cannot be captured");
    DeviceGuard g(h->cfg.device);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (h->stream && hipStreamIsCapturing(h->stream, &cs) == hipSuccess && cs != hipStreamCaptureStatusNone)
      fail(FMSKF_EINVAL, "fmskf_tick_many_loglik cannot be captured");
    // the input forms and checks of fmskf_tick_many; host inputs are staged, nothing is launched
    TickIn t = resolve_inputs(h, in, true, true, n_ticks, tick_stride);
    // every allocation before the first launch: a failure leaves the state as it was
    const uint64_t pitch = out->pitch ? out->pitch : n;
    const bool accumulate = (out->flags & FMSKF_LL_ACCUMULATE) != 0;
    LoglikOut lo{out->n_meas, out->nis_sum, out->logdet_sum, out->innov_sum, out->innov_outer, pitch,
                 out->total ? ensure_partial(h) : nullptr, accumulate ? 1u : 0u};
    double *total = out->total;
    Piece pc[6] = {{out->n_meas, 4, 1, 0},      {out->nis_sum, 8, 1, 0},      {out->logdet_sum, 8, 1, 0},
                   {out->innov_sum, 8, 4, 0},   {out->innov_outer, 8, 10, 0}, {out->total, 8, 1, 0}};
    if (host) {
      uint64_t bytes = 0;
      for (int k = 0; k < 6; k++) {
        if (!pc[k].user) continue;
        pc[k].off = bytes;
        const uint64_t cols = k == 5 ? 4 : pc[k].rows > 1 ? pitch : n;
        const uint64_t b = (bytes_mul(bytes_mul(cols, pc[k].rows), pc[k].elem) + 255) & ~(uint64_t)255;
        if (b > (uint64_t)SIZE_MAX - bytes) fail(FMSKF_ENOMEM, "log-likelihood output staging too large");
        bytes += b;
      }
      char *stg = (char *)h->out_for(bytes);
      auto at = [&](int k) { return pc[k].user ? stg + pc[k].off : nullptr; };
      lo.n_meas = (uint32_t *)at(0);
      lo.nis_sum = (double *)at(1);
      lo.logdet_sum = (double *)at(2);
      lo.innov_sum = (double *)at(3);
      lo.innov_outer = (double *)at(4);
      total = (double *)at(5);
    }
    // the row of piece k: its bytes, and the bytes between rows (the same on both sides)
    auto row = [&](int k) { return (size_t)(k == 5 ? 4 : n) * pc[k].elem; };
    auto step = [&](int k) { return (size_t)(pc[k].rows > 1 ? pitch : k == 5 ? 4 : n) * pc[k].elem; };
    // a pending asynchronous ensemble event: its fold runs stand-alone, as ahead of fmskf_tick_many
    ens_flush(h);
    if (host && accumulate) {  // the caller's values, staged in
      char *stg = (char *)h->oscratch;
      for (int k = 0; k < 6; k++)
        if (pc[k].user)
          hip_check(hipMemcpy2DAsync(stg + pc[k].off, step(k), pc[k].user, step(k), row(k), pc[k].rows,
                                     hipMemcpyHostToDevice, h->stream), "log-likelihood outputs H2D");
    }
    h->time_begin();
    launch_check(launch_kf6_loglik(h->s, t, h->kf6, h->cfg.trig == FMSKF_TRIG_LIBM, lo, total, h->stream),
                 "log-likelihood launch");
    h->time_end();
    if (host) {
      char *stg = (char *)h->oscratch;
      for (int k = 0; k < 6; k++)
        if (pc[k].user)
          hip_check(hipMemcpy2DAsync(pc[k].user, step(k), stg + pc[k].off, step(k), row(k), pc[k].rows,
                                     hipMemcpyDeviceToHost, h->stream), "log-likelihood outputs D2H");
      finish_out(h, out->mem);
    }
  });
}

}  // extern "C"
