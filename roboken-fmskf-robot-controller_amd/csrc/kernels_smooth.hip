// kernels_smooth.hip -- fixed-interval (Rauch-Tung-Striebel) smoothing of a replayed window of
// KF6 ticks (fmskf_tick_many_smooth) for gfx950: two launches, one robot per lane.
//
// Forward: k_kf6 (kernels_kf6.hip) built from the same lane functions in the same order -- so the
// state it leaves is fmskf_tick_many's bit for bit -- plus, before each tick, a store of the
// lane's 27 prior values into the history (fmskf_internal.hpp SmoothHist): 16 B in + 108 B of
// history per robot-tick, the state read and written once per launch.
//
// Backward: one launch looping t = T-1 .. 0 with the smoothed estimate of tick t+1 carried in
// registers (smooth_lane.hpp SmoothCarry; the recursion and why it has this form are there).
// Every prior is loaded once and used by two consecutive ticks: as "the prior of t+1" for the
// gain of tick t, then, with the tick's inputs, to rebuild the forward pass's own x+[t] (kf6_innov,
// kf_update: the forward pass's bits).  124 B read + 24 B written per robot-tick, + 84 B with P_s.
// vmcnt retires in order, so the 27 + 4 dwords of tick t-1 are issued as soon as the registers of
// the prior of t+1 are free, a whole tick of arithmetic ahead of their first use (ping-pong
// registers, as k_kf6 does for its inputs); the sine table is staged in LDS so the trig lookups
// wait on lgkmcnt only.
//
// The input descriptors are the chunk-based form that is valid for any N (kf6_load_in without
// SMALL), as the gated kernels take them.
#include "smooth_lane.hpp"

#pragma clang fp contract(off)

namespace fmskf {

template <class O>
__global__ __launch_bounds__(kBlock) void k_kf6_smooth_fwd(SmoothFwdArgs aa) {
  const Kf6Args &a = aa.k;
  __shared__ float stab[O::LIBM ? 1 : 513];
  const uint64_t n = a.n;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < (uint32_t)n;
  const uint32_t ic = live ? i : (uint32_t)n - 1u;
  const uint32_t T = a.in.n_ticks;
  float x[6], P[21];
  Kf6Lo<O> lo;
  Kf6Gate<O, false> gt;
  Kf6In ma, mb;
  kf6_load_state<O>(a.x, a.P, a.pitch, ic, x, P);
  const auto old = kf6_keep_old<kf6_mask<O>()>(P);
  ma = kf6_load_in<O>(a.in, n, 0, ic);
  stage_table<O::LIBM>(stab, a.in.sintab);
  for (uint32_t t = 0; t < T; t += 2) {
    if (t + 1 < T) mb = kf6_load_in<O>(a.in, n, t + 1, ic);
    hist_store(aa.h, t, ic, live, x, P);
    kf6_tick1<O>(ma, stab, a.prm, x, P, lo, gt);
    if (t + 1 >= T) break;
    if (t + 2 < T) ma = kf6_load_in<O>(a.in, n, t + 2, ic);
    hist_store(aa.h, t + 1, ic, live, x, P);
    kf6_tick1<O>(mb, stab, a.prm, x, P, lo, gt);
  }
  if (live) kf6_store_state<O>(a.x, a.P, a.pitch, i, x, P, old);
  nan_guard(x, P, a.counters, live);
}

struct SmoothLane {
  uint32_t hb, li;
  bool live;
};

template <bool WP>
__device__ __forceinline__ void smooth_out(const SmoothBwdArgs &a, uint32_t t, const SmoothLane &ln,
                                           const SmoothCarry<WP> &c) {
  smooth_store<6>(a.o.x, t, a.o.pitch, a.n, ln.hb, ln.li, ln.live, c.x);
  if constexpr (WP) smooth_store<21>(a.o.P, t, a.o.pitch, a.n, ln.hb, ln.li, ln.live, c.P);
}

// the second half of tick t: x+[t] from the tick's prior (x, P: left as they are, the next tick
// down needs them) and inputs, x_s[t] = x+[t] + e, the stores
template <class O, bool WP>
__device__ __forceinline__ void smooth_finish(const SmoothBwdArgs &a, const float *stab, uint32_t t,
                                              const SmoothLane &ln, const Kf6In &m, const float (&x)[6],
                                              const float (&P)[21], const float (&e)[6], SmoothCarry<WP> &c) {
  float xf[6], Pf[21];  // Pf: dead behind the update, the compiler drops its arithmetic
#pragma unroll
  for (int k = 0; k < 6; k++) xf[k] = x[k];
#pragma unroll
  for (int k = 0; k < 21; k++) Pf[k] = P[k];
  smooth_filtered<O>(a.prm, stab, m, xf, Pf);
  c.finish(xf, e);
  smooth_out<WP>(a, t, ln, c);
}

template <class O, bool WP>
__global__ __launch_bounds__(kBlock) void k_kf6_smooth_bwd(SmoothBwdArgs a) {
  __shared__ float stab[O::LIBM ? 1 : 513];
  const uint64_t n = a.n;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < (uint32_t)n;
  const uint32_t ic = live ? i : (uint32_t)n - 1u;
  const SmoothLane ln{blockIdx.x * kBlock, ic - blockIdx.x * kBlock, live};
  const uint32_t T = a.in.n_ticks;
  const float dt = a.prm.dt;
  float xa[6], Pa[21], xb[6], Pb[21], e[6];
  Kf6In ma, mb;
  SmoothCarry<WP> c;
  hist_load(a.h, T - 1, ic, xa, Pa);
  ma = kf6_load_in<O>(a.in, n, T - 1, ic);
  stage_table<O::LIBM>(stab, a.in.sintab);
  if (T >= 2) {
    hist_load(a.h, T - 2, ic, xb, Pb);
    mb = kf6_load_in<O>(a.in, n, T - 2, ic);
  }
  {  // the window's last tick: its filtered state
    float xf[6], Pf[21];
#pragma unroll
    for (int k = 0; k < 6; k++) xf[k] = xa[k];
#pragma unroll
    for (int k = 0; k < 21; k++) Pf[k] = Pa[k];
    smooth_filtered<O>(a.prm, stab, ma, xf, Pf);
    c.start(xf, Pf);
    smooth_out<WP>(a, T - 1, ln, c);
  }
  // t: the carried tick, its prior in (xa, Pa); tick t-1's prior and inputs in (xb, Pb, mb).
  // Unrolled by two over the ping-pong registers: the prior of t-2 is issued into the registers of
  // the prior of t as soon as the gain of tick t-1 is formed
  for (uint32_t t = T - 1; t > 0; t--) {
    c.back(xa, Pa, a.prm.q, dt, e);
    if (t >= 2) {
      hist_load(a.h, t - 2, ic, xa, Pa);
      ma = kf6_load_in<O>(a.in, n, t - 2, ic);
    }
    smooth_finish<O, WP>(a, stab, t - 1, ln, mb, xb, Pb, e, c);
    if (--t == 0) break;
    c.back(xb, Pb, a.prm.q, dt, e);
    if (t >= 2) {
      hist_load(a.h, t - 2, ic, xb, Pb);
      mb = kf6_load_in<O>(a.in, n, t - 2, ic);
    }
    smooth_finish<O, WP>(a, stab, t - 1, ln, ma, xa, Pa, e, c);
  }
}

static bool smooth_args_ok(const TickIn &in, const Kf6Params &p, const SmoothHist &hist) {
  return !p.lo && !in.ens_blocks && !in.fold_blocks && in.n_ticks != 0 && hist.x && hist.P;
}

int launch_kf6_smooth_fwd(const DevState &s, const TickIn &in, const Kf6Params &p, bool libm, const SmoothHist &hist,
                          hipStream_t st) {
  if (!smooth_args_ok(in, p, hist)) return (int)hipErrorInvalidValue;
  const SmoothFwdArgs fa{{s.n, s.pitch, (float *)s.x, (float *)s.P, in, s.counters, p}, hist};
  with_bools([&](auto LIBM, auto VALID, auto REC) {
    k_kf6_smooth_fwd<Opt<LIBM(), true, true, false, VALID(), REC()>><<<grid_for(s.n), kBlock, 0, st>>>(fa);
  }, libm, in.valid != nullptr, in.rec != nullptr);
  return (int)hipGetLastError();
}

int launch_kf6_smooth_bwd(const DevState &s, const TickIn &in, const Kf6Params &p, bool libm, const SmoothHist &hist,
                          const SmoothOut &out, hipStream_t st) {
  if (!smooth_args_ok(in, p, hist) || !out.x || out.pitch < s.n) return (int)hipErrorInvalidValue;
  const SmoothBwdArgs ba{s.n, in, p, hist, out};
  with_bools([&](auto LIBM, auto VALID, auto REC, auto WP) {
    k_kf6_smooth_bwd<Opt<LIBM(), true, true, false, VALID(), REC()>, WP()><<<grid_for(s.n), kBlock, 0, st>>>(ba);
  }, libm, in.valid != nullptr, in.rec != nullptr, out.P != nullptr);
  return (int)hipGetLastError();
}

}  // namespace fmskf
