// kernels_em.hip -- the EM sufficient statistics for Q and R of a replayed window of KF6 ticks
// (fmskf_tick_many_em) for gfx950: one robot per lane.  The forward pass is the smoother's
// (kernels_smooth.hip launch_kf6_smooth_fwd: fmskf_tick_many's bits, every prior into the history);
// here the backward launch and the fold of the fleet total.
//
// Backward: k_kf6_smooth_bwd's loop with P_s carried (SmoothCarry<true>) -- t = T-1 .. 0, every
// prior loaded once into ping-pong registers and used by two consecutive ticks, the history read
// non-temporally, the sine table in LDS -- and no [T]-sized store: each step back adds its
// transition term to 21 accumulators through SmoothCarry::back's tap, each measured tick its
// measurement term to 10 (em_lane.hpp; the accumulators are per-lane LDS columns).  124 B read per
// robot-tick and nothing written; at most 4 + 31 * 8 B written per robot and launch, and as much
// read again with FMSKF_EM_ACCUMULATE.
//
// The fleet total is deterministic: every block reduces its lanes' fp64 values in a fixed tree
// and writes one partial per quantity (em_store); k_window_fold (window_lane.hpp), one block, adds
// the partials in block order.  No floating-point atomics.
#include "em_lane.hpp"

#pragma clang fp contract(off)

namespace fmskf {

static_assert(kEmLds * kBlock * sizeof(double) + 513 * sizeof(float) + (kBlock / 64) * kEmTotal * sizeof(double) <= 65536,
              "accumulator columns, sine table and reduction buffer: 64 KiB of static LDS");

// the second half of tick t: x+[t] from the tick's prior (x, P: left as they are, the next tick
// down needs them) and inputs, x_s[t] = x+[t] + e, the measurement term
template <class O>
__device__ __forceinline__ void em_finish(const EmArgs &a, const float *stab, const Kf6In &m, const float (&x)[6],
                                          const float (&P)[21], const float (&e)[6], SmoothCarry<true> &c,
                                          EmAcc &acc) {
  float xf[6], Pf[21];  // Pf: dead behind the update, the compiler drops its arithmetic
#pragma unroll
  for (int k = 0; k < 6; k++) xf[k] = x[k];
#pragma unroll
  for (int k = 0; k < 21; k++) Pf[k] = P[k];
  const bool meas = smooth_filtered<O>(a.prm, stab, m, xf, Pf);
  c.finish(xf, e);
  if (meas) acc.template measured<O::LIBM>(m, stab, c);
}

// Two waves per SIMD, as k_kf6_smooth_bwd with P_s has: the compiler's report (tools/resource_usage.py;
// the table is in DESIGN.md section 3 and profiles/em.json) shows no scratch in any instantiation.
template <class O>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_kf6_em_bwd(EmArgs a) {
  __shared__ float stab[O::LIBM ? 1 : 513];
  __shared__ double cols[kEmLds * kBlock];
  __shared__ double red[kBlock / 64][kEmTotal];
  const uint64_t n = a.n;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < (uint32_t)n;
  const uint32_t ic = live ? i : (uint32_t)n - 1u;
  const uint32_t T = a.in.n_ticks;
  const float dt = a.prm.dt;
  float xa[6], Pa[21], xb[6], Pb[21], e[6];
  Kf6In ma, mb;
  SmoothCarry<true> c;
  EmAcc acc;
  EmTap tap{acc};
  hist_load(a.h, T - 1, ic, xa, Pa);
  ma = kf6_load_in<O>(a.in, n, T - 1, ic);
  acc.init(cols);
  stage_table<O::LIBM>(stab, a.in.sintab);
  if (T >= 2) {
    hist_load(a.h, T - 2, ic, xb, Pb);
    mb = kf6_load_in<O>(a.in, n, T - 2, ic);
  }
  {  // the window's last tick: its filtered state, its measurement term
    float xf[6], Pf[21];
#pragma unroll
    for (int k = 0; k < 6; k++) xf[k] = xa[k];
#pragma unroll
    for (int k = 0; k < 21; k++) Pf[k] = Pa[k];
    const bool meas = smooth_filtered<O>(a.prm, stab, ma, xf, Pf);
    c.start(xf, Pf);
    if (meas) acc.template measured<O::LIBM>(ma, stab, c);
  }
  // t: the carried tick, its prior in (xa, Pa); tick t-1's prior and inputs in (xb, Pb, mb), as in
  // k_kf6_smooth_bwd
  for (uint32_t t = T - 1; t > 0; t--) {
    c.back(xa, Pa, a.prm.q, dt, e, tap);
    if (t >= 2) {
      hist_load(a.h, t - 2, ic, xa, Pa);
      ma = kf6_load_in<O>(a.in, n, t - 2, ic);
    }
    em_finish<O>(a, stab, mb, xb, Pb, e, c, acc);
    if (--t == 0) break;
    c.back(xb, Pb, a.prm.q, dt, e, tap);
    if (t >= 2) {
      hist_load(a.h, t - 2, ic, xb, Pb);
      mb = kf6_load_in<O>(a.in, n, t - 2, ic);
    }
    em_finish<O>(a, stab, ma, xa, Pa, e, c, acc);
  }
  em_store(a.o, n, ic, live, T - 1, acc, red);
}

int launch_kf6_em_bwd(const DevState &s, const TickIn &in, const Kf6Params &p, bool libm, const SmoothHist &hist,
                      const EmOut &out, double *total, hipStream_t st) {
  if (p.lo || in.ens_blocks || in.fold_blocks || in.n_ticks == 0 || !hist.x || !hist.P || out.pitch < s.n ||
      (total && !out.partial))
    return (int)hipErrorInvalidValue;
  const EmArgs ea{s.n, in, p, hist, out};
  const dim3 g = grid_for(s.n);
  with_bools([&](auto LIBM, auto VALID, auto REC) {
    k_kf6_em_bwd<Opt<LIBM(), true, true, false, VALID(), REC()>><<<g, kBlock, 0, st>>>(ea);
  }, libm, in.valid != nullptr, in.rec != nullptr);
  int e = (int)hipGetLastError();
  if (e || !total) return e;
  k_window_fold<kEmTotal, 128><<<1, kBlock, 0, st>>>(out.partial, g.x, total, out.accumulate);
  return (int)hipGetLastError();
}

}  // namespace fmskf
