// kernels_loglik.hip -- the innovation (prediction-error) log-likelihood of a replayed window of
// KF6 ticks (fmskf_tick_many_loglik) for gfx950: one loop launch, one robot per lane, and a small
// second launch when the fleet total is asked for.
//
// The loop is k_kf6's (kernels_kf6.hip), as k_kf6_smooth_fwd's is: clamped index, the inputs of
// tick t+1 loaded into ping-pong registers while tick t computes (vmcnt retires in order, so
// nothing is loaded between them and their use), the sine table staged in LDS so the trig lookups
// wait on lgkmcnt only, the chunk-based input descriptors that are valid for any N.  Each measured
// tick feeds the lane's accumulators between the update's factor and apply phases
// (loglik_lane.hpp); the state it leaves is fmskf_tick_many's bit for bit.  The sums are stored
// once, after the last tick, with the state: 108 + 16 T bytes read and 108 + 20 written per robot
// and launch, + 112 with the innovation sums (MOM: a compile-time variant, so the likelihood-only
// launch carries neither their registers nor their operations), and as much read again with
// FMSKF_LL_ACCUMULATE.
//
// The fleet total is deterministic: every block reduces its lanes' fp64 values in a fixed tree
// and writes one partial per quantity (loglik_store); k_window_fold (window_lane.hpp), one block,
// adds the partials in block order.  No floating-point atomics.
#include "loglik_lane.hpp"

#pragma clang fp contract(off)

namespace fmskf {

// waves_per_eu as k_kf6 has it.  The compiler's report (tools/resource_usage.py; the whole table and
// k_kf6's own figures are in DESIGN.md section 3 and profiles/loglik.json), no scratch anywhere:
// likelihood-only 94-116 VGPRs, 4-5 waves per SIMD; innovation sums 125-126 VGPRs, 4 waves with
// the table trig, and 130-131, 3 waves with libm, whose variants would spill 12-16 bytes per lane
// at 4 waves and therefore get 3.  Without the attribute the unmasked table kernels take 127 and
// 186 VGPRs (4 and 2 waves).
template <class O, bool MOM>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(MOM && O::LIBM ? 3 : 4, 8))) void k_kf6_loglik(LoglikArgs aa) {
  const Kf6Args &a = aa.k;
  __shared__ float stab[O::LIBM ? 1 : 513];
  __shared__ double red[kBlock / 64][4];
  const uint64_t n = a.n;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < (uint32_t)n;
  const uint32_t ic = live ? i : (uint32_t)n - 1u;
  const uint32_t T = a.in.n_ticks;
  float x[6], P[21];
  LoglikAcc<MOM> acc;
  Kf6In ma, mb;
  kf6_load_state<O>(a.x, a.P, a.pitch, ic, x, P);
  const auto old = kf6_keep_old<kf6_mask<O>()>(P);
  ma = kf6_load_in<O>(a.in, n, 0, ic);
  stage_table<O::LIBM>(stab, a.in.sintab);
  for (uint32_t t = 0; t < T; t += 2) {
    if (t + 1 < T) mb = kf6_load_in<O>(a.in, n, t + 1, ic);
    loglik_tick1<O>(ma, stab, a.prm, x, P, acc);
    if (t + 1 >= T) break;
    if (t + 2 < T) ma = kf6_load_in<O>(a.in, n, t + 2, ic);
    loglik_tick1<O>(mb, stab, a.prm, x, P, acc);
  }
  if (live) kf6_store_state<O>(a.x, a.P, a.pitch, i, x, P, old);
  nan_guard(x, P, a.counters, live);
  loglik_store<MOM>(aa.o, n, ic, live, acc, red);
}

int launch_kf6_loglik(const DevState &s, const TickIn &in, const Kf6Params &p, bool libm, const LoglikOut &out,
                      double *total, hipStream_t st) {
  if (p.lo || in.ens_blocks || in.fold_blocks || in.n_ticks == 0 || out.pitch < s.n || (total && !out.partial))
    return (int)hipErrorInvalidValue;
  const LoglikArgs la{{s.n, s.pitch, (float *)s.x, (float *)s.P, in, s.counters, p}, out};
  const dim3 g = grid_for(s.n);
  with_bools([&](auto LIBM, auto VALID, auto REC, auto MOM) {
    k_kf6_loglik<Opt<LIBM(), true, true, false, VALID(), REC()>, MOM()><<<g, kBlock, 0, st>>>(la);
  }, libm, in.valid != nullptr, in.rec != nullptr, out.innov_sum != nullptr || out.innov_outer != nullptr);
  int e = (int)hipGetLastError();
  if (e || !total) return e;
  k_window_fold<4, kBlock><<<1, kBlock, 0, st>>>(out.partial, g.x, total, out.accumulate);
  return (int)hipGetLastError();
}

}  // namespace fmskf
