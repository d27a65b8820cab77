// kernels_trace.hip -- the per-tick trace of a replayed window of KF6 ticks
// (fmskf_tick_many_trace) for gfx950: one loop launch, one robot per lane.
//
// The loop is k_kf6's (kernels_kf6.hip), as k_kf6_smooth_fwd's and k_kf6_loglik's are: clamped
// index, the inputs of tick t+1 loaded into ping-pong registers while tick t computes (vmcnt
// retires in order, so nothing is loaded between them and their use), the sine table staged in
// LDS, the chunk-based input descriptors that are valid for any N.  Behind every tick the lane
// stores the tick's NIS, status and applied byte (trace_lane.hpp), and behind every `every`-th
// tick its state from the registers; the state it leaves is fmskf_tick_many's bit for bit, on a
// gated handle (GATED: GateArgs' lane struct and the unchanged kf6_tick1) the gate state too.
// Per robot-tick 16 B read and 4 + 1 + 1 written, + 24 / every for x and 84 / every for P; the
// state (and the gate word) read and written once per launch.
//
// ROWS: the launch stores state rows.  A compile-time variant, so the launch without them carries
// neither the countdown nor the row stores in its loop.
#include "trace_lane.hpp"

#pragma clang fp contract(off)

namespace fmskf {

// one tick and its per-tick stores; rows: the countdown to the next state row and the rows stored
template <class O, bool GATED, bool ROWS, class G>
__device__ __forceinline__ void trace_step(const TraceArgs &aa, const float *stab, uint32_t t, const TraceLane &ln,
                                           const Kf6In &m, float (&x)[6], float (&P)[21], G &gt, uint32_t &left,
                                           uint32_t &j) {
  const Kf6Args &a = aa.k;
  uint32_t status;
  float nis = 0.f;
  if constexpr (GATED) {
    Kf6Lo<O> lo;
    kf6_tick1<O>(m, stab, a.prm, x, P, lo, gt);
    status = gt.word & 3u;
    nis = gt.nis;
  } else {
    status = trace_tick1<O>(m, stab, a.prm, x, P, nis);
  }
  trace_put(aa.o, t, a.n, ln, status, nis);
  if constexpr (ROWS) {
    if (--left == 0) {
      trace_rows(aa.o, j, a.n, ln, x, P);
      left = aa.o.every;
      j++;
    }
  }
}

// waves_per_eu as k_kf6 has it
template <class O, bool GATED, bool ROWS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 8))) void k_kf6_trace(TraceArgs aa) {
  const Kf6Args &a = aa.k;
  __shared__ float stab[O::LIBM ? 1 : 513];
  const uint64_t n = a.n;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < (uint32_t)n;
  const uint32_t ic = live ? i : (uint32_t)n - 1u;
  const TraceLane ln{blockIdx.x * kBlock, ic - blockIdx.x * kBlock, live};
  const uint32_t T = a.in.n_ticks;
  float x[6], P[21];
  Kf6Gate<O, GATED> gt;
  Kf6In ma, mb;
  uint32_t left = aa.o.every, j = 0;
  kf6_load_state<O>(a.x, a.P, a.pitch, ic, x, P);
  const auto old = kf6_keep_old<kf6_mask<O>()>(P);
  if constexpr (GATED) gt.load(aa.g, ic, n);
  ma = kf6_load_in<O>(a.in, n, 0, ic);
  stage_table<O::LIBM>(stab, a.in.sintab);
  for (uint32_t t = 0; t < T; t += 2) {
    if (t + 1 < T) mb = kf6_load_in<O>(a.in, n, t + 1, ic);
    trace_step<O, GATED, ROWS>(aa, stab, t, ln, ma, x, P, gt, left, j);
    if (t + 1 >= T) break;
    if (t + 2 < T) ma = kf6_load_in<O>(a.in, n, t + 2, ic);
    trace_step<O, GATED, ROWS>(aa, stab, t + 1, ln, mb, x, P, gt, left, j);
  }
  if (live) {
    kf6_store_state<O>(a.x, a.P, a.pitch, i, x, P, old);
    if constexpr (GATED) gt.store(aa.g, i, n);
  }
  nan_guard(x, P, a.counters, live);
}

int launch_kf6_trace(const DevState &s, const TickIn &in, const Kf6Params &p, const GateDev *gate, bool libm,
                     const TraceOut &out, hipStream_t st) {
  const bool rows = out.x != nullptr || out.P != nullptr;
  if (p.lo || in.ens_blocks || in.fold_blocks || in.n_ticks == 0 || out.pitch < s.n ||
      (gate && (!gate->word || !gate->nis)) || (rows && (out.every == 0 || out.every > in.n_ticks)) ||
      (!rows && !out.nis && !out.status && !out.applied))
    return (int)hipErrorInvalidValue;
  const TraceArgs ta{{s.n, s.pitch, (float *)s.x, (float *)s.P, in, s.counters, p}, gate ? *gate : GateDev{}, out};
  with_bools([&](auto LIBM, auto VALID, auto REC, auto GATED, auto ROWS) {
    k_kf6_trace<Opt<LIBM(), true, true, false, VALID(), REC()>, GATED(), ROWS()><<<grid_for(s.n), kBlock, 0, st>>>(ta);
  }, libm, in.valid != nullptr, in.rec != nullptr, gate != nullptr, rows);
  return (int)hipGetLastError();
}

}  // namespace fmskf
