// trace_lane.hpp -- lane functions of the per-tick trace of a replayed window of KF6 ticks
// (kernels_trace.hip, fmskf_tick_many_trace): the tick that also returns what it decided, and the
// stores of one tick's values.
//
// Per tick and robot the trace holds three values: the status (FMSKF_GATE_*), the NIS the tick
// evaluated, and the `applied` byte, 1 where the measurement update ran.  On a gated handle they
// are read off the lane's gate state behind the unchanged kf6_tick1 (kf6_lane.hpp): the low two
// bits of the gate word are the tick's status, and gate.nis is the tick's NIS whenever that status
// is not NONE.  On an ungated handle the tick is loglik_tick1's sequence -- kf6_innov,
// kf_update_factor, kf_nis, kf_update_apply, which is kf_update bit for bit -- so the NIS is the
// value a monitor-only gate reports, every measured tick is ACCEPTED and applied.  A tick without
// a measurement is NONE, not applied, and its NIS the quiet NaN 0x7FC00000.
//
// The `applied` plane has the format of fmskf_tick_inputs.valid: a rejected update is the
// valid == 0 skip bit for bit and an applied or forced one the ungated update, so an ungated
// handle fed that plane repeats a gated handle's trajectory exactly.
#pragma once
#include "smooth_lane.hpp"

#pragma clang fp contract(off)

namespace fmskf {

struct TraceArgs {
  Kf6Args k;
  GateDev g;  // all zero for an ungated handle
  TraceOut o;
};

constexpr uint32_t kTraceNoNis = 0x7FC00000u;

// One ungated tick: the update split where the NIS is known, then kf6_tick1's plain predict.
// Returns the tick's status; nis: its NIS when measured
template <class O>
__device__ __forceinline__ uint32_t trace_tick1(const Kf6In &m, const float *tab, const Kf6Params &prm,
                                                float (&x)[6], float (&P)[21], float &nis) {
  uint32_t status = FMSKF_GATE_NONE;
  if (!O::VALID || m.valid) {
    float y[4], U[4][6], dinv[4], w[4];
    kf6_innov<O::LIBM>(m, tab, x, y);
    kf_update_factor<MdKF6>(P, y, prm.r, U, dinv, w);
    nis = kf_nis(w, dinv);
    kf_update_apply<MdKF6>(x, P, U, dinv, w);
    status = FMSKF_GATE_ACCEPTED;
  }
  const float dt = prm.dt;
  x[0] = dfma(dt, x[3], x[0]);
  x[1] = dfma(dt, x[4], x[1]);
  x[2] = wrap_pi(dfma(dt, x[5], x[2]));
  kf_predict_cov<MdKF6>(P, [&](int, int) { return dt; }, prm.q);
  return status;
}

// The lane's place in the output planes: hb the first robot of its 256-robot chunk (wave-uniform),
// li its slot there, live: the lane stores
struct TraceLane {
  uint32_t hb, li;
  bool live;
};

// One tick's values at row t of the three per-tick planes: a descriptor per plane over the rest of
// the row from the block's chunk on, so neither the tick nor the pitch enters a 32-bit offset.  The
// planes are optional: their pointers are kernel arguments, the branches uniform.  The NIS plane is
// written once in whole lines and not read again (non-temporal, as the smoother's rows); a wave
// covers 64 bytes of a byte plane, half a line, which the L2 merges with its neighbour wave's
// (default policy).  Byte stores, so a byte plane may have any alignment and any pitch.
__device__ __forceinline__ void trace_put(const TraceOut &o, uint32_t t, uint64_t n, const TraceLane &ln,
                                          uint32_t status, float nis) {
  const uint64_t row = (uint64_t)t * o.pitch + ln.hb, left = n - ln.hb;
  if (ln.live) {
    if (o.nis)
      st_f32<st_pol(kStateNT)>(rsrc(o.nis + row, left * 4), ln.li * 4u, 0,
                               status != FMSKF_GATE_NONE ? nis : __builtin_bit_cast(float, kTraceNoNis));
    if (o.status) __builtin_amdgcn_raw_buffer_store_b8((uint8_t)status, rsrc(o.status + row, left), ln.li, 0, 0);
    if (o.applied) {
      const bool ap = status == FMSKF_GATE_ACCEPTED || status == FMSKF_GATE_FORCED;
      __builtin_amdgcn_raw_buffer_store_b8((uint8_t)(ap ? 1 : 0), rsrc(o.applied + row, left), ln.li, 0, 0);
    }
  }
}

// State row j (the state after tick (j + 1) * every - 1), from the registers: the smoother's
// dense row store
__device__ __forceinline__ void trace_rows(const TraceOut &o, uint32_t j, uint64_t n, const TraceLane &ln,
                                           const float (&x)[6], const float (&P)[21]) {
  if (o.x) smooth_store<6>(o.x, j, o.pitch, n, ln.hb, ln.li, ln.live, x);
  if (o.P) smooth_store<21>(o.P, j, o.pitch, n, ln.hb, ln.li, ln.live, P);
}

}  // namespace fmskf
