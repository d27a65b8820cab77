// kernels_gate.hip -- the KF6 tick with the chi-square innovation gate (fmskf_set_gate) for
// gfx950.
//
// The gated tick is the plain one (kernels_kf6.hip: one robot per lane, x and packed P in VGPRs,
// the same lane functions, the same input forms) with the update split where the innovation is
// known: the factorisation S = L D L^T, U = L^-1 H P and w = L^-1 y are formed first
// (kf_update_factor), NIS = sum w[a] * (w[a] / D[a]) costs four more operations on values in
// registers, and only the apply phase (kf_update_apply: x += U^T vw, P -= U^T V) sits behind the
// per-lane decision.  Rejecting lanes skip it, applying lanes run exactly the ungated operations:
// nothing of the applied path depends on the decision, so an applied update is kf_update bit for
// bit and a rejected one is the valid == 0 skip.
//
// Gate state: one uint32 word per robot (status, run, rejects: fmskf_internal.hpp GateDev) read
// and written, one float NIS written: two plain [N] planes addressed per 256-robot chunk through
// scalar descriptors like the inputs, with the state's cache policy.  12 B per robot-tick on top
// of the plain tick's 232.  The tick loop keeps the word in a register across its ticks.
//
// The kernels take their own argument struct (GateArgs): the ungated kernels' TickIn / Kf6Params
// / KfArgs are embedded as they are, nothing is added to them.  Kernel forms: two robots per lane
// while state + inputs fit the Infinity Cache, one per lane past it, for a streamed
// (non-temporal) state and for fmskf_correct, the tick loop for fmskf_tick_many -- the plain
// launcher's regimes (kernels_kf6.hip launch_o).  Input descriptors are always the chunk-based
// form that is valid for any N (kf6_load_in without SMALL).  No fused ensemble record and no
// compensated positions: the callers take the stand-alone record / refuse the gate.
#include "kf6_lane.hpp"

#pragma clang fp contract(off)

namespace fmskf {

struct GateArgs {
  KfArgs<MdKF6, Kf6Params> k;
  GateDev g;
};

// the gate plane's 256-robot chunk of instance ic (clamped, so in bounds): wave-uniform, since a
// wave's lanes -- the clamped ones included -- lie in one chunk
__device__ __forceinline__ uint32_t gate_chunk(uint32_t ic) {
  return (uint32_t)__builtin_amdgcn_readfirstlane(ic) & ~(uint32_t)(kBlock - 1);
}

// One robot's gated tick.  word: the robot's gate word, updated; nis / seen: the NIS of this
// tick's measurement and that there was one (left alone otherwise)
template <class O>
__device__ __forceinline__ void kf6_tick1_gated(const Kf6In &m, const float *tab, const Kf6Params &prm,
                                                const GateDev &g, float (&x)[6], float (&P)[21],
                                                uint32_t &word, float &nis, bool &seen) {
  uint32_t status = FMSKF_GATE_NONE;
  uint32_t run = (word >> kGateRunShift) & kGateRunMax, rej = word >> kGateRejShift;
  if (!O::VALID || m.valid) {
    float y[4], U[4][6], dinv[4], w[4];
    kf6_innov<O::LIBM>(m, tab, x, y);
    kf_update_factor<MdKF6>(P, y, prm.r, U, dinv, w);
    float v = w[0] * (w[0] * dinv[0]);
#pragma unroll
    for (int a = 1; a < 4; a++) v = dfma(w[a], w[a] * dinv[a], v);
    const bool forced = g.max_run > 0 && run >= g.max_run;
    const bool apply = forced || v <= g.nis_max;
    if (apply) kf_update_apply<MdKF6>(x, P, U, dinv, w);
    status = forced ? FMSKF_GATE_FORCED : apply ? FMSKF_GATE_ACCEPTED : FMSKF_GATE_REJECTED;
    run = apply ? 0u : min(run + 1u, kGateRunMax);
    rej = apply ? rej : min(rej + 1u, kGateRejMax);
    nis = v;
    seen = true;
  }
  word = status | (run << kGateRunShift) | (rej << kGateRejShift);
  if (O::PRED) {
    using OP = Opt<O::LIBM, false, true, O::SMALL, false>;
    Kf6Lo<OP> l;
    kf6_tick1<OP>(m, tab, prm, x, P, l);
  }
}

// Single gated tick (or gated correct), R robots per lane as k_kf6p: robots i, i + G, the inputs
// of all R loaded up front.  Lanes past N load instance N-1 (clamped, in bounds) and compute on
// it; only their stores and NaN count are masked off.
template <int WPE, int R, class O>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(WPE, 8))) void k_kf6g(GateArgs ga) {
  const KfArgs<MdKF6, Kf6Params> &a = ga.k;
  const uint64_t n = a.n;
  const uint32_t nn = (uint32_t)n, last = nn - 1u;
  const uint32_t G = gridDim.x * kBlock;
  const uint32_t i0 = blockIdx.x * kBlock + threadIdx.x;
  float x[6], P[21];
  __shared__ float wtab[O::LIBM ? 1 : kBlock / 64][O::LIBM ? 1 : kWaveTab];
  float *stab = wtab[O::LIBM ? 0 : threadIdx.x >> 6];
  WaveTable<O::LIBM> tv(a.in.sintab);
  Kf6In m[R];
#pragma unroll
  for (int r = 0; r < R; r++) m[r] = kf6_load_in<O>(a.in, n, 0, min(i0 + r * G, last));
#pragma unroll
  for (int r = 0; r < R; r++) {
    const uint32_t i = i0 + r * G;
    const bool live = i < nn;
    const uint32_t ic = live ? i : last;
    const uint32_t hb = gate_chunk(ic), li = ic - hb;
    kf6_load_state<O>(a.x, a.P, a.pitch, ic, x, P);
    uint32_t word = ld_chunk<uint32_t, O::CP>(ga.g.word, hb, n, li);
    if (r == 0) tv.store(stab);
    float nis = 0.f;
    bool seen = false;
    kf6_tick1_gated<O>(m[r], stab, a.prm, ga.g, x, P, word, nis, seen);
    if (live) {
      kf6_store_state<O>(a.x, a.P, a.pitch, i, x, P);
      st_chunk<uint32_t, st_pol(O::CP)>(ga.g.word, hb, n, li, word);
      if (seen) st_chunk<float, st_pol(O::CP)>(ga.g.nis, hb, n, li, nis);
    }
    nan_guard(x, P, a.counters, live);
  }
}

// fmskf_tick_many: T gated ticks per launch, the state and the gate word in VGPRs throughout,
// the gate word loaded and stored once; the inputs of the next tick are loaded while the current
// one computes (ping-pong input registers, as k_kf6)
template <int WPE, class O>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(WPE, 8))) void k_kf6gm(GateArgs ga) {
  const KfArgs<MdKF6, Kf6Params> &a = ga.k;
  const uint64_t n = a.n;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < (uint32_t)n;
  const uint32_t ic = live ? i : (uint32_t)n - 1u;
  const uint32_t hb = gate_chunk(ic), li = ic - hb;
  const uint32_t T = a.in.n_ticks;
  float x[6], P[21];
  __shared__ float wtab[O::LIBM ? 1 : kBlock / 64][O::LIBM ? 1 : kWaveTab];
  float *stab = wtab[O::LIBM ? 0 : threadIdx.x >> 6];
  WaveTable<O::LIBM> tv(a.in.sintab);
  Kf6In ma, mb;
  kf6_load_state<O>(a.x, a.P, a.pitch, ic, x, P);
  uint32_t word = ld_chunk<uint32_t, O::CP>(ga.g.word, hb, n, li);
  ma = kf6_load_in<O>(a.in, n, 0, ic);
  tv.store(stab);
  float nis = 0.f;
  bool seen = false;
  for (uint32_t t = 0; t < T; t += 2) {
    if (t + 1 < T) mb = kf6_load_in<O>(a.in, n, t + 1, ic);
    kf6_tick1_gated<O>(ma, stab, a.prm, ga.g, x, P, word, nis, seen);
    if (t + 1 >= T) break;
    if (t + 2 < T) ma = kf6_load_in<O>(a.in, n, t + 2, ic);
    kf6_tick1_gated<O>(mb, stab, a.prm, ga.g, x, P, word, nis, seen);
  }
  if (live) {
    kf6_store_state<O>(a.x, a.P, a.pitch, i, x, P);
    st_chunk<uint32_t, st_pol(O::CP)>(ga.g.word, hb, n, li, word);
    if (seen) st_chunk<float, st_pol(O::CP)>(ga.g.nis, hb, n, li, nis);
  }
  nan_guard(x, P, a.counters, live);
}

__global__ __launch_bounds__(kBlock) void k_gate_unpack(const uint32_t *word, uint64_t n, uint8_t *status,
                                                        uint8_t *run, uint32_t *rejects) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint32_t w = word[i];
  if (status) status[i] = (uint8_t)(w & 3u);
  if (run) run[i] = (uint8_t)((w >> kGateRunShift) & kGateRunMax);
  if (rejects) rejects[i] = w >> kGateRejShift;
}

// FMSKF_KF6_VARIANT as the plain launcher reads it (kernels_kf6.hip): 12 forces two robots per
// lane, 15 one; the result does not depend on it
static int gate_variant() {
  static int v = [] {
    const char *e = getenv("FMSKF_KF6_VARIANT");
    const int x = e ? atoi(e) : 0;
    return x == 12 || x == 15 ? x : 0;
  }();
  return v;
}

template <bool LIBM, bool VALID, bool REC>
static void launch_gate_lvr(const GateArgs &ga, bool pred, hipStream_t st) {
  const uint64_t n = ga.k.n;
  // state + gate bytes per robot, and with one tick's 16-byte inputs
  constexpr uint64_t SB = 108 + 8, RB = SB + 16;
  if (ga.k.in.n_ticks > 1) {
    k_kf6gm<4, Opt<LIBM, true, true, false, VALID, REC>><<<grid_for(n), kBlock, 0, st>>>(ga);
    return;
  }
  if (!pred) {  // fmskf_correct
    k_kf6g<4, 1, Opt<LIBM, true, false, false, VALID, REC>><<<grid_for(n), kBlock, 0, st>>>(ga);
    return;
  }
  const int v = gate_variant();
  const bool nt = state_nt(n * SB);
  if (!nt && v != 15 && (v == 12 || n * RB <= (256ull << 20))) {
    // resident in the Infinity Cache: two robots per lane under the plain tick's occupancy caps
    const unsigned g = (unsigned)((n + 2 * kBlock - 1) / (2 * kBlock));
    const bool rec_half = REC && n * RB <= (128ull << 20);
    const unsigned lds = FMSKF_LDS_CAP("FMSKF_KF6P_LDS", true, rec_half ? 48u * 1024u : 32u * 1024u);
    k_kf6g<4, 2, Opt<LIBM, true, true, false, VALID, REC>><<<g, kBlock, lds, st>>>(ga);
  } else if (nt) {
    const unsigned lds = FMSKF_LDS_CAP("FMSKF_KF6_LDS", true, 48u * 1024u);
    k_kf6g<4, 1, Opt<LIBM, true, true, false, VALID, REC, true>><<<grid_for(n), kBlock, lds, st>>>(ga);
  } else {
    const unsigned lds = FMSKF_LDS_CAP("FMSKF_KF6_LDS", false, 48u * 1024u);
    k_kf6g<4, 1, Opt<LIBM, true, true, false, VALID, REC>><<<grid_for(n), kBlock, lds, st>>>(ga);
  }
}

template <bool LIBM>
static void launch_gate_l(const GateArgs &ga, bool pred, hipStream_t st) {
  const bool valid = ga.k.in.valid != nullptr;
  if (ga.k.in.rec) {
    if (valid) launch_gate_lvr<LIBM, true, true>(ga, pred, st);
    else launch_gate_lvr<LIBM, false, true>(ga, pred, st);
  } else {
    if (valid) launch_gate_lvr<LIBM, true, false>(ga, pred, st);
    else launch_gate_lvr<LIBM, false, false>(ga, pred, st);
  }
}

int launch_kf6_gate(const DevState &s, const TickIn &in, const Kf6Params &p, const GateDev &g, bool libm,
                    bool pred, hipStream_t st) {
  if (p.lo || in.ens_blocks || in.fold_blocks || !g.word || !g.nis) return (int)hipErrorInvalidValue;
  if (!pred && in.n_ticks != 1) return (int)hipErrorInvalidValue;
  const GateArgs ga{{s.n, s.pitch, (float *)s.x, (float *)s.P, in, s.counters, p}, g};
  if (libm) launch_gate_l<true>(ga, pred, st);
  else launch_gate_l<false>(ga, pred, st);
  return (int)hipGetLastError();
}

int launch_gate_unpack(const uint32_t *word, uint64_t n, uint8_t *status, uint8_t *run, uint32_t *rejects,
                       hipStream_t st) {
  k_gate_unpack<<<grid_for(n), kBlock, 0, st>>>(word, n, status, run, rejects);
  return (int)hipGetLastError();
}

}  // namespace fmskf
