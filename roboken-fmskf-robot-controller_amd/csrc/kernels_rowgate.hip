// kernels_rowgate.hip -- the EKF9 tick with the per-row innovation gate (fmskf_set_row_gate) for
// gfx950.
//
// With a diagonal R the EKF9 update is six scalar updates in sequence (kf_update_seq: heading,
// gyro z, ax, ay, vbx, vby).  The row-gated tick is the plain one (kernels_kf.hip: x and packed P
// in VGPRs, the same lane functions of ekf9_lane.hpp, the same tiled state) with each scalar row
// behind its own decision (kf_update_seq_gated): d2 = y * (y / s) is one more product on values
// the row already holds, a rejecting lane branches around the row's x / y / P sub-loops, an
// applying lane runs exactly the ungated operations.  So an update with every row applied is
// kf_update_seq bit for bit, one with every row rejected is the valid == 0 skip, and any other
// pattern is the ungated update with R[a][a] = +inf on the rejected rows (up to the sign of a
// zero).
//
// Gate state: one uint64 word per robot (six 2-bit statuses, six 8-bit runs: kf_generic.hpp
// kRowGate*) in a plain [N] plane, read and written once per launch, and with FMSKF_ROW_GATE_D2
// six float planes [6][pitch] of the rows' d2, written for robots that had a measurement; all
// addressed per 256-robot chunk through scalar descriptors (ld_chunk / st_chunk) with the state's
// cache policy.  16 B per robot-tick on top of the plain tick's 456, 40 B with d2.
//
// The kernels take their own argument struct (RowGateArgs) embedding the plain kernels' KfArgs
// unchanged.  Kernel forms, after the plain launcher's regimes (kernels_kf.hip launch_ekf9_s):
// two robots per lane (k_ekf9p's shape) while the state fits the Infinity Cache, one per lane
// (k_ekf9t's shape) past it -- streamed non-temporal -- and for libm trig and fmskf_correct, the
// tick loop (k_ekf9's shape, the word in a register across the ticks) for fmskf_tick_many.  No
// fused ensemble record, no ISR form, no compensated positions: the callers take the stand-alone
// record / the three-kernel ISR / refuse the gate.
#include "ekf9_lane.hpp"

#pragma clang fp contract(off)

namespace fmskf {

struct RowGateArgs {
  KfArgs<MdEKF9, Ekf9Params> k;
  RowGateDev g;
};

// One robot's row-gated tick.  word: the robot's gate word, updated (a call without a
// measurement clears the statuses and keeps the runs); d2 / seen: the rows' d2 of this tick's
// measurement and that there was one (left alone otherwise)
template <bool LIBM, bool PRED>
__device__ __forceinline__ void ekf9_tick1_gated(const KfArgs<MdEKF9, Ekf9Params> &a, const RowGateDev &g,
                                                 const uint4 raw, bool have, const float *stab, float (&x)[9],
                                                 float (&P)[45], float &lo, uint64_t &word, float (&d2)[6],
                                                 bool &seen) {
  if (have) {
    float y[6];
    ekf9_innov(raw, x, lo, y);
    kf_update_seq_gated<MdEKF9, 2>(x, P, y, a.prm.r, g.d2_max, g.max_run, word, d2, &lo);
    th_norm(x[2], lo);
    seen = true;
  } else {
    word &= ~kRowGateStatusMask;
  }
  if (PRED) ekf9_tick1<LIBM, false, true, true>(a, raw, false, stab, x, P, lo);
}

// the gate state of one robot stored: its word, and the rows' d2 when they are kept and the robot
// had a measurement.  hb0: the robot's 256-robot chunk (wave-uniform), sl: its slot in it
template <int CP>
__device__ __forceinline__ void rowgate_store(const RowGateDev &g, uint64_t hb0, uint64_t n, uint32_t sl,
                                              uint64_t word, const float (&d2)[6], bool seen) {
  st_chunk<uint64_t, st_pol(CP)>(g.word, hb0, n, sl, word);
  if ((g.flags & FMSKF_ROW_GATE_D2) && seen) {
#pragma unroll
    for (int a = 0; a < 6; a++) st_chunk<float, st_pol(CP)>(g.d2 + a * g.d2_pitch, hb0, n, sl, d2[a]);
  }
}

// Single row-gated tick (PRED) or row-gated correct, one robot per lane as k_ekf9t: clamped index
// for lanes past N (only their stores and NaN count are masked), every load issued before the
// table store
template <bool LIBM, bool PRED, int CP>
__global__ __launch_bounds__(kBlock) void k_ekf9tg(RowGateArgs ga) {
  constexpr int N = 9, NP = 45;
  const KfArgs<MdEKF9, Ekf9Params> &a = ga.k;
  const uint32_t bid = blockIdx.x;
  __shared__ float wtab[LIBM ? 1 : kBlock / 64][LIBM ? 1 : kWaveTab];
  float *stab = wtab[LIBM ? 0 : threadIdx.x >> 6];
  const uint64_t n = a.n;
  const uint64_t i = (uint64_t)bid * kBlock + threadIdx.x;
  const bool live = i < n;
  const uint64_t ic = live ? i : n - 1;
  float x[N], P[NP];
  WaveTable<LIBM> tv(a.in.sintab);
  const uint32_t sl = tile_slot(n, bid);
  const TileRows<float, N, CP> tx(a.x, bid, sl, 0);
  const TileRows<float, NP, CP> tp(a.P, bid, sl, 0);
#pragma unroll
  for (int k = 0; k < N; k++) x[k] = tx.ld(k);
#pragma unroll
  for (int k = 0; k < NP; k++) P[k] = tp.ld(k);
  const bool have = a.in.valid == nullptr || a.in.valid[ic];
  const uint4 raw = ekf9_raw_at<false>(a.in.raw, ic);
  const uint64_t hb0 = (uint64_t)bid * kBlock;
  float lo = ld_chunk<float, CP>(a.prm.thlo, hb0, n, sl);
  uint64_t word = ld_chunk<uint64_t, CP>(ga.g.word, hb0, n, sl);
  tv.store(stab);
  float d2[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  bool seen = false;
  ekf9_tick1_gated<LIBM, PRED>(a, ga.g, raw, have, stab, x, P, lo, word, d2, seen);
  if (live) {
    st_chunk<float, st_pol(CP)>(a.prm.thlo, hb0, n, sl, lo);
    rowgate_store<CP>(ga.g, hb0, n, sl, word, d2, seen);
#pragma unroll
    for (int k = 0; k < N; k++) tx.st(k, x[k]);
#pragma unroll
    for (int k = 0; k < NP; k++) tp.st(k, P[k]);
  }
  nan_guard(x, P, a.counters, live);
}

// Two robots per lane (256-robot chunks b and b + G of the tiled state, G the grid) as k_ekf9p:
// robot B's state, raw record and gate word are loaded before robot A's update.  A block without
// a partner chunk computes on its own chunk again and stores nothing of it.
template <int CP>
__global__ __launch_bounds__(kBlock) void k_ekf9pg(RowGateArgs ga) {
  constexpr int N = 9, NP = 45;
  const KfArgs<MdEKF9, Ekf9Params> &a = ga.k;
  const uint32_t bid = blockIdx.x;
  __shared__ float wtab[kBlock / 64][kWaveTab];
  float *stab = wtab[threadIdx.x >> 6];
  const uint64_t n = a.n;
  const uint32_t ntiles = (uint32_t)((n + kBlock - 1) / kBlock);  // chunks of kBlock instances
  const uint32_t ta = bid, tb0 = bid + gridDim.x;
  const bool has_b = tb0 < ntiles;  // block-uniform
  const uint32_t tb = has_b ? tb0 : ta;
  const uint32_t t = threadIdx.x;
  auto slot = [&](uint32_t tile) -> uint32_t {
    const uint64_t b0 = (uint64_t)tile * kBlock;
    return b0 + t < n ? t : (uint32_t)(n - 1 - b0);
  };
  const uint64_t ha0 = (uint64_t)ta * kBlock, hb0 = (uint64_t)tb * kBlock;
  const uint64_t ia = ha0 + t, ib = hb0 + t;
  const bool live_a = ia < n, live_b = has_b && ib < n;
  const uint64_t iac = live_a ? ia : n - 1, ibc = ib < n ? ib : n - 1;
  WaveTable<false> tv(a.in.sintab);
  const TileRows<float, N, CP> txa(a.x, ta, slot(ta), 0), txb(a.x, tb, slot(tb), 0);
  const TileRows<float, NP, CP> tpa(a.P, ta, slot(ta), 0), tpb(a.P, tb, slot(tb), 0);
  float xa[N], Pa[NP], xb[N], Pb[NP];
#pragma unroll
  for (int k = 0; k < N; k++) xa[k] = txa.ld(k);
#pragma unroll
  for (int k = 0; k < NP; k++) Pa[k] = tpa.ld(k);
  const uint4 ra = ekf9_raw_at<true>(a.in.raw, iac);
  const uint4 rb = ekf9_raw_at<true>(a.in.raw, ibc);
  const bool hva = a.in.valid == nullptr || a.in.valid[iac];
  const bool hvb = a.in.valid == nullptr || a.in.valid[ibc];
#pragma unroll
  for (int k = 0; k < N; k++) xb[k] = txb.ld(k);
#pragma unroll
  for (int k = 0; k < NP; k++) Pb[k] = tpb.ld(k);
  float loa = ld_chunk<float, CP>(a.prm.thlo, ha0, n, slot(ta));
  float lob = ld_chunk<float, CP>(a.prm.thlo, hb0, n, slot(tb));
  uint64_t wa = ld_chunk<uint64_t, CP>(ga.g.word, ha0, n, slot(ta));
  uint64_t wb = ld_chunk<uint64_t, CP>(ga.g.word, hb0, n, slot(tb));
  tv.store(stab);
  {
    float d2[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool seen = false;
    ekf9_tick1_gated<false, true>(a, ga.g, ra, hva, stab, xa, Pa, loa, wa, d2, seen);
    if (live_a) {
      st_chunk<float, st_pol(CP)>(a.prm.thlo, ha0, n, slot(ta), loa);
      rowgate_store<CP>(ga.g, ha0, n, slot(ta), wa, d2, seen);
#pragma unroll
      for (int k = 0; k < N; k++) txa.st(k, xa[k]);
#pragma unroll
      for (int k = 0; k < NP; k++) tpa.st(k, Pa[k]);
    }
    nan_guard(xa, Pa, a.counters, live_a);
  }
  {
    float d2[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    bool seen = false;
    ekf9_tick1_gated<false, true>(a, ga.g, rb, hvb, stab, xb, Pb, lob, wb, d2, seen);
    if (live_b) {
      st_chunk<float, st_pol(CP)>(a.prm.thlo, hb0, n, slot(tb), lob);
      rowgate_store<CP>(ga.g, hb0, n, slot(tb), wb, d2, seen);
#pragma unroll
      for (int k = 0; k < N; k++) txb.st(k, xb[k]);
#pragma unroll
      for (int k = 0; k < NP; k++) tpb.st(k, Pb[k]);
    }
    nan_guard(xb, Pb, a.counters, live_b);
  }
}

// fmskf_tick_many: T row-gated ticks per launch as k_ekf9, the state and the gate word in VGPRs
// throughout, the word loaded and stored once; the next tick's raw record and validity byte are
// loaded while the current tick computes.  d2 leaves the last evaluated values.
template <bool LIBM>
__global__ __launch_bounds__(kBlock) void k_ekf9gm(RowGateArgs ga) {
  constexpr int N = 9, NP = 45;
  const KfArgs<MdEKF9, Ekf9Params> &a = ga.k;
  __shared__ float stab[LIBM ? 1 : 513];
  if (!LIBM) {
    for (int k = threadIdx.x; k < 513; k += kBlock) stab[k] = a.in.sintab[k];
    __syncthreads();
  }
  const uint64_t n = a.n;
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < n;
  const uint64_t ic = live ? i : n - 1;
  const uint32_t T = a.in.n_ticks;
  const uint64_t st = a.in.stride;
  auto raw_at = [&](uint32_t t) -> uint4 { return reinterpret_cast<const uint4 *>(a.in.raw)[(uint64_t)t * st + ic]; };
  auto have_at = [&](uint32_t t) -> bool { return a.in.valid == nullptr || a.in.valid[(uint64_t)t * st + ic]; };
  float x[N], P[NP];
  const uint32_t sl = tile_slot(n);
  const TileRows<float, N> tx(a.x, sl);
  const TileRows<float, NP> tp(a.P, sl);
#pragma unroll
  for (int k = 0; k < N; k++) x[k] = tx.ld(k);
#pragma unroll
  for (int k = 0; k < NP; k++) P[k] = tp.ld(k);
  const uint64_t hb0 = (uint64_t)blockIdx.x * kBlock;
  float lo = ld_chunk<float, 0>(a.prm.thlo, hb0, n, sl);
  uint64_t word = ld_chunk<uint64_t, 0>(ga.g.word, hb0, n, sl);
  float d2[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  bool seen = false;
  uint4 ra = raw_at(0), rb;
  bool ha = have_at(0), hb;
  for (uint32_t t = 0; t < T; t += 2) {
    if (t + 1 < T) {
      rb = raw_at(t + 1);
      hb = have_at(t + 1);
    }
    ekf9_tick1_gated<LIBM, true>(a, ga.g, ra, ha, stab, x, P, lo, word, d2, seen);
    if (t + 1 >= T) break;
    if (t + 2 < T) {
      ra = raw_at(t + 2);
      ha = have_at(t + 2);
    }
    ekf9_tick1_gated<LIBM, true>(a, ga.g, rb, hb, stab, x, P, lo, word, d2, seen);
  }
  if (live) {
    st_chunk<float, st_pol(0)>(a.prm.thlo, hb0, n, sl, lo);
    rowgate_store<0>(ga.g, hb0, n, sl, word, d2, seen);
#pragma unroll
    for (int k = 0; k < N; k++) tx.st(k, x[k]);
#pragma unroll
    for (int k = 0; k < NP; k++) tp.st(k, P[k]);
  }
  nan_guard(x, P, a.counters, live);
}

// fmskf_get_row_gate: the words into status [6][N] and run [6][N] planes
__global__ __launch_bounds__(kBlock) void k_rowgate_unpack(const uint64_t *word, uint64_t n, uint8_t *status,
                                                           uint8_t *run) {
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const uint64_t w = word[i];
#pragma unroll
  for (int a = 0; a < 6; a++) {
    if (status) status[a * n + i] = (uint8_t)((w >> (2 * a)) & 3u);
    if (run) run[a * n + i] = (uint8_t)((w >> (kRowGateRunShift + 8 * a)) & kRowGateRunMax);
  }
}

// FMSKF_EKF9_VARIANT as the plain launcher reads it (kernels_kf.hip): 2 forces two robots per
// lane, 4 one; the result does not depend on it
static int rowgate_variant() {
  static const int v = [] {
    const char *e = getenv("FMSKF_EKF9_VARIANT");
    const int x = e ? atoi(e) : 0;
    return x == 2 || x == 4 ? x : 0;
  }();
  return v;
}

template <bool LIBM>
static void launch_rowgate_l(const RowGateArgs &ga, bool pred, hipStream_t st) {
  const uint64_t n = ga.k.n;
  const dim3 g = grid_for(n);
  constexpr uint64_t SB = 220 + 8;  // state + gate word bytes per robot
  if (ga.k.in.n_ticks > 1) {
    k_ekf9gm<LIBM><<<g, kBlock, 0, st>>>(ga);
    return;
  }
  if (!pred) {  // fmskf_correct
    k_ekf9tg<LIBM, false, 0><<<g, kBlock, 0, st>>>(ga);
    return;
  }
  const bool nt = state_nt(n * SB);
  if constexpr (!LIBM) {
    const int var = rowgate_variant();
    const int v = var ? var : (n * SB <= (256ull << 20) ? 2 : 4);
    if (v == 2) {
      // the plain two-per-lane tick's occupancy cap (kernels_kf.hip: FMSKF_EKF9P_LDS)
      const uint32_t ntiles = (uint32_t)((n + kBlock - 1) / kBlock);
      const dim3 g2((ntiles + 1) / 2);
      const unsigned lds = FMSKF_LDS_CAP("FMSKF_EKF9P_LDS", true, 64u * 1024u);
      if (nt) k_ekf9pg<kStateNT><<<g2, kBlock, lds, st>>>(ga);
      else k_ekf9pg<0><<<g2, kBlock, lds, st>>>(ga);
      return;
    }
  }
  // past the Infinity Cache the plain one-per-lane tick's cap (FMSKF_EKF9_LDS)
  const unsigned lds = LIBM ? 0u : FMSKF_LDS_CAP("FMSKF_EKF9_LDS", nt, 64u * 1024u);
  if (nt) k_ekf9tg<LIBM, true, kStateNT><<<g, kBlock, lds, st>>>(ga);
  else k_ekf9tg<LIBM, true, 0><<<g, kBlock, lds, st>>>(ga);
}

int launch_ekf9_rowgate(const DevState &s, const TickIn &in, const Ekf9Params &p, const RowGateDev &g,
                        bool libm, bool pred, hipStream_t st) {
  if (!FMSKF_TILED || !s.tile || !s.thlo || s.xlo || in.ens_blocks || in.fold_blocks || !in.raw || !g.word ||
      !g.d2 || g.d2_pitch < s.n || !ekf9_r_diagonal(p.r))
    return (int)hipErrorInvalidValue;
  if (!pred && in.n_ticks != 1) return (int)hipErrorInvalidValue;
  RowGateArgs ga{{s.n, s.pitch, (float *)s.x, (float *)s.P, in, s.counters, p}, g};
  ga.k.prm.thlo = s.thlo;
  ga.k.prm.clo = nullptr;
  if (libm) launch_rowgate_l<true>(ga, pred, st);
  else launch_rowgate_l<false>(ga, pred, st);
  return (int)hipGetLastError();
}

int launch_rowgate_unpack(const uint64_t *word, uint64_t n, uint8_t *status, uint8_t *run, hipStream_t st) {
  k_rowgate_unpack<<<grid_for(n), kBlock, 0, st>>>(word, n, status, run);
  return (int)hipGetLastError();
}

}  // namespace fmskf
