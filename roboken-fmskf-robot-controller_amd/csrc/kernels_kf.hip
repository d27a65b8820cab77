// kernels_kf.hip -- 9-state EKF (fp32) and 12-state KF (fp64) tick kernels for gfx950.
//
// One filter instance per lane; the per-instance state (x and the packed symmetric P)
// lives in VGPRs for the whole launch, so a tick reads and writes each state byte
// exactly once (HBM-bound by design, no MFMA: matrices are <= 12x12 per instance).
// State planes are SoA: lane i of a wave touches consecutive addresses of every plane.
// F / H / Q / R are shared: H and the sparsity of F are compile-time model traits
// (kf_generic.hpp), Q / R / dt ride in the kernarg segment (scalar loads, SGPRs).
// The 6-state headline kernel lives in kernels_kf6.hip.
// The EKF9 per-row innovation gate (fmskf_set_row_gate) is an instantiation of the EKF9 tick
// kernels on RowGateArgs (ekf9_lane.hpp): one more lane struct loaded with the state and stored
// with it, the gated sequential update inside ekf9_tick1, the plain handle's launch regimes.
#include "can_lane.hpp"
#include "ctrl_lane.hpp"
#include "ekf9_lane.hpp"
#include "ens_device.hpp"

#pragma clang fp contract(off)

namespace fmskf {

// the COMP low-part rows of one 256-robot chunk (tiled like x, kKf6LoRows rows)
template <bool COMP, int CP>
struct Ekf9Lo {
  float v[COMP ? kKf6LoRows : 1];
  __device__ __forceinline__ void load(const float *clo, uint32_t chunk, uint32_t slot) {
    if constexpr (COMP) {
      const TileRows<float, kKf6LoRows, CP> t(const_cast<float *>(clo), chunk, slot, 0);
#pragma unroll
      for (int k = 0; k < (int)kKf6LoRows; k++) v[k] = t.ld(k);
    }
  }
  __device__ __forceinline__ void store(float *clo, uint32_t chunk, uint32_t slot) const {
    if constexpr (COMP) {
      const TileRows<float, kKf6LoRows, CP> t(clo, chunk, slot, 0);
#pragma unroll
      for (int k = 0; k < (int)kKf6LoRows; k++) t.st(k, v[k]);
    }
  }
};

// tick_many: T ticks per launch, state in VGPRs; the next tick's raw record (16 B) and validity
// byte are loaded while the current tick computes (ping-pong registers, loop unrolled by two).
// A: Ekf9Args, or RowGateArgs for a row-gated handle (every tick kernel here): the lane's gate
// state is loaded with the other loads and stored with the state, the gate word held across the
// ticks.
template <bool LIBM, bool UPD, bool PRED, bool SEQ, bool COMP = false, class A = Ekf9Args>
__global__ __launch_bounds__(kBlock) void k_ekf9(A aa) {
  constexpr int N = 9, NP = 45;
  const Ekf9Args &a = kf_args(aa);
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
  auto raw_at = [&](uint32_t t) -> uint4 {
    return UPD ? reinterpret_cast<const uint4 *>(a.in.raw)[(uint64_t)t * st + ic] : make_uint4(0, 0, 0, 0);
  };
  auto have_at = [&](uint32_t t) -> bool {
    return a.in.valid == nullptr || a.in.valid[(uint64_t)t * st + ic];
  };
  float x[N], P[NP];
  const TileRows<float, N> tx(a.x, tile_slot(n));
  const TileRows<float, NP> tp(a.P, tile_slot(n));
#pragma unroll
  for (int k = 0; k < N; k++) x[k] = tx.ld(k);
#pragma unroll
  for (int k = 0; k < NP; k++) P[k] = tp.ld(k);
  float lo = a.prm.thlo[ic];
  Ekf9Lo<COMP, 0> cl;
  cl.load(a.prm.clo, blockIdx.x, tile_slot(n));
  Ekf9GateOf<A, 0> gt;
  gt.load(gate_dev(aa), (uint64_t)blockIdx.x * kBlock, n, tile_slot(n));
  uint4 ra = raw_at(0), rb;
  bool ha = have_at(0), hb;
  for (uint32_t t = 0; t < T; t += 2) {
    if (t + 1 < T) {
      rb = raw_at(t + 1);
      hb = have_at(t + 1);
    }
    ekf9_tick1<LIBM, UPD, PRED, SEQ, COMP>(aa, ra, ha, stab, x, P, lo, cl.v, gt);
    if (t + 1 >= T) break;
    if (t + 2 < T) {
      ra = raw_at(t + 2);
      ha = have_at(t + 2);
    }
    ekf9_tick1<LIBM, UPD, PRED, SEQ, COMP>(aa, rb, hb, stab, x, P, lo, cl.v, gt);
  }
  if (live) {
    a.prm.thlo[i] = lo;
    cl.store(a.prm.clo, blockIdx.x, tile_slot(n));
    gt.store(gate_dev(aa), (uint64_t)blockIdx.x * kBlock, n, tile_slot(n));
#pragma unroll
    for (int k = 0; k < N; k++) tx.st(k, x[k]);
#pragma unroll
    for (int k = 0; k < NP; k++) tp.st(k, P[k]);
  }
  nan_guard(x, P, a.counters, live);
}

// Single tick, straight line (as k_kf6t): no tick loop, clamped index for lanes past N (only
// their stores and NaN count are masked), every load issued before the table barrier.
// ENS: the record epilogue of fmskf_tick_ensemble (ens_device.hpp)
template <bool LIBM, bool UPD, bool PRED, bool SEQ, int CP = 0, bool ENS = false, bool COMP = false,
          class A = Ekf9Args>
__global__ __launch_bounds__(kBlock) void k_ekf9t(A aa) {
  constexpr int N = 9, NP = 45;
  static_assert(!ENS || std::is_same<A, Ekf9Args>::value, "no fused ensemble record with the row gate");
  const Ekf9Args &a = kf_args(aa);
  uint32_t bid = blockIdx.x;  // the tick block (the carried fold blocks come first)
  if constexpr (ENS) {
    if (ens_fold_front<9>(a.in, bid)) return;
  }
  __shared__ float wtab[LIBM ? 1 : kBlock / 64][LIBM ? 1 : kWaveTab];
  float *stab = wtab[LIBM ? 0 : threadIdx.x >> 6];
  const uint64_t n = a.n;
  const uint64_t i = (uint64_t)bid * kBlock + threadIdx.x;
  const bool live = i < n;
  const uint64_t ic = live ? i : n - 1;
  float x[N], P[NP];
  WaveTable<LIBM> tv(a.in.sintab);  // wave-private table copy, loads issued first
  const uint32_t sl = tile_slot(n, bid);
  const TileRows<float, N, CP> tx(a.x, bid, sl, 0);
  const TileRows<float, NP, CP> tp(a.P, bid, sl, 0);
#pragma unroll
  for (int k = 0; k < N; k++) x[k] = tx.ld(k);
#pragma unroll
  for (int k = 0; k < NP; k++) P[k] = tp.ld(k);
  const bool have = a.in.valid == nullptr || a.in.valid[ic];
  const uint4 raw = UPD ? ekf9_raw_at<false>(a.in.raw, ic) : make_uint4(0, 0, 0, 0);
  const uint64_t hb0 = (uint64_t)bid * kBlock;
  float lo = ld_chunk<float, CP>(a.prm.thlo, hb0, n, sl);
  Ekf9Lo<COMP, CP> cl;
  cl.load(a.prm.clo, bid, sl);
  Ekf9GateOf<A, CP> gt;
  gt.load(gate_dev(aa), hb0, n, sl);
  tv.store(stab);
  ekf9_tick1<LIBM, UPD, PRED, SEQ, COMP>(aa, raw, have, stab, x, P, lo, cl.v, gt);
  if (live) {
    st_chunk<float, st_pol(CP)>(a.prm.thlo, hb0, n, sl, lo);
    cl.store(a.prm.clo, bid, sl);
    gt.store(gate_dev(aa), hb0, n, sl);
#pragma unroll
    for (int k = 0; k < N; k++) tx.st(k, x[k]);
#pragma unroll
    for (int k = 0; k < NP; k++) tp.st(k, P[k]);
  }
  nan_guard(x, P, a.counters, live);
  if constexpr (ENS) {
    float xs[1][N];
#pragma unroll
    for (int k = 0; k < N; k++) xs[0][k] = x[k];
    const bool lv[1] = {live};
    ens_epilogue<9, 1>(a.in, xs, lv, bid);
  }
}

// The firmware ISR for the 9-state EKF in one pass (round 5; as k_isr_kf6 for KF6): the EKF9
// tick of k_ekf9t (cached tiled state), then the control half of VEHICLE_CTRL::update on the
// control step's rpm (the caller's plane or the ingested motor state, as fmskf_control reads
// it), then the 0x200 frame; every load of both steps issued before either computes.  One robot
// per lane, the clamped-index form.  Bit-identical to fmskf_tick + fmskf_control +
// fmskf_can_tx.  CPC: the control planes' cache policy.  CAN (fmskf_isr_tick_can): the tick's
// four C610 frames per robot first (can_lane.hpp), their rpm handed to the wheel loops in
// registers instead of read back from the motor state (the EKF9 measurement keeps the raw record).
// CNT: the motor state streamed non-temporal, so that it does not evict the cache-resident EKF9
// state (can_nt; 2^20 robots: 194 -> 155.4-156.2 us per tick against 195.8 for the two calls,
// kbench, two passes)
template <bool LIBM, bool SEQ, int CPC, bool COMP, bool CAN = false, bool CNT = false>
__global__ __launch_bounds__(kBlock) void k_isr_ekf9(KfArgs<MdEKF9, Ekf9Params> a, CtrlDev c, CtrlPrm p,
                                                    uint8_t *frames, const int16_t *rpm, CanArgs can) {
  constexpr int N = 9, NP = 45;
  const uint32_t bid = blockIdx.x;
  __shared__ float wtab[LIBM ? 1 : kBlock / 64][LIBM ? 1 : kWaveTab];
  float *stab = wtab[LIBM ? 0 : threadIdx.x >> 6];
  const uint64_t n = a.n;
  const uint64_t i = (uint64_t)bid * kBlock + threadIdx.x;
  const bool live = i < n;
  const uint64_t ic = live ? i : n - 1;
  Can4Lane<CNT> cl4;
  if constexpr (CAN) cl4.load(can, (uint64_t)bid * kBlock, (uint32_t)(ic - (uint64_t)bid * kBlock));
  float x[N], P[NP];
  WaveTable<LIBM> tv(a.in.sintab);
  const uint32_t sl = tile_slot(n, bid);
  const TileRows<float, N, 0> tx(a.x, bid, sl, 0);
  const TileRows<float, NP, 0> tp(a.P, bid, sl, 0);
#pragma unroll
  for (int k = 0; k < N; k++) x[k] = tx.ld(k);
#pragma unroll
  for (int k = 0; k < NP; k++) P[k] = tp.ld(k);
  const bool have = a.in.valid == nullptr || a.in.valid[ic];
  const uint4 raw = ekf9_raw_at<false>(a.in.raw, ic);
  const uint64_t hb0 = (uint64_t)bid * kBlock;
  float lo = ld_chunk<float, 0>(a.prm.thlo, hb0, n, sl);
  Ekf9Lo<COMP, 0> cl;
  cl.load(a.prm.clo, bid, sl);
  uint2 rw;
  if constexpr (!CAN) rw = reinterpret_cast<const uint2 *>(rpm)[ic];
  CtrlLane<CPC> L;
  L.load(c, (uint32_t)ic);
  tv.store(stab);
  if constexpr (CAN) rw = cl4.step(can, live);
  Ekf9Gate<false, 0> gt;  // no gated form: the row-gated handle takes the three-kernel ISR
  ekf9_tick1<LIBM, true, true, SEQ, COMP>(a, raw, have, stab, x, P, lo, cl.v, gt);
  if (live) {
    st_chunk<float, st_pol(0)>(a.prm.thlo, hb0, n, sl, lo);
    cl.store(a.prm.clo, bid, sl);
#pragma unroll
    for (int k = 0; k < N; k++) tx.st(k, x[k]);
#pragma unroll
    for (int k = 0; k < NP; k++) tp.st(k, P[k]);
  }
  nan_guard(x, P, a.counters, live);
  if (live) {
    const uint2 cw = L.step(c, p, (uint32_t)i, rw);
    if (frames) reinterpret_cast<uint2 *>(frames)[i] = tx_frame(cw);
  }
  if constexpr (CAN) cl4.finish(can, live);
}

// Two robots per lane (256-robot chunks b and b + G of the tiled state, G the tick blocks):
// robot B's 54 state loads and its raw record are issued before robot A's update, so they
// stream in while A computes (see launch_ekf9).
// A block without a partner chunk computes on its own chunk again and stores nothing of it.
template <bool LIBM, bool SEQ, int CP, bool ENS = false, bool COMP = false, class A = Ekf9Args>
__global__ __launch_bounds__(kBlock) void k_ekf9p(A aa) {
  constexpr int N = 9, NP = 45;
  static_assert(!ENS || std::is_same<A, Ekf9Args>::value, "no fused ensemble record with the row gate");
  const Ekf9Args &a = kf_args(aa);
  uint32_t bid = blockIdx.x;  // the tick block (the carried fold blocks come first)
  if constexpr (ENS) {
    if (ens_fold_front<9>(a.in, bid)) return;
  }
  __shared__ float wtab[LIBM ? 1 : kBlock / 64][LIBM ? 1 : kWaveTab];
  float *stab = wtab[LIBM ? 0 : threadIdx.x >> 6];
  const uint64_t n = a.n;
  const uint32_t ntiles = (uint32_t)((n + kBlock - 1) / kBlock);  // chunks of kBlock instances
  const uint32_t ta = bid, tb0 = bid + (ENS ? a.in.ens_grid : gridDim.x);
  const bool has_b = tb0 < ntiles;  // block-uniform
  const uint32_t tb = has_b ? tb0 : ta;
  const uint32_t t = threadIdx.x;
  auto slot = [&](uint32_t tile) -> uint32_t {
    const uint64_t b0 = (uint64_t)tile * kBlock;
    return b0 + t < n ? t : (uint32_t)(n - 1 - b0);
  };
  const uint64_t ia = (uint64_t)ta * kBlock + t, ib = (uint64_t)tb * kBlock + t;
  const bool live_a = ia < n, live_b = has_b && ib < n;
  const uint64_t iac = live_a ? ia : n - 1, ibc = ib < n ? ib : n - 1;
  WaveTable<LIBM> tv(a.in.sintab);
  const TileRows<float, N, CP> txa(a.x, ta, slot(ta), 0), txb(a.x, tb, slot(tb), 0);
  const TileRows<float, NP, CP> tpa(a.P, ta, slot(ta), 0), tpb(a.P, tb, slot(tb), 0);
  float xa[N], Pa[NP], xb[N], Pb[NP];
#pragma unroll
  for (int k = 0; k < N; k++) xa[k] = txa.ld(k);
#pragma unroll
  for (int k = 0; k < NP; k++) Pa[k] = tpa.ld(k);
  const uint4 ra = ekf9_raw_at<true>(a.in.raw, iac);
  const uint4 rb = ekf9_raw_at<true>(a.in.raw, ibc);
  const bool ha = a.in.valid == nullptr || a.in.valid[iac];
  const bool hb = a.in.valid == nullptr || a.in.valid[ibc];
#pragma unroll
  for (int k = 0; k < N; k++) xb[k] = txb.ld(k);
#pragma unroll
  for (int k = 0; k < NP; k++) Pb[k] = tpb.ld(k);
  float loa = ld_chunk<float, CP>(a.prm.thlo, (uint64_t)ta * kBlock, n, slot(ta));
  float lob = ld_chunk<float, CP>(a.prm.thlo, (uint64_t)tb * kBlock, n, slot(tb));
  Ekf9Lo<COMP, CP> cla, clb;
  cla.load(a.prm.clo, ta, slot(ta));
  clb.load(a.prm.clo, tb, slot(tb));
  Ekf9GateOf<A, CP> gta, gtb;
  gta.load(gate_dev(aa), (uint64_t)ta * kBlock, n, slot(ta));
  gtb.load(gate_dev(aa), (uint64_t)tb * kBlock, n, slot(tb));
  tv.store(stab);
  ekf9_tick1<LIBM, true, true, SEQ, COMP>(aa, ra, ha, stab, xa, Pa, loa, cla.v, gta);
  if (live_a) {
    st_chunk<float, st_pol(CP)>(a.prm.thlo, (uint64_t)ta * kBlock, n, slot(ta), loa);
    cla.store(a.prm.clo, ta, slot(ta));
    gta.store(gate_dev(aa), (uint64_t)ta * kBlock, n, slot(ta));
#pragma unroll
    for (int k = 0; k < N; k++) txa.st(k, xa[k]);
#pragma unroll
    for (int k = 0; k < NP; k++) tpa.st(k, Pa[k]);
  }
  nan_guard(xa, Pa, a.counters, live_a);
  float xs[ENS ? 2 : 1][N];
  if constexpr (ENS) {
#pragma unroll
    for (int k = 0; k < N; k++) xs[0][k] = xa[k];
  }
  ekf9_tick1<LIBM, true, true, SEQ, COMP>(aa, rb, hb, stab, xb, Pb, lob, clb.v, gtb);
  if (live_b) {
    st_chunk<float, st_pol(CP)>(a.prm.thlo, (uint64_t)tb * kBlock, n, slot(tb), lob);
    clb.store(a.prm.clo, tb, slot(tb));
    gtb.store(gate_dev(aa), (uint64_t)tb * kBlock, n, slot(tb));
#pragma unroll
    for (int k = 0; k < N; k++) txb.st(k, xb[k]);
#pragma unroll
    for (int k = 0; k < NP; k++) tpb.st(k, Pb[k]);
  }
  nan_guard(xb, Pb, a.counters, live_b);
  if constexpr (ENS) {
#pragma unroll
    for (int k = 0; k < N; k++) xs[1][k] = xb[k];
    const bool lv[2] = {live_a, live_b};
    ens_epilogue<9, 2>(a.in, xs, lv, bid);
  }
}

// SEQ: R has no base/tip cross terms -> group-sequential update (base group, then tip group
// with the innovation of the updated state); otherwise the joint 8-measurement update.
template <bool SEQ, bool UPD, bool PRED>
__global__ __launch_bounds__(kBlock) void k_kf12d(KfArgs<MdKF12D, Kf12dParams> a) {
  constexpr int N = 12, NP = 78, M = 8;
  const uint64_t n = a.n;
  const uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  double x[N], P[NP];
  constexpr uint32_t tl = tile_w<double>();
#pragma unroll
  for (int k = 0; k < N; k++) x[k] = a.x[st_at(tl, 0, N, k, i)];
#pragma unroll
  for (int k = 0; k < NP; k++) P[k] = a.P[st_at(tl, 0, NP, k, i)];
  const double dt = a.prm.dt;
  const auto fdt = [&](int, int) { return dt; };
  for (uint32_t t = 0; t < a.in.n_ticks; t++) {
    const uint64_t base = (uint64_t)t * a.in.stride * M;
    if (UPD) {
      if (a.in.valid == nullptr || a.in.valid[(uint64_t)t * a.in.stride + i]) {
        if (SEQ) {
          double y[4];
#pragma unroll
          for (int q = 0; q < 4; q++) y[q] = a.in.z[base + q * a.in.stride + i] - x[MdKF12D_G1::h1(q)];
          y[0] = wrap_innov(y[0]);
          kf_update<MdKF12D_G1>(x, P, y, a.prm.r);
#pragma unroll
          for (int q = 0; q < 4; q++)
            y[q] = a.in.z[base + (4 + q) * a.in.stride + i] - x[MdKF12D_G2::h1(q)];
          kf_update<MdKF12D_G2>(x, P, y, a.prm.r2);
        } else {
          double y[M];
#pragma unroll
          for (int q = 0; q < M; q++) y[q] = a.in.z[base + q * a.in.stride + i] - x[MdKF12D::h1(q)];
          y[0] = wrap_innov(y[0]);
          kf_update<MdKF12D>(x, P, y, a.prm.r);
        }
      }
    }
    if (PRED) {
#pragma unroll
      for (int q = 0; q < 6; q++) {
        const int p = q < 3 ? q : q + 3;
        x[p] = dfma(dt, x[p + 3], x[p]);
      }
      x[2] = wrap_pi(x[2]);
      kf_predict_cov<MdKF12D, decltype(fdt), double, 12, 78, true>(P, fdt, a.prm.q);
    }
  }
#pragma unroll
  for (int k = 0; k < N; k++) a.x[st_at(tl, 0, N, k, i)] = x[k];
#pragma unroll
  for (int k = 0; k < NP; k++) a.P[st_at(tl, 0, NP, k, i)] = P[k];
  nan_guard(x, P, a.counters);
}

// ---------------------------------------------------------------------------
// KF12D, R positive definite: decorrelated scalar-sequential update (oracle
// orc_kf12d_decor_update) and the F P F^T + Q predict done per 2x2 (pos, vel) pair block.
// Only one 12-entry HP row is live at a time (the joint / group LDL^T updates hold 8x12 or
// 4x12 update matrices), so x, P and the temporaries fit 256 VGPRs: two waves per SIMD to
// overlap the fp64 arithmetic (~4 cycles per wave64 FMA) with the 1504-byte stream.
// ---------------------------------------------------------------------------
__device__ __forceinline__ constexpr int kf12_pos(int k) { return k < 3 ? k : k + 3; }

// Cinv and Q are 114 wave-uniform doubles (a device buffer, prm.coef).  Loaded all at once
// they exceed the scalar register file and spill through v_writelane / v_readlane; a pointer
// the compiler cannot see through keeps each group's scalar loads at the point of use.
typedef const __attribute__((address_space(4))) double *kparam_ptr;
__device__ __forceinline__ kparam_ptr opaque_param(const double *p) {
  uint64_t v = (uint64_t)p;
  asm volatile("" : "+s"(v));
  return (kparam_ptr)v;
}

// Exact-zero coefficients are skipped (the canonical order of the oracle's
// orc_kf12d_decor_update: a zero C^-1 entry contributes nothing, every sum starts from +0, and
// fma(c, p, +0) = c p up to the sign of a zero).  C^-1 of the default R (diagonal but for the
// two wheel velocities) is mostly exact zeros: 11 of the 20 off-diagonal entries the update
// reads, each a 12-wide dfma row of HP plus the innovation term.  SP (the host checked that
// every C^-1 entry off the diagonal and (3,2), and every Q entry outside the (pos, vel) pair
// blocks, is zero): those terms are dropped at compile time; the entries that may be nonzero
// are added through a select (the same bits as skipping a zero), as every entry is when !SP.
// Measured: runtime branches on the scalar coefficient instead of selects took the kernel to
// 256 VGPRs (1 wave per SIMD) and were not kept.
__device__ __forceinline__ constexpr bool kf12_cinv_sp(int a, int b) { return a == b || (a == 3 && b == 2); }
__device__ __forceinline__ double fma_nz(double c, double p, double acc) {
  const double v = dfma(c, p, acc);
  return c != 0.0 ? v : acc;
}

template <bool BLK, bool SP>
__device__ __forceinline__ void kf12d_decor_update(double (&x)[12], double (&P)[78], double (&y)[8],
                                                   const double *ci) {
#pragma unroll
  for (int a = 0; a < 8; a++) {
    const int b0 = (BLK && a >= 4) ? 4 : 0;
    const kparam_ptr c = opaque_param(ci + a * (a + 1) / 2);
    // the diagonal of C^-1 is 1 / C[a][a] > 0 (R positive definite): a plain fma; the other
    // entries through fma_nz (or, under SP, dropped where the host found them zero)
    auto term = [&](int b, double p, double acc) -> double {
      return b == a ? dfma(c[b], p, acc) : fma_nz(c[b], p, acc);
    };
    // constant trip counts (b over 0..7, filtered): every index stays compile-time after
    // unrolling (a b0..a loop left P indexed at run time, in scratch)
    auto used = [&](int b) { return b >= b0 && b <= a && (!SP || kf12_cinv_sp(a, b)); };
    double hp[12];
#pragma unroll
    for (int j = 0; j < 12; j++) {
      double s = 0.0;
#pragma unroll
      for (int b = 0; b < 8; b++)
        if (used(b)) s = term(b, P[pk(MdKF12D::h1(b), j)], s);
      hp[j] = s;
    }
    double s = 0.0, nu = 0.0;
#pragma unroll
    for (int b = 0; b < 8; b++)
      if (used(b)) s = term(b, hp[MdKF12D::h1(b)], s);
    s = s + 1.0;
#pragma unroll
    for (int b = 0; b < 8; b++)
      if (used(b)) nu = term(b, y[b], nu);
    const double si = 1.0 / s;
    const double g = nu * si;
#pragma unroll
    for (int j = 0; j < 12; j++) x[j] = dfma(hp[j], g, x[j]);
#pragma unroll
    for (int b = 0; b < 8; b++) y[b] = dfma(-hp[MdKF12D::h1(b)], g, y[b]);
#pragma unroll
    for (int i = 0; i < 12; i++) {
      const double t = hp[i] * si;
#pragma unroll
      for (int j = 0; j <= i; j++) P[pk(i, j)] = dfma(-t, hp[j], P[pk(i, j)]);
    }
  }
}

// P <- F P F^T + Q with F = I + dt (pos <- vel): every 2x2 block {p_k, v_k} x {p_l, v_l} maps
// from its own four entries (a b / c d): pp = (a + dt c) + dt (b + dt d), vp = c + dt d,
// pv = b + dt d, vv = d; bit-identical to the generic T = F P, T F^T form (kf_predict_cov).
// Exactly-zero Q entries are not added (kf_predict_cov's SKIPQ); SP: the blocks k != l have
// no Q at all (checked on the host)
template <bool SP>
__device__ __forceinline__ void kf12d_predict_cov(double (&P)[78], double dt, const double *Q) {
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const kparam_ptr q = opaque_param(Q);
#pragma unroll
    for (int l = 0; l <= k; l++) {
      const bool hasq = !SP || k == l;
      auto addq = [&](double v, int e) -> double {
        if (!hasq) return v;
        const double qe = q[e];
        const double w = v + qe;
        return qe != 0.0 ? w : v;
      };
      const int pk_ = kf12_pos(k), vk = pk_ + 3, pl = kf12_pos(l), vl = pl + 3;
      const double a = P[pk(pk_, pl)], b = P[pk(pk_, vl)], c = P[pk(vk, pl)], d = P[pk(vk, vl)];
      const double t01 = dfma(dt, d, b);
      P[pk(pk_, pl)] = addq(dfma(dt, t01, dfma(dt, c, a)), pk(pk_, pl));
      P[pk(vk, pl)] = addq(dfma(dt, d, c), pk(vk, pl));
      if (k != l) P[pk(pk_, vl)] = addq(t01, pk(pk_, vl));
      P[pk(vk, vl)] = addq(d, pk(vk, vl));
    }
  }
}

// The block's chunk of its tile through scalar descriptors (TileRows): a 32-bit lane offset per
// access and no 64-bit address math.
// ENS: the record epilogue of fmskf_tick_ensemble; every lane then stays to the block
// reduction (lanes past N tick instance N-1, a clamped index, and store nothing)
template <bool BLK, bool UPD, bool PRED, int CP = 0, bool ENS = false, bool SP = false>
__global__ __launch_bounds__(kBlock) void k_kf12s(KfArgs<MdKF12D, Kf12dParams> a) {
  constexpr int N = 12, NP = 78, M = 8;
  uint32_t bid = blockIdx.x;  // the tick block (the carried fold blocks come first)
  if constexpr (ENS) {
    if (ens_fold_front<12>(a.in, bid)) return;
  }
  const uint64_t n = a.n;
  const uint64_t i0 = (uint64_t)bid * kBlock + threadIdx.x;
  const bool live = i0 < n;
  if (!ENS && !live) return;
  const uint64_t i = live ? i0 : n - 1;
  double x[N], P[NP];
  // Left from the planar form, whose store offsets the fence after the tick loop kept from being
  // held across it: an opaque scalar use of the pitch between the loop and the stores.  Nothing
  // reads ps, but without the pair every k_kf12s compiles to other code (the pitch load and a
  // shift go, the scalar registers and the placement of the store offsets change), and that has
  // not been measured
  uint32_t ps = (uint32_t)a.pitch * 8u;
  // without ENS lanes past N returned above, so a lane's slot is its thread index
  const uint32_t slot = ENS ? tile_slot(n, bid) : threadIdx.x;
  const TileRows<double, N, CP> tx(a.x, bid, slot, 0);
  const TileRows<double, NP, CP> tp(a.P, bid, slot, 0);
#pragma unroll
  for (int k = 0; k < N; k++) x[k] = tx.ld(k);
#pragma unroll
  for (int k = 0; k < NP; k++) P[k] = tp.ld(k);
  const double dt = a.prm.dt;
  for (uint32_t t = 0; t < a.in.n_ticks; t++) {
    if (UPD) {
      if (a.in.valid == nullptr || a.in.valid[(uint64_t)t * a.in.stride + i]) {
        const double *z = a.in.z + (uint64_t)t * a.in.stride * M;
        double y[M];
#pragma unroll
        for (int q = 0; q < M; q++) y[q] = z[q * a.in.stride + i] - x[MdKF12D::h1(q)];
        y[0] = wrap_innov(y[0]);
        kf12d_decor_update<BLK, SP>(x, P, y, a.prm.coef);
      }
    }
    if (PRED) {
#pragma unroll
      for (int q = 0; q < 6; q++) {
        const int p = kf12_pos(q);
        x[p] = dfma(dt, x[p + 3], x[p]);
      }
      x[2] = wrap_pi(x[2]);
      kf12d_predict_cov<SP>(P, dt, a.prm.coef + 36);
    }
  }
  asm volatile("" : "+s"(ps));  // (see ps above)
  if (live) {
#pragma unroll
    for (int k = 0; k < N; k++) tx.st(k, x[k]);
#pragma unroll
    for (int k = 0; k < NP; k++) tp.st(k, P[k]);
  }
  nan_guard(x, P, a.counters, live);
  if constexpr (ENS) {
    double xs[1][N];
#pragma unroll
    for (int k = 0; k < N; k++) xs[0][k] = x[k];
    const bool lv[1] = {live};
    ens_epilogue<12, 1>(a.in, xs, lv, bid);
  }
}

// fused tick + record (fmskf_tick_ensemble): the default single-tick kernel with the record
// epilogue (and the carried fold blocks past the tick blocks when in.fold_blocks is set);
// returns the tick grid (= the number of block records)
template <bool LIBM, bool SEQ, bool COMP>
static int launch_ekf9_ens(KfArgs<MdEKF9, Ekf9Params> a, hipStream_t st) {
  const unsigned carry = a.in.fold_blocks ? (unsigned)EnsRec<9>::LEN : 0u;
  const LaunchRegime r = ekf9_ens_regime(a.n, COMP, LIBM);
  const unsigned ntiles = grid_for(a.n).x, g = r.two ? (ntiles + 1) / 2 : ntiles;
  a.in.ens_grid = g;
  with_bools([&](auto TWO, auto NT) {
    constexpr int CP = NT() ? kStateNT : 0;
    if constexpr (TWO() && !LIBM)
      launch_signal(k_ekf9p<false, SEQ, CP, true, COMP>, dim3(g + carry), r.lds, st, a.in.ens_done, a);
    else if constexpr (!TWO())
      launch_signal(k_ekf9t<LIBM, true, true, SEQ, CP, true, COMP>, dim3(g + carry), r.lds, st, a.in.ens_done, a);
  }, r.two, r.nt);
  return (int)g;
}

// A: Ekf9Args, or RowGateArgs for a row-gated handle (update launches with a diagonal R only:
// launch_ekf9_rowgate).  The single full tick goes by ekf9_regime (launch_regime.hpp); every other
// form is one robot per lane, cached and uncapped
template <bool LIBM, bool SEQ, bool COMP, class A>
static void launch_ekf9_l(const A &aa, bool upd, bool pred, hipStream_t st) {
  constexpr bool GATED = std::is_same<A, RowGateArgs>::value;
  const Ekf9Args &a = kf_args(aa);
  const dim3 g = grid_for(a.n);
  const bool many = a.in.n_ticks != 1;
  if (!many && upd && pred) {
    const LaunchRegime r = ekf9_regime(a.n, COMP, GATED, LIBM);
    with_bools([&](auto TWO, auto NT) {
      constexpr int CP = NT() ? kStateNT : 0;
      if constexpr (TWO() && !LIBM)
        k_ekf9p<false, SEQ, CP, false, COMP, A><<<dim3((g.x + 1) / 2), kBlock, r.lds, st>>>(aa);
      else if constexpr (!TWO())
        k_ekf9t<LIBM, true, true, SEQ, CP, false, COMP, A><<<g, kBlock, r.lds, st>>>(aa);
    }, r.two, r.nt);
    return;
  }
  with_bools([&](auto MANY, auto UPD, auto PRED) {
    constexpr bool FULL = UPD() && PRED();
    // predict-only launches run no update: one (SEQ = false) instantiation serves both
    constexpr bool S = UPD() && SEQ;
    // the row-gated handle has the full tick_many and the single correct alone
    constexpr bool HAVE = MANY() ? FULL || (!GATED && (UPD() || PRED())) : !FULL && (UPD() || (!GATED && PRED()));
    if constexpr (HAVE) {
      if constexpr (MANY()) k_ekf9<LIBM, UPD(), PRED(), S, COMP, A><<<g, kBlock, 0, st>>>(aa);
      else k_ekf9t<LIBM, UPD(), PRED(), S, 0, false, COMP, A><<<g, kBlock, 0, st>>>(aa);
    }
  }, many, upd, pred || !upd);
}

int launch_ekf9(const DevState &s, const TickIn &in, const Ekf9Params &p, bool libm, bool upd,
                bool pred, hipStream_t st, int *ens_nb) {
  KfArgs<MdEKF9, Ekf9Params> a{s.n, s.pitch, (float *)s.x, (float *)s.P, in, s.counters, p};
  a.prm.thlo = s.thlo;
  a.prm.clo = s.xlo;  // FMSKF_CFG_COMP_POS
  if (!s.thlo) return (int)hipErrorInvalidValue;
  if ((in.ens_blocks && (!ens_nb || !upd || !pred || in.n_ticks != 1)) || (in.fold_blocks && !in.ens_blocks))
    return (int)hipErrorInvalidValue;
  // canonical update order (oracle orc_ekf9_tick): sequential scalar updates when R is
  // diagonal (SEQ), the joint LDL^T update otherwise
  with_bools([&](auto LIBM, auto SEQ, auto COMP) {
    if (in.ens_blocks) *ens_nb = launch_ekf9_ens<LIBM(), SEQ(), COMP()>(a, st);
    else launch_ekf9_l<LIBM(), SEQ(), COMP()>(a, upd, pred, st);
  }, libm, ekf9_r_diagonal(p.r), s.xlo != nullptr);
  return (int)hipGetLastError();
}

// The row-gated handle (fmskf_set_row_gate): the same kernels on RowGateArgs through the same
// regimes, with the gate word in the bytes per robot.  No fused ensemble record, no ISR form, no
// compensated positions: the callers take the stand-alone record / the three-kernel ISR / refuse
// the gate.
int launch_ekf9_rowgate(const DevState &s, const TickIn &in, const Ekf9Params &p, const RowGateDev &g,
                        bool libm, bool pred, hipStream_t st) {
  if (!s.tile || !s.thlo || s.xlo || in.ens_blocks || in.fold_blocks || !in.raw || !g.word ||
      !g.d2 || g.d2_pitch < s.n || !ekf9_r_diagonal(p.r))
    return (int)hipErrorInvalidValue;
  if (!pred && in.n_ticks != 1) return (int)hipErrorInvalidValue;
  RowGateArgs ga{{s.n, s.pitch, (float *)s.x, (float *)s.P, in, s.counters, p}, g};
  ga.k.prm.thlo = s.thlo;
  ga.k.prm.clo = nullptr;
  with_bools([&](auto LIBM) { launch_ekf9_l<LIBM(), true, false>(ga, true, pred, st); }, libm);
  return (int)hipGetLastError();
}

template <bool CAN>
static int isr_ekf9_l(const DevState &s, const TickIn &in, const Ekf9Params &prm, bool libm, const CtrlDev &c,
                      const CtrlPrm &p, const int16_t *rpm, uint8_t *frames, hipStream_t st, const CanArgs &can) {
  if (c.n == 0) return 0;
  const uint64_t sb = ekf9_state_bytes(s.xlo != nullptr);
  if (!s.thlo || in.n_ticks != 1 || !in.raw || (!CAN && !rpm) || state_nt(s.n * sb) || !ctrl_small(c))
    return (int)hipErrorNotSupported;
  KfArgs<MdEKF9, Ekf9Params> a{s.n, s.pitch, (float *)s.x, (float *)s.P, in, s.counters, prm};
  a.prm.thlo = s.thlo;
  a.prm.clo = s.xlo;
  const bool nt = state_nt(ctrl_state_bytes(c) + s.n * sb);
  const unsigned lds = nt ? FMSKF_LDS_CAP("FMSKF_ISR_LDS", true, 48u * 1024u) : 0u;
  // CNT (CAN only): the EKF9 state and the motor state together past the Infinity Cache: the
  // motor state streams non-temporal and the EKF9 state stays resident
  with_bools([&](auto LIBM, auto SEQ, auto COMP, auto NT, auto CNT) {
    if constexpr (CAN || !CNT())
      k_isr_ekf9<LIBM(), SEQ(), NT() ? kStateNT : 0, COMP(), CAN, CNT()>
          <<<grid_for(c.n), kBlock, lds, st>>>(a, c, p, frames, rpm, can);
  }, libm, ekf9_r_diagonal(prm.r), s.xlo != nullptr, nt, CAN && can_nt_flag(can));
  return (int)hipGetLastError();
}

// fmskf_isr_tick for EKF9 in one kernel where it applies: one tick, the tiled EKF9 state
// cache-resident (past the Infinity Cache the tick kernel streams it non-temporal under its own
// occupancy cap: three kernels, as for KF6), the control planes in one 4 GiB window.
// hipErrorNotSupported otherwise
int launch_isr_ekf9(const DevState &s, const TickIn &in, const Ekf9Params &prm, bool libm, const CtrlDev &c,
                    const CtrlPrm &p, const int16_t *rpm, uint8_t *frames, hipStream_t st) {
  return isr_ekf9_l<false>(s, in, prm, libm, c, p, rpm, frames, st, CanArgs{});
}

// the same with the tick's CAN RX fused in front (fmskf_isr_tick_can: no caller rpm)
int launch_isr_ekf9_can(const DevState &s, const TickIn &in, const Ekf9Params &prm, bool libm, const CtrlDev &c,
                        const CtrlPrm &p, uint8_t *frames, const uint8_t *can_frames, const int16_t *can_stamps,
                        const int8_t dir[4], hipStream_t st) {
  CanArgs ca;
  if (!can_args(s, can_frames, can_stamps, dir, ca)) return (int)hipErrorNotSupported;
  ca.nt = can_nt(s);
  return isr_ekf9_l<true>(s, in, prm, libm, c, p, nullptr, frames, st, ca);
}

int launch_kf12d(const DevState &s, const TickIn &in, const Kf12dParams &p, bool upd, bool pred,
                 hipStream_t st, int *ens_nb) {
  KfArgs<MdKF12D, Kf12dParams> a{s.n, s.pitch, (double *)s.x, (double *)s.P, in, s.counters, p};
  const dim3 g = grid_for(s.n);
  const LaunchRegime r = kf12d_regime(s.n);
  const bool nt = r.nt;
  // SP (the default R and Q: sparse C^-1 and Q, checked on the host) implies BLK
  const bool sp = p.sparse != 0, blk = kf12d_sequential(p.r);
  if (in.fold_blocks && !in.ens_blocks) return (int)hipErrorInvalidValue;
  if (in.ens_blocks) {
    // fused tick + record (fmskf_tick_ensemble): the default kernel (decorrelated update) with
    // the record epilogue; one record per tick block
    if (!p.decor || !ens_nb || !upd || !pred || in.n_ticks != 1) return (int)hipErrorInvalidValue;
    a.in.ens_grid = g.x;
    const dim3 ge(g.x + (in.fold_blocks ? (unsigned)EnsRec<12>::LEN : 0u));  // + the carried fold
    with_bools([&](auto BLK, auto SP, auto NT) {
      if constexpr (BLK() || !SP())
        launch_signal(k_kf12s<BLK(), true, true, NT() ? kStateNT : 0, true, SP()>, ge, 0, st, in.ens_done, a);
    }, sp || blk, sp, nt);
    *ens_nb = (int)g.x;
    return (int)hipGetLastError();
  }
  if (p.decor) {
    if (upd && pred) {
      with_bools([&](auto BLK, auto SP, auto NT) {
        if constexpr (BLK() || !SP())
          k_kf12s<BLK(), true, true, NT() ? kStateNT : 0, false, SP()><<<g, kBlock, r.lds, st>>>(a);
      }, sp || blk, sp, nt);
    } else if (upd) {
      with_bools([&](auto BLK) { k_kf12s<BLK(), true, false><<<g, kBlock, 0, st>>>(a); }, blk);
    } else {  // a predict runs no update: one (BLK = false) instantiation serves both
      k_kf12s<false, false, true><<<g, kBlock, 0, st>>>(a);
    }
  } else if (upd) {
    with_bools([&](auto SEQ, auto PRED) { k_kf12d<SEQ(), true, PRED()><<<g, kBlock, 0, st>>>(a); }, blk, pred);
  } else {  // as above: one (SEQ = false) instantiation
    k_kf12d<false, false, true><<<g, kBlock, 0, st>>>(a);
  }
  return (int)hipGetLastError();
}

}  // namespace fmskf
