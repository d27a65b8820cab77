// kernels_kf6.hip -- the headline 6-state fp32 KF tick (BASELINE.json configs[1], SURVEY.md
// 8(d) cfg 2) for gfx950.
//
// One robot per lane, x (6) and packed P (21) in VGPRs; a tick = measurement frontend
// (yaw, gyro z, 4 wheel rpm -> z, the reference's deg2rad / mecanum FK / rotation,
// VD_vehicle_controller.cpp:21-51) + LDL^T-form update + F P F^T + Q predict, one read and
// one write of every state byte: 232 algorithmic bytes per instance-tick (the write of the
// masked cross-covariance planes, kf6_lane.hpp, is issued only where a lane's value changed).
// The mask belongs to the launch regime (kf6_wide, launch_regime.hpp): the two-per-lane full tick takes all
// eight cross planes (Opt WIDE) while state + inputs fill at most half the Infinity Cache, every
// other launch their position half (kKf6SkipMask); the kernels without WIDE are the code they
// were before the split (profiles/kf6_half_cache_bodies.json).
//
// In that same half-cache regime a direct launch also leaves out the loads of the cross planes its
// wave is known to hold zero (Opt ZL on ZeroArgs; kf6_lane.hpp kKf6ZeroLoad, kf6_zero_loads in
// launch_regime.hpp): one flag word per 64-robot chunk, read through the scalar path ahead of the
// state loads, a wave-uniform branch around the masked planes' loads (issued last), the new word
// stored by lane 0 of the owning wave behind the state.  Memory holds every plane of every robot
// as an unconditional tick leaves it; whether a launch may trust the flags is the host's decision
// (api_ctx.hpp check_handle), never a captured one.  The kernels without ZL are the code they
// were (profiles/kf6_zero_loads_bodies.json).
//
// A plain full tick launched right behind an asynchronous ensemble event carries that event's
// fold (Opt FOLD): the LEN fold blocks of ens_fold_front ahead of its tick blocks, as the record
// tick of the next event would carry them, and no record epilogue.  The host decides (run_tick);
// a launch without a pending fold takes the plain instantiation, whose code FOLD does not touch.
//
// Memory-path design (MI355X_MICROARCH.md: s_waitcnt vmcnt is in-order, so any load issued
// after the state loads makes every later wait cover them):
//  * the 2 KiB TABLE512 sine table is staged in LDS (per wave in the single-tick kernel, per
//    block in the loop kernels), so the trig lookups in the middle of the math wait on
//    lgkmcnt only, never behind the state loads;
//  * the tiled state is addressed through buffer descriptors built from kernel arguments (T8):
//    one descriptor per array over the lane's tile, a 32-bit lane byte offset and a per-row
//    scalar soffset, so the loop needs almost no scalar or vector address math (the inputs:
//    kf6_load_in, whose SMALL instantiation keeps the array-base form while n < 51M);
//  * whether a validity mask exists is a compile-time choice (no conditional load whose
//    merge would force a full vmcnt(0) drain);
//  * tick_many loads the inputs of tick t+1 before computing tick t.
//
// The chi-square innovation gate (fmskf_set_gate) is an instantiation of the same kernels on
// GateArgs (kf6_lane.hpp): one more lane struct loaded with the state and stored with it, the
// gated update inside kf6_tick1, the launch regimes of the plain handle (kf6_regime, launch_regime.hpp).
#include "ens_device.hpp"
#include "kf6_lane.hpp"

#pragma clang fp contract(off)

namespace fmskf {

// tick_many: T ticks per launch, state in VGPRs throughout; the inputs of the next tick are
// loaded while the current one computes.  Unrolled by two with ping-pong input registers
// (ma / mb) so no input record is copied around the loop; clamped index, no live branch.
// A: Kf6Args, or GateArgs for a gated handle (every tick kernel here): the lane's gate state is
// loaded with the other loads and stored with the state, the gate word held across the ticks.
template <int WPE, class O, class A = Kf6Args>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(WPE, 8))) void k_kf6(A aa) {
  const Kf6Args &a = kf_args(aa);
  __shared__ float stab[O::LIBM ? 1 : 513];
  const uint64_t n = a.n;
  const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
  const bool live = i < (uint32_t)n;
  const uint32_t ic = live ? i : (uint32_t)n - 1u;
  const uint32_t T = a.in.n_ticks;
  float x[6], P[21];
  Kf6Lo<O> lo;
  Kf6GateOf<O, A> gt;
  Kf6In ma, mb;
  kf6_load_state<O>(a.x, a.P, a.pitch, ic, x, P);
  const auto old = kf6_keep_old<kf6_mask<O>()>(P);  // as loaded: compared after the launch's last tick
  kf6_load_lo<O>(a.prm.lo, ic, lo);
  gt.load(gate_dev(aa), ic, n);
  if (O::UPD) ma = kf6_load_in<O>(a.in, n, 0, ic);
  stage_table<O::LIBM>(stab, a.in.sintab);
  for (uint32_t t = 0; t < T; t += 2) {
    if (O::UPD && t + 1 < T) mb = kf6_load_in<O>(a.in, n, t + 1, ic);
    kf6_tick1<O>(ma, stab, a.prm, x, P, lo, gt);
    if (t + 1 >= T) break;
    if (O::UPD && t + 2 < T) ma = kf6_load_in<O>(a.in, n, t + 2, ic);
    kf6_tick1<O>(mb, stab, a.prm, x, P, lo, gt);
  }
  if (live) {
    kf6_store_state<O>(a.x, a.P, a.pitch, i, x, P, old);
    kf6_store_lo<O>(a.prm.lo, i, lo);
    gt.store(gate_dev(aa), i, n);
  }
  nan_guard(x, P, a.counters, live);
}

// Single tick, straight line: no tick loop (so no loop-carried register copies) and no
// live/dead branch around the loads: lanes past N load instance N-1 (a clamped index, always
// in bounds), compute on it, and only their stores and NaN count are masked off.
// No gated instantiation: a gated handle's one-per-lane launches take k_kf6p with R = 1 (launch_one).
template <int WPE, class O>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(WPE, 8))) void k_kf6t(Kf6Args a) {
  uint32_t bid = blockIdx.x;
  if constexpr (O::ENS || O::FOLD) {
    if (ens_fold_front<6>(a.in, bid)) return;
  }
  const uint64_t n = a.n;
  const uint32_t i = bid * kBlock + threadIdx.x;
  const bool live = i < (uint32_t)n;
  const uint32_t ic = live ? i : (uint32_t)n - 1u;
  float x[6], P[21];
  Kf6In m;
  // wave-private copy of the sine table: its loads are issued first (vmcnt retires in order)
  // and no block barrier couples the four waves' memory phases (~1% over a block-shared copy)
  __shared__ float wtab[O::LIBM ? 1 : kBlock / 64][O::LIBM ? 1 : kWaveTab];
  float *stab = wtab[O::LIBM ? 0 : threadIdx.x >> 6];
  WaveTable<O::LIBM> tv(a.in.sintab);
  Kf6Lo<O> lo;
  Kf6Gate<O, false> gt;
  kf6_load_state<O>(a.x, a.P, a.pitch, ic, x, P);
  const auto old = kf6_keep_old<kf6_mask<O>()>(P);
  kf6_load_lo<O>(a.prm.lo, ic, lo);
  if (O::UPD) m = kf6_load_in<O>(a.in, n, 0, ic);
  tv.store(stab);
  kf6_tick1<O>(m, stab, a.prm, x, P, lo, gt);
  if (live) {
    kf6_store_state<O>(a.x, a.P, a.pitch, i, x, P, old);
    kf6_store_lo<O>(a.prm.lo, i, lo);
  }
  nan_guard(x, P, a.counters, live);
  if constexpr (O::ENS) {
    float xs[1][6];
#pragma unroll
    for (int k = 0; k < 6; k++) xs[0][k] = x[k];
    const bool lv[1] = {live};
    ens_epilogue<6, 1>(a.in, xs, lv, bid);
  }
}

// R robots per lane (i, i + G, ..., G = the tick blocks' lane count), the tick inputs of all R
// loaded up front: robot r's inputs (fresh from HBM) arrive while robots 0..r-1 are loaded,
// computed and stored; one register set for the state, 1/R of the grid.
template <int WPE, int R, class O, class A = Kf6Args>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(WPE, 8))) void k_kf6p(A aa) {
  const Kf6Args &a = kf_args(aa);
  uint32_t bid = blockIdx.x;
  if constexpr (O::ENS || O::FOLD) {
    if (ens_fold_front<6>(a.in, bid)) return;
  }
  const uint64_t n = a.n;
  const uint32_t nn = (uint32_t)n, last = nn - 1u;
  const uint32_t G = (O::ENS || O::FOLD ? a.in.ens_grid : gridDim.x) * kBlock;
  const uint32_t i0 = bid * kBlock + threadIdx.x;
  float x[6], P[21];
  __shared__ float wtab[O::LIBM ? 1 : kBlock / 64][O::LIBM ? 1 : kWaveTab];
  float *stab = wtab[O::LIBM ? 0 : threadIdx.x >> 6];
  WaveTable<O::LIBM> tv(a.in.sintab);
  Kf6In m[R];
  float xs[O::ENS ? R : 1][6];
  bool lv[R];
  uint32_t zf[O::ZL ? R : 1];  // ZL: the robots' chunk words, read up front with the inputs
  if constexpr (O::ZL) {
#pragma unroll
    for (int r = 0; r < R; r++) zf[r] = kf6_zero_flag(aa.flags, min(i0 + r * G, last));
  }
  if (O::UPD) {
#pragma unroll
    for (int r = 0; r < R; r++) m[r] = kf6_load_in<O>(a.in, n, 0, min(i0 + r * G, last));
  }
#pragma unroll
  for (int r = 0; r < R; r++) {
    const uint32_t i = i0 + r * G;
    const bool live = i < nn;
    Kf6Lo<O> lo;
    Kf6GateOf<O, A> gt;
    if constexpr (O::ZL) kf6_load_state_zl<O>(a.x, a.P, live ? i : last, aa.trusted && zf[r], x, P);
    else kf6_load_state<O>(a.x, a.P, a.pitch, live ? i : last, x, P);
    const auto old = kf6_keep_old<kf6_mask<O>()>(P);
    kf6_load_lo<O>(a.prm.lo, live ? i : last, lo);
    gt.load(gate_dev(aa), live ? i : last, n);
    if (r == 0) tv.store(stab);
    kf6_tick1<O>(m[r], stab, a.prm, x, P, lo, gt);
    if (live) {
      kf6_store_state<O>(a.x, a.P, a.pitch, i, x, P, old);
      kf6_store_lo<O>(a.prm.lo, i, lo);
      gt.store(gate_dev(aa), i, n);
    }
    if constexpr (O::ZL) {
      // the chunk's word after this tick, stored by lane 0 of the wave that owns the chunk (lane 0
      // live; a wave wholly past N has seen one robot of another wave's chunk and stores nothing):
      // where it changed, or in an untrusted launch always (the rebuild)
      const uint32_t nf = kf6_zero_now(P) ? 1u : 0u;
      if (live && (threadIdx.x & 63u) == 0 && (!aa.trusted || nf != zf[r])) aa.flags[i / kZeroChunk] = nf;
    }
    nan_guard(x, P, a.counters, live);
    if constexpr (O::ENS) {
#pragma unroll
      for (int k = 0; k < 6; k++) xs[r][k] = x[k];
    }
    lv[r] = live;
  }
  if constexpr (O::ENS) ens_epilogue<6, R>(a.in, xs, lv, bid);
}

// A FOLD instantiation on the tick grid g: the LEN fold blocks of the pending ensemble event
// ahead of the tick blocks, as launch_ens_o launches a record tick that carries one
template <class A>
static void launch_fold(void (*k)(A), A aa, unsigned g, unsigned lds, hipStream_t st) {
  kf_args_mut(aa).in.ens_grid = g;
  launch_signal(k, dim3(g + (unsigned)EnsRec<6>::LEN), lds, st, kf_args(aa).in.ens_done, aa);
}

// One robot per lane: k_kf6t, or for a gated handle k_kf6p's single-robot form, the shape its
// one-per-lane launches always had (the inputs are loaded ahead of the state; through k_kf6t the
// gated tick at 2^24 measured 642-643 us against 633, profiles/gate_fold_ab.json)
template <class O, class A>
static void launch_one(const A &aa, unsigned lds, hipStream_t st) {
  const dim3 g = grid_for(kf_args(aa).n);
  if constexpr (std::is_same<A, GateArgs>::value) k_kf6p<4, 1, O, A><<<g, kBlock, lds, st>>>(aa);
  else if constexpr (O::FOLD) launch_fold(k_kf6t<4, O>, aa, g.x, lds, st);
  else k_kf6t<4, O><<<g, kBlock, lds, st>>>(aa);
}

// A: Kf6Args, or GateArgs for a gated handle (bytes per robot: + the gate word and the NIS)
// z: the handle's zero flags where the caller maintains their trust (Kf6Zero), else null
template <class O, class A>
static void launch_o(const A &aa, hipStream_t st, Kf6Zero *z = nullptr) {
  constexpr bool GATED = std::is_same<A, GateArgs>::value;
  const Kf6Args &a = kf_args(aa);
  if constexpr (GATED && !O::PRED) {  // the gated fmskf_correct: one robot per lane, uncapped
    launch_one<O>(aa, 0u, st);
  } else {
    if (a.in.n_ticks != 1) {
      k_kf6<4, O, A><<<grid_for(a.n), kBlock, 0, st>>>(aa);
      return;
    }
    const LaunchRegime r = kf6_regime(a.n, O::COMP, GATED, a.in.rec != nullptr);
    // the streamed (non-temporal) kernels exist for the full tick only; in a two-per-lane launch
    // only when forced, since that regime's state fits the cache
    constexpr bool NT = O::UPD && O::PRED;
    if (r.two) {
      const unsigned g = (unsigned)((a.n + 2 * kBlock - 1) / (2 * kBlock));
      if constexpr (NT && !GATED) {
        // the ungated full tick: streamed, with the wide mask (kf6_wide; never COMP, whose
        // kernels stay as they were) and / or carrying a pending ensemble fold (run_tick)
        const bool wide = !O::COMP && kf6_wide(a.n), fold = a.in.fold_blocks != nullptr;
        // the wide mask's kernels with the loads of known zeros left out (Opt ZL)
        // (zl implies wide: the lambda below has no kernel for Z without W, nor for COMP)
        const bool zl = wide && z && z->flags && kf6_zero_loads(a.n);
        if (r.nt || wide || fold) {
          with_bools([&](auto N, auto W, auto F, auto Z) {
            using ON = std::conditional_t<N(), WithNT<O>, O>;
            using OW = std::conditional_t<W() && !O::COMP, WithWide<ON>, ON>;
            if constexpr (Z() && W() && !O::COMP) {
              const ZeroArgs za{aa, z->flags, z->trusted ? 1u : 0u};
              if constexpr (F()) launch_fold(k_kf6p<4, 2, WithZero<WithFold<OW>>, ZeroArgs>, za, g, r.lds, st);
              else k_kf6p<4, 2, WithZero<OW>, ZeroArgs><<<g, kBlock, r.lds, st>>>(za);
              z->used = true;
            } else if constexpr (!Z()) {
              if constexpr (F()) launch_fold(k_kf6p<4, 2, WithFold<OW>, A>, aa, g, r.lds, st);
              else k_kf6p<4, 2, OW, A><<<g, kBlock, r.lds, st>>>(aa);
            }
          }, r.nt, wide, fold, zl);
          return;
        }
      }
      k_kf6p<4, 2, O, A><<<g, kBlock, r.lds, st>>>(aa);
      return;
    }
    if constexpr (NT && !GATED) {
      if (a.in.fold_blocks) {  // one robot per lane, carrying a pending ensemble fold
        with_bools([&](auto N) { launch_one<WithFold<std::conditional_t<N(), WithNT<O>, O>>>(aa, r.lds, st); }, r.nt);
        return;
      }
    }
    with_bools([&](auto N) { launch_one<std::conditional_t<N() && NT, WithNT<O>, O>>(aa, r.lds, st); }, r.nt);
  }
}

// fused tick + ensemble record (fmskf_tick_ensemble): the kernel launch_o picks by default,
// with the record epilogue (and the carried fold blocks ahead of the tick blocks when
// in.fold_blocks is set); returns the tick grid (= the number of block records).  Four robots
// per lane (half the block reductions per robot) measured slower: K = 1 at 2^20 40.8-41.0 us
// per tick against 38.6-39.0 (kbench, two alternating passes)
template <class O>
static int launch_ens_o(KfArgs<MdKF6, Kf6Params> a, hipStream_t st, Kf6Zero *z) {
  using E = WithEns<O>;
  const unsigned carry = a.in.fold_blocks ? (unsigned)EnsRec<6>::LEN : 0u;
  const LaunchRegime r = kf6_ens_regime(a.n, O::COMP);
  const unsigned g = r.two ? (unsigned)((a.n + 2 * kBlock - 1) / (2 * kBlock)) : grid_for(a.n).x;
  a.in.ens_grid = g;
  // two per lane: the write-back mask of the plain tick of the same regime (kf6_wide)
  const bool wide = r.two && !O::COMP && kf6_wide(a.n);
  // the last bool implies wide, and wide implies two: the combinations without a kernel below
  with_bools([&](auto TWO, auto N, auto W, auto Z) {
    using EN = std::conditional_t<N(), WithNT<E>, E>;
    if constexpr (TWO()) {
      using EW = std::conditional_t<W() && !O::COMP, WithWide<EN>, EN>;
      if constexpr (Z() && W() && !O::COMP) {
        const ZeroArgs za{a, z->flags, z->trusted ? 1u : 0u};
        launch_signal(k_kf6p<4, 2, WithZero<EW>, ZeroArgs>, dim3(g + carry), r.lds, st, a.in.ens_done, za);
        z->used = true;
      } else if constexpr (!Z()) {
        launch_signal(k_kf6p<4, 2, EW>, dim3(g + carry), r.lds, st, a.in.ens_done, a);
      }
    } else if constexpr (!W() && !Z()) {
      launch_signal(k_kf6t<4, EN>, dim3(g + carry), r.lds, st, a.in.ens_done, a);
    }
  }, r.two, r.nt, wide, wide && z && z->flags && kf6_zero_loads(a.n));
  return (int)g;
}

template <class O>
static void launch_sel(const KfArgs<MdKF6, Kf6Params> &a, hipStream_t st, int *ens_nb, Kf6Zero *z) {
  if constexpr (O::UPD && O::PRED) {
    if (ens_nb) {
      *ens_nb = launch_ens_o<O>(a, st, z);
      return;
    }
  }
  launch_o<O>(a, st, z);
}

int launch_kf6(const DevState &s, const TickIn &in, const Kf6Params &p, bool libm, bool upd,
               bool pred, hipStream_t st, int *ens_nb, Kf6Zero *z) {
  if (z) z->used = false;
  KfArgs<MdKF6, Kf6Params> a{s.n, s.pitch, (float *)s.x, (float *)s.P, in, s.counters, p};
  const bool small = kf6_small(s);  // Opt::SMALL
  const bool valid = upd && in.valid != nullptr, rec = upd && in.rec != nullptr;
  const bool comp = p.lo != nullptr;  // FMSKF_CFG_COMP_POS
  int *nb = in.ens_blocks && upd && pred && in.n_ticks == 1 ? ens_nb : nullptr;
  // a carried fold rides on a full single tick alone: with the record epilogue (launch_ens_o) or,
  // for a plain tick, in the FOLD instantiations (launch_o)
  if ((in.ens_blocks && !nb) || (in.fold_blocks && !(upd && pred && in.n_ticks == 1)))
    return (int)hipErrorInvalidValue;
  if (upd) {
    with_bools([&](auto LIBM, auto PRED, auto REC, auto COMP, auto SMALL, auto VALID) {
      launch_sel<Opt<LIBM(), true, PRED(), SMALL(), VALID(), REC(), false, false, COMP()>>(a, st, nb, z);
    }, libm, pred, rec, comp, small, valid);
  } else {  // a predict reads no input: SMALL, VALID and REC cannot change its code
    with_bools([&](auto LIBM, auto COMP) {
      launch_o<Opt<LIBM(), false, true, true, false, false, false, false, COMP()>>(a, st);
    }, libm, comp);
  }
  return (int)hipGetLastError();
}

// The gated handle (fmskf_set_gate): the same kernels on GateArgs through the same regimes.
// Input descriptors are always the chunk-based form that is valid for any N (kf6_load_in without
// SMALL).  No fused ensemble record and no compensated positions: the callers take the
// stand-alone record / refuse the gate.
int launch_kf6_gate(const DevState &s, const TickIn &in, const Kf6Params &p, const GateDev &g, bool libm,
                    bool pred, hipStream_t st) {
  if (p.lo || in.ens_blocks || in.fold_blocks || !g.word || !g.nis) return (int)hipErrorInvalidValue;
  if (!pred && in.n_ticks != 1) return (int)hipErrorInvalidValue;
  const GateArgs ga{{s.n, s.pitch, (float *)s.x, (float *)s.P, in, s.counters, p}, g};
  with_bools([&](auto LIBM, auto PRED, auto VALID, auto REC) {
    launch_o<Opt<LIBM(), true, PRED(), false, VALID(), REC()>>(ga, st);
  }, libm, pred, in.valid != nullptr, in.rec != nullptr);
  return (int)hipGetLastError();
}

}  // namespace fmskf
