// kf6_lane.hpp -- one robot's 6-state KF tick as lane functions (inputs, state load / store,
// measurement frontend, update + predict, the optional gate state), shared by the KF6 tick
// kernels (kernels_kf6.hip, plain and gated instantiations) and the fused firmware ISR
// (kernels_ctrl.hip k_isr_kf6).  Canonical operation order of the oracle (orc_kf6_tick), so
// every kernel built from these is bit-exact to it.
#pragma once
#include <type_traits>
#include "kf_generic.hpp"

#pragma clang fp contract(off)

namespace fmskf {

// REC: the inputs come as 16-byte fmskf_kf6_record's (one 16-byte load per lane) instead of
// the yaw / gyro / rpm planes (three loads): measured 41.6 -> 39.5 us per tick at 2^20
// NT: the state is loaded and stored non-temporal (fmskf_internal.hpp state_nt)
// ENS: the tick also writes its block's ensemble record of the post-tick state
// (fmskf_tick_ensemble; ens_device.hpp), so the record costs no second pass over x
// COMP: FMSKF_CFG_COMP_POS -- px, py, P00, P10, P11 carried as hi + lo (Kf6Params::lo, 5 tiled
// rows), every addition to them a TwoSum (oracle orc_kf6_tick_comp)
template <bool LIBM_, bool UPD_, bool PRED_, bool SMALL_, bool VALID_, bool REC_ = false, bool NT_ = false,
          bool ENS_ = false, bool COMP_ = false>
struct Opt {
  static constexpr bool LIBM = LIBM_, UPD = UPD_, PRED = PRED_, SMALL = SMALL_, VALID = VALID_,
                        REC = REC_, NT = NT_, ENS = ENS_, COMP = COMP_;
  static constexpr int CP = NT_ ? kStateNT : 0;
  static constexpr bool WIDE = false, FOLD = false, ZL = false;
  using Plain = Opt;
};
template <class O>
using WithNT = Opt<O::LIBM, O::UPD, O::PRED, O::SMALL, O::VALID, O::REC, true, O::ENS, O::COMP>;
template <class O>
using WithEns = Opt<O::LIBM, O::UPD, O::PRED, O::SMALL, O::VALID, O::REC, O::NT, true, O::COMP>;
template <class O>
using WithComp = Opt<O::LIBM, O::UPD, O::PRED, O::SMALL, O::VALID, O::REC, O::NT, O::ENS, true>;
// WIDE: the write-back mask holds all eight cross-covariance planes (kKf6SkipWide below) instead
// of their position half; chosen per launch regime (kernels_kf6.hip kf6_wide)
// FOLD: a plain tick whose grid has the fold blocks of a pending ensemble event ahead of its tick
// blocks (ens_device.hpp ens_fold_front), as the ENS kernels have, but writes no record itself
// Both ride on a type derived from the Opt, not on two more parameters of it: a parameter, even
// a defaulted one, is part of every instantiation's symbol, and the kernels without either trait
// keep theirs.  WithNT / WithEns / WithComp build a plain Opt, so these two are applied last.
template <class O, bool WIDE_, bool FOLD_>
struct OptX : O {
  static constexpr bool WIDE = WIDE_, FOLD = FOLD_;
};
template <class O>
using WithWide = OptX<typename O::Plain, true, O::FOLD>;
template <class O>
using WithFold = OptX<typename O::Plain, O::WIDE, true>;
// ZL: the launch skips the loads of the cross planes its wave is known to hold zero (kKf6ZeroLoad
// below, ZeroArgs); on WIDE instantiations only, applied after WithWide / WithFold.  A type of its
// own for the same reason: the kernels without it keep their symbols and their code.
template <class O>
struct OptZ : O {
  static_assert(O::WIDE && !O::COMP, "zero-load skipping rides on the wide write-back mask");
  static constexpr bool ZL = true;
};
template <class O>
using WithZero = OptZ<O>;

// the compensated entries of COMP: x 0-1 (px, py), packed P 0-2 (P00, P10, P11)
constexpr unsigned kKf6CXM = kPosCXM;
constexpr unsigned long long kKf6CPM = kPosCPM;
// the lane's low parts (COMP), one register when unused
template <class O>
struct Kf6Lo {
  float v[O::COMP ? kKf6LoRows : 1];
};

struct Kf6In {
  float yaw, gz;
  uint2 rpm;
  uint32_t valid;
};

// Kernel arguments.  A handle with the chi-square innovation gate (fmskf_set_gate) launches the
// same tick kernels instantiated on GateArgs: the plain arguments embedded as they are (nothing
// is added to KfArgs / TickIn / Kf6Params, so the plain kernels' argument offsets do not move),
// then the gate.
using Kf6Args = KfArgs<MdKF6, Kf6Params>;
struct GateArgs {
  Kf6Args k;
  GateDev g;
};
// The ZL instantiations take the plain arguments wrapped the same way: then the handle's zero
// flags (one word per 64-robot chunk, below) and whether this launch may trust them.
struct ZeroArgs {
  Kf6Args k;
  uint32_t *flags;
  uint32_t trusted;
};
struct NoGate {};
__host__ __device__ __forceinline__ const Kf6Args &kf_args(const Kf6Args &a) { return a; }
__host__ __device__ __forceinline__ const Kf6Args &kf_args(const GateArgs &a) { return a.k; }
__host__ __device__ __forceinline__ const Kf6Args &kf_args(const ZeroArgs &a) { return a.k; }
// the launchers' own copy, which they complete (ens_grid): a name of its own, so that no call of
// kf_args resolves differently
inline Kf6Args &kf_args_mut(Kf6Args &a) { return a; }
inline Kf6Args &kf_args_mut(ZeroArgs &a) { return a.k; }
__device__ __forceinline__ NoGate gate_dev(const Kf6Args &) { return {}; }
__device__ __forceinline__ NoGate gate_dev(const ZeroArgs &) { return {}; }
__device__ __forceinline__ const GateDev &gate_dev(const GateArgs &a) { return a.g; }

template <int CP = 0>
__device__ __forceinline__ float ld_f32(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff) {
  return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, voff, soff, CP));
}
template <int CP = 0>
__device__ __forceinline__ void st_f32(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff,
                                       float v) {
  __builtin_amdgcn_raw_buffer_store_b32(__builtin_bit_cast(uint32_t, v), r, voff, soff, CP);
}

// The per-tick inputs are read exactly once: load them non-temporal (gfx950 `nt`, aux bit 1)
// so the fresh 16 MB per tick at 2^20 displaces less of the state from the caches (measured
// 43.6 -> 42.7 us per tick with a 64-tick input ring).
#ifndef FMSKF_IN_CPOL
#define FMSKF_IN_CPOL 2
#endif
// inputs of one tick; planes of tick t start at t * stride elements
template <class O>
__device__ __forceinline__ Kf6In kf6_load_in(const TickIn &in, uint64_t n, uint64_t t, uint32_t i) {
  const uint64_t tb = t * in.stride;
  // Past the SMALL range (N >= ~51M) descriptors start at the block's first instance hb
  // (wave-uniform: every lane of a block, clamped ones included, lies in [hb, hb + 255]), so the
  // 32-bit lane offsets stay below 4 KiB for any N up to the 2^30 cap (a lane offset of i * 16
  // would wrap past 2^28 robots).  SMALL keeps the array-base form: ~0.2 us per 2^20 tick less.
  const uint32_t hb = O::SMALL ? 0u : __builtin_amdgcn_readfirstlane(i) & ~(uint32_t)(kBlock - 1);
  const uint32_t li = i - hb;
  const uint64_t base = tb + hb, left = n - hb;
  Kf6In m;
  if constexpr (O::REC) {
    const auto r = __builtin_amdgcn_raw_buffer_load_b128(rsrc(in.rec + base * 4, left * 16), li * 16u, 0,
                                                         FMSKF_IN_CPOL);
    // bit_cast a prvalue copy: on a vector-element lvalue clang's __builtin_bit_cast reads
    // element 0 (measured: r[1] came back as r[0])
    const uint32_t w0 = r[0], w1 = r[1];
    m.yaw = __builtin_bit_cast(float, w0);
    m.gz = __builtin_bit_cast(float, w1);
    m.rpm = make_uint2(r[2], r[3]);
    m.valid = O::VALID ? (uint32_t)in.valid[tb + i] : 1u;
    return m;
  }
  // the yaw / gyro z planes, or for a NULL one the IMU state's Yaw / GZ words (fmskf_device.hpp
  // tick_yaw): one dword per lane either way (with both from the IMU state, the same dword twice)
  const bool yw = (in.imu_words & 1u) != 0, gw = (in.imu_words & 2u) != 0;
  m.yaw = tick_yaw(yw, __builtin_amdgcn_raw_buffer_load_b32(rsrc(in.yaw_deg + base, left * 4), li * 4u, 0,
                                                            FMSKF_IN_CPOL));
  m.gz = tick_gz(gw, __builtin_amdgcn_raw_buffer_load_b32(rsrc(in.gyro_z + base, left * 4), li * 4u, 0,
                                                          FMSKF_IN_CPOL));
  const auto rr = __builtin_amdgcn_raw_buffer_load_b64(rsrc(in.rpm + base * 4, left * 8), li * 8u, 0,
                                                       FMSKF_IN_CPOL);
  m.rpm = make_uint2(rr[0], rr[1]);
  m.valid = O::VALID ? (uint32_t)in.valid[tb + i] : 1u;
  return m;
}

// The tiled state (fmskf_internal.hpp st_at, 2048 robots per tile row): the tile is wave-uniform
// (a wave's 64 robots, the clamped ones included, lie in one 256-robot chunk), so each array is
// one scalar descriptor over its tile and each row a scalar offset.  The pitch is not part of a
// tiled address; load and store still take it (unnamed), because without the callers' dead read
// of it four k_kf6p instantiations (libm, mask, records, fused record) get another register
// allocation (81 -> 89 VGPRs): left for a change that is allowed to alter the compiled code
template <class O>
__device__ __forceinline__ void kf6_load_state(const float *xg, const float *Pg, uint64_t, uint32_t i,
                                               float (&x)[6], float (&P)[21]) {
  constexpr uint32_t W = tile_w<float>();
  const uint32_t tl = (uint32_t)__builtin_amdgcn_readfirstlane(i / W);
  const uint32_t c = (i - tl * W) * 4u;
  const auto rx = rsrc(xg + (uint64_t)tl * (6 * W), 6 * W * 4), rp = rsrc(Pg + (uint64_t)tl * (21 * W), 21 * W * 4);
#pragma unroll
  for (int k = 0; k < 6; k++) x[k] = ld_f32<O::CP>(rx, c, k * W * 4);
#pragma unroll
  for (int k = 0; k < 21; k++) P[k] = ld_f32<O::CP>(rp, c, k * W * 4);
}

// Write-back only where changed.  KF6 has constant F and H and rotates the wheel velocity by the
// MEASURED yaw, so neither update nor predict couples the heading pair (theta, omega) with the
// translation quad (px, py, vx, vy): with a block-diagonal Q, R and P0 (the default tuning) their
// cross-covariance planes stay what they were, tick after tick.  The planes in kKf6SkipMask (bit k
// = packed plane k) are stored only by the lanes whose bit pattern differs from the loaded one, so
// a wave in which no lane changed issues no store and dirties no line; memory holds the same bytes
// either way, for any Q, R and state.  Bits, not floats: -0.0 -> +0.0 and a NaN are written.
// Structural planes only (not those that merely converge under one tuning), so a tick costs the
// same at every step.  The cross planes are 3, 4, 8, 12, 15, 16, 18, 19 (P20 P21 P32 P42 P50 P51
// P53 P54); the default mask is their position half, P20 P21 P50 P51 (profiles/kf6_skip_store_ab.json).
// The mask is a template argument of everything below: an instantiation with Opt's WIDE trait
// takes all eight (kKf6SkipWide), every other one the narrow default (kf6_mask).
#ifndef FMSKF_KF6_SKIP_MASK
#define FMSKF_KF6_SKIP_MASK ((1u << 3) | (1u << 4) | (1u << 15) | (1u << 16))
#endif
constexpr uint32_t kKf6SkipMask = FMSKF_KF6_SKIP_MASK;
constexpr uint32_t kKf6SkipWide = kKf6SkipMask | (1u << 8) | (1u << 12) | (1u << 18) | (1u << 19);
constexpr bool kf6_mask_ok(uint32_t m) { return (m >> 21) == 0 && (m & (uint32_t)kKf6CPM) == 0; }
static_assert(kf6_mask_ok(kKf6SkipMask) && kf6_mask_ok(kKf6SkipWide),
              "packed P planes only, none of the compensated ones");
template <class O>
constexpr uint32_t kf6_mask() {
  return O::WIDE ? kKf6SkipWide : kKf6SkipMask;
}
template <uint32_t M>
constexpr bool kf6_skip(int k) {
  return ((M >> k) & 1u) != 0;
}
template <uint32_t M>
constexpr int kf6_skip_slot(int k) {
  return __builtin_popcount(M & ((1u << k) - 1u));
}
// the loaded bit patterns of the masked planes
template <uint32_t M = kKf6SkipMask>
struct Kf6Old {
  static_assert(kf6_mask_ok(M), "packed P planes only, none of the compensated ones");
  uint32_t v[__builtin_popcount(M) ? __builtin_popcount(M) : 1];
};
template <uint32_t M = kKf6SkipMask>
__device__ __forceinline__ Kf6Old<M> kf6_keep_old(const float (&P)[21]) {
  Kf6Old<M> o;
#pragma unroll
  for (int k = 0; k < 21; k++)
    if (kf6_skip<M>(k)) o.v[kf6_skip_slot<M>(k)] = __builtin_bit_cast(uint32_t, P[k]);
  return o;
}
// plane k of P (k a constant once the callers' loops are unrolled): every lane, or for a masked
// plane the lanes whose bits changed
template <int SP, uint32_t M>
__device__ __forceinline__ void kf6_st_p(__amdgpu_buffer_rsrc_t r, uint32_t voff, uint32_t soff, int k, float v,
                                         const Kf6Old<M> &old) {
  if (kf6_skip<M>(k) && __builtin_bit_cast(uint32_t, v) == old.v[kf6_skip_slot<M>(k)]) return;
  st_f32<SP>(r, voff, soff, v);
}

template <class O, uint32_t M>
__device__ __forceinline__ void kf6_store_state(float *xg, float *Pg, uint64_t, uint32_t i, const float (&x)[6],
                                                const float (&P)[21], const Kf6Old<M> &old) {
  constexpr int SP = st_pol(O::CP);
  constexpr uint32_t W = tile_w<float>();
  const uint32_t tl = (uint32_t)__builtin_amdgcn_readfirstlane(i / W);
  const uint32_t c = (i - tl * W) * 4u;
  const auto rx = rsrc(xg + (uint64_t)tl * (6 * W), 6 * W * 4), rp = rsrc(Pg + (uint64_t)tl * (21 * W), 21 * W * 4);
#pragma unroll
  for (int k = 0; k < 6; k++) st_f32<SP>(rx, c, k * W * 4, x[k]);
#pragma unroll
  for (int k = 0; k < 21; k++) kf6_st_p<SP>(rp, c, k * W * 4, k, P[k], old);
}

// Loads of zeros left out (Opt ZL).  Under a block-diagonal tuning the cross planes are +0.0 in
// every robot at every tick, and the wide write-back mask already stores none of them; the planes
// in kKf6ZeroLoad (a subset of kKf6SkipWide) are then not loaded either.  The handle owns one word
// per 64-robot chunk (Kf6Zero, fmskf_internal.hpp): set = those planes hold the bit pattern 0 in
// memory for every robot of the chunk (-0.0 is not zero here).  A wave's 64 robots, the clamped
// ones included, lie in one chunk, so the word and the branch on it are wave-uniform: a branch
// around the loads, not a select of a loaded value.  The always-needed rows are issued first; a
// skipped plane is +0.0f with 0 as its remembered bits, so compute and write-back are the same
// operations on the same values as after loading the zeros, and memory ends up holding what an
// unconditional tick leaves.  The flags are only as good as the host's knowledge of who wrote P
// since they were rebuilt: the launch says whether it trusts them (ZeroArgs::trusted; the rule is
// in api_ctx.hpp), and an untrusted one loads everything and rewrites every word.
// The mask is all eight cross planes: the largest one with which every KF6-fed row of a --full
// bench line still reads frac <= 0.97 against the 232 B price (headline 0.957; the position half
// alone read 0.924 and gained 1.9 %, less than five times the parent's spread, against 5.4 %;
// profiles/kf6_zero_loads_ab.json).  -DFMSKF_KF6_ZERO_LOAD_MASK builds another subset.
#ifndef FMSKF_KF6_ZERO_LOAD_MASK
#define FMSKF_KF6_ZERO_LOAD_MASK kKf6SkipWide
#endif
constexpr uint32_t kKf6ZeroLoad = FMSKF_KF6_ZERO_LOAD_MASK;
static_assert(kKf6ZeroLoad != 0 && (kKf6ZeroLoad & ~kKf6SkipWide) == 0, "cross planes of the wide mask only");
constexpr uint32_t kZeroChunk = 64;  // robots per flag word: one wave's
// the chunk word of (clamped) robot ic, read through the scalar path: no vmcnt slot
__device__ __forceinline__ uint32_t kf6_zero_flag(const uint32_t *flags, uint32_t ic) {
  return flags[(uint32_t)__builtin_amdgcn_readfirstlane(ic) / kZeroChunk];
}
// kf6_load_state with the kKf6ZeroLoad planes last and, with `skip` (wave-uniform), not at all
template <class O>
__device__ __forceinline__ void kf6_load_state_zl(const float *xg, const float *Pg, uint32_t i, bool skip,
                                                  float (&x)[6], float (&P)[21]) {
  constexpr uint32_t W = tile_w<float>();
  const uint32_t tl = (uint32_t)__builtin_amdgcn_readfirstlane(i / W);
  const uint32_t c = (i - tl * W) * 4u;
  const auto rx = rsrc(xg + (uint64_t)tl * (6 * W), 6 * W * 4), rp = rsrc(Pg + (uint64_t)tl * (21 * W), 21 * W * 4);
#pragma unroll
  for (int k = 0; k < 6; k++) x[k] = ld_f32<O::CP>(rx, c, k * W * 4);
#pragma unroll
  for (int k = 0; k < 21; k++)
    if (!kf6_skip<kKf6ZeroLoad>(k)) P[k] = ld_f32<O::CP>(rp, c, k * W * 4);
  // The zeros are written ahead of the branch, each into a register of its own that the
  // conditional load then overwrites: a zero moved in on the skipping side of the branch would be
  // a write to a register the other side has a load pending on, and the wait the compiler puts in
  // front of it drains every load of the robot (measured in the listing: vmcnt(3) .. vmcnt(0)
  // ahead of the first arithmetic).  Only the listing shows this: look at it again when the
  // compiler changes.  From an asm statement, so that the value is a register like a loaded one
  // and the arithmetic on it is not specialised.
#pragma unroll
  for (int k = 0; k < 21; k++)
    if (kf6_skip<kKf6ZeroLoad>(k)) asm volatile("v_mov_b32 %0, 0" : "=v"(P[k]));
  if (!skip) {
#pragma unroll
    for (int k = 0; k < 21; k++)
      if (kf6_skip<kKf6ZeroLoad>(k)) P[k] = ld_f32<O::CP>(rp, c, k * W * 4);
  }
}
// whether every lane of the wave holds the bit pattern 0 in every kKf6ZeroLoad plane
__device__ __forceinline__ bool kf6_zero_now(const float (&P)[21]) {
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < 21; k++)
    if (kf6_skip<kKf6ZeroLoad>(k)) any |= __builtin_bit_cast(uint32_t, P[k]);
  return __builtin_amdgcn_ballot_w64(any != 0) == 0;
}

// the COMP low-part rows, tiled like x ([N/W][5][W], one scalar descriptor per tile)
template <class O>
__device__ __forceinline__ void kf6_load_lo(const float *lg, uint32_t i, Kf6Lo<O> &l) {
  if constexpr (O::COMP) {
    constexpr uint32_t W = tile_w<float>();
    const uint32_t tl = (uint32_t)__builtin_amdgcn_readfirstlane(i / W);
    const uint32_t c = (i - tl * W) * 4u;
    const auto r = rsrc(lg + (uint64_t)tl * (kKf6LoRows * W), kKf6LoRows * W * 4);
#pragma unroll
    for (int k = 0; k < (int)kKf6LoRows; k++) l.v[k] = ld_f32<O::CP>(r, c, k * W * 4);
  }
}
template <class O>
__device__ __forceinline__ void kf6_store_lo(float *lg, uint32_t i, const Kf6Lo<O> &l) {
  if constexpr (O::COMP) {
    constexpr uint32_t W = tile_w<float>();
    const uint32_t tl = (uint32_t)__builtin_amdgcn_readfirstlane(i / W);
    const uint32_t c = (i - tl * W) * 4u;
    const auto r = rsrc(lg + (uint64_t)tl * (kKf6LoRows * W), kKf6LoRows * W * 4);
#pragma unroll
    for (int k = 0; k < (int)kKf6LoRows; k++) st_f32<st_pol(O::CP)>(r, c, k * W * 4, l.v[k]);
  }
}

// The lane's gate state (fmskf_internal.hpp GateDev): the robot's gate word read and written (the
// tick loop holds it across its ticks), the NIS of the launch's last measurement written when
// there was one -- two plain [N] planes addressed per 256-robot chunk through scalar descriptors
// like the inputs, with the state's cache policy: 12 B per robot-tick on top of the plain tick's
// 232.  The chunk of instance ic (clamped, so in bounds) is wave-uniform, since a wave's lanes --
// the clamped ones included -- lie in one chunk.  Without a gate (ON false) the struct is empty
// and its members compile to nothing.
__device__ __forceinline__ uint32_t gate_chunk(uint32_t ic) {
  return (uint32_t)__builtin_amdgcn_readfirstlane(ic) & ~(uint32_t)(kBlock - 1);
}
template <class O, bool ON_>
struct Kf6Gate {
  static constexpr bool ON = false;
  __device__ __forceinline__ void load(NoGate, uint32_t, uint64_t) {}
  __device__ __forceinline__ void store(NoGate, uint32_t, uint64_t) const {}
};
template <class O>
struct Kf6Gate<O, true> {
  static constexpr bool ON = true;
  static_assert(O::UPD && !O::COMP && !O::ENS, "the gate: plain state, no fused ensemble record");
  uint32_t hb, li, word, word0, max_run;
  float nis_max, nis;
  bool seen;
  __device__ __forceinline__ void load(const GateDev &g, uint32_t ic, uint64_t n) {
    hb = gate_chunk(ic);
    li = ic - hb;
    word = word0 = ld_chunk<uint32_t, O::CP>(g.word, hb, n, li);
    max_run = g.max_run;
    nis_max = g.nis_max;
    nis = 0.f;
    seen = false;
  }
  // a live lane's clamped index is its own, so the slot of the load is the slot of the store;
  // the word (an accepting robot's stays what it was) is written only where it changed
  __device__ __forceinline__ void store(const GateDev &g, uint32_t, uint64_t n) const {
    if (word != word0) st_chunk<uint32_t, st_pol(O::CP)>(g.word, hb, n, li, word);
    if (seen) st_chunk<float, st_pol(O::CP)>(g.nis, hb, n, li, nis);
  }
};
// the gate struct that goes with a kernel's argument type
template <class O, class A>
using Kf6GateOf = Kf6Gate<O, std::is_same<A, GateArgs>::value>;

// copy the sine table to the block's LDS: all global loads first, then the LDS writes, one barrier
template <bool LIBM>
__device__ __forceinline__ void stage_table(float *stab, const float *g) {
  if (!LIBM) {
    const int t = threadIdx.x;
    const float a = g[t], b = g[t + kBlock];
    const float c = t == 0 ? g[2 * kBlock] : 0.f;
    stab[t] = a;
    stab[t + kBlock] = b;
    if (t == 0) stab[2 * kBlock] = c;
    __syncthreads();
  }
}
static_assert(2 * kBlock + 1 == 513, "table staging assumes 256-thread blocks");

// z = (deg2rad(yaw), -deg2rad(gz), wheel velocity rotated by the measured heading)
// (imu_task_main.cpp:102-104, util_mymath.hpp:16, imu_if_wt901c.cpp:113,
//  VD_vehicle_controller.cpp:21-33,47-51); y = z - H x with the heading innovation wrapped
template <bool LIBM>
__device__ __forceinline__ void kf6_innov(const Kf6In &m, const float *tab, const float (&x)[6],
                                          float (&y)[4]) {
  int16_t r[4];
  unpack4(m.rpm, r);
  const float th = deg2rad(m.yaw);
  const float om = -deg2rad(m.gz);
  float vx, vy, vth;
  mdir_to_vdir(rpm_to_mvel(r[0]), rpm_to_mvel(r[1]), rpm_to_mvel(r[2]), rpm_to_mvel(r[3]), vx, vy,
               vth);
  // the sin/cos policies reduce any angle themselves (no normalize_rad_0to2pi needed)
  const float c = cos_p<LIBM>(th, tab), s = sin_p<LIBM>(th, tab);
  const float z2 = (vx * c - vy * s) * 0.001f;
  const float z3 = (vx * s + vy * c) * 0.001f;
  y[0] = wrap_innov(th - x[2]);
  y[1] = om - x[5];
  y[2] = z2 - x[3];
  y[3] = z3 - x[4];
}

// g: the lane's gate state.  With the gate the update is split where the innovation is known:
// S = L D L^T, U = L^-1 H P and w = L^-1 y are formed first (kf_update_factor), the NIS costs
// four more operations on values in registers (kf_nis), and only the apply phase sits behind the
// per-lane decision.  Rejecting lanes skip it, applying lanes run exactly the ungated operations:
// nothing of the applied path depends on the decision, so an applied update is kf_update bit for
// bit and a rejected one is the valid == 0 skip.  g.word is updated; g.nis / g.seen: the NIS of
// this tick's measurement and that there was one (left alone otherwise)
template <class O, class G>
__device__ __forceinline__ void kf6_tick1(const Kf6In &m, const float *tab, const Kf6Params &prm,
                                          float (&x)[6], float (&P)[21], Kf6Lo<O> &l, G &g) {
  if constexpr (G::ON) {
    uint32_t status = FMSKF_GATE_NONE;
    uint32_t run = (g.word >> kGateRunShift) & kGateRunMax, rej = g.word >> kGateRejShift;
    if (!O::VALID || m.valid) {
      float y[4], U[4][6], dinv[4], w[4];
      kf6_innov<O::LIBM>(m, tab, x, y);
      kf_update_factor<MdKF6>(P, y, prm.r, U, dinv, w);
      const float v = kf_nis(w, dinv);
      const bool forced = g.max_run > 0 && run >= g.max_run;
      const bool apply = forced || v <= g.nis_max;
      if (apply) kf_update_apply<MdKF6>(x, P, U, dinv, w);
      status = forced ? FMSKF_GATE_FORCED : apply ? FMSKF_GATE_ACCEPTED : FMSKF_GATE_REJECTED;
      run = apply ? 0u : min(run + 1u, kGateRunMax);
      rej = apply ? rej : min(rej + 1u, kGateRejMax);
      g.nis = v;
      g.seen = true;
    }
    g.word = status | (run << kGateRunShift) | (rej << kGateRejShift);
  } else if (O::UPD && (!O::VALID || m.valid)) {
    float y[4];
    kf6_innov<O::LIBM>(m, tab, x, y);
    if constexpr (O::COMP) kf_update<MdKF6, -1, float, 6, 4, 21, kKf6CXM, kKf6CPM>(x, P, y, prm.r, nullptr, l.v);
    else kf_update<MdKF6>(x, P, y, prm.r);
  }
  if (O::PRED) {
    const float dt = prm.dt;
    if constexpr (O::COMP) {
      th_add(x[0], l.v[0], dt * x[3]);
      th_add(x[1], l.v[1], dt * x[4]);
      th_norm(x[0], l.v[0]);
      th_norm(x[1], l.v[1]);
      x[2] = wrap_pi(dfma(dt, x[5], x[2]));
      kf_predict_cov_c<MdKF6, kKf6CXM, kKf6CPM>(P, [&](int, int) { return dt; }, prm.q, l.v);
    } else {
      x[0] = dfma(dt, x[3], x[0]);
      x[1] = dfma(dt, x[4], x[1]);
      x[2] = wrap_pi(dfma(dt, x[5], x[2]));
      kf_predict_cov<MdKF6>(P, [&](int, int) { return dt; }, prm.q);
    }
  }
}

}  // namespace fmskf
