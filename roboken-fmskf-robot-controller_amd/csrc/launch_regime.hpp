// launch_regime.hpp -- what the tick and ISR launchers decide from, stated once: the bytes per
// robot of every model's state, the Infinity Cache budget, the read-once environment knobs and the
// launch regimes built on them.  Host only, nothing from HIP (tests/native/regime_table.cpp builds
// it with a plain C++ compiler); fmskf_internal.hpp includes it.
#pragma once
#include <cstdint>
#include <cstdlib>
#include "../../include/fmskf.h"

namespace fmskf {

// ---------------------------------------------------------------------------
// environment knobs
// ---------------------------------------------------------------------------
inline const char *env_knob(const char *name) { return getenv(name); }
// an integer knob, read once per call site; DFLT while unset
#define FMSKF_ENV_INT(NAME, DFLT)                       \
  ([]() -> int {                                        \
    static const int v_ = [] {                          \
      const char *e_ = ::fmskf::env_knob(NAME);         \
      return e_ ? atoi(e_) : (int)(DFLT);               \
    }();                                                \
    return v_;                                          \
  }())
// Occupancy cap for the kernels that stream their state from HBM: dynamic LDS per block limits
// the resident blocks per CU (160 KiB / bytes), so fewer tile / plane streams compete for the
// HBM channels.  The environment variable (read once per call site) overrides the byte count.
#define FMSKF_LDS_CAP(NAME, HBM, DFLT)                                 \
  ([&]() -> unsigned {                                                 \
    const int v_ = FMSKF_ENV_INT(NAME, -1);                            \
    return v_ >= 0 ? (unsigned)v_ : ((HBM) ? (unsigned)(DFLT) : 0u);   \
  }())

// ---------------------------------------------------------------------------
// bytes per robot
// ---------------------------------------------------------------------------
constexpr uint32_t kKf6LoRows = 5;  // FMSKF_CFG_COMP_POS: the low parts of px, py, P00, P10, P11
// x (nx rows) and the packed symmetric P of one robot
constexpr uint64_t xp_bytes(uint64_t nx, uint64_t elem) { return (nx + nx * (nx + 1) / 2) * elem; }
// KF6: + the low-part rows under COMP, + the gate word and the NIS of a gated handle
constexpr uint64_t kf6_state_bytes(bool comp, bool gated = false) {
  return xp_bytes(6, 4) + (comp ? kKf6LoRows * 4 : 0) + (gated ? 4 + 4 : 0);
}
constexpr uint64_t kKf6InBytes = 16;  // one tick's KF6 inputs: yaw, gyro z, four int16 rpm
// EKF9: + the heading's low part (thlo), + the low-part rows under COMP, + the row-gate word
constexpr uint64_t ekf9_state_bytes(bool comp, bool gated = false) {
  return xp_bytes(9, 4) + 4 + (comp ? kKf6LoRows * 4 : 0) + (gated ? 8 : 0);
}
constexpr uint64_t kKf12dStateBytes = xp_bytes(12, 8);
// RS: x (six floats) and the four previous encoder sums
constexpr uint64_t kRsStateBytes = 6 * 4 + 4 * 8;
// The RS tick's algorithmic bytes per robot-tick, which launch_rs holds against the cache: the
// three pose floats and the four previous sums read and written, the four new sums and the yaw
// read (the tick also reads the rpm and writes the velocities, which are not counted)
constexpr uint64_t kRsTickBytes = 2 * (3 * 4 + 4 * 8) + 4 * 8 + 4;
// the motor state (CAN RX) and one tick's CAN frames and stamps
constexpr uint64_t kMotorStateBytes = 66, kCanInBytes = 40;
static_assert(kf6_state_bytes(false) == 108 && kf6_state_bytes(false, true) == 116 && kf6_state_bytes(true) == 128, "");
static_assert(ekf9_state_bytes(false) == 220 && ekf9_state_bytes(false, true) == 228 && ekf9_state_bytes(true) == 240, "");
static_assert(kKf12dStateBytes == 720 && kRsStateBytes == 56 && kRsTickBytes == 124, "");
static_assert(kf6_state_bytes(false) + kKf6InBytes == 124, "");

// bytes per robot of a handle's estimator state (x, P and the hidden low-part rows): the part
// of the working set the ingest kernels' cache policies have to leave room for
constexpr uint64_t est_state_bytes(uint32_t model, bool comp) {
  return model == FMSKF_MODEL_RS ? kRsStateBytes
         : model == FMSKF_MODEL_KF6 ? kf6_state_bytes(comp)
         : model == FMSKF_MODEL_EKF9 ? ekf9_state_bytes(comp)
                                     : kKf12dStateBytes;
}

// ---------------------------------------------------------------------------
// the cache budget
// ---------------------------------------------------------------------------
constexpr uint64_t kInfinityCacheBytes = 256ull << 20;
constexpr bool fits_cache(uint64_t bytes) { return bytes <= kInfinityCacheBytes; }
constexpr bool fits_half_cache(uint64_t bytes) { return bytes <= kInfinityCacheBytes / 2; }

// Cache policy of the per-tick state stream.  When the state is several times the 256 MiB
// Infinity Cache, every state byte is read once and written once per tick from HBM; loading
// and storing it non-temporal (gfx950 `nt`, buffer aux bit 1) measured 15% faster on the
// tiled pattern at 2^22 EKF9 robots (tools/membench.hip: 352 -> 299 us), while it is slower
// when the state fits the Infinity Cache.  FMSKF_STATE_NT=0|1 forces it off or on.
inline bool state_nt(uint64_t state_bytes) {
  const int force = FMSKF_ENV_INT("FMSKF_STATE_NT", -1);
  if (force >= 0) return force != 0;
  return !fits_cache(state_bytes);
}

// ---------------------------------------------------------------------------
// launch regimes: two robots per lane or one, whether the state streams past the caches (nt), the
// dynamic-LDS occupancy cap
// ---------------------------------------------------------------------------
struct LaunchRegime {
  bool two, nt;
  unsigned lds;
};

// Variant (FMSKF_KF6_VARIANT, read once) for single-tick launches; default 0:
//   0: k_kf6p with 2 robots per lane while 124 B x N fits the Infinity Cache, else 15
//   15: one instance per lane, grid = N/256, straight-line single-tick kernel (k_kf6t)
//   12: k_kf6p with 2 robots per lane at any N
// (the tests force 12 / 15 at small N to check both kernels).  Measured and removed: 3 or 4
// robots per lane (38.0 us at 2^20 against 37.4-38.6 for 2), the single tick through the
// tick-loop kernel, and persistent double-buffered kernels at 2-8 blocks per CU (5-20% slower).
inline int kf6_variant() {
  const int x = FMSKF_ENV_INT("FMSKF_KF6_VARIANT", 0);
  return x == 12 || x == 15 ? x : 0;
}

// The launch regime of a single KF6 tick / predict / correct, shared by the plain and the gated
// handles.  nt tests the state alone (with the gate word and NIS where there are any), two the
// state plus one tick's inputs.  The gated family has no streamed two-per-lane kernel: its
// streamed state always goes one robot per lane
inline LaunchRegime kf6_regime(uint64_t n, bool comp, bool gated, bool rec) {
  const int v = kf6_variant();
  const uint64_t sb = kf6_state_bytes(comp, gated), rb = sb + kKf6InBytes;
  const bool nt = state_nt(n * sb);
  if ((!gated || !nt) && (v == 12 || (v == 0 && fits_cache(n * rb)))) {
    // state + one tick's inputs resident in the 256 MiB Infinity Cache: two robots per lane,
    // both robots' inputs loaded up front, one wave round (2^20: 39.7 -> 37.4-38.1 us,
    // 2^21: 75.9 -> 71.5; at 2^24, HBM-bound, it is 3% slower than one robot per lane)
    if (v == 12) return {true, nt, 0u};
    // 32 KiB of dynamic LDS: at most 5 blocks per CU.  kbench, records, two passes: 2^20
    // 38.2-38.5 -> 37.2-37.3 us (24 KiB 37.6-37.7, 40 KiB 37.4-37.5); 2^21 71.6-71.8 -> 70.5-70.9.
    // Records fed while state + inputs fill at most half the cache (2^20 robots): 48 KiB, 3
    // blocks per CU (round 3, kbench, three alternating passes on one box: 32 KiB 36.99-37.14 us,
    // 48 KiB 36.67-36.93, 64 KiB 36.61-36.97, 80 KiB 44.0, uncapped 38.0).  Plane inputs and
    // 2^21 records stay at 32 KiB (48 KiB: 2^20 planes 37.49 -> 37.72-38.07, 2^21 records
    // 68.3-68.4 -> 69.0, 2^21 planes 69.5-69.7 -> 71.2-71.4)
    const bool rec_half = rec && fits_half_cache(n * rb);
    return {true, nt, FMSKF_LDS_CAP("FMSKF_KF6P_LDS", true, rec_half ? 48u * 1024u : 32u * 1024u)};
  }
  // past the Infinity Cache: at most 3 blocks per CU (48 KiB of dynamic LDS).  2^24, records,
  // kbench, one box, two passes: 691-704 us uncapped, 671-684 at 32 KiB, 627-641 at 48 KiB,
  // 626-639 at 64 KiB, 809-826 at 80 KiB (two blocks of 4 waves per CU are too few)
  return {false, nt, FMSKF_LDS_CAP("FMSKF_KF6_LDS", nt, 48u * 1024u)};
}

// Which write-back mask a two-per-lane full tick (ungated, not COMP) takes: the eight cross planes
// (Opt WIDE) while state + one tick's inputs fill at most half the Infinity Cache, the position
// half past that.  The split is NOT the hardware's: the wide mask measured faster at 2^21 and 2^24
// too (profiles/kf6_skip_store_ab.json).  It is the roofline check's: tests/test_gpu_bench_line.py
// prices every KF6 row at the algorithmic 232 B per robot-tick and wants the row below that model's
// bandwidth ceiling, and the project holds every KF6-fed row of a --full line to frac <= 0.97.
// With the wide mask the 2^21 shard row read 0.983; the headline regime has room (0.913;
// profiles/kf6_half_cache_ab.json).
// FMSKF_KF6_SKIP_WIDE (read once): 0 narrow in every regime, 1 wide in every two-per-lane full
// tick, unset by the regime.
inline bool kf6_wide(uint64_t n) {
  const int force = FMSKF_ENV_INT("FMSKF_KF6_SKIP_WIDE", -1);
  if (force == 0 || force == 1) return force == 1;
  return fits_half_cache(n * (kf6_state_bytes(false) + kKf6InBytes));
}

// Whether a two-per-lane full tick (ungated, not COMP) with the wide mask also leaves out the loads
// of the cross planes its wave is known to hold zero (Opt ZL, kf6_lane.hpp kKf6ZeroLoad): the
// half-cache regime of kf6_wide, for the same reason -- the headline row has room under the 232 B
// price for the bytes no longer fetched (frac 0.901 -> 0.957), the rows past half the cache have
// less (the 2^21 shard row reads 0.93 as it is; profiles/kf6_zero_loads_ab.json).  The launcher asks only where the wide
// mask is taken, a direct launch has the handle's flags and the tuning can keep the planes zero.
// FMSKF_KF6_ZERO_LOADS (read once): 0 off, 1 on wherever the wide mask is taken, unset by the regime.
// The flag kernels exist with the wide mask only, and the knob does not move kf6_wide: past half
// the cache 1 alone changes nothing, with FMSKF_KF6_SKIP_WIDE=1 it reaches every two-per-lane full tick.
inline bool kf6_zero_loads(uint64_t n) {
  const int force = FMSKF_ENV_INT("FMSKF_KF6_ZERO_LOADS", -1);
  if (force == 0 || force == 1) return force == 1;
  return fits_half_cache(n * (kf6_state_bytes(false) + kKf6InBytes));
}

// The fused KF6 tick + ensemble record: two per lane while state + one tick's inputs fit the
// cache, nt on the state alone.  FMSKF_KF6_VARIANT is not consulted here
inline LaunchRegime kf6_ens_regime(uint64_t n, bool comp) {
  const uint64_t sb = kf6_state_bytes(comp);
  const bool nt = state_nt(n * sb);
  // 32 KiB in every regime, not the plain record-fed tick's 48 KiB at 2^20 (kf6_regime): the
  // record epilogue wants the fifth block per CU.  kbench ens_async, records, 2^20, three
  // alternating passes on one box: K = 1 36.18-36.37 us per tick at 32 KiB against 38.08-38.20 at
  // 48 KiB; the bench's K = 16 region shape (20 ticks, one event) 34.29-34.47 against 34.47-34.49
  if (fits_cache(n * (sb + kKf6InBytes))) return {true, nt, FMSKF_LDS_CAP("FMSKF_KF6PE_LDS", true, 32u * 1024u)};
  // past the Infinity Cache the record epilogue (fp64 sums and their cross-lane reduction)
  // wants a smaller cap than the plain tick: 2^24, kbench, two passes: 738 us at 48 KiB,
  // 665-670 at 32 KiB, 680-689 at 24 KiB, 722-724 uncapped (the plain tick: 619-628)
  return {false, nt, FMSKF_LDS_CAP("FMSKF_KF6E_LDS", nt, 32u * 1024u)};
}

// The launch regime of a single full EKF9 tick, shared by the plain and the row-gated handles: two
// robots per lane (k_ekf9p) while the state alone -- with the gate word where there
// is one -- fits the 256 MiB Infinity Cache, else one per lane (k_ekf9t); FMSKF_EKF9_VARIANT
// (read once) forces one of them, 2 = k_ekf9p, 4 = k_ekf9t (the tests' cross-check at small N).
// Measured (kbench, one box, two passes): 2^20 k_ekf9t 74.8-74.9 us, k_ekf9p 71.2-71.9; 2^22
// (HBM) k_ekf9t 336-338, k_ekf9p 339.  A raised-priority load phase (s_setprio 3 while issuing
// the loads) measured 71.2-73.9 at 2^20 and 342-343 at 2^22 and was removed.
inline LaunchRegime ekf9_regime(uint64_t n, bool comp, bool gated, bool libm) {
  const uint64_t sb = ekf9_state_bytes(comp, gated);
  const bool nt = state_nt(n * sb);
  const int var = FMSKF_ENV_INT("FMSKF_EKF9_VARIANT", 0);
  const int v = var == 2 || var == 4 ? var : (fits_cache(n * sb) ? 2 : 4);
  // 64 KiB of dynamic LDS (2 blocks per CU): 2^20 71.2 -> 70.5-70.7 us (two passes)
  if (!libm && v == 2) return {true, nt, FMSKF_LDS_CAP("FMSKF_EKF9P_LDS", true, 64u * 1024u)};
  if (libm) return {false, nt, 0u};
  // Past the Infinity Cache (non-temporal state) the occupancy is capped at 2 blocks per CU
  // with 64 KiB of dynamic LDS: fewer concurrent tile streams per HBM channel.  2^22:
  // 334.3-338.7 us uncapped, 332 at 32 KiB, 329.7-331.0 at 48 KiB, 326.8-330.9 at 64 KiB,
  // 382-383 at 80 KiB (kbench, two boxes, two passes each); the same-bytes tiled pattern
  // (membench) 299 us.  FMSKF_EKF9_LDS overrides the byte count.
  return {false, nt, FMSKF_LDS_CAP("FMSKF_EKF9_LDS", nt, 64u * 1024u)};
}

// The fused EKF9 tick + ensemble record: both tests on the state alone.  FMSKF_EKF9_VARIANT is
// not consulted here
inline LaunchRegime ekf9_ens_regime(uint64_t n, bool comp, bool libm) {
  const uint64_t sb = ekf9_state_bytes(comp);
  const bool nt = state_nt(n * sb);
  if (!libm && fits_cache(n * sb)) return {true, nt, FMSKF_LDS_CAP("FMSKF_EKF9P_LDS", true, 64u * 1024u)};
  // past the Infinity Cache the record epilogue (fp64 sums and their cross-lane reduction)
  // wants one more block per CU than the plain tick: 2^22, kbench, two passes: 331-335 us at
  // 64 KiB (2 blocks per CU), 307-308 at 32 KiB (3), 316 uncapped
  return {false, nt, libm ? 0u : FMSKF_LDS_CAP("FMSKF_EKF9E_LDS", nt, 32u * 1024u)};
}

// KF12D: always one robot per lane; nt on the state alone (the cap applies to the plain full tick)
inline LaunchRegime kf12d_regime(uint64_t n) {
  const bool nt = state_nt(n * kKf12dStateBytes);
  return {false, nt, FMSKF_LDS_CAP("FMSKF_KF12D_LDS", nt, 0u)};
}

// The fused RS correct + predict: two robots per lane unless FMSKF_RS_TWO=0 (A/B switch: one
// robot per lane); nt on the tick's algorithmic bytes (kRsTickBytes)
inline LaunchRegime rs_regime(uint64_t n) {
  const bool nt = state_nt(n * kRsTickBytes);
  // past the Infinity Cache: 2 blocks per CU (64 KiB of dynamic LDS).  2^24, kbench, two
  // passes: 436.7-448.2 us uncapped, 429-430 at 48 KiB, 418.5-424.5 at 64 KiB
  return {FMSKF_ENV_INT("FMSKF_RS_TWO", 1) != 0, nt, FMSKF_LDS_CAP("FMSKF_RS_LDS", nt, 64u * 1024u)};
}

}  // namespace fmskf
