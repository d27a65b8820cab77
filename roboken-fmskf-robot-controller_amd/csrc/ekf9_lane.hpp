// ekf9_lane.hpp -- one robot's EKF9 tick in registers: the measurement frontend, the raw-record
// load, the optional row-gate state and the update + nonlinear predict, shared by the EKF9 tick
// kernels (kernels_kf.hip, plain and row-gated instantiations) and the fused ISR (k_isr_ekf9).
#pragma once
#include <type_traits>
#include "kf_generic.hpp"

#pragma clang fp contract(off)

namespace fmskf {

// Kernel arguments.  A handle with the per-row innovation gate (fmskf_set_row_gate) launches the
// same tick kernels instantiated on RowGateArgs: the plain arguments embedded unchanged, then the
// gate.
using Ekf9Args = KfArgs<MdEKF9, Ekf9Params>;
struct RowGateArgs {
  Ekf9Args k;
  RowGateDev g;
};
struct NoRowGate {};
__host__ __device__ __forceinline__ const Ekf9Args &kf_args(const Ekf9Args &a) { return a; }
__host__ __device__ __forceinline__ const Ekf9Args &kf_args(const RowGateArgs &a) { return a.k; }
__device__ __forceinline__ NoRowGate gate_dev(const Ekf9Args &) { return {}; }
__device__ __forceinline__ const RowGateDev &gate_dev(const RowGateArgs &a) { return a.g; }

// The lane's row-gate state (fmskf_internal.hpp RowGateDev): one uint64 word per robot (six 2-bit
// statuses, six 8-bit runs: kf_generic.hpp kRowGate*) in a plain [N] plane, read and written once
// per launch (the tick loop holds it across its ticks), and with FMSKF_ROW_GATE_D2 six float
// planes [6][pitch] of the rows' d2, written for robots that had a measurement (after a tick loop:
// the last evaluated values); all addressed per 256-robot chunk through scalar descriptors
// (ld_chunk / st_chunk) with the state's cache policy CP.  16 B per robot-tick on top of the
// plain tick's 456, 40 B with d2.  hb0: the robot's 256-robot chunk (wave-uniform), sl: its slot
// in it.  Without a gate (ON false) the struct is empty and its members compile to nothing.
template <bool ON_, int CP>
struct Ekf9Gate {
  static constexpr bool ON = false;
  __device__ __forceinline__ void load(NoRowGate, uint64_t, uint64_t, uint32_t) {}
  __device__ __forceinline__ void store(NoRowGate, uint64_t, uint64_t, uint32_t) const {}
};
template <int CP>
struct Ekf9Gate<true, CP> {
  static constexpr bool ON = true;
  uint64_t word;
  float d2[6];
  bool seen;
  __device__ __forceinline__ void load(const RowGateDev &g, uint64_t hb0, uint64_t n, uint32_t sl) {
    word = ld_chunk<uint64_t, CP>(g.word, hb0, n, sl);
#pragma unroll
    for (int a = 0; a < 6; a++) d2[a] = 0.f;
    seen = false;
  }
  __device__ __forceinline__ void store(const RowGateDev &g, uint64_t hb0, uint64_t n, uint32_t sl) const {
    st_chunk<uint64_t, st_pol(CP)>(g.word, hb0, n, sl, word);
    if ((g.flags & FMSKF_ROW_GATE_D2) && seen) {
#pragma unroll
      for (int a = 0; a < 6; a++) st_chunk<float, st_pol(CP)>(g.d2 + a * g.d2_pitch, hb0, n, sl, d2[a]);
    }
  }
};
// the gate struct that goes with a kernel's argument type
template <class A, int CP>
using Ekf9GateOf = Ekf9Gate<std::is_same<A, RowGateArgs>::value, CP>;

// EKF9 z from raw WT901 registers (imu_if_wt901c.cpp:96-99,107-113) + wheel rpm; the heading
// innovation against the compensated heading x[2] + lo
__device__ __forceinline__ void ekf9_innov(const uint4 w, const float (&x)[9], float lo, float (&y)[6]) {
  int16_t a[4], r[4];
  unpack4(make_uint2(w.x, w.y), a);
  unpack4(make_uint2(w.z, w.w), r);
  const float yaw = (float)a[0] / 32768.0f * 180.0f;
  const float gz = (float)a[1] / 32768.0f * 2000.0f;
  const float ax = (float)a[2] / 32768.0f * 16.0f;
  const float ay = -((float)a[3] / 32768.0f * 16.0f);
  float vx, vy, vth;
  mdir_to_vdir(rpm_to_mvel(r[0]), rpm_to_mvel(r[1]), rpm_to_mvel(r[2]), rpm_to_mvel(r[3]), vx, vy,
               vth);
  const float z0 = deg2rad(yaw), z1 = deg2rad(gz), z2 = ax * K::g0, z3 = ay * K::g0;
  const float z4 = vx * 0.001f, z5 = vy * 0.001f;
  y[0] = wrap_innov((z0 - x[2]) - lo);
  y[1] = z1 - (x[5] + x[6]);
  y[2] = z2 - x[7];
  y[3] = z3 - x[8];
  y[4] = z4 - x[3];
  y[5] = z5 - x[4];
}

// one robot's 16-byte raw record of a single tick, read once; NT: non-temporal (gfx950 `nt`).
// Measured (kbench, one box, two passes): 2^20 (two robots per lane) 74.1-74.2 -> 73.0-73.4 us
// with nt; 2^22 (one per lane, HBM) 334.6-335.6 plain vs 337.5-338.3 nt: k_ekf9p uses nt,
// k_ekf9t plain loads
template <bool NT>
__device__ __forceinline__ uint4 ekf9_raw_at(const int16_t *raw, uint64_t i) {
  if constexpr (NT) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    const u32x4 v = __builtin_nontemporal_load(reinterpret_cast<const u32x4 *>(raw) + i);
    return make_uint4(v[0], v[1], v[2], v[3]);
  } else {
    return reinterpret_cast<const uint4 *>(raw)[i];
  }
}

// one EKF9 tick (update with the measurement frontend, then the nonlinear predict)
// SEQ: R is diagonal -> the sequential scalar update (kf_update_seq), else the joint LDL^T one
// lo: the compensated heading's low part (th_add, kf_generic.hpp)
// COMP: FMSKF_CFG_COMP_POS -- px, py, P00, P10, P11 compensated too (cl: their five low parts;
// oracle orc_ekf9_tick_comp)
// gt: the lane's row-gate state.  With the gate each scalar row of the sequential update sits
// behind its own decision (kf_update_seq_gated): d2 = y * (y / s) is one more product on values
// the row already holds, a rejecting lane branches around the row's x / y / P sub-loops, an
// applying lane runs exactly the ungated operations.  So an update with every row applied is
// kf_update_seq bit for bit, one with every row rejected is the valid == 0 skip, and any other
// pattern is the ungated update with R[a][a] = +inf on the rejected rows (up to the sign of a
// zero).  gt.word is updated (a call without a measurement clears the statuses and keeps the
// runs); gt.d2 / gt.seen: the rows' d2 of this tick's measurement and that there was one
template <bool LIBM, bool UPD, bool PRED, bool SEQ, bool COMP = false, class A, class G>
__device__ __forceinline__ void ekf9_tick1(const A &aa, const uint4 raw, bool have, const float *stab,
                                           float (&x)[9], float (&P)[45], float &lo, float *cl, G &gt) {
  constexpr unsigned CXM = COMP ? kPosCXM : 0u;
  constexpr unsigned long long CPM = COMP ? kPosCPM : 0ull;
  const Ekf9Args &a = kf_args(aa);
  const float dt = a.prm.dt;
  if constexpr (G::ON) {
    static_assert(UPD && SEQ && !COMP, "the row gate: diagonal R, plain state");
    if (have) {
      float y[6];
      ekf9_innov(raw, x, lo, y);
      kf_update_seq_gated<MdEKF9, 2>(x, P, y, a.prm.r, gate_dev(aa).d2_max, gate_dev(aa).max_run, gt.word, gt.d2,
                                     &lo);
      th_norm(x[2], lo);
      gt.seen = true;
    } else {
      gt.word &= ~kRowGateStatusMask;
    }
  } else if (UPD && have) {
    float y[6];
    ekf9_innov(raw, x, lo, y);
    if constexpr (SEQ) kf_update_seq<MdEKF9, 2, float, 9, 6, 45, CXM, CPM>(x, P, y, a.prm.r, &lo, cl);
    else kf_update<MdEKF9, 2, float, 9, 6, 45, CXM, CPM>(x, P, y, a.prm.r, &lo, cl);
    th_norm(x[2], lo);
  }
  if (PRED) {
    // f(x): mecanum body velocity rotated into the world frame (the reference's
    // odometry, VD_vehicle_controller.cpp:47-51, generalised) + its Jacobian
    const float rr = normalize_rad_0to2pi(x[2]);
    const float c = cos_p<LIBM>(rr, stab), s = sin_p<LIBM>(rr, stab);
    const float vwx = x[3] * c - x[4] * s;
    const float vwy = x[3] * s + x[4] * c;
    const float f02 = -(vwy * dt), f03 = c * dt, f04 = -(s * dt);
    const float f12 = vwx * dt, f13 = s * dt, f14 = c * dt;
    if constexpr (COMP) {
      th_add(x[0], cl[0], vwx * dt);
      th_add(x[1], cl[1], vwy * dt);
      th_norm(x[0], cl[0]);
      th_norm(x[1], cl[1]);
    } else {
      x[0] = x[0] + vwx * dt;
      x[1] = x[1] + vwy * dt;
    }
    th_add(x[2], lo, x[5] * dt);
    wrap_pi_c(x[2], lo);
    th_norm(x[2], lo);
    x[3] = x[3] + x[7] * dt;
    x[4] = x[4] + x[8] * dt;
    auto fv = [&](int r, int k) -> float {
      if (r == 0) return k == 2 ? f02 : k == 3 ? f03 : f04;
      if (r == 1) return k == 2 ? f12 : k == 3 ? f13 : f14;
      return dt;
    };
    if constexpr (COMP) kf_predict_cov_c<MdEKF9, kPosCXM, kPosCPM>(P, fv, a.prm.q, cl);
    else kf_predict_cov<MdEKF9>(P, fv, a.prm.q);
  }
}

}  // namespace fmskf
