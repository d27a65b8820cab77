// ekf9_lane.hpp -- one robot's EKF9 tick in registers: the measurement frontend, the raw-record
// load and the update + nonlinear predict, shared by the plain tick kernels (kernels_kf.hip) and
// the row-gated ones (kernels_rowgate.hip).
#pragma once
#include "kf_generic.hpp"

#pragma clang fp contract(off)

namespace fmskf {

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
template <bool LIBM, bool UPD, bool PRED, bool SEQ, bool COMP = false>
__device__ __forceinline__ void ekf9_tick1(const KfArgs<MdEKF9, Ekf9Params> &a, const uint4 raw,
                                           bool have, const float *stab, float (&x)[9],
                                           float (&P)[45], float &lo, float *cl = nullptr) {
  constexpr unsigned CXM = COMP ? kPosCXM : 0u;
  constexpr unsigned long long CPM = COMP ? kPosCPM : 0ull;
  const float dt = a.prm.dt;
  if (UPD && have) {
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
