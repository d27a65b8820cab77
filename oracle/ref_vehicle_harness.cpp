/*
 * ref_vehicle_harness.cpp -- driver around the REFERENCE's own VDT::VEHICLE_CTRL,
 * VDT::MOTOR_IF_M2006 and UTIL::VelInterpConstJerk (src/VehicleDrive/VD_vehicle_controller.cpp,
 * VD_motor_if_m2006.cpp, src/Utility/util_vel_interp.hpp, util_mymath.hpp, with the
 * util_controller.hpp / util_iir.hpp they include), compiled unmodified from /root/reference by
 * oracle/Makefile into oracle/_ref/libvehicle_ref.so.
 *
 * TEST INFRASTRUCTURE ONLY.  Two stand-in headers (oracle/ref_standin/global_config.hpp and
 * arm_math.h) replace Arduino.h and CMSIS-DSP: fixed-width integers, PI, arm_sqrt_f32 as the
 * correctly rounded square root, and arm_sin_f32 / arm_cos_f32 forwarded to the oracle's own
 * table restatement (so the table algorithm is NOT pinned by anything this harness records).
 *
 * The harness builds the objects the way VD_task_main.cpp:75-108,157-160 does (four motor
 * interfaces, four FF_PI_D, three constant-jerk interpolators, one VEHICLE_CTRL over a Parts
 * record, set_FF_limit on the four controllers), with the caller's motor directions, gains,
 * limits and current limit.  The firmware's objects are statics, i.e. zeroed before their
 * constructors run, and VEHICLE_CTRL, MOTOR_IF_M2006::Status and s16_rawCurr_tgt have members
 * no constructor writes: the objects are therefore constructed in calloc'ed storage.
 */
#include <stdint.h>
#include <stdlib.h>

#include <new>

#include "VD_vehicle_controller.hpp"
#include "../Utility/util_mymath.hpp"

using namespace VDT;

namespace {

struct Vehicle {
  MOTOR_IF_M2006 *motor[4];
  UTIL::FF_PI_D *ctrl[4];
  UTIL::VelInterpConstJerk *interp[3];
  VEHICLE_CTRL::Parts *parts;
  VEHICLE_CTRL *vhcl;
  void *mem[13];
  int nmem;
};

template <class T> void *zeroed(Vehicle *v) {
  void *p = calloc(1, sizeof(T));
  v->mem[v->nmem++] = p;
  return p;
}

}  // namespace

extern "C" {

void *ref_vehicle_new(const int8_t dir[4], float ctrl_freq_hz, float ff_gain, float p_gain,
                      float i_gain, float d_gain, float i_limit, float lpf_freq_hz, float ff_limit,
                      float interp_ts, int16_t curr_limit_raw) {
  Vehicle *v = (Vehicle *)calloc(1, sizeof(Vehicle));
  for (int w = 0; w < 4; w++) {
    v->motor[w] = new (zeroed<MOTOR_IF_M2006>(v)) MOTOR_IF_M2006(dir[w]);
    v->motor[w]->set_rawCurr_lim(curr_limit_raw);
    v->ctrl[w] = new (zeroed<UTIL::FF_PI_D>(v))
        UTIL::FF_PI_D(ctrl_freq_hz, ff_gain, p_gain, i_gain, d_gain, i_limit, lpf_freq_hz);
    v->ctrl[w]->set_FF_limit(ff_limit);
  }
  for (int a = 0; a < 3; a++)
    v->interp[a] = new (zeroed<UTIL::VelInterpConstJerk>(v)) UTIL::VelInterpConstJerk(interp_ts);
  v->parts = (VEHICLE_CTRL::Parts *)zeroed<VEHICLE_CTRL::Parts>(v);
  for (int a = 0; a < 3; a++) v->parts->p_vel_interp[a] = v->interp[a];
  for (int w = 0; w < 4; w++) {
    v->parts->p_motor[w] = v->motor[w];
    v->parts->p_ctrl[w] = v->ctrl[w];
  }
  v->vhcl = new (zeroed<VEHICLE_CTRL>(v)) VEHICLE_CTRL(*v->parts);
  return v;
}

void ref_vehicle_free(void *h) {
  Vehicle *v = (Vehicle *)h;
  for (int k = 0; k < v->nmem; k++) free(v->mem[k]); /* trivially destructible members only */
  free(v);
}

/* CAN_CTRL's receive path: one C610 feedback frame of wheel w (FL, BL, BR, FR) with its stamp */
void ref_vehicle_rx(void *h, int w, const uint8_t frame[8], int16_t stamp) {
  MOTOR_IF_M2006::CanMsgRx msg;
  msg.u8_angle_h = frame[0];
  msg.u8_angle_l = frame[1];
  msg.u8_speed_h = frame[2];
  msg.u8_speed_l = frame[3];
  msg.u8_curr_h = frame[4];
  msg.u8_curr_l = frame[5];
  msg.u8_rsev[0] = frame[6];
  msg.u8_rsev[1] = frame[7];
  ((Vehicle *)h)->motor[w]->rx_callback(&msg, stamp);
}

void ref_vehicle_power(void *h, int on) {
  if (on) ((Vehicle *)h)->vhcl->start();
  else ((Vehicle *)h)->vhcl->stop();
}

void ref_vehicle_set_target_vel(void *h, const float vel[3], const float acl[3], const float jrk[3]) {
  Direction v = {vel[0], vel[1], vel[2]}, a = {acl[0], acl[1], acl[2]}, j = {jrk[0], jrk[1], jrk[2]};
  ((Vehicle *)h)->vhcl->set_target_vel(v, a, j);
}

/* VDT::can_tx_routine_intr's estimator + control part: the IMU yaw in degrees through the
 * reference's own deg2rad into set_now_yaw_world, then update() */
void ref_vehicle_tick(void *h, float yaw_deg) {
  Vehicle *v = (Vehicle *)h;
  v->vhcl->set_now_yaw_world(UTIL::mymath::deg2rad(yaw_deg));
  v->vhcl->update();
}

/* pose (m, m, rad), vel (mm/s, mm/s, rad/s), vel_tgt, get_rawCurr_tgt x4, get_rawAngleSum x4 and
 * get_status_latest x4: st_i16 [4][4] = microsec_id, rawAngle, rawSpeedRpm, rawCurr per wheel,
 * st_f32 [4][2] = dltOutAngle_rad, SpeedRadPS per wheel */
void ref_vehicle_read(void *h, float pose[3], float vel[3], float vel_tgt[3], int16_t curr[4],
                      int64_t sum[4], int16_t st_i16[16], float st_f32[8]) {
  Vehicle *v = (Vehicle *)h;
  Direction d;
  v->vhcl->get_vehicle_pos_m_latest(d);
  pose[0] = d.x, pose[1] = d.y, pose[2] = d.th;
  v->vhcl->get_vehicle_vel_mmps_latest(d);
  vel[0] = d.x, vel[1] = d.y, vel[2] = d.th;
  v->vhcl->get_vehicle_vel_tgt_mmps_latest(d);
  vel_tgt[0] = d.x, vel_tgt[1] = d.y, vel_tgt[2] = d.th;
  for (int w = 0; w < 4; w++) {
    curr[w] = v->motor[w]->get_rawCurr_tgt();
    sum[w] = v->motor[w]->get_rawAngleSum();
    MOTOR_IF_M2006::Status s;
    v->motor[w]->get_status_latest(s);
    st_i16[4 * w + 0] = s.s16_microsec_id;
    st_i16[4 * w + 1] = s.s16_rawAngle;
    st_i16[4 * w + 2] = s.s16_rawSpeedRpm;
    st_i16[4 * w + 3] = s.s16_rawCurr;
    st_f32[2 * w + 0] = s.flt_dltOutAngle_rad;
    st_f32[2 * w + 1] = s.flt_SpeedRadPS;
  }
}

}  // extern "C"
