/*
 * fmskf.h -- C ABI of the MI355X batched state-estimation engine (libfmskf.so).
 *
 * Drop-in for the IMU + mecanum-odometry fusion path of
 * Moryu-Io/Roboken-FMSKF-robot-controller, batched over N independent robots
 * ("instances").  Every per-tick entry point keeps the reference's per-tick call
 * shape (src/VehicleDrive/VD_task_main.cpp:366-372):
 *
 *     can_tx_routine_intr():  set_now_yaw_world(deg2rad(IMT::get_status_now_yaw()));   -> fmskf_correct
 *                             vhclCtrl.update();                                          -> fmskf_predict
 *                             (fused: fmskf_tick)
 *
 * Plain C: opaque handle, plain pointers and sizes, int status codes, no torch
 * types, no exceptions across the boundary.  All arrays are caller-owned; the
 * library never retains a caller pointer after a call returns.  Arrays are
 * "planes" (structure of arrays): plane k of an array with N instances starts
 * at element k*N.  `mem` says whether the caller's pointers are host
 * (FMSKF_MEM_HOST) or device (FMSKF_MEM_DEVICE, on the handle's device).
 *
 * Tick entry points are asynchronous on the handle's HIP stream
 * (fmskf_set_stream); fmskf_sync waits for them.  One handle per host thread;
 * distinct handles are independent.
 *
 * Reference interfaces replaced (file:line in the reference repository):
 *   IMT::IMU_IF / IMU_IF_WT901C          src/Imu/imu_if_base.hpp:8-32, imu_if_wt901c.hpp:8-42
 *   IMT::get_status_now_yaw / _imu       src/Imu/imu_task_main.cpp:86-104
 *   WIT SDK byte input                   lib/wt901c/wit_c_sdk.c:132-198
 *   VDT::MOTOR_IF_M2006::rx_callback     src/VehicleDrive/VD_motor_if_m2006.cpp:32-72
 *   VDT::VEHICLE_CTRL::set_now_yaw_world src/VehicleDrive/VD_vehicle_controller.hpp:57
 *   VDT::VEHICLE_CTRL::update (odometry) src/VehicleDrive/VD_vehicle_controller.cpp:6-51
 *   VEHICLE_CTRL::get_vehicle_*_latest   src/VehicleDrive/VD_vehicle_controller.hpp:59-60
 *   VDT::get_status_now_vehicle_pos_world/vel  src/VehicleDrive/VD_task_main.cpp:374-395
 *   VEHICLE_CTRL::update (control part)  src/VehicleDrive/VD_vehicle_controller.cpp:53-98
 *   VEHICLE_CTRL::set_target_vel/start/stop  VD_vehicle_controller.cpp:100-104, .hpp:54-55
 *   UTIL::VelInterpConstJerk / FF_PI_D   src/Utility/util_vel_interp.hpp:25-157,
 *                                        util_controller.hpp:92-186, util_iir.hpp:13-57
 *   CAN_CTRL::tx_routine                 src/VehicleDrive/VD_can_controller.hpp:43-55
 *   VehicleInfo publish                  src/RobotManager/RM_task_main.cpp:772-823
 */
#ifndef FMSKF_H_
#define FMSKF_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3: fmskf_tick_inputs.angle_sum_pitch (the former unchecked `reserved` word), fmskf_config.flags,
 * the asynchronous ensemble entry points, fmskf_comm_info, fmskf_get_motor_status */
#define FMSKF_ABI_VERSION 3u

/* ---- status codes (every entry point returns one) ------------------------ */
#define FMSKF_OK 0
#define FMSKF_EINVAL 1   /* bad argument / shape / state */
#define FMSKF_ENOMEM 2   /* device or host allocation failed */
#define FMSKF_EDEVICE 3  /* HIP error, or no usable GPU */
#define FMSKF_ERCCL 4    /* collective failed (multi-GPU ensemble path) */
#define FMSKF_ENOTSUP 5  /* entry point not valid for this model */

/* ---- models --------------------------------------------------------------- */
/* RS: reference semantics.  State = the firmware's VEHICLE_CTRL pose/velocity.
 *     correct = theta hard overwrite (P == 0, R == 0), predict = the odometry
 *     integrator bit for bit (VD_vehicle_controller.cpp:11-51).
 * KF6:  6-state linear KF (px, py, theta, vx, vy, omega), fp32; z = (theta,
 *       omega, vx_world, vy_world) formed in-kernel from yaw, gyro z, wheel rpm.
 * EKF9: 9-state EKF (px, py, theta, vbx, vby, omega, gyro bias, abx, aby), fp32,
 *       nonlinear mecanum f(); z formed in-kernel from 8 raw int16 words.
 * KF12D: 12-state linear KF in fp64: KF6's base + arm tip (tx, ty, tz, tvx, tvy,
 *       tvz); z = 8 fp64 (theta, omega, vx_w, vy_w, tx, ty, tz, tvz).          */
#define FMSKF_MODEL_RS 0u
#define FMSKF_MODEL_KF6 1u
#define FMSKF_MODEL_EKF9 2u
#define FMSKF_MODEL_KF12D 3u

/* sin/cos policy for util_mymath.hpp:44-45 (arm_sin_f32 / arm_cos_f32) */
#define FMSKF_TRIG_TABLE512 0u /* CMSIS-DSP algorithm: 512-entry table + linear interpolation */
#define FMSKF_TRIG_LIBM 1u     /* device sinf/cosf */

#define FMSKF_MEM_HOST 0u
#define FMSKF_MEM_DEVICE 1u

typedef struct fmskf_ctx *fmskf_handle;

typedef struct fmskf_config {
  uint32_t abi_version;  /* = FMSKF_ABI_VERSION */
  uint32_t model;        /* FMSKF_MODEL_* */
  uint64_t n_instances;  /* N */
  int32_t device;        /* HIP device ordinal */
  uint32_t trig;         /* FMSKF_TRIG_* */
  double dt;             /* tick period [s]; the reference ticks at 1 kHz (VD_task_main.cpp:22,165) */
  /* Noise / initial covariance, packed lower triangle, row-major (k = i*(i+1)/2 + j).
   * Used by the KF models (n = 6, 9, 12; m = 4, 6, 8); ignored by RS. */
  double q[78];
  double r[36];
  double p0[78];
  int8_t motor_dir[4];   /* FL, BL, BR, FR: +1 / -1 (VD_task_main.cpp:75-78) */
  uint32_t imu_read_reg; /* register index for 0x5F REGVALUE frames; init() leaves q0 = 0x51 */
  uint32_t flags;        /* FMSKF_CFG_* (0 = the defaults) */
  uint32_t reserved;     /* must be 0 */
} fmskf_config;

/* KF6, EKF9: carry the open-loop integrals -- px, py and the position block of P (P[0][0],
 * P[1][0], P[1][1]) -- as compensated fp32 pairs (hi + lo; every addition to them a TwoSum), so
 * that they track the float64 filter over long horizons (60 s at 1 kHz within 1e-5, where plain
 * fp32 drifts to 2e-5 - 6e-5).  fmskf_get_state returns hi (hi + lo rounded is hi); the lo parts
 * are readable through fmskf_get_state_lo.  +40 B per robot-tick (KF6 232 -> 272, EKF9 456 ->
 * 496).  Off by default: the plain fp32 filters are the headline and cfg 3. */
#define FMSKF_CFG_COMP_POS 1u

/* Fill defaults for `model` with `n` instances (dt = 1 ms, TABLE512, reference motor
 * directions, model-specific Q/R/P0).  Pure host function (no GPU needed). */
int fmskf_config_init(fmskf_config *cfg, uint32_t model, uint64_t n);

/* ---- lifecycle ------------------------------------------------------------ */
int fmskf_create(const fmskf_config *cfg, fmskf_handle *out);
int fmskf_destroy(fmskf_handle h);
/* Zero-initialised state, as the firmware's static objects at boot
 * (VD_vehicle_controller.hpp:73-77), P = P0 for KF models; the
 * control state too (power off), keeping the control parameters. */
int fmskf_reset(fmskf_handle h);
int fmskf_set_stream(fmskf_handle h, void *hip_stream); /* hipStream_t; NULL = default */
int fmskf_sync(fmskf_handle h);
int fmskf_get_config(fmskf_handle h, fmskf_config *out);
const char *fmskf_strerror(int status);
/* last error message of the calling thread ("" if none) */
const char *fmskf_last_error(void);
int fmskf_abi_version(void);
/* state dimension n, measurement dimension m and state element size for a model */
int fmskf_model_dims(uint32_t model, uint32_t *n, uint32_t *m, uint32_t *elem_bytes);

/* ---- ingest: device boundary --------------------------------------------- */
/* IMU task tick (IMT::main, imu_task_main.cpp:43-82 at 100 Hz): per instance, feed one
 * poll's UART bytes through the WT901 parser (wit_c_sdk.c:132-198), then
 * IMU_IF_WT901C::update (imu_if_wt901c.cpp:83-89): is_error = no quaternion frame
 * since the last good poll; else refresh the Data page (updateData, :91-129).
 * bytes: instance i's bytes at bytes + i*stride, len[i] <= stride.
 * latch_qinit != 0 makes the poll init() (:63-76): WitInit first empties the parser window
 * (wit_c_sdk.c:355-362: the head of a frame split across the poll before is dropped), the
 * bytes are parsed, and after a good poll the page is refreshed and q_init latched; init()'s
 * getDataImmediately (:149-158) does not write is_error, so after a good latching poll the
 * flag keeps the last update()'s answer.  (init() also re-reads register q0; the handle's
 * imu_read_reg is configuration and a latch leaves it, which is the firmware's behaviour at
 * the default 0x51.) */
int fmskf_ingest_wt901(fmskf_handle h, const uint8_t *bytes, uint32_t stride, const uint32_t *len,
                       int latch_qinit, uint32_t mem);

/* CAN RX (VD_can_controller.hpp:65-95 -> MOTOR_IF_M2006::rx_callback): frames [N][4][8]
 * (FL, BL, BR, FR; C610 payload: angle, rpm, current big-endian), stamps [N][4]
 * (int16 us, micros() & 0x7FFF), present [N] bitmask (bit w = wheel w has a frame;
 * NULL = all four).  Updates the device-resident motor state. */
int fmskf_ingest_can(fmskf_handle h, const uint8_t *frames, const int16_t *stamps,
                     const uint8_t *present, uint32_t mem);

/* ---- per tick -------------------------------------------------------------- */
/* One robot's KF6 tick record, 16 bytes: the three KF6 inputs of one robot in one
 * contiguous record (the sensor packet a robot would ship per tick).  Passing records
 * instead of the yaw / gyro / rpm planes lets each lane fetch its inputs with one 16-byte
 * load instead of three (measured 41.6 -> 39.5 us per 2^20-robot tick on MI355X). */
typedef struct fmskf_kf6_record {
  float yaw_deg;     /* IMT::get_status_now_yaw */
  float gyro_z_dps;  /* IMU_IF::Data.gyro[2] */
  int16_t rpm[4];    /* s16_rawSpeedRpm FL, BL, BR, FR */
} fmskf_kf6_record;

/* Inputs of one tick.  Every plane pointer may be NULL: the kernel then reads the
 * device-resident value the ingest entry points produced (full pipeline). */
typedef struct fmskf_tick_inputs {
  uint32_t mem;              /* FMSKF_MEM_HOST or FMSKF_MEM_DEVICE for all pointers below */
  /* plane pitch of angle_sum in elements (single-tick calls; 0 = N, >= N otherwise).  A padded
   * pitch keeps the four sum planes off a power-of-two stride, which aliases in the memory-side
   * cache: the RS tick at 2^20 robots reads [4][2^20] sums measurably slower than [4][2^20 + 512]
   * (fmskf_tick_many takes the plane pitch from tick_stride) */
  uint32_t angle_sum_pitch;
  const float *yaw_deg;      /* [N] IMT::get_status_now_yaw (deg, [-180,180)); RS, KF6 */
  const float *gyro_z_dps;   /* [N] IMU_IF::Data.gyro[2] (deg/s, as published); KF6 */
  const int16_t *rpm;        /* [N][4] Status.s16_rawSpeedRpm FL,BL,BR,FR; RS, KF6 */
  const int64_t *angle_sum;  /* [4][angle_sum_pitch] MOTOR_IF_M2006::get_rawAngleSum; RS */
  const int16_t *raw;        /* [N][8] EKF9 words: Yaw, GZ, AX, AY registers, rpm x4 */
  const double *z;           /* [8][N] KF12D measurements */
  const uint8_t *valid;      /* [N] measurement present (0 = predict only); NULL = all */
  /* KF6 only: [N] records replacing yaw_deg, gyro_z_dps and rpm (which must then be NULL);
   * tick_many: [T][N], advancing by tick_stride records per tick */
  const fmskf_kf6_record *kf6_rec;
} fmskf_tick_inputs;

/* correct: RS -> theta = deg2rad(yaw) (VD_task_main.cpp:368); KF models -> update. */
int fmskf_correct(fmskf_handle h, const fmskf_tick_inputs *in);
/* predict: RS -> VEHICLE_CTRL::update odometry (VD_vehicle_controller.cpp:11-51);
 * KF models -> time update (x <- f(x), P <- F P F^T + Q). */
int fmskf_predict(fmskf_handle h, const fmskf_tick_inputs *in);
/* fused correct-then-predict, one kernel, one pass over the state (the hot path) */
int fmskf_tick(fmskf_handle h, const fmskf_tick_inputs *in);
/* T fused ticks in one launch, state held on chip between ticks.  Inputs are T
 * consecutive tick records: each plane pointer advances by tick_stride elements
 * per tick (tick_stride >= N; for [N][k] planes by tick_stride*k). */
int fmskf_tick_many(fmskf_handle h, const fmskf_tick_inputs *in, uint32_t n_ticks,
                    uint64_t tick_stride);

/* ---- fixed-interval smoothing of a replayed window (KF6) ----------------------- */
/* fmskf_tick_many returns a filter's answer: the state after the last tick.  The estimate a
 * replayed log wants at tick t uses the measurements after t as well: the fixed-interval
 * (Rauch-Tung-Striebel) smoother.  For KF6 it is exact and cheap: F and H are constant, and the
 * measurement is rebuilt bit for bit from the recorded inputs.
 *
 * fmskf_tick_many_smooth takes the inputs of fmskf_tick_many (records or the three planes, an
 * optional `valid` mask, host or device memory; explicit planes required) and does two things.
 * 1. It advances the handle exactly as fmskf_tick_many(h, in, n_ticks, tick_stride) would: x, P
 *    and every counter are bit for bit what that call leaves.
 * 2. With, for tick t = 0 .. T-1, the prior (x-[t], P-[t]) = the state before the tick, the
 *    filtered state (x+[t], P+[t]) = after the tick's measurement update (the prior where
 *    valid == 0), and the prior of t+1 the predict of the filtered state, it writes for every t
 *    the estimate of the state at tick t's measurement time given all T measurements:
 *        x_s[T-1] = x+[T-1],  P_s[T-1] = P+[T-1]
 *        C = P+[t] F^T (P-[t+1])^-1
 *        x_s[t] = x+[t] + C (x_s[t+1] - x-[t+1]),  P_s[t] = P+[t] + C (P_s[t+1] - P-[t+1]) C^T
 *    the heading difference wrapped as the innovation is wrapped, the output heading wrapped
 *    into [-pi, pi).  The kernels form these numbers in fp32 by an equivalent recursion without
 *    cancellation (C = F^-1 (I - Q (P-[t+1])^-1), csrc/smooth_lane.hpp), so a smoothed variance
 *    stays positive while a robot's prior is still the diffuse P0; it needs P-[t+1] positive
 *    definite.  tests/smooth_ref.py holds the float64 definition and the bound the fp32 results
 *    are held to.
 * Two launches: the ticks, storing every tick's prior (108 B per robot and tick) into a
 * workspace the handle owns, then one backward pass.  The workspace only grows;
 * fmskf_smooth_workspace_bytes is a pure query (at least 108 * N * n_ticks),
 * fmskf_smooth_reserve allocates ahead of time so that a timed loop never allocates, and
 * fmskf_smooth_reserve(h, 0) or fmskf_destroy frees it.  No checkpoint contains it.  Host outputs
 * are staged on the device and copied out on the handle's stream; the call returns when they are
 * complete.  Device outputs are asynchronous on the handle's stream.  fmskf_set_timing /
 * fmskf_last_kernel_ms cover both passes.
 *
 * FMSKF_ENOTSUP: a model other than KF6, a handle with FMSKF_CFG_COMP_POS, a handle with a gate
 * set (its accept / force decisions are recorded per tick by fmskf_tick_many_trace, whose
 * `applied` plane lets an ungated handle replay the gated trajectory).  FMSKF_EINVAL: out or
 * out->x NULL, reserved != 0, a bad mem flag, pitch non-zero and below N, n_ticks == 0,
 * everything fmskf_tick_many refuses, a call inside a graph capture.  Each is raised before
 * anything is launched, and the handle is untouched.  FMSKF_ENOMEM: the workspace or the output
 * staging cannot be allocated; that happens before the first launch, so the state is untouched
 * then too. */
typedef struct fmskf_smooth_out {
  uint32_t mem;       /* FMSKF_MEM_HOST or FMSKF_MEM_DEVICE for x and P */
  uint32_t reserved;  /* must be 0 */
  uint64_t pitch;     /* elements between consecutive rows; 0 = N, otherwise >= N */
  float *x;           /* [T][6][pitch]  smoothed state of every tick; required */
  float *P;           /* [T][21][pitch] smoothed covariance, packed like fmskf_get_state; NULL = not formed */
} fmskf_smooth_out;

int fmskf_tick_many_smooth(fmskf_handle h, const fmskf_tick_inputs *in, uint32_t n_ticks,
                           uint64_t tick_stride, const fmskf_smooth_out *out);
int fmskf_smooth_workspace_bytes(fmskf_handle h, uint32_t n_ticks, uint64_t *bytes);
int fmskf_smooth_reserve(fmskf_handle h, uint32_t n_ticks);   /* grow-only; 0 frees */

/* ---- innovation log-likelihood of a replayed window (KF6) ---------------------- */
/* How well a given Q and R explain a log: per robot, over the measured ticks of a window,
 *     log L = -1/2 * sum_t ( NIS_t + log det S_t + 4 log 2 pi )
 * the innovation (prediction-error) log-likelihood, the objective a Q / R fit maximises and the
 * score that ranks candidate parameter sets; sum NIS / n_meas is the consistency check (4 for the
 * four measurement rows of a consistent filter).  The call returns the three sums, so
 * log L = -0.5 * (nis_sum + logdet_sum + n_meas * 4 log 2 pi).
 *
 * fmskf_tick_many_loglik takes the inputs of fmskf_tick_many (records or the three planes, an
 * optional `valid` mask, host or device memory; explicit planes required).
 * 1. It advances the handle exactly as fmskf_tick_many(h, in, n_ticks, tick_stride) would: x, P
 *    and every counter are bit for bit what that call leaves (the non-finite guard counts in
 *    counter [0] as that call's launch does).
 * 2. For every tick that carries a measurement for the robot (`valid` NULL or non-zero), from the
 *    state before the tick's update: y the innovation (the heading component wrapped as the update
 *    wraps it); with S = H P H^T + R = L D L^T, w = L^-1 y and dinv = 1 / D the update's own
 *    operands, NIS = the value of the chi-square gate (nis = w[0]*(w[0]*dinv[0]), then
 *    fma(w[a], w[a]*dinv[a], nis), a = 1..3: what a monitor-only fmskf_set_gate reports, bit for
 *    bit) and log det S = -sum_a log dinv[a].  A tick without a measurement contributes nothing.
 * 3. The sums over the window are carried in registers, in fp32, with no transcendental per tick:
 *    nis_sum as a compensated pair (every addition a TwoSum), stored as (double)hi + (double)lo;
 *    logdet_sum as E * ln 2 + log(pm), where every dinv[a] is split exactly (frexp) into mantissa
 *    and exponent, the four mantissas are multiplied as ((m0*m1)*m2)*m3, that product into the
 *    running mantissa pm, pm is split again and all exponents are added to the int32 E: four
 *    roundings of 2^-24 per measured tick in the log domain on top of dinv's own fp32 error, and
 *    one fp64 log per robot at the store, logdet_sum = -((double)E * ln 2 + log((double)pm)).
 *    innov_sum / innov_outer (either non-NULL selects the kernel variant that carries them): the
 *    sums of y[a] and of the fp32 products y[i]*y[j], each a compensated fp32 pair like nis_sum,
 *    stored as double.  csrc/loglik_lane.hpp; tests/loglik_ref.py holds the float64 definition
 *    and the bound the results are held to.
 *    A robot is left out when any dinv[a] of a measured tick is not a positive finite number or a
 *    NIS is NaN: its nis_sum and logdet_sum are NaN, its n_meas is still the count, and it does
 *    not enter `total`, whose [3] counts such robots.
 * 4. total = { sum n_meas, sum nis_sum, sum logdet_sum, robots left out } over the robots not left
 *    out, in fp64, deterministic: a fixed tree inside every 256-robot block, one partial per block
 *    in a scratch the handle owns (allocated by the first call that asks for the total, freed by
 *    fmskf_destroy; no checkpoint contains it), the partials added in block order by a second
 *    small launch.  No floating-point atomics: two calls on the same state and inputs write the
 *    same bytes everywhere.
 * 5. FMSKF_LL_ACCUMULATE, for a log replayed in chunks: every per-robot output and every element
 *    of total becomes old + new (one fp64 addition; n_meas an integer addition) instead of new.
 *    The chunks advance the state as one call over the whole window does, bit for bit, as chunks
 *    of fmskf_tick_many do.
 * Every output pointer is optional, but not all of them.  Host outputs are mirrored on the device
 * (the innovation planes at the caller's pitch) and copied out on the handle's stream, the
 * caller's values copied in first with FMSKF_LL_ACCUMULATE; the call returns when they are
 * complete, and elements past N of a padded row are left alone.  Device outputs are asynchronous
 * on the handle's stream; the double arrays must be 8-byte aligned, n_meas 4-byte.
 * fmskf_set_timing / fmskf_last_kernel_ms record the call's launches as one entry.
 * 108 + 16 T bytes read and at most 108 + 20 written per robot, + 112 with the innovation sums.
 *
 * FMSKF_ENOTSUP: a model other than KF6, a handle with FMSKF_CFG_COMP_POS, a handle with a gate
 * set (the smoother's exclusions).  FMSKF_EINVAL: out NULL, every output pointer NULL, unknown
 * flags, a bad mem flag, pitch non-zero and below N, n_ticks == 0, a misaligned device output,
 * everything fmskf_tick_many refuses, a call inside a graph capture.  FMSKF_ENOMEM: the scratch or
 * the host staging cannot be allocated.  Each is raised before anything is launched, and the
 * handle's state is untouched. */
typedef struct fmskf_loglik_out {
  uint32_t mem;        /* FMSKF_MEM_HOST or FMSKF_MEM_DEVICE for every pointer below */
  uint32_t flags;      /* FMSKF_LL_* ; unknown bits: FMSKF_EINVAL */
  uint64_t pitch;      /* innov_* planes: elements between rows; 0 = N, otherwise >= N */
  uint32_t *n_meas;    /* [N] ticks of the window that carried a measurement for the robot */
  double *nis_sum;     /* [N] sum of NIS over those ticks */
  double *logdet_sum;  /* [N] sum of log det S over those ticks */
  double *innov_sum;   /* [4][pitch]  sum of y (heading wrapped as the update wraps it); optional */
  double *innov_outer; /* [10][pitch] sum of y y^T, packed lower triangle (k = i*(i+1)/2 + j); optional */
  double *total;       /* [4] fleet: sum n_meas, sum nis_sum, sum logdet_sum, robots left out; optional */
} fmskf_loglik_out;
#define FMSKF_LL_ACCUMULATE 1u  /* add to what the caller's arrays (total included) hold, not overwrite */

int fmskf_tick_many_loglik(fmskf_handle h, const fmskf_tick_inputs *in, uint32_t n_ticks,
                           uint64_t tick_stride, const fmskf_loglik_out *out);

/* ---- EM sufficient statistics for Q and R of a replayed window (KF6) ----------- */
/* The smoother gives the states Q and R are fitted against, the log-likelihood the objective they
 * are fitted by; this call gives the fit's step.  For a linear-Gaussian model the M-step of the EM
 * algorithm is closed form: with w[t] = x[t+1] - F x[t] the process noise of the step t -> t+1 and
 * v[t] = z[t] - H x[t] the measurement noise of a measured tick,
 *     Q = sum_t E[w w^T | all T measurements] / n_trans,  R = sum_t E[v v^T | all] / n_meas
 * under the smoothed distribution of the window.  With x_s, P_s the smoothed estimates of
 * fmskf_tick_many_smooth and P_{t,t+1} = C P_s[t+1] the lag-one covariance (C that call's gain),
 *     E[w w^T | all] = s s^T + P_s[t+1] - F P_{t,t+1} - P_{t,t+1}^T F^T + F P_s[t] F^T,
 *                      s = x_s[t+1] - F x_s[t]                               (t = 0 .. T-2)
 *     E[v v^T | all] = v v^T + H P_s[t] H^T,  v = z[t] - H x_s[t]            (measured t = 0 .. T-1)
 * the heading components wrapped as the smoother and the update wrap them.  The kernels form the
 * first in fp32 as s s^T + (Q - Q Pi Q) + (Pi Q)^T P_s[t+1] (Pi Q), Pi = (P-[t+1])^-1,
 * s = Q Pi (x_s[t+1] - x-[t+1]): the same quantity as a sum of three positive semidefinite terms
 * from the smoother's own operands, so that it does not cancel while a prior is still the diffuse
 * P0 (csrc/em_lane.hpp).  Every tick's term is added to an fp64 accumulator: the sums do not lose
 * accuracy with T.  tests/em_ref.py holds the float64 definition and the bound the results are
 * held to.
 *
 * fmskf_tick_many_em takes the inputs of fmskf_tick_many (records or the three planes, an
 * optional `valid` mask, host or device memory; explicit planes required).
 * 1. It advances the handle exactly as fmskf_tick_many(h, in, n_ticks, tick_stride) would: x, P
 *    and every counter are bit for bit what that call leaves.
 * 2. Two launches and a small third for the total: fmskf_tick_many_smooth's forward pass into the
 *    same workspace (fmskf_smooth_reserve, fmskf_smooth_workspace_bytes), then one backward pass
 *    that writes nothing of size T: 124 B read per robot-tick, at most 4 + 31 * 8 B written per
 *    robot.
 * 3. sq [21][pitch]: per robot the sum over t = 0 .. T-2 of E[w w^T | all], packed lower triangle
 *    (k = i*(i+1)/2 + j).  n_trans = T - 1 for every robot: the last predict of the window, from
 *    tick T-1 to T, is not a term, and with T = 1 every sq entry is 0.  sr [10][pitch]: per robot
 *    the sum over its measured ticks of E[v v^T | all]; n_meas [N] counts them.
 * 4. A robot is left out when any of its 31 sums is not finite: its sq and sr are NaN, its n_meas
 *    is still the count, and it enters neither the sums nor the counts of `total`.
 * 5. total [34] = { sum n_trans, sum n_meas, robots left out, sq[21], sr[10] } over the robots not
 *    left out, in fp64, deterministic like fmskf_tick_many_loglik's: a fixed tree inside every
 *    256-robot block, one partial per quantity and block in a scratch the handle owns (allocated
 *    by the first call that asks for the total, freed by fmskf_destroy; no checkpoint contains
 *    it), the partials added in block order by a small launch.  No floating-point atomics: two
 *    calls on the same state and inputs write the same bytes everywhere.
 * 6. FMSKF_EM_ACCUMULATE: every per-robot output and every element of total becomes old + new (one
 *    fp64 addition; n_meas an integer addition), so that several windows, or several logs, feed one
 *    M-step.  Every call smooths its own window independently of the others: a log cut into two
 *    windows is not the log smoothed as one, and the transition between two windows is not a term
 *    of either.
 * 7. fmskf_em_mstep, pure host: q[k] = total[3 + k] / total[0], r[k] = total[24 + k] / total[1], the
 *    packed Q and R a new handle's fmskf_config takes.  FMSKF_EINVAL: a NULL argument, a non-finite
 *    entry of total, total[0] <= 0 or total[1] <= 0.
 * Every output pointer is optional, but not all of them.  Host outputs, their staging and
 * FMSKF_EM_ACCUMULATE's copy-in behave as in fmskf_tick_many_loglik; device outputs are
 * asynchronous on the handle's stream, the double arrays 8-byte aligned, n_meas 4-byte.
 * fmskf_set_timing / fmskf_last_kernel_ms cover all launches of the call.
 *
 * FMSKF_ENOTSUP: the smoother's cases.  FMSKF_EINVAL: out NULL, every output pointer NULL, unknown
 * flags, a bad mem flag, pitch non-zero and below N, n_ticks == 0, a misaligned device output,
 * everything fmskf_tick_many refuses, a call inside a graph capture.  FMSKF_ENOMEM: the workspace,
 * the scratch or the host staging cannot be allocated.  Each is raised before anything is
 * launched, and the handle's state is untouched. */
typedef struct fmskf_em_out {
  uint32_t mem;      /* FMSKF_MEM_HOST or FMSKF_MEM_DEVICE for every pointer below */
  uint32_t flags;    /* FMSKF_EM_ACCUMULATE; unknown bits: FMSKF_EINVAL */
  uint64_t pitch;    /* sq / sr planes: elements between rows; 0 = N, otherwise >= N */
  uint32_t *n_meas;  /* [N] measured ticks of the window; optional */
  double *sq;        /* [21][pitch] per robot: sum over t = 0..T-2 of E[w w^T | all], packed lower triangle; optional */
  double *sr;        /* [10][pitch] per robot: sum over measured t of (v v^T + H P_s[t] H^T); optional */
  double *total;     /* [34] fleet: sum n_trans, sum n_meas, robots left out, sq[21], sr[10]; optional */
} fmskf_em_out;
#define FMSKF_EM_ACCUMULATE 1u  /* add to what the caller's arrays (total included) hold, not overwrite */
#define FMSKF_EM_TOTAL_LEN 34u

int fmskf_tick_many_em(fmskf_handle h, const fmskf_tick_inputs *in, uint32_t n_ticks,
                       uint64_t tick_stride, const fmskf_em_out *out);
int fmskf_em_mstep(const double *total, double *q /*[21]*/, double *r /*[10]*/);

/* ---- per-tick trace of a replayed window (KF6, gated or not) ------------------- */
/* The calls above return the end of a window or a sum over it.  This one returns what the filter
 * did at every tick: the NIS time series (the standard consistency diagnostic: when did a robot
 * start slipping?), the gate's decision of every tick, and the filtered trajectory, decimated if
 * wanted -- in one launch instead of T single ticks each followed by a readout of the fleet.
 *
 * fmskf_tick_many_trace takes the inputs of fmskf_tick_many (records or the three planes, an
 * optional `valid` mask, host or device memory; explicit planes required).  KF6 without
 * FMSKF_CFG_COMP_POS, with or without a gate (fmskf_set_gate, below).
 * 1. It advances the handle exactly as fmskf_tick_many(h, in, n_ticks, tick_stride) would: x, P
 *    and every counter are bit for bit what that call leaves (the non-finite guard counts in
 *    counter [0] as that call's launch does), and on a gated handle the gate state too: status,
 *    run, rejects and the last evaluated NIS.
 * 2. Per tick t and robot, rows t of the three per-tick planes:
 *    gated handle, robot measured at tick t (`valid` NULL or non-zero): status[t] the gate's
 *      decision (FMSKF_GATE_ACCEPTED / REJECTED / FORCED), nis[t] the NIS the tick evaluated,
 *      applied or not, applied[t] 1 for ACCEPTED or FORCED, else 0;
 *    ungated handle, robot measured: status[t] = FMSKF_GATE_ACCEPTED, applied[t] = 1, nis[t] the
 *      value a monitor-only gate (nis_max = +INFINITY, max_consecutive = 0) reports, bit for bit;
 *    no measurement (valid == 0): status[t] = FMSKF_GATE_NONE, applied[t] = 0, nis[t] the quiet
 *      NaN 0x7FC00000.
 * 3. `applied` has the format of fmskf_tick_inputs.valid with tick_stride == pitch.  A rejected
 *    update is the valid == 0 skip bit for bit and an applied or forced one the ungated update, so
 *    an ungated handle of the same configuration, set to the state the gated handle had before the
 *    window (fmskf_get_state / fmskf_set_state) and fed the same inputs with valid = applied,
 *    repeats the gated trajectory exactly; fmskf_tick_many_smooth, fmskf_tick_many_loglik and
 *    fmskf_tick_many_em, which refuse a gated handle, work on that one.
 * 4. State rows: row j of x / P is the state after tick (j + 1) * every - 1, i.e. what
 *    fmskf_get_state returns after (j + 1) * every ticks; n_ticks / every rows, rounded down.
 * Only the declared rows and columns are written: columns [N, pitch) and memory past the last row
 * are left alone.  Every output pointer is optional, but not all of them.  One launch;
 * fmskf_set_timing / fmskf_last_kernel_ms record it as one entry.  Host outputs are mirrored on
 * the device at the caller's pitch and copied out on the handle's stream; the call returns when
 * they are complete.  Device outputs are asynchronous on the handle's stream; the float planes
 * must be 4-byte aligned, the byte planes may have any alignment and any pitch.
 * 16 B read and 4 + 1 + 1 B written per robot-tick, + 24 / every for x and 84 / every for P; the
 * state is read and written once per launch.
 *
 * FMSKF_ENOTSUP: a model other than KF6, a handle with FMSKF_CFG_COMP_POS.  FMSKF_EINVAL: out
 * NULL, every output pointer NULL, reserved or reserved2 non-zero, a bad mem flag, pitch non-zero
 * and below N, n_ticks == 0, x or P given with every == 0 or every > n_ticks, a misaligned device
 * float plane, everything fmskf_tick_many refuses, a call inside a graph capture.  FMSKF_ENOMEM:
 * the host staging cannot be allocated.  Each is raised before anything is launched, and the
 * handle's state is untouched. */
typedef struct fmskf_trace_out {
  uint32_t mem;        /* FMSKF_MEM_HOST or FMSKF_MEM_DEVICE for every pointer below */
  uint32_t reserved;   /* must be 0 */
  uint64_t pitch;      /* elements between consecutive rows of every plane; 0 = N, otherwise >= N */
  uint32_t every;      /* read only when x or P is given: 1 .. n_ticks */
  uint32_t reserved2;  /* must be 0 */
  float   *nis;        /* [T][pitch]  NIS evaluated at tick t */
  uint8_t *status;     /* [T][pitch]  FMSKF_GATE_NONE / ACCEPTED / REJECTED / FORCED of tick t */
  uint8_t *applied;    /* [T][pitch]  1 where tick t's update was applied, else 0: the format of
                          fmskf_tick_inputs.valid with tick_stride == pitch */
  float   *x;          /* [T/every][6][pitch]  state after ticks every, 2*every, ... */
  float   *P;          /* [T/every][21][pitch] packed like fmskf_get_state; NULL = not stored */
} fmskf_trace_out;

int fmskf_tick_many_trace(fmskf_handle h, const fmskf_tick_inputs *in, uint32_t n_ticks,
                          uint64_t tick_stride, const fmskf_trace_out *out);

/* ---- chi-square innovation gate (KF6) ---------------------------------------- */
/* Off by default: a handle that never sets a gate runs the kernels and computes the bits it
 * always did, and writes the checkpoints it always wrote.
 *
 * With a gate set, every KF6 measurement update -- fmskf_tick, fmskf_correct, each tick of
 * fmskf_tick_many, whatever the input form (planes, kf6_rec, NULL planes reading the ingest
 * state, with or without a `valid` mask) -- first forms, per robot, the normalized innovation
 * squared NIS = y^T S^-1 y from the operands of the update itself: with S = L D L^T, w = L^-1 y
 * and vw = D^-1 w (y's heading component wrapped to [-pi, pi) as the update wraps it),
 * nis = w[0]*vw[0], then nis = fma(w[a], vw[a], nis) for a = 1..3 (single rounding, as every fma
 * of the update).  With `run` the robot's current count of consecutive rejections:
 *     forced = max_consecutive > 0 && run >= max_consecutive
 *     apply  = forced || nis <= nis_max          (a NaN NIS is rejected unless forced)
 * A rejected robot's update is skipped exactly as valid == 0 skips it: x and P are untouched by
 * the update, and the predict still runs.  An applied update is the ungated update bit for bit.
 *
 * Per-robot gate state (fmskf_get_gate):
 *   status   FMSKF_GATE_* of the last updating call: NONE when it carried no measurement for
 *            the robot (valid == 0) or none ran yet; FORCED whenever `forced` held, whatever
 *            the NIS; else ACCEPTED or REJECTED
 *   run      consecutive rejections, saturating at 255 (so a max_consecutive above 255 never
 *            forces); 0 after any applied update; unchanged by a call without a measurement
 *   rejects  total rejections since create / reset / load, saturating at 2^22 - 1
 *   nis      the last evaluated NIS (applied or not); unchanged when the robot had no
 *            measurement; 0 before the first
 * fmskf_tick_many leaves the last tick's status and the last evaluated nis.
 *
 * nis_max = +INFINITY with max_consecutive = 0 is monitor-only: nothing is rejected, the state
 * equals an ungated handle's bit for bit, and NIS is reported.
 *
 * KF6 without FMSKF_CFG_COMP_POS only: fmskf_set_gate returns FMSKF_ENOTSUP for RS, EKF9, KF12D
 * and FMSKF_CFG_COMP_POS handles; FMSKF_EINVAL for a nis_max that is NaN or <= 0, and inside a
 * graph capture.  Setting a gate on a handle that has none starts from a zero gate state;
 * changing the thresholds of a set gate keeps the state; NULL turns the gate off.
 * fmskf_get_gate returns FMSKF_EINVAL while no gate is set.
 *
 * fmskf_reset zeroes the gate state and keeps the configuration; fmskf_set_state leaves the gate
 * state alone; fmskf_save_state writes it as an optional section group when a gate is set (a
 * gate-less handle's file is unchanged), fmskf_load_state restores it into a gated handle, resets
 * the gate state when the file has none, and ignores the file's when the handle has no gate.
 *
 * The fused forms have no gated counterpart and take the fallbacks they already have: with a
 * gate set fmskf_isr_tick / fmskf_isr_tick_can run the CAN RX kernel (where it applies), the
 * gated tick, the control step and the frame (counters [1] and [2] count them as ever), and
 * fmskf_tick_ensemble / fmskf_tick_ensemble_begin tick gated, then run the stand-alone record.
 * All of them can be captured (fmskf_graph_begin) like the plain tick.  A gated tick moves
 * 244 B per robot instead of 232: the gate word read and written, the NIS written. */
typedef struct fmskf_gate {
  float nis_max;            /* reject the measurement when !(NIS <= nis_max); +INFINITY: monitor only */
  uint32_t max_consecutive; /* after this many rejections in a row the next measurement is applied
                               whatever its NIS (re-acquisition; 0 = never force) */
} fmskf_gate;
int fmskf_set_gate(fmskf_handle h, const fmskf_gate *g);   /* NULL = gate off (the default) */

#define FMSKF_GATE_NONE 0      /* no measurement for this robot in the last updating call (valid == 0, or none yet) */
#define FMSKF_GATE_ACCEPTED 1
#define FMSKF_GATE_REJECTED 2
#define FMSKF_GATE_FORCED 3    /* applied because max_consecutive was reached */
/* all [N]; any pointer may be NULL */
int fmskf_get_gate(fmskf_handle h, float *nis, uint8_t *status, uint8_t *run, uint32_t *rejects, uint32_t mem);

/* ---- per-row innovation gate (EKF9) ------------------------------------------- */
/* Off by default: a handle that never sets a row gate runs the kernels and computes the bits it
 * always did, and writes the checkpoints it always wrote.
 *
 * With the default diagonal R the EKF9 measurement update is six scalar updates in sequence, in
 * the row order heading, gyro z, ax, ay, vbx, vby, each on the state the previous one left.  The
 * row gate decides each scalar row on its own normalised innovation, so one slipping wheel drops
 * the two wheel rows and keeps the IMU rows, and one heading glitch drops the heading row alone.
 *
 * With a row gate set, every EKF9 measurement update -- fmskf_tick, fmskf_correct, each tick of
 * fmskf_tick_many, with or without a `valid` mask -- is that loop over a = 0..5 on the
 * innovation y (the heading component against the compensated heading and wrapped to [-pi, pi),
 * as ever).  At row a, hp = H_a P, s = H_a hp + R[a][a], si = 1 / s and g = y[a] * si are formed
 * exactly as in the ungated update; then, with run[a] the row's count of consecutive rejections,
 *     d2     = y[a] * g                       (one rounded product: y[a]^2 / s)
 *     forced = max_consecutive > 0 && run[a] >= max_consecutive
 *     apply  = forced || d2 <= d2_max[a]      (a NaN d2 is rejected unless forced)
 * An applied row runs exactly the operations of the ungated loop: x += hp g (the heading through
 * its compensated sum), the later innovations y[b] -= (H_b hp) g, P -= (hp si) hp^T.  A rejected
 * row touches nothing: not x, not the heading's low part, not P, not the later y[b].  The
 * heading's renormalisation after the loop and the predict run as ever.  So
 *   - an update in which every row is applied equals the ungated update bit for bit;
 *   - an update in which every row is rejected equals the valid == 0 skip;
 *   - any other pattern equals the ungated sequential update with R[a][a] = +INFINITY on the
 *     rejected rows, value for value (1 / inf = 0 makes every term of such a row an exact zero);
 *     only the sign of a zero may differ.
 *
 * Per-robot, per-row gate state (fmskf_get_row_gate; planes [FMSKF_EKF9_ROWS][N], row-major):
 *   status  FMSKF_GATE_* of the last updating call: NONE in every row when it carried no
 *           measurement for the robot (valid == 0) or none ran yet; FORCED whenever `forced`
 *           held, whatever d2; else ACCEPTED or REJECTED
 *   run     0 after an applied row, +1 after a rejected one, saturating at 255; unchanged by a
 *           call without a measurement
 *   d2      the last evaluated value (applied or not), kept only with FMSKF_ROW_GATE_D2;
 *           unchanged when the robot had no measurement; 0 before the first
 * fmskf_tick_many leaves the last tick's status and the last evaluated d2.
 *
 * All six d2_max = +INFINITY with max_consecutive = 0 is monitor-only: nothing is rejected, the
 * state equals an ungated handle's bit for bit, and d2 is reported.
 *
 * EKF9 without FMSKF_CFG_COMP_POS and with a diagonal R (the sequential form) only:
 * fmskf_set_row_gate returns FMSKF_ENOTSUP for RS, KF6, KF12D, EKF9 with FMSKF_CFG_COMP_POS and
 * an EKF9 handle whose R has an off-diagonal term; FMSKF_EINVAL for a d2_max entry that is NaN
 * or <= 0, for max_consecutive > 255, for unknown flag bits, and inside a graph capture.
 * Setting a gate on a handle that has none starts from a zero gate state; changing the thresholds
 * or flags of a set gate keeps the state; NULL turns it off.  fmskf_get_row_gate returns
 * FMSKF_EINVAL while no row gate is set, and when d2 is asked for and the gate was set without
 * FMSKF_ROW_GATE_D2.
 *
 * fmskf_reset zeroes the gate state and keeps the configuration; fmskf_set_state leaves the gate
 * state alone; fmskf_save_state writes it as an optional section group (the words, then the d2
 * planes; the last group of the body) only while a row gate is set, so every other handle's file
 * is byte for byte what it was; fmskf_load_state restores the group into a row-gated handle,
 * zeroes the gate state when the file has none, and ignores the file's group when the handle has
 * no row gate.  fmskf_set_gate (KF6) and fmskf_correct_pose are untouched by and independent of
 * the row gate.
 *
 * The fused forms have no row-gated counterpart and take the fallbacks the KF6 gate takes: with a
 * row gate set fmskf_isr_tick / fmskf_isr_tick_can run the CAN RX kernel (where it applies), the
 * gated tick, the control step and the frame (counters [1] and [2] count them), and
 * fmskf_tick_ensemble / fmskf_tick_ensemble_begin tick gated, then run the stand-alone record.
 * All of them can be captured (fmskf_graph_begin) like the plain tick.  A row-gated tick moves
 * 472 B per robot instead of 456 (the gate word read and written), 496 B with the d2 planes. */
#define FMSKF_EKF9_ROWS 6          /* heading, gyro z, ax, ay, vbx, vby: the order of the update */
#define FMSKF_ROW_GATE_D2 1u       /* keep every row's last evaluated d2 (+24 B stored per robot-tick) */
typedef struct fmskf_row_gate {
  float d2_max[FMSKF_EKF9_ROWS];   /* row a is rejected when !(d2[a] <= d2_max[a]); +INFINITY: never */
  uint32_t max_consecutive;        /* 0 = never force; else a row rejected this many times in a row is
                                      applied whatever its d2 (per row; runs saturate at 255) */
  uint32_t flags;                  /* FMSKF_ROW_GATE_* */
} fmskf_row_gate;
int fmskf_set_row_gate(fmskf_handle h, const fmskf_row_gate *g);   /* NULL = off (the default) */
/* status [6][N] (FMSKF_GATE_NONE / ACCEPTED / REJECTED / FORCED), run [6][N], d2 [6][N]; any may be NULL */
int fmskf_get_row_gate(fmskf_handle h, uint8_t *status, uint8_t *run, float *d2, uint32_t mem);

/* ---- absolute pose fixes (KF6, EKF9) ------------------------------------------ */
/* The tick's measurements are heading, yaw rate and wheel velocity: px and py are open-loop
 * integrals and their covariance only grows.  fmskf_correct_pose fuses low-rate absolute fixes
 * (a ceiling camera, UWB, a lidar landmark: 10-30 Hz, a few percent of the fleet per tick) into
 * the listed robots -- unlike fmskf_set_state, which overwrites x and P.
 *
 * Every listed robot gets one measurement update of its current state with H selecting states
 * 0, 1 (px, py) and, with FMSKF_FIX_HEADING, 2 (theta), and R from `prm`: the model's own update
 * in its operation order (factorisation S = L D L^T, w = L^-1 y, then x += U^T D^-1 w,
 * P -= U^T D^-1 U), with NIS = y^T S^-1 y formed between the two phases exactly as the gate above
 * forms it (nis = w[0]*vw[0], then single-rounded fmas for a = 1..m-1) and
 *     apply = nis <= prm->nis_max             (+INFINITY: no gate; a NaN NIS never applies)
 * The heading innovation is wrapped to [-pi, pi) as the model's own update wraps it; the heading
 * state is left as fmskf_correct leaves it (no extra wrap).  No predict runs, and a robot that is
 * not listed is neither read nor written.  Compensated states go through their pairs as in the
 * model's own update: the EKF9 heading (innovation against hi + lo, TwoSum addition,
 * renormalised), and with FMSKF_CFG_COMP_POS KF6's px, py (innovation against hi + lo), P00, P10,
 * P11 (TwoSum additions into the low-part rows, renormalised after the update).
 *
 * status[k]: FMSKF_GATE_ACCEPTED, FMSKF_GATE_REJECTED or FMSKF_FIX_IGNORED; nis[k]: the evaluated
 * NIS, 0 for an ignored entry.  Either may be NULL.  A rejected fix leaves the robot's x, P and
 * low parts bit for bit.  The call keeps nothing between calls: the handle's persistent gate
 * (fmskf_set_gate) is neither read nor changed, and reset, checkpoints and fmskf_set_state are
 * unaffected.
 *
 * `robot` must be strictly ascending (the gathers of a sorted list coalesce; see DESIGN.md for
 * the cost model).  A host list (FMSKF_MEM_HOST) is validated before anything is launched:
 * ascending order, robot < N, and prm (R finite with a positive diagonal, nis_max not NaN and
 * > 0, no unknown flag bits); a violation returns FMSKF_EINVAL and changes nothing (prm is
 * validated for a device list too).  A device list (16-byte aligned: each lane reads its fix with
 * one 16-byte load) cannot be validated on the host: the kernel
 * ignores any entry with robot >= N and any entry whose robot is not above the entry before it,
 * reports FMSKF_FIX_IGNORED for it and counts it in fmskf_get_counters slot [3].  A device list
 * that is unsorted in some other way (say 5, 3, 5) is a caller error: no access leaves the
 * handle's arrays, but the result for the robots listed twice is unspecified.
 *
 * count == 0 is FMSKF_OK with no launch.  fixes / nis / status in host memory are staged like
 * every other host call; the call is asynchronous on the handle's stream (host outputs: complete
 * on return), with device pointers it can be captured by fmskf_graph_begin, its launch is
 * recorded by fmskf_set_timing like a tick-kernel launch, and a state that goes non-finite is
 * counted in counter [0].
 *
 * KF6 (plain and FMSKF_CFG_COMP_POS) and EKF9 (plain); FMSKF_ENOTSUP for RS, KF12D and EKF9
 * with FMSKF_CFG_COMP_POS. */
typedef struct fmskf_pose_fix {   /* 16 bytes, one per fixed robot */
  uint32_t robot;                 /* instance index */
  float x_m, y_m;                 /* world position, as fmskf_get_pose reports it */
  float theta_rad;                /* world heading; read only with FMSKF_FIX_HEADING */
} fmskf_pose_fix;

#define FMSKF_FIX_HEADING 1u      /* z = (px, py, theta), m = 3; otherwise z = (px, py), m = 2 */

typedef struct fmskf_pose_fix_params {
  double r[6];       /* packed lower triangle of the fix noise, 3x3 (k = i*(i+1)/2 + j); without
                        FMSKF_FIX_HEADING only the 2x2 block r[0..2] is read */
  float nis_max;     /* apply a fix only when NIS <= nis_max; +INFINITY = no gate (NaN never applies) */
  uint32_t flags;    /* FMSKF_FIX_* */
} fmskf_pose_fix_params;

#define FMSKF_FIX_IGNORED 4       /* status: malformed entry (robot >= N, or not above its predecessor) */

int fmskf_correct_pose(fmskf_handle h, const fmskf_pose_fix *fixes, uint64_t count,
                       const fmskf_pose_fix_params *prm,
                       float *nis, uint8_t *status,   /* [count], either may be NULL */
                       uint32_t mem);

/* ---- range updates against surveyed anchors (KF6, EKF9) ------------------------- */
/* A UWB tag does not deliver a position: it delivers one range to one anchor at a time, in short
 * bursts of two to four anchors.  fmskf_correct_range fuses each range directly into the listed
 * robot's current estimate -- one scalar measurement with its own gate, linearised on that
 * estimate; the antenna's lever arm makes the heading observable -- instead of a multilaterated
 * position with an invented covariance through fmskf_correct_pose.
 *
 * Anchors.  The handle owns a device table of up to FMSKF_RANGE_ANCHORS_MAX surveyed anchors, one
 * 16-byte row (x, y, z, 0) each.  fmskf_set_anchors replaces the table from host xyz [count][3]
 * (the copy is ordered on the handle's stream); count == 0 clears it.  FMSKF_EINVAL for count >
 * FMSKF_RANGE_ANCHORS_MAX, a NULL xyz with count > 0, a non-finite coordinate, and inside a graph
 * capture.  fmskf_get_anchors writes min(count, capacity) rows to host xyz (NULL with capacity 0:
 * the count alone) and the table's size to *count.  Anchors are configuration: fmskf_reset keeps
 * them, and checkpoints neither write nor read them (the file of a handle with anchors is byte
 * for byte that of one without).
 *
 * The measurement, in fp32, every operation rounded on its own (no contraction), with correctly
 * rounded square root and divisions, in this order.  (c, s) = the handle's own cos / sin of the
 * heading state (fmskf_config.trig, as fmskf_eval_trig evaluates it; EKF9: of the heading's high
 * part); (lx, ly, lz) = prm->tag; (ax, ay, az) the anchor; r the entry's var_m2 when > 0, else
 * prm->var_m2:
 *     rx = c*lx - s*ly            ry = s*lx + c*ly
 *     dx = (px - ax) + rx         dy = (py - ay) + ry         dz = lz - az
 *          with FMSKF_CFG_COMP_POS  dx = ((px_hi - ax) + px_lo) + rx, dy likewise
 *     d  = sqrt((dx*dx + dy*dy) + dz*dz)
 *     !(d >= d_min):  status FMSKF_RANGE_NEAR, d2 = 0, nothing is touched (a NaN d included)
 *     di = 1/d        H = (dx*di, dy*di, (dy*rx - dx*ry)*di, 0, ...)
 *     hp[j] = (H0*P[0][j] + H1*P[1][j]) + H2*P[2][j]           j = 0 .. n-1 (the high parts of P)
 *     S  = ((H0*hp[0] + H1*hp[1]) + H2*hp[2]) + r
 *     si = 1/S        y = range_m - d        g = y*si        d2 = y*g
 *     apply = d2 <= d2_max                   (+INFINITY: no gate; a NaN d2 never applies)
 *     applied:  x[j] = x[j] + hp[j]*g        P[i][j] = P[i][j] - (hp[i]*si)*hp[j]   (i >= j)
 * The EKF9 heading takes its term by TwoSum into its low part and is renormalised; with
 * FMSKF_CFG_COMP_POS px, py, P00, P10 and P11 take theirs by TwoSum into the low-part rows and are
 * renormalised.  Both renormalisations follow every applied entry, so that a burst in one call
 * equals the same entries in successive calls bit for bit.  No predict runs and the heading is
 * not wrapped again (as in fmskf_correct_pose).  The handle's persistent gates are neither read
 * nor changed, and the call keeps nothing between calls.
 *
 * Lists.  `robot` is non-descending.  A run -- a maximal sequence of consecutive entries with the
 * same robot, one burst -- is applied in list order, each entry on the state the one before
 * left, by one pass over the robot's rows: they are read once and written once, and only if an
 * entry was applied.  status[k]: FMSKF_GATE_ACCEPTED, FMSKF_GATE_REJECTED, FMSKF_RANGE_NEAR or
 * FMSKF_FIX_IGNORED; d2[k]: the evaluated d2, 0 for a NEAR or ignored entry.  Either may be NULL;
 * every entry's outputs are written exactly once.  An entry is ignored when
 *   - its run's first entry has robot >= N (the whole run),
 *   - its run's first entry has a robot below its predecessor's (the whole run),
 *   - its own anchor is at or above the table's size (that entry alone is skipped), or
 *   - the entry FMSKF_RANGE_RUN_MAX places before it has the same robot (a run's entries past
 *     the first FMSKF_RANGE_RUN_MAX).
 * A host list is validated before anything is launched: any of these is FMSKF_EINVAL and nothing
 * changes.  A device list (16-byte aligned) cannot be validated on the host: the kernel ignores
 * such entries and counts them in fmskf_get_counters slot [5].  A device list that is unsorted in
 * some other way (5, 3, 5) is a caller error: no access leaves the handle's arrays, but the
 * result for robots whose entries are not consecutive is unspecified.
 *
 * FMSKF_ENOTSUP for RS, KF12D and EKF9 with FMSKF_CFG_COMP_POS (the models fmskf_correct_pose
 * refuses).  FMSKF_EINVAL for: no anchors set; a NULL prm; var_m2 not finite or <= 0; d2_max NaN
 * or <= 0; d_min not finite or <= 0; a non-finite tag; flags or reserved not 0; a bad mem; a NULL
 * list with count > 0; a host list inside a graph capture; count > FMSKF_RANGE_RUN_MAX * N.
 * count == 0 is FMSKF_OK with no launch.  Host lists and outputs are staged like
 * fmskf_correct_pose's (complete on return); with device pointers the call is asynchronous on the
 * handle's stream and can be captured by fmskf_graph_begin.  fmskf_set_timing records the launch;
 * a robot that an applied entry leaves non-finite is counted in counter [0] (a robot whose every
 * entry is rejected, NEAR or ignored is neither stored nor counted). */
#define FMSKF_RANGE_ANCHORS_MAX 1024u
#define FMSKF_RANGE_RUN_MAX 8u     /* entries of one robot in one call */
#define FMSKF_RANGE_NEAR 5         /* status: predicted distance below d_min, nothing done */

int fmskf_set_anchors(fmskf_handle h, const float *xyz /* host [count][3] */, uint32_t count);
int fmskf_get_anchors(fmskf_handle h, float *xyz, uint32_t capacity, uint32_t *count);

typedef struct fmskf_range_fix {   /* 16 bytes, one per measured range */
  uint32_t robot;
  uint32_t anchor;                 /* index into the anchor table */
  float range_m;
  float var_m2;                    /* > 0: this range's variance; anything else: prm->var_m2 */
} fmskf_range_fix;

typedef struct fmskf_range_params {
  float tag[3];    /* antenna: lx, ly in the body frame [m], lz its height in the anchors' z frame */
  float var_m2;    /* default range variance, finite, > 0 */
  float d2_max;    /* apply when d2 <= d2_max; > 0; +INFINITY: no gate; NaN d2 never applies */
  float d_min;     /* finite, > 0: below it the direction is undefined -> FMSKF_RANGE_NEAR */
  uint32_t flags;  /* must be 0 */
  uint32_t reserved; /* must be 0 */
} fmskf_range_params;

int fmskf_correct_range(fmskf_handle h, const fmskf_range_fix *fixes, uint64_t count,
                        const fmskf_range_params *prm,
                        float *d2, uint8_t *status,   /* [count], either may be NULL */
                        uint32_t mem);

/* ---- robots selected by their state; state of listed robots (KF6, EKF9) --------- */
/* The per-robot signals of the entry points above -- a state gone non-finite (counter [0] says
 * that some did, not which), a position covariance grown too large, a gate that keeps rejecting
 * -- matter for a few robots in a million.  fmskf_select finds them on the device and writes the
 * strictly ascending list fmskf_correct_pose and the two subset calls below take, so the caller
 * neither copies the fleet's state to the host nor touches the rest of the fleet.
 *
 * A robot is selected when ANY of the requested criteria holds:
 *   FMSKF_SEL_NONFINITE  any element of its x or packed P (the rows fmskf_get_state returns, not
 *                        the hidden low parts) is NaN or +-Inf
 *   FMSKF_SEL_POS_VAR    P[0][0] + P[1][1] > pos_var_min: one fp32 addition of packed rows 0 and
 *                        2, a strict compare; a NaN sum does not select
 *   FMSKF_SEL_GATE_RUN   consecutive rejections >= run_min: on a KF6 handle with fmskf_set_gate
 *                        its run, on an EKF9 handle with fmskf_set_row_gate any row a with bit a
 *                        of row_mask set and run[a] >= run_min
 *
 * *count receives the number of robots that match, never capped by `capacity`.
 * robots[0 .. min(*count, capacity)) receives the matching robots in strictly ascending order --
 * with more matches than `capacity`, the first `capacity` of them -- and reason[k], when `reason`
 * is not NULL, the OR of the requested criteria that held for robots[k] (never 0).  Entries past
 * that are not written.  capacity == 0 with robots == NULL is a count-only call.  Two calls on
 * the same state write the same bytes.
 *
 * FMSKF_EINVAL for unknown criteria bits or none, a NaN pos_var_min (with FMSKF_SEL_POS_VAR),
 * run_min outside 1..255 (with FMSKF_SEL_GATE_RUN), a row_mask that is not a nonzero subset of
 * 0x3F on EKF9 with FMSKF_SEL_GATE_RUN or not 0 otherwise, FMSKF_SEL_GATE_RUN on a handle whose
 * gate (KF6) or row gate (EKF9) is not set, a NULL count, a NULL robots with capacity > 0, and
 * inside a graph capture.
 *
 * With FMSKF_MEM_HOST the call is complete on return.  With FMSKF_MEM_DEVICE robots, reason and
 * count (8-byte aligned) are device pointers and the call is asynchronous on the handle's stream.
 * The call reads the state and changes nothing of the handle: no persistent state, nothing in a
 * checkpoint.  Its scratch (one flag byte per robot, one count per 256 robots) is allocated on
 * first use and freed by fmskf_destroy.  fmskf_set_timing records the call's launches (four; the
 * subset calls below: one) as one entry, like a tick-kernel launch.
 *
 * KF6 (plain and FMSKF_CFG_COMP_POS) and EKF9 (plain); FMSKF_ENOTSUP for RS, KF12D and EKF9 with
 * FMSKF_CFG_COMP_POS -- the models of fmskf_correct_pose, for all three entry points. */
#define FMSKF_SEL_NONFINITE 1u  /* any element of the robot's x or packed P (the hi rows) is NaN or +-Inf */
#define FMSKF_SEL_POS_VAR   2u  /* P[0][0] + P[1][1] > pos_var_min: one fp32 addition of packed rows 0 and 2,
                                   strict compare; a NaN sum does not select */
#define FMSKF_SEL_GATE_RUN  4u  /* consecutive rejections >= run_min: KF6 with fmskf_set_gate its run; EKF9
                                   with fmskf_set_row_gate any row a with bit a of row_mask set and
                                   run[a] >= run_min */
typedef struct fmskf_select_params {
  uint32_t criteria;    /* FMSKF_SEL_* bits, at least one; a robot is selected when ANY of them holds */
  float pos_var_min;    /* read only with FMSKF_SEL_POS_VAR; not NaN */
  uint32_t run_min;     /* read only with FMSKF_SEL_GATE_RUN; 1..255 */
  uint32_t row_mask;    /* EKF9 + FMSKF_SEL_GATE_RUN: nonzero subset of 0x3F; must be 0 otherwise */
} fmskf_select_params;

int fmskf_select(fmskf_handle h, const fmskf_select_params *prm,
                 uint32_t *robots, uint8_t *reason,   /* [capacity]; reason may be NULL */
                 uint64_t capacity, uint64_t *count, uint32_t mem);

/* Read (get) or overwrite (set) the state of the listed robots alone.  x is [n][count], p_packed
 * [n(n+1)/2][count] and lo [rows][count] float (rows as fmskf_get_state_lo reports it): dense
 * planes of pitch `count`, column k is robot robots[k].  Any of the three may be NULL; a non-NULL
 * lo on a model that keeps no low rows is FMSKF_EINVAL.
 *
 * get: column k equals column robots[k] of fmskf_get_state / fmskf_get_state_lo, bit for bit.
 * set: only the listed robots' rows change, by the rules of fmskf_set_state applied per listed
 * robot: a given x restarts the heading low part (EKF9) at 0; with FMSKF_CFG_COMP_POS a given x or
 * p_packed restarts the position low parts at 0; a given lo replaces the restarted value.  So a
 * get followed by a set with all three arrays restores the listed robots bit for bit.  Gate state
 * is left alone; a set of x invalidates the ensemble shift snapshot.
 *
 * `robots` follows the list rules of fmskf_correct_pose: strictly ascending; a host list is
 * validated before anything is launched (FMSKF_EINVAL for an entry that is not above its
 * predecessor or is >= N, and nothing changes); in a device list the kernel ignores any entry that
 * is >= N or not above the entry before it -- a get leaves that entry's output column unwritten, a
 * set changes nothing for it -- and counts it in fmskf_get_counters slot [4].  count == 0 is
 * FMSKF_OK with no launch; count > N is FMSKF_EINVAL.  One mem flag covers the list and the
 * arrays.  With device pointers both calls are asynchronous on the handle's stream and can be
 * captured by fmskf_graph_begin; a host list inside a capture is FMSKF_EINVAL.  An array past
 * 4 GiB is reached through 64-bit lane addresses and non-temporal accesses, as in
 * fmskf_correct_pose; FMSKF_LIST_BIG=1 (read once, at the first launch) forces that form. */
int fmskf_get_state_subset(fmskf_handle h, const uint32_t *robots, uint64_t count,
                           float *x, float *p_packed, float *lo, uint32_t mem);
int fmskf_set_state_subset(fmskf_handle h, const uint32_t *robots, uint64_t count,
                           const float *x, const float *p_packed, const float *lo, uint32_t mem);

/* ---- readout --------------------------------------------------------------- */
/* VEHICLE_CTRL::get_vehicle_pos_m_latest (x m, y m, th rad).  Any pointer may be NULL. */
int fmskf_get_pose(fmskf_handle h, float *x, float *y, float *th, uint32_t mem);
/* VEHICLE_CTRL::get_vehicle_vel_mmps_latest (body frame mm/s, mm/s, rad/s) */
int fmskf_get_vel(fmskf_handle h, float *vx, float *vy, float *vth, uint32_t mem);
/* Full model state: x [n][N] and P packed [n(n+1)/2][N] in the model's element type
 * (float, or double for KF12D); RS: x = (x, y, th, vx, vy, vth) floats, P unused.
 * Hidden compensation rows are not part of x / P: EKF9's heading low part and, with
 * FMSKF_CFG_COMP_POS, KF6's position low parts.  get_state returns the hi rows; set_state
 * restarts every low part at 0, so a get_state / set_state round trip is exact only up to the
 * low parts (fmskf_get_state_lo / fmskf_set_state_lo carry them; fmskf_save_state /
 * fmskf_load_state keep everything). */
int fmskf_get_state(fmskf_handle h, void *x, void *p_packed, uint32_t mem);
int fmskf_set_state(fmskf_handle h, const void *x, const void *p_packed, uint32_t mem);
/* The hidden low-part rows [rows][N] float: EKF9's heading (1 row), then with
 * FMSKF_CFG_COMP_POS the 5 rows px, py, P[0][0], P[1][0], P[1][1] (KF6: those 5 only); *rows
 * receives the count (0: the model keeps none, and lo may be NULL).  set_state_lo after
 * set_state restores a handle bit for bit. */
int fmskf_get_state_lo(fmskf_handle h, float *lo, uint32_t *rows, uint32_t mem);
int fmskf_set_state_lo(fmskf_handle h, const float *lo, uint32_t mem);
/* RS: the int64 s64_rawAngleSumPrev [4][N] (VD_vehicle_controller.hpp:75) */
int fmskf_get_prev_sum(fmskf_handle h, int64_t *prev, uint32_t mem);
/* Checkpoint / resume: every per-robot array of the handle (estimator state,
 * RS encoder sums, NaN counters, and the IMU / motor ingest and control state when they
 * exist, with the control parameters) written byte for byte in its device layout, and read
 * back into a handle of the same model, N and ABI; resuming continues bit-identically.
 * Ingest / control state the checkpoint does not hold is reset to its initial value on load.
 * The handle's fmskf_config (noise, geometry) is its own: the saved copy is not applied.
 * Synchronous; EINVAL on I/O errors or a checkpoint that does not match the handle, in which
 * case load leaves the handle's state untouched (lengths are validated before any copy). */
int fmskf_save_state(fmskf_handle h, const char *path);
int fmskf_load_state(fmskf_handle h, const char *path);
/* IMU_IF::Data page [16][N] (accel3, gyro3, mag3, angle3, qut4) of each robot's last successful
 * poll (zeros before one), formed here from the register words that poll left (updateData,
 * imu_if_wt901c.cpp:91-129; the ingest keeps the words, not the page), is_error [N] */
int fmskf_get_imu(fmskf_handle h, float *data, uint8_t *is_error, uint32_t mem);
/* WT901 register file sReg [0x90][N] (int16) and parser bytes pending [N] */
int fmskf_get_imu_regs(fmskf_handle h, int16_t *regs, uint8_t *pending, uint32_t mem);
/* Motor state [N][4]: angle, rpm, curr (int16), angle_sum [4][N] int64,
 * speed_radps [4][N] float (MOTOR_IF_M2006::Status + s64_rawAngleSum) */
int fmskf_get_motors(fmskf_handle h, int16_t *angle, int16_t *rpm, int16_t *curr,
                     int64_t *angle_sum, float *speed_radps, uint32_t mem);
/* MOTOR_IF_M2006::get_status_latest (VD_motor_if_m2006.hpp:23-30,47-50) for every wheel of every
 * robot, [N][4] each (FL, BL, BR, FR): s16_microsec_id, s16_rawAngle, s16_rawSpeedRpm,
 * s16_rawCurr, flt_dltOutAngle_rad (VD_motor_if_m2006.cpp:64: the raw angle difference of the
 * last two frames, not wrap-corrected, as the firmware computes it -- a wheel crossing 8191 -> 0
 * reports about -2*pi/36 rad -- x OUT_RAD_PER_RAW_ANGLE x GEAR_RATIO_INV, formed at readout from
 * the last two angles), flt_SpeedRadPS.  Any pointer may be NULL. */
int fmskf_get_motor_status(fmskf_handle h, int16_t *microsec_id, int16_t *angle, int16_t *rpm,
                           int16_t *curr, float *dlt_out_angle_rad, float *speed_radps, uint32_t mem);
/* counters: [0] = instances whose state went non-finite (NaN/Inf guard), counted per launch:
 * every tick kernel of KF6, EKF9 and KF12D (fmskf_tick, fmskf_correct, fmskf_predict,
 * fmskf_tick_many, fmskf_tick_ensemble / fmskf_tick_ensemble_begin, fmskf_isr_tick,
 * fmskf_isr_tick_can; gated or not) adds one for every robot of the fleet whose x or packed P is
 * not finite as the launch stores it.  A robot that stays bad is therefore counted again by every
 * later launch: [0] is a count of robot-launches, not of distinct robots (fmskf_select with
 * FMSKF_SEL_NONFINITE names the robots).  fmskf_tick_many over T ticks is one launch and counts a
 * robot once, T single ticks count it T times.  The guard tests the sum of the robot's x and P
 * elements, so a state of finite elements whose sum overflows counts too (a sum of at most 90
 * elements: only with elements near the top of the format's range).  The hidden low parts
 * (fmskf_get_state_lo) are not inspected.  fmskf_correct_pose counts the fixes it applied only,
 * those whose robot it stores non-finite, and visits no robot that is not listed.  A listed robot
 * with a NaN in what the fix's NIS reads (its position block: px, py, P00, P10, P11, their low
 * parts, with a heading fix theta and its covariance entries too) has a NaN NIS, is
 * FMSKF_GATE_REJECTED and is not counted.  One that is non-finite only elsewhere has a finite NIS,
 * and so may one with an Inf and no NaN in its position block (P00 = +Inf gives 1 / S = 0): where
 * nis_max admits the NIS the fix is applied, the robot stored and counted.  (After a tick's
 * update a bad robot is as a rule NaN in every element.)  FMSKF_MODEL_RS is never counted (its
 * kernels have no guard).  fmskf_set_state, fmskf_set_state_subset and the readouts leave [0]
 * alone, fmskf_reset zeroes it, fmskf_save_state / fmskf_load_state keep and restore it.
 * [1] = calls of
 * fmskf_isr_tick_can that ran the CAN RX as a kernel of its own before the ISR (a caller rpm /
 * angle sums / KF6 records, CAN buffers not 16-byte (frames) / 8-byte (stamps) aligned, or a
 * regime where the ISR is not one kernel); [2] = ISRs (fmskf_isr_tick or fmskf_isr_tick_can)
 * that ran as the estimator tick, the control step and the 0x200 frame in three kernels instead
 * of one (KF12D; KF6 / EKF9 past the Infinity Cache; KF6 with a gate set, which also counts in
 * [1]).  Results are identical either way; [1] and
 * [2] count since create / reset and are not checkpointed.  [3] = entries of device fix lists
 * that fmskf_correct_pose ignored as malformed (FMSKF_FIX_IGNORED); since create / reset, not
 * checkpointed either.  [4] = entries of device robot lists that fmskf_get_state_subset /
 * fmskf_set_state_subset ignored as malformed; since create / reset, not checkpointed.
 * [5] = entries of device range lists that fmskf_correct_range ignored (FMSKF_FIX_IGNORED: a run
 * whose first entry has robot >= N or a robot below its predecessor's, an anchor index at or
 * above the table's size, a run's entries past the first FMSKF_RANGE_RUN_MAX); since create /
 * reset, not checkpointed.  fmskf_correct_range counts in [0] the robots it stores non-finite, as
 * fmskf_correct_pose does: a robot with a NaN in P00, P10 or P11 has a NaN d2, is
 * FMSKF_GATE_REJECTED and is not counted; one with a NaN px or py has a NaN predicted distance,
 * is FMSKF_RANGE_NEAR and is not counted either. */
int fmskf_get_counters(fmskf_handle h, uint64_t *counters, uint32_t n_counters);

/* ---- ensemble statistics (mean / covariance of x across instances) --------- */
/* Record layout: {count, mean[n], M2 packed[n(n+1)/2]} in fp64 (28 doubles for n=6).
 * fmskf_ensemble_partial writes this rank's record; ranks all-gather the records
 * (RCCL over xGMI, one process per GPU) and fmskf_ensemble_combine folds them in
 * rank order -> deterministic.  `out` may be host or device per mem.
 * The moment sums are accumulated about a shift vector: robot 0's state when the first
 * record after create / reset / set_state / load_state (or fmskf_graph_begin) is taken.  It
 * stays pinned until the next of those calls, so successive records of one state are bitwise
 * identical; M2 loses relative precision only if the fleet drifts many standard deviations
 * away from that snapshot (reset or set_state takes a new one). */
int fmskf_ensemble_record_len(fmskf_handle h, uint32_t *len);
int fmskf_ensemble_partial(fmskf_handle h, double *out, uint32_t mem);
/* fmskf_tick, then this rank's record of the post-tick state (as fmskf_ensemble_partial) in
 * one call.  KF6, EKF9 and KF12D (tiled state, positive-definite R): one tick kernel that also
 * reduces the state it stores, from registers, to per-block records (cross-lane swaps + DPP,
 * no second pass over x), then the fold; the RS model and the KF12D fallback updates tick,
 * then run the stand-alone record.  Records of one state are bitwise identical
 * whichever call produced them only up to fp64 rounding (same shift, different summation
 * order); each call is bitwise reproducible. */
int fmskf_tick_ensemble(fmskf_handle h, const fmskf_tick_inputs *in, double *out, uint32_t mem);
/* host-side: records [n_records][len] -> mean [n], cov packed [n(n+1)/2] (unbiased) */
int fmskf_ensemble_combine(uint32_t n_state, const double *records, uint32_t n_records,
                           double *mean, double *cov_packed);

/* Native multi-GPU path: one process per GPU, an RCCL communicator owned by
 * the handle, the ensemble record all-gathered over xGMI on the handle's stream.  RCCL
 * (librccl.so.1) is resolved at run time, so the library has no link-time dependency on it;
 * FMSKF_ERCCL when it cannot be loaded or a collective fails.
 *   rank 0: fmskf_comm_unique_id(id); distribute the 128 bytes to every rank (any channel);
 *   every rank: fmskf_comm_init(h, id, rank, world); then fmskf_ensemble_stats(h, ...). */
#define FMSKF_COMM_ID_BYTES 128
int fmskf_comm_unique_id(uint8_t id[FMSKF_COMM_ID_BYTES]);
int fmskf_comm_init(fmskf_handle h, const uint8_t id[FMSKF_COMM_ID_BYTES], int rank, int world);
/* The handle's communicator as RCCL itself reports it (ncclCommCount, ncclCommUserRank);
 * EINVAL when the handle has none. */
int fmskf_comm_info(fmskf_handle h, int *world, int *rank);
/* The file the RCCL entry points were resolved from (dladdr of ncclAllGather), or "" while no
 * communicator call has loaded RCCL yet or when it cannot be loaded.  It never loads RCCL itself,
 * and the string stays valid and unchanged for the life of the process.  FMSKF_RCCL_LIBRARY may
 * name another file for the tests' one-GPU loopback stand-in: the library is accepted only if
 * its dynamic symbol table (read from the file before it is loaded, so a rejected file's
 * constructors never run) exports `fmskf_rccl_stand_in`.  That refuses an RCCL build or another
 * collective library picked up by mistake; it is not a defence against a hostile library, which
 * can export the same marker -- an environment that can set FMSKF_RCCL_LIBRARY can already load
 * code into the process. */
const char *fmskf_rccl_library(void);
/* mean [n], cov packed [n(n+1)/2] (unbiased) over every robot of every rank (the ranks of
 * fmskf_comm_init; without a communicator, this handle's robots): device partial record,
 * ncclAllGather, fold in rank order on the host -> identical on every rank, deterministic. */
int fmskf_ensemble_stats(fmskf_handle h, double *mean, double *cov_packed);

/* Asynchronous form of the same exchange, for callers that keep ticking while the records
 * travel (record fused into the tick, gather on a separate stream overlapping
 * the next tick).  Nothing blocks the host:
 *   fmskf_tick_ensemble_begin: fmskf_tick whose kernel also writes this rank's block records
 *     of the post-tick state (KF6, EKF9, KF12D with a positive-definite R; other models tick,
 *     then run the stand-alone record), on the handle's stream;
 *   fmskf_ensemble_begin: the stand-alone record of the current state (no tick);
 *   the record's fold rides in the next begin's tick kernel (extra blocks past its tick
 *   blocks), or runs ahead of the next fmskf_tick, or at fmskf_ensemble_end when nothing
 *   came first; with a communicator of fmskf_comm_init of more than one rank, ncclAllGather
 *   and the copy of the gathered records to pinned host memory then run on the handle's side
 *   stream (one rank: the gather is the identity, the fold writes the pinned slot).  No tick on
 *   the handle's stream waits for the gather, and no call waits on the host.
 *   fmskf_ensemble_end: waits for the OLDEST pending begin and returns its mean [n] and
 *     covariance packed [n(n+1)/2] (unbiased, rank-order fold: identical on every rank,
 *     deterministic).  EINVAL when nothing is pending.
 * At most four begins may be pending (EINVAL on a fifth).  Every rank must issue the same
 * sequence of begins (it is a collective).  Not valid inside a graph capture. */
int fmskf_tick_ensemble_begin(fmskf_handle h, const fmskf_tick_inputs *in);
int fmskf_ensemble_begin(fmskf_handle h);
int fmskf_ensemble_end(fmskf_handle h, double *mean, double *cov_packed);
/* fmskf_ensemble_end that also returns the robots the gathered records count (the sum of their
 * count rows) and how many records were folded (the communicator's size; 1 without one).  Any
 * pointer may be NULL. */
int fmskf_ensemble_end_count(fmskf_handle h, double *mean, double *cov_packed, double *count,
                             uint32_t *n_records);
/* How long the exchange of the result the last fmskf_ensemble_end / _end_count collected took on
 * the handle's side stream: ncclAllGather of the record plus the copy of the gathered records to
 * pinned host memory, between two timing events recorded around them (ms).  -1 when that result
 * needed no exchange (no communicator, or one of a single rank: the fold wrote the pinned slot
 * itself) or none was collected yet.  Lets an N > 1 run say what its collective costs beside the
 * tick. */
int fmskf_ensemble_exchange_ms(fmskf_handle h, float *ms);

/* ---- vehicle control step -------------------------- */
/* Per-robot control state is allocated on the first call of any entry point below
 * (~250 B per robot); zero-initialised like the firmware's static objects, power off. */
typedef struct fmskf_ctrl_params {
  /* FF_PI_D construction (VD_task_main.cpp:86-89): built for 100 Hz (U32_VD_TASK_CTRL_FREQ_HZ)
   * although stepped by the 1 kHz ISR -- the reference's quirk, kept as the default */
  float ctrl_freq_hz;  /* 100 */
  float ff_gain;       /* 0.0075 */
  float p_gain;        /* 0.02 */
  float i_gain;        /* 0.01 */
  float d_gain;        /* 0.0 */
  float i_limit;       /* 0.5 */
  float lpf_freq_hz;   /* 10 (velocity LPF of PI_D, util_controller.hpp:99-101) */
  float ff_limit;      /* 1.0 (set_FF_limit, VD_task_main.cpp:157-160) */
  float interp_ts;     /* VelInterpConstJerk sample time 1/1000 s (VD_task_main.cpp:95-97) */
  int16_t curr_limit_raw; /* MOTOR_IF_M2006::s16_rawCurr_lim 3000 (VD_motor_if_m2006.hpp:62) */
  int16_t reserved;
} fmskf_ctrl_params;

int fmskf_ctrl_params_init(fmskf_ctrl_params *p);
/* takes effect from the next control step; controller state is kept */
int fmskf_set_ctrl_params(fmskf_handle h, const fmskf_ctrl_params *p);
/* VEHICLE_CTRL::start / stop: on [N] (nonzero = on); NULL = all on */
int fmskf_set_power(fmskf_handle h, const uint8_t *on, uint32_t mem);
/* VEHICLE_CTRL::set_target_vel -> VelInterpConstJerk::set_target_params per axis.
 * vel, acl, jrk: [3][N] planes (x mm/s, y mm/s, th rad/s); mask [N] (NULL = every robot). */
int fmskf_set_target_vel(fmskf_handle h, const float *vel, const float *acl, const float *jrk,
                         const uint8_t *mask, uint32_t mem);
/* The control half of VEHICLE_CTRL::update, one tick: interpolators, conv_Vdir_to_Mdir, the
 * four FF_PI_D loops on the measured wheel speed, set_CurrA_tgt.  rpm [N][4] (FL,BL,BR,FR
 * s16_rawSpeedRpm); NULL = the device motor state fmskf_ingest_can keeps. */
int fmskf_control(fmskf_handle h, const int16_t *rpm, uint32_t mem);
/* CAN_CTRL::tx_routine: frames [N][8] = the 0x200 payload (big-endian raw currents) */
int fmskf_can_tx(fmskf_handle h, uint8_t *frames, uint32_t mem);
/* The firmware ISR in one call (VDT::can_tx_routine_intr, VD_task_main.cpp:366-372): correct,
 * VEHICLE_CTRL::update (estimator time update, then the control half on the same rpm record),
 * M_CAN.tx_routine.  Inputs as fmskf_tick (NULL planes = the device-resident ingest state);
 * frames [N][8] receives the 0x200 payloads (NULL: no frame, the current targets are still
 * kept).  Models RS, KF6 and EKF9 run as ONE kernel (one pass over the estimator state, the
 * tick inputs and the control state; KF6 / EKF9 with their state past the Infinity Cache:
 * three); KF12D runs its tick kernel, then the control step and the frame.  Results are
 * identical to fmskf_tick + fmskf_control + fmskf_can_tx in sequence. */
int fmskf_isr_tick(fmskf_handle h, const fmskf_tick_inputs *in, uint8_t *frames, uint32_t mem);
/* The tick's CAN RX and the ISR in one call: fmskf_ingest_can(h, can_frames, can_stamps, NULL,
 * mem) -- the four C610 frames of every robot present, MOTOR_IF_M2006::rx_callback
 * (VD_motor_if_m2006.cpp) -- then fmskf_isr_tick(h, in, frames, mem).  can_frames [N][4][8],
 * can_stamps [N][4] as fmskf_ingest_can.  Models KF6 (no caller rpm / records in `in`), EKF9
 * (no caller rpm) and RS (no caller rpm / angle sums) run it as ONE kernel: the received rpm
 * (RS: and the new angle sums) feed the estimator (EKF9: the wheel loops only, its measurement
 * is the raw record) and the four wheel loops from registers (otherwise, and where the ISR
 * itself is not one kernel, the two calls run).
 * Results are identical to the two calls in sequence. */
int fmskf_isr_tick_can(fmskf_handle h, const uint8_t *can_frames, const int16_t *can_stamps,
                       const fmskf_tick_inputs *in, uint8_t *frames, uint32_t mem);
/* readout: vel_tgt [3][N] (get_vehicle_vel_tgt_mmps_latest), curr_raw [N][4]
 * (get_rawCurr_tgt), wheel_tgt / wheel_ctrl [4][N] (FF_PI_D get_target / last output), all as
 * the last control step (fmskf_control or an ISR call) left them.  Any pointer may be NULL.
 * The step itself stores only the state its next tick reads and the currents: the first readout
 * (or checkpoint, or fmskf_set_power) after a step forms vel_tgt / wheel_tgt / wheel_ctrl from
 * that state with the step's parameters, one small kernel on the handle's stream; changing the
 * parameters, targets or power flags after a step does not change what this returns. */
int fmskf_get_ctrl(fmskf_handle h, float *vel_tgt, int16_t *curr_raw, float *wheel_tgt,
                   float *wheel_ctrl, uint32_t mem);

/* ---- VehicleInfo export -------------------------------- */
/* The ROS VehicleInfo message as RM_task_main.cpp:772-823 fills it (VehicleInfo.msg,
 * VehiclePosition.msg, ImuInfo.msg, FloorDetection.msg), natural C alignment, 84 bytes. */
typedef struct fmskf_vehicle_info {
  int32_t pos_x, pos_y;   /* (int32_t)(x_m * 1000.0f): truncation, ARM saturation */
  float pos_theta;        /* rad */
  int32_t vel_x, vel_y;   /* (int32_t)(mm/s) */
  float vel_theta;        /* rad/s */
  uint8_t imu_fault;      /* 0xFF when IMU_IF::isError (every imu field 0), else 0 */
  uint8_t pad_[3];
  float imu_q[4];         /* qx qy qz qw = Data.qut[0..3] */
  float imu_g[3];         /* Data.gyro */
  float imu_a[3];         /* Data.accel */
  uint8_t floor[8];       /* right left forward back rightforward leftforward rightback leftback */
  float cam_pitch;
  uint32_t fault;
} fmskf_vehicle_info;

/* out [N] records; floor [N][8], cam_pitch [N], fault [N] come from subsystems outside the
 * path and may be NULL (zero). */
int fmskf_export_vehicle_info(fmskf_handle h, fmskf_vehicle_info *out, const uint8_t *floor,
                              const float *cam_pitch, const uint32_t *fault, uint32_t mem);

/* ---- HIP graph of a per-tick call sequence ------------------------------------- */
/* Record the device work of the entry points called between begin and end (on the handle's
 * stream, which must be a stream set with fmskf_set_stream, not the null stream) into a HIP
 * graph, then replay it: one launch per tick for launch-bound (small-N) fleets.  Only
 * device-pointer calls (FMSKF_MEM_DEVICE, or NULL planes reading the device state) can be
 * captured; a call that needs a host round trip fails during capture.  A new begin
 * replaces the previous graph.  A replay starts from the handle's current state, whatever
 * direct calls came since the capture: the results are those of the captured calls made
 * directly at that point (with the control parameters of the capture). */
int fmskf_graph_begin(fmskf_handle h);
int fmskf_graph_end(fmskf_handle h);
int fmskf_graph_launch(fmskf_handle h, uint32_t times);

/* ---- diagnostics ------------------------------------------------------------ */
/* Evaluate the device sin/cos policy on x[n] (device pointers when mem = DEVICE). */
int fmskf_eval_trig(fmskf_handle h, const float *x, float *s, float *c, uint64_t n, uint32_t mem);
/* Per-launch kernel timing with HIP events recorded on the handle's stream around
 * every tick-kernel launch (enable resets the record).  fmskf_last_kernel_ms: the
 * last launch; fmskf_kernel_time_total: sum and count of all launches since
 * enable (waits for the last one).  At most 65536 launches are recorded. */
int fmskf_set_timing(fmskf_handle h, int enable);
int fmskf_last_kernel_ms(fmskf_handle h, float *ms);
int fmskf_kernel_time_total(fmskf_handle h, double *total_ms, uint32_t *count);

#ifdef __cplusplus
}
#endif
#endif /* FMSKF_H_ */
