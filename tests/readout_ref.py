"""Reference of the readout path (fmskf_get_pose / fmskf_get_vel / fmskf_export_vehicle_info) in
plain numpy, from the dense state x that set_state / get_state use.  It shares no code with the
library or with the oracle: tests/test_readout_cpu.py pins it to the oracle's C conversions before
tests/test_gpu_readout.py lets it judge a kernel.

Units are those of include/fmskf.h: pose (m, m, rad), velocity in the body frame (mm/s, mm/s,
rad/s).  RS keeps both as they are read; EKF9 keeps body m/s; KF6 / KF12D keep world m/s and
are rotated by -theta at readout."""
import numpy as np

from fmskf.engine import VEHICLE_INFO_DTYPE

MODELS = ("rs", "kf6", "ekf9", "kf12d")
F32_1000 = np.float32(1000)

# The export's edge table (fp32 values): signed zeros, fractions that truncate toward zero,
# the int32 limits in mm (2147483.5 m and 2147483.75 m give the fp32 products 2^31 - 128 and
# 2^31), values past them, an fp32 product that overflows, infinities, NaN, the smallest
# subnormal
EDGE_TABLE = np.array([0.0, -0.0, 0.9999e-3, -0.9999e-3, 1.9995, -1.9995, 2147483.5, 2147483.75,
                       -2147483.75, 3e9, -3e9, 1e36, np.inf, -np.inf, np.nan, 1.401298464e-45],
                      np.float32)
# velocity rows only: the float32 just below 2^31 and 2^31 itself (as mm/s for RS, whose rows
# are read as they are; the stored m/s times 1000 otherwise)
EDGE_VEL_EXTRA = np.array([np.nextafter(np.float32(2.0**31), np.float32(0)), 2.0**31], np.float32)
# KF12D only (fp64 state narrowed to float before the conversion): overflow of the narrowing, a
# double exactly halfway between two floats (ties to even: 1.5 + 2^-24 -> 1.5), a subnormal double
EDGE_F64_EXTRA = np.array([1e300, 1.5 + 2.0**-24, 5e-324], np.float64)


def pose(model, x):
    """[3, N] float32: rows 0..2 (KF12D: narrowed from double)"""
    assert model in MODELS
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(np.asarray(x)[:3]).astype(np.float32)


def vel(model, x):
    """[3, N] body velocity.  RS and EKF9: float32.  KF6 / KF12D: np.longdouble, unrounded (the
    caller narrows it with .astype(np.float32) where it needs the float the kernel stores)."""
    assert model in MODELS
    x = np.asarray(x)
    if model == "rs":
        return np.ascontiguousarray(x[3:6]).astype(np.float32)
    if model == "ekf9":
        assert x.dtype == np.float32
        with np.errstate(over="ignore", invalid="ignore"):
            return np.stack([x[3] * F32_1000, x[4] * F32_1000, x[5]]).astype(np.float32)
    th, vx, vy = (x[k].astype(np.longdouble) for k in (2, 3, 4))
    k = np.longdouble(1000)
    with np.errstate(invalid="ignore", over="ignore"):
        c, s = np.cos(th), np.sin(th)
        return np.stack([(vx * c + vy * s) * k, (-vx * s + vy * c) * k, x[5].astype(np.longdouble)])


def vel_f32(model, x):
    with np.errstate(over="ignore", invalid="ignore"):
        return vel(model, x).astype(np.float32)


def ulp_f32(v):
    """spacing of float32 at |v| (v finite, any float type), as float64"""
    a = np.abs(np.asarray(v)).astype(np.float64)
    _, e = np.frexp(a)  # a = m 2^e, m in [0.5, 1)
    return np.where(a == 0, 2.0**-149, np.ldexp(1.0, np.maximum(e - 24, -149)))


def body_vel_bound(ref, vx, vy):
    """The bound on |got - ref| of a KF6 / KF12D body velocity component, ref the unrounded
    longdouble value: half an fp32 ulp for the final narrowing, plus 2^-48 * 1000 (|vx| + |vy|)
    for the double arithmetic (device cos / sin within 2 ulp = 2^-51 each, three more double
    roundings of 2^-53 each: under 2^-49 of the magnitudes, doubled as margin)."""
    mag = np.abs(np.asarray(vx, np.float64)) + np.abs(np.asarray(vy, np.float64))
    return 0.5 * ulp_f32(ref) + 2.0**-48 * 1000.0 * mag


def arm_i32(f):
    """Cortex-M7 VCVT.S32.F32 of float32 values: truncate toward zero, saturate, NaN -> 0"""
    t = np.trunc(np.asarray(f, np.float32).astype(np.float64))
    t = np.where(np.isnan(t), 0.0, t)
    return np.clip(t, -2.0**31, 2.0**31 - 1).astype(np.int64).astype(np.int32)


def vehicle_info(pose, vel, imu_data, is_error, floor=None, cam=None, fault=None):
    """[N] VEHICLE_INFO_DTYPE records from pose / vel [3, N] float32 (readout units), the IMU
    data page [16, N] and error flags [N]; floor [N, 8], cam [N], fault [N] or None (zero)"""
    pose, vel = np.asarray(pose), np.asarray(vel)
    assert pose.dtype == np.float32 and vel.dtype == np.float32
    n = pose.shape[1]
    rec = np.zeros(n, VEHICLE_INFO_DTYPE)
    with np.errstate(over="ignore", invalid="ignore"):
        rec["pos_x"] = arm_i32(pose[0] * F32_1000)  # an fp32 product
        rec["pos_y"] = arm_i32(pose[1] * F32_1000)
    rec["pos_theta"] = pose[2]
    rec["vel_x"] = arm_i32(vel[0])
    rec["vel_y"] = arm_i32(vel[1])
    rec["vel_theta"] = vel[2]
    err = np.asarray(is_error) != 0
    ok = ~err
    d = np.asarray(imu_data, np.float32)
    rec["imu_fault"] = np.where(err, 0xFF, 0)
    rec["imu_q"][ok] = d[12:16, ok].T
    rec["imu_g"][ok] = d[3:6, ok].T
    rec["imu_a"][ok] = d[0:3, ok].T
    if floor is not None:
        rec["floor"] = floor
    if cam is not None:
        rec["cam_pitch"] = cam
    if fault is not None:
        rec["fault"] = fault
    return rec
