"""Helpers of the firmware-fixture tests (test_vehicle_golden_cpu.py, test_gpu_vehicle_golden.py):
decoding tests/golden/vehicle_ref.npz and imu_ref.npz, which hold what the reference's own
VEHICLE_CTRL / MOTOR_IF_M2006 / VelInterpConstJerk / IMU_IF_WT901C answered (generators:
tests/golden/make_golden_vehicle.py, make_golden_imu.py).  Nothing here reads the reference."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
VEHICLE_NPZ = os.path.join(GOLDEN, "vehicle_ref.npz")
IMU_NPZ = os.path.join(GOLDEN, "imu_ref.npz")


def load(path):
    d = np.load(path)
    return {k: d[k] for k in d.files}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def group_gains(d, g):
    """oracle.ctrl_params keywords of config group g"""
    kw = {str(k): float(v) for k, v in zip(d["gain_keys"], d["group_gains"][g])}
    kw["ts"] = np.float32(d["group_gains"][g][list(d["gain_keys"]).index("ts")])
    kw["clim"] = int(kw["clim"])
    return kw


def engine_ctrl_params(d, g):
    """fmskf.Engine.set_ctrl_params keywords of config group g"""
    kw = group_gains(d, g)
    return dict(ctrl_freq_hz=kw["c_freq"], ff_gain=kw["ff"], p_gain=kw["pg"], i_gain=kw["ig"], d_gain=kw["dg"],
                i_limit=kw["ilim"], lpf_freq_hz=kw["lpf"], ff_limit=kw["fflim"], interp_ts=float(kw["ts"]),
                curr_limit_raw=kw["clim"])


def power_events(d, s):
    """{tick: on} of scenario s"""
    return {int(t): int(on) for ss, t, on in d["power_ev"] if ss == s}


def target_events(d, s):
    """{tick: (vel [3], acl [3], jrk [3])} of scenario s"""
    return {int(t): d["target_val"][k] for k, (ss, t) in enumerate(d["target_ev"]) if ss == s}


def tx_frames(curr):
    """CAN_CTRL::tx_routine's 0x200 payload of raw current targets [..., 4] int16: high byte, low
    byte per wheel (formed here from the fixture's get_rawCurr_tgt, not by the code under test)"""
    u = np.asarray(curr, np.int16).astype(np.int64) & 0xFFFF
    out = np.empty(u.shape[:-1] + (8,), np.uint8)
    out[..., 0::2] = u >> 8
    out[..., 1::2] = u & 0xFF
    return out


def imu_streams(d):
    """yield (name, [(bytes uint8 array, latch, data [16] float32, is_error)]) per stream"""
    ob = op = 0
    for s, name in enumerate(d["name"]):
        polls = []
        for _ in range(int(d["n_polls"][s])):
            n = int(d["poll_len"][op])
            polls.append((d["bytes"][ob:ob + n], bool(d["latch"][op]), d["data"][op], int(d["is_error"][op])))
            ob += n
            op += 1
        yield str(name), polls
