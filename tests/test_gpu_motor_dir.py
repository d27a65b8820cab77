"""Motor directions by wheel.  Every other GPU test runs motor_dir = (1, 1, -1, -1), with which wheels
0 and 1 always take can_wheel's / curr_to_raw's `dir == 1` path and wheels 2 and 3 the other: an
index slip inside either pair -- in the wheel-per-lane CAN kernel, the robot-per-lane one or the
fused ISRs' can_args copy -- changes nothing.  With param_cases.MOTOR_DIRS and the default together
every wheel sees both signs and no two wheels always agree.

Against orc.MotorBatch(n, dirs) (the firmware's rx_callback, VD_motor_if_m2006.cpp) and
orc.CtrlBatch(..., motor_dir=dirs) (the current scaling of VEHICLE_CTRL::update), as the oracle
restates them; every comparison exact, floats as bit patterns.  N = 1 and 1001, 20 ticks."""
import ctypes as C

import numpy as np
import pytest

from fmskf import Engine

import param_cases as pc
import seq_ref

pytestmark = pytest.mark.gpu

SIZES = (1, 1001)
T = 20


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def eq(got, want, what):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


def _frames(rng, n):
    """random C610 frames with the edge words in: angle 0 and 8191, rpm and current -32768 and
    32767 (the `(int16_t)(v * dir)` wrap of -32768 * -1), on about a tenth of the wheels each"""
    ang = rng.integers(0, 8192, (n, 4))
    rpm = rng.integers(-9000, 9000, (n, 4))
    cur = rng.integers(-10000, 10000, (n, 4))
    for a, edges in ((ang, (0, 8191)), (rpm, (-32768, 32767)), (cur, (-32768, 32767))):
        u = rng.random((n, 4))
        a[u < 0.05] = edges[0]
        a[u > 0.95] = edges[1]
    if n == 1:  # the lone robot meets every edge within the run
        k = int(rng.integers(4))
        ang[0, k], rpm[0, (k + 1) % 4], cur[0, (k + 2) % 4] = rng.choice([0, 8191]), rng.choice([-32768, 32767]), -32768
    fr = np.zeros((n, 4, 8), np.uint8)
    for k, v in enumerate((ang, rpm, cur)):
        u = np.asarray(v, np.int64) & 0xFFFF
        fr[:, :, 2 * k] = (u >> 8).astype(np.uint8)
        fr[:, :, 2 * k + 1] = (u & 0xFF).astype(np.uint8)
    fr[:, :, 6:] = rng.integers(0, 256, (n, 4, 2), dtype=np.uint8)
    stamps = rng.integers(0, 0x8000, (n, 4)).astype(np.int16)
    return fr, stamps


def _rx(orc, mb, frames, stamps, present):
    """orc_can_ingest_batch with a `present` mask (MotorBatch.rx takes every wheel)"""
    frames, stamps = np.ascontiguousarray(frames, np.uint8), np.ascontiguousarray(stamps, np.int16)
    orc.lib().orc_can_ingest_batch(mb.n, C.cast(mb.m, C.c_void_p), frames.ctypes.data_as(C.c_void_p),
                                   stamps.ctypes.data_as(C.c_void_p),
                                   None if present is None else present.ctypes.data_as(C.c_void_p))


def _same_motors(e, mb, what):
    """every motor-state field: fmskf_get_motors (the angle sums among them) and fmskf_get_motor_status"""
    f = mb.field
    m, st = e.get_motors(), e.get_motor_status()
    for key, want in (("angle", f("angle")), ("rpm", f("rpm")), ("curr", f("curr")), ("angle_sum", f("angle_sum").T),
                      ("speed_radps", f("speed_radps").T)):
        eq(m[key], want, f"{what}: {key}")
    for key, want in (("microsec_id", f("micro")), ("angle", f("angle")), ("rpm", f("rpm")), ("curr", f("curr")),
                      ("dlt_out_angle_rad", f("dlt_out_angle_rad")), ("speed_radps", f("speed_radps"))):
        eq(st[key], want, f"{what}: status {key}")


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("form", ["robot_per_lane", "wheel_per_lane"])
@pytest.mark.parametrize("dirs", pc.MOTOR_DIRS)
def test_ingest_can(orc, dirs, form, n):
    """fmskf_ingest_can in both kernel forms: k_can4 (robot per lane: no `present` mask, aligned
    buffers) and k_can (wheel per lane: with a mask)"""
    rng = np.random.default_rng([n, 17] + [d + 1 for d in dirs])
    mb = orc.MotorBatch(n, dirs)
    seen = np.zeros(6, bool)
    with Engine("rs", n, motor_dir=dirs) as e:
        for t in range(T):
            fr, st = _frames(rng, n)
            assert fr.ctypes.data % 16 == 0 and st.ctypes.data % 8 == 0
            present = rng.integers(0, 16, n).astype(np.uint8) if form == "wheel_per_lane" else None
            e.ingest_can(fr, st, present)
            _rx(orc, mb, fr, st, present)
            w = fr.astype(np.int64)
            ang, rpm, cur = ((w[:, :, 2 * k] << 8) | w[:, :, 2 * k + 1] for k in range(3))
            seen |= [np.any(ang == 0), np.any(ang == 8191), np.any(rpm == 0x8000), np.any(rpm == 0x7FFF),
                     np.any(cur == 0x8000), np.any(cur == 0x7FFF)]
            if t % 5 == 4 or t < 2:
                _same_motors(e, mb, f"dirs {dirs} {form} tick {t}")
    assert n == 1 or seen.all()
    assert np.any(mb.field("angle_sum") != 0)


def _kw(model, inp, t):
    return dict(yaw_deg=inp.yaw[t]) if model == "rs" else dict(yaw_deg=inp.yaw[t], gyro_z_dps=inp.gz[t])


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("model", ["rs", "kf6"])
@pytest.mark.parametrize("dirs", pc.MOTOR_DIRS)
def test_control_and_isr_forms(orc, dirs, model, n):
    """the control step on the ingested motor state (ingest_can, tick, control, can_tx), isr_tick
    and isr_tick_can: currents, 0x200 frames, control outputs, motor state and estimator state
    against the oracle fleet (seq_ref.Fleet with these directions)"""
    prm = pc.default_params(model, motor_dir=dirs)
    inp = seq_ref.Inputs(model, n, T + 1, 11)
    fleet = seq_ref.Fleet(orc, model, n, inp, prm=prm)
    names = ("can", "isr", "split")
    eng = {k: Engine(model, n, motor_dir=dirs) for k in names}
    try:
        for e in eng.values():
            e.set_power(inp.power(-1) | (n == 1))
            e.set_target_vel(*inp.target(-1)[:3])
        fleet.ref.set_power(inp.power(-1) | (n == 1))
        fleet.ref.set_target_vel(*inp.target(-1)[:3])
        for t in range(T):
            f, s = inp.can(t)
            kw = _kw(model, inp, t)
            got = {"can": eng["can"].isr_tick_can(f, s, **kw)}
            eng["isr"].ingest_can(f, s)
            got["isr"] = eng["isr"].isr_tick(**kw)
            eng["split"].ingest_can(f, s)
            eng["split"].tick(**kw)
            eng["split"].control()
            got["split"] = eng["split"].can_tx()
            want = fleet.apply("fused")
            xo, Po = fleet.state()
            for k in names:
                eq(got[k], want, f"{k}: 0x200 frames of tick {t}")
                x, P = eng[k].get_state()
                eq(x, xo, f"{k}: x after tick {t}")
                if Po is not None:
                    eq(P, Po, f"{k}: P after tick {t}")
        for k in names:
            c = eng[k].get_ctrl()
            for key, v in fleet.ctrl().items():
                eq(c[key], v, f"{k}: get_ctrl {key}")
            _same_motors(eng[k], fleet.mb, k)
        assert np.any(fleet.ref.curr() != 0)
    finally:
        for e in eng.values():
            e.close()


@pytest.mark.parametrize("dirs", pc.MOTOR_DIRS)
def test_control_step_caller_rpm(orc, dirs):
    """fmskf_control on a caller's rpm (curr_to_raw(amp, dir, lim) per wheel) against orc.CtrlBatch"""
    n = 1001
    rng = np.random.default_rng(5)
    inp = seq_ref.Inputs("kf6", n, 2, 12)
    ref = orc.CtrlBatch(n, motor_dir=dirs)
    with Engine("kf6", n, motor_dir=dirs) as e:
        e.set_power(None)
        ref.set_power(np.ones(n, np.uint8))
        e.set_target_vel(*inp.target(0))
        ref.set_target_vel(*inp.target(0))
        for t in range(T):
            rpm = rng.integers(-9000, 9000, (n, 4)).astype(np.int16)
            e.control(rpm)
            ref.step(rpm)
        got = e.get_ctrl()
        frames = e.can_tx()
    eq(got["curr"], ref.curr(), "curr")
    eq(got["wheel_tgt"], ref.wheel("tgt"), "wheel_tgt")
    eq(got["wheel_ctrl"], ref.wheel("ctrl"), "wheel_ctrl")
    eq(frames, orc.can_tx(ref.curr()), "0x200 frames")
    assert np.any(ref.curr() != 0)
