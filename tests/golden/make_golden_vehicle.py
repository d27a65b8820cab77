"""Generate tests/golden/vehicle_ref.npz from the REFERENCE's own VEHICLE_CTRL.

Runs VDT::VEHICLE_CTRL::update with four MOTOR_IF_M2006 (rx_callback), four UTIL::FF_PI_D and
three UTIL::VelInterpConstJerk (src/VehicleDrive/VD_vehicle_controller.cpp, VD_motor_if_m2006.cpp,
src/Utility/util_vel_interp.hpp, util_mymath.hpp, util_controller.hpp, util_iir.hpp; compiled
unmodified from /root/reference by oracle/Makefile into oracle/_ref/libvehicle_ref.so, built the
way VD_task_main.cpp:75-108,157-160 builds them) over seeded scenarios.  Every tick feeds the
wheels' C610 frames that are present, then set_now_yaw_world(deg2rad(yaw)) and update(), and
records the pose, the velocity, the velocity target, get_rawCurr_tgt x4, get_rawAngleSum x4
and get_status_latest x4.  The file stores every input and every recorded output of every tick.

The reference files need Arduino.h and CMSIS-DSP, which do not exist here; oracle/ref_standin/
holds stand-ins (fixed-width integers, PI, arm_sqrt_f32 as the correctly rounded square root).
arm_sin_f32 / arm_cos_f32 forward to the oracle's own restatement of the CMSIS table algorithm:
this fixture does NOT pin that algorithm.

Scenarios run in config groups (motor directions, controller gains, current limit: the things
a handle of the library holds once for all its robots):
  group 0  firmware directions (1, 1, -1, -1), firmware gains, current limit 3000
  group 1  every direction +1, firmware gains
  group 2  directions (-1, 1, 1, -1), custom gains with a D term at ctrl_freq_hz = 1000,
           current limit 32767 (raw current commands between 32768 and 2^31: the int16 narrowing)
They cover: both direction branches of rx_callback; frame angles with the top bits set; stamps
that wrap at 0x7FFF and at 16 bits; wheels that miss frames (a present mask), whole ticks
without a frame; the int32 +-4096 delta wrap of the speed path and the int16 one of the sum;
angle sums past +-2^15; headings across +-180 and at exactly -180, 0 and 179.99 degrees; a
trapezoid, the short-move square-root branch, retargets in each of the three phases, a sign
reversal, a target equal to the current velocity, MOVE and STOP accelerations / jerks, power off
in mid-ramp and on again; saturation of the feed-forward, the integrator and the current limit.

Left out, because an x86 build of the firmware does not behave there as the Cortex-M7 does (the
oracle's ARM-semantics known answers stay the only pin; asserted before the reference is called):
equal successive stamps of a wheel (usec_dlt == 0 traps on x86; the first frame against the
zeroed status included) and a float -> int conversion of a NaN or a value outside int32
(checked on the oracle's wheel_ctrl).

Run only where /root/reference exists:  python tests/golden/make_golden_vehicle.py
The output is data (inputs and expected outputs), committed; nothing of the reference travels
with it.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle  # noqa: E402

OUT = os.path.join(HERE, "vehicle_ref.npz")
T = 320
GAIN_KEYS = ["c_freq", "ff", "pg", "ig", "dg", "ilim", "lpf", "fflim", "ts", "clim"]
FIRMWARE = dict(oracle.CTRL_DEFAULTS)
CUSTOM = dict(c_freq=1000.0, ff=0.01, pg=0.12, ig=0.3, dg=0.002, ilim=2.0, lpf=35.0, fflim=1.5,
              ts=np.float32(1.0) / np.float32(1000.0), clim=32767)
GROUPS = [((1, 1, -1, -1), FIRMWARE), ((1, 1, 1, 1), FIRMWARE), ((-1, 1, 1, -1), CUSTOM)]
# VD_task_main.cpp:29-48
MOVE = ([1000.0, 1000.0, 30.0], [10000.0, 10000.0, 300.0])
STOP = ([2000.0, 2000.0, 70.0], [30000.0, 30000.0, 1000.0])


def _be16(v):
    u = np.asarray(v, np.int64) & 0xFFFF
    return (u >> 8).astype(np.uint8), (u & 0xFF).astype(np.uint8)


def wheel_frames(rng, dirs, speed, top_bits=0.0, random_angle=0.0):
    """C610 frames [T][4][8] for wheels turning `speed` [T][4] counts per tick in the vehicle's
    sense (what rx_callback sums after the direction): sensor angle, rpm, a current; the two
    reserved bytes zero.  top_bits / random_angle: share of frames whose angle word has bits
    13-15 set / is any 16-bit word."""
    d = np.asarray(dirs, np.int64)[None, :]
    pos = np.cumsum(np.rint(speed).astype(np.int64), axis=0) + rng.integers(0, 8192, (1, 4))
    ang = np.mod(pos * d, 8192)
    hi = rng.random(ang.shape) < top_bits
    ang = np.where(hi, ang | (rng.integers(1, 8, ang.shape) << 13), ang)
    rnd = rng.random(ang.shape) < random_angle
    ang = np.where(rnd, rng.integers(0, 65536, ang.shape), ang)
    rpm = np.clip(np.rint(speed * (60000.0 / 8192.0)), -32768, 32767).astype(np.int64) * d
    cur = (rpm // 8) + 100
    fr = np.zeros(speed.shape + (8,), np.uint8)
    for k, v in enumerate((ang, rpm, cur)):
        fr[..., 2 * k], fr[..., 2 * k + 1] = _be16(v)
    return fr


def smooth_speed(rng, peak, segments=6):
    """[T][4] piecewise-linear wheel speeds (counts per tick) within +-peak, both signs"""
    knots = np.sort(np.concatenate([[0, T - 1], rng.choice(np.arange(1, T - 1), segments - 1, replace=False)]))
    out = np.zeros((T, 4))
    for w in range(4):
        vals = rng.uniform(-peak, peak, knots.size)
        out[:, w] = np.interp(np.arange(T), knots, vals)
    return out


def stamps15(off=0):
    """the firmware's 15-bit microsecond stamps (they wrap 32767 -> 0 about every 33rd tick)"""
    t = np.arange(T)[:, None]
    return (((t + 1) * 1000 + np.arange(4)[None, :] * 7 + off) & 0x7FFF).astype(np.int16)


def stamps16(step=1000, off=0):
    """16-bit stamps: the int16 goes negative, so a delta leaves +-0x7FFF at the wrap"""
    t = np.arange(T, dtype=np.int64)[:, None]
    return (((t + 1) * step + np.arange(4)[None, :] * 7 + off) & 0xFFFF).astype(np.uint16).view(np.int16)


def yaw_walk(rng, start, rate, exact=()):
    """headings in degrees wrapped into [-180, 180), with exact values planted at given ticks"""
    y = start + np.cumsum(rate + rng.normal(0, 0.05, T))
    y = ((y + 180.0) % 360.0) - 180.0
    y = y.astype(np.float32)
    for t, v in exact:
        y[t] = np.float32(v)
    return y


def scenarios(rng):
    """list of dicts: name, group, frames, stamps, present, yaw, power [(tick, on)],
    targets [(tick, vel, acl, jrk)]"""
    S = []
    full = np.full(T, 15, np.uint8)

    def add(name, group, speed, stamps, yaw, power, targets, present=None, **kw):
        S.append(dict(name=name, group=group, frames=wheel_frames(rng, GROUPS[group][0], speed, **kw),
                      stamps=stamps, present=full.copy() if present is None else present, yaw=yaw,
                      power=power, targets=targets))

    def tg(t, vel, set_=MOVE):
        return (t, vel, set_[0], set_[1])

    # ---- group 0: firmware directions and gains
    add("trapezoid_then_stop", 0, smooth_speed(rng, 300), stamps15(), yaw_walk(rng, 170.0, 0.2, [(5, -180.0), (6, 0.0), (7, 179.99)]),
        [(0, 1)], [tg(2, [150.0, 0.0, 0.0]), tg(262, [0.0, 0.0, 0.0], STOP)])
    add("short_move_sqrt", 0, smooth_speed(rng, 1500), stamps15(3), yaw_walk(rng, -175.0, -0.3),
        [(0, 1)], [tg(1, [50.0, -30.0, 0.5]), tg(200, [50.0, -30.0, 0.5]), tg(260, [-20.0, 10.0, -0.2])])
    add("retarget_each_phase", 0, smooth_speed(rng, 3900), stamps15(11), yaw_walk(rng, 0.0, 1.7),
        # x axis: 50 falls in the jerk-up phase, 160 in the constant-acceleration phase; a retarget in the
        # jerk-down phase is random_angle_words' at 150 (tests/test_vehicle_golden_cpu.py counts them)
        [(0, 1)], [tg(3, [200.0, 120.0, 2.0]), tg(50, [260.0, 60.0, 3.0]), tg(160, [80.0, 200.0, 1.0], STOP),
                   tg(215, [300.0, -100.0, 4.0]), tg(285, [0.0, 0.0, 0.0], STOP)])
    add("sign_reversal", 0, smooth_speed(rng, 3500), stamps15(), yaw_walk(rng, 179.0, 0.05, [(100, 179.99), (101, -180.0)]),
        [(0, 1)], [tg(1, [200.0, 0.0, 6.0]), tg(180, [-200.0, 0.0, -6.0]), tg(300, [-200.0, 0.0, -6.0])])
    add("power_cycle_mid_ramp", 0, smooth_speed(rng, 2000), stamps15(), yaw_walk(rng, 30.0, -2.5),
        [(0, 1), (90, 0), (140, 1), (141, 0), (150, 1)],
        [tg(2, [400.0, -400.0, 0.0]), tg(100, [100.0, 0.0, 0.0]), tg(145, [100.0, 100.0, 1.0]), tg(160, [-300.0, 50.0, -2.0], STOP)])
    pres = full.copy()
    miss = rng.random(T) < 0.3
    pres[miss] = rng.integers(0, 16, int(miss.sum())).astype(np.uint8)
    pres[0] = 15
    add("missed_frames_stamps16", 0, smooth_speed(rng, 900), stamps16(1000), yaw_walk(rng, -90.0, 0.4),
        [(0, 1)], [tg(4, [120.0, 80.0, -1.0])], present=pres)
    sp = smooth_speed(rng, 3000)
    sp[120:130] = 0.0  # ticks where no wheel moved
    add("standstill_and_top_bits", 0, sp, stamps16(1371, 5), yaw_walk(rng, 0.0, 0.0, [(120, 0.0), (121, -180.0)]),
        [(10, 1)], [tg(0, [90.0, 0.0, 0.0]), tg(20, [90.0, 0.0, 0.0]), tg(220, [0.0, -250.0, 0.0])], top_bits=0.2)
    add("random_angle_words", 0, smooth_speed(rng, 500), stamps15(29), yaw_walk(rng, 100.0, 3.0),
        [(0, 1)], [tg(5, [-60.0, 40.0, 1.5]), tg(150, [10.0, 10.0, 0.0], STOP)], random_angle=0.15)
    # ---- group 1: every direction +1
    one = np.ones((T, 4))
    add("all_plus_forward_fast", 1, one * np.linspace(500, 4000, T)[:, None], stamps15(), yaw_walk(rng, -179.5, -0.01),
        [(0, 1)], [tg(1, [400.0, 0.0, 0.0])])
    add("all_plus_backward_fast", 1, -one * np.linspace(4000, 800, T)[:, None], stamps16(1000, 17), yaw_walk(rng, 45.0, 0.9),
        [(0, 1)], [tg(1, [-400.0, 0.0, 0.0]), tg(250, [0.0, 0.0, 0.0], STOP)])
    pres = full.copy()
    pres[5::7] = 0b1010
    pres[9::13] = 0
    add("all_plus_masked_top_bits", 1, smooth_speed(rng, 2500), stamps16(997, 3), yaw_walk(rng, 0.0, -1.1),
        [(0, 1), (200, 0), (230, 1)], [tg(2, [0.0, 300.0, -3.0]), tg(120, [0.0, 300.0, 3.0]), tg(240, [150.0, 0.0, 0.0])],
        present=pres, top_bits=0.1)
    add("all_plus_rotation", 1, smooth_speed(rng, 1200) * np.array([-1, -1, 1, 1]), stamps15(101), yaw_walk(rng, 10.0, 5.0),
        [(0, 1)], [tg(1, [0.0, 0.0, 6.0]), tg(150, [0.0, 0.0, -18.0]), tg(300, [0.0, 0.0, 0.0], STOP)])
    # ---- group 2: custom gains (a D term at 1000 Hz), current limit 32767
    add("custom_big_currents", 2, smooth_speed(rng, 300), stamps15(), yaw_walk(rng, 0.0, 0.3),
        [(0, 1)], [tg(1, [400.0, 0.0, 0.0]), tg(200, [-400.0, 300.0, 0.0], STOP)])
    add("custom_tracking", 2, smooth_speed(rng, 3800), stamps16(1000, 9), yaw_walk(rng, -60.0, -0.7),
        [(0, 1)], [tg(1, [250.0, 250.0, 2.0]), tg(130, [250.0, -250.0, -2.0]), tg(260, [0.0, 0.0, 0.0])])
    pres = full.copy()
    pres[rng.random(T) < 0.15] = 0b0110
    add("custom_masked_power", 2, smooth_speed(rng, 2200), stamps16(1003, 1), yaw_walk(rng, 178.0, 0.6),
        [(0, 1), (170, 0), (175, 1)], [tg(3, [-300.0, 100.0, 5.0]), tg(60, [300.0, -100.0, -5.0]), tg(180, [50.0, 50.0, 0.0])],
        present=pres, random_angle=0.05)
    add("custom_equal_target_top_bits", 2, smooth_speed(rng, 3999), stamps15(55), yaw_walk(rng, 0.0, 0.0, [(50, 179.99), (51, -180.0), (52, 0.0)]),
        [(0, 1)], [tg(1, [0.0, 0.0, 0.0]), tg(20, [330.0, 0.0, 0.0]), tg(300, [330.0, 0.0, 0.0])], top_bits=0.3)
    return S


def check_exclusions(sc):
    """the x86 exclusions that can be seen in the inputs: a present wheel never repeats its last stamp
    (the status starts zeroed, so the first stamp is not 0 either)"""
    last = np.zeros(4, np.int64)
    for t in range(T):
        for w in range(4):
            if (int(sc["present"][t]) >> w) & 1:
                assert int(sc["stamps"][t, w]) != last[w], (sc["name"], t, w, "equal successive stamps")
                last[w] = int(sc["stamps"][t, w])


def check_float_to_int(sc, prm, dirs):
    """replay on the oracle: no wheel's current command leaves int32 or is a NaN"""
    mb = oracle.MotorBatch(1, dirs)
    cb = oracle.CtrlBatch(1, prm, dirs)
    pw, tg = dict(sc["power"]), {e[0]: e[1:] for e in sc["targets"]}
    for t in range(T):
        if t in pw:
            cb.set_power(pw[t])
        if t in tg:
            cb.set_target_vel(*(np.asarray(a, np.float32)[:, None] for a in tg[t]))
        mb.rx(sc["frames"][t][None], sc["stamps"][t][None], sc["present"][t:t + 1])
        cb.step(mb.field("rpm"))
        raw = cb.wheel("ctrl").astype(np.float64) * 1000.0
        assert np.all(np.isfinite(raw)) and np.all(np.abs(raw) < 2.0 ** 31), (sc["name"], t, raw)


def run_reference(sc, prm_kw, dirs):
    v = oracle.RefVehicle(dirs, **prm_kw)
    out = dict(pose=[], vel=[], vel_tgt=[], curr=[], angle_sum=[], st_i16=[], st_f32=[])
    pw, tg = dict(sc["power"]), {e[0]: e[1:] for e in sc["targets"]}
    for t in range(T):
        if t in pw:
            v.power(pw[t])
        if t in tg:
            v.set_target_vel(*tg[t])
        for w in range(4):
            if (int(sc["present"][t]) >> w) & 1:
                v.rx(w, sc["frames"][t, w], sc["stamps"][t, w])
        v.tick(sc["yaw"][t])
        r = v.read()
        for k in out:
            out[k].append(r[k])
    v.close()
    return {k: np.stack(a) for k, a in out.items()}


def generate():
    """the fixture as a dict of arrays"""
    oracle.build()
    rng = np.random.default_rng(0x56484343)
    scs = scenarios(rng)
    outs = []
    for sc in scs:
        dirs, g = GROUPS[sc["group"]]
        sc["frames"] = np.ascontiguousarray(sc["frames"])
        sc["stamps"] = np.ascontiguousarray(sc["stamps"])
        check_exclusions(sc)
        check_float_to_int(sc, oracle.ctrl_params(**g), dirs)
        outs.append(run_reference(sc, g, dirs))
    pev = [(s, t, on) for s, sc in enumerate(scs) for t, on in sc["power"]]
    tev = [(s, e[0]) for s, sc in enumerate(scs) for e in sc["targets"]]
    tval = [e[1:] for sc in scs for e in sc["targets"]]
    d = dict(name=np.array([sc["name"] for sc in scs]), group=np.array([sc["group"] for sc in scs], np.int32),
             group_dirs=np.array([g[0] for g in GROUPS], np.int8), gain_keys=np.array(GAIN_KEYS),
             group_gains=np.array([[float(g[1][k]) for k in GAIN_KEYS] for g in GROUPS], np.float32),
             frames=np.stack([sc["frames"] for sc in scs]), stamps=np.stack([sc["stamps"] for sc in scs]),
             present=np.stack([sc["present"] for sc in scs]), yaw_deg=np.stack([sc["yaw"] for sc in scs]),
             power_ev=np.array(pev, np.int32), target_ev=np.array(tev, np.int32),
             target_val=np.array(tval, np.float32))
    for k in outs[0]:
        d[k] = np.stack([o[k] for o in outs])
    return d


def main():
    d = generate()
    np.savez_compressed(OUT, **d)
    print(f"wrote {OUT}: {len(d['name'])} scenarios x {T} ticks, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
