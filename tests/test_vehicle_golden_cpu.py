"""The oracle against the firmware's own VEHICLE_CTRL, MOTOR_IF_M2006, VelInterpConstJerk and
IMU_IF_WT901C (CPU).

tests/golden/vehicle_ref.npz and imu_ref.npz hold what the reference's own files answered,
compiled against the stand-in headers of oracle/ref_standin/ (generators: tests/golden/
make_golden_vehicle.py, make_golden_imu.py, which list the scenarios).  Here the oracle's
restatement replays every input and must give every recorded output at every tick or poll, bit
for bit: M2006 and MotorBatch (rx_callback: angle, rpm, current, stamp, the angle delta, the
filtered speed, the int64 sum), rs_tick (the pose and the velocity), CtrlBatch (the velocity
targets and the raw currents) and can_tx (the 0x200 payload of those currents), Wt901 (the Data
page and is_error).

Not pinned by these fixtures: arm_sin_f32 / arm_cos_f32 (the stand-in forwards them to the
oracle's own table restatement); equal successive stamps, float -> int conversions of NaN or
out-of-range values and a latch on a poll without a quaternion frame (an x86 build of the
firmware does not behave there as the Cortex-M7 does; tests/test_oracle_known_answers.py keeps
their ARM semantics).

Found by these fixtures, both in init() (the q_init latch): it does not write is_error, so a
latching poll after a failed one leaves the flag set (the restatement and the kernel cleared
it); and it begins with WitInit, which empties the parser window, so the head of a frame split
across the poll before is dropped (they kept it and completed the frame).

test_fixtures_regenerate runs only where the reference was built (oracle/_ref): both
generators, run again, must give the committed files.
"""
import importlib.util
import os

import numpy as np
import pytest

import golden_replay as gr
from golden_replay import bits

VEH = gr.load(gr.VEHICLE_NPZ)
IMU = gr.load(gr.IMU_NPZ)
S, T = VEH["frames"].shape[:2]
ST_I16 = ("micro", "angle", "rpm", "curr")          # MOTOR_IF_M2006::Status, in the fixture's order
ST_F32 = ("dlt_out_angle_rad", "speed_radps")


def test_fixture_covers_what_it_claims():
    """the scenarios hold the cases their generator lists (a later regeneration cannot lose them)"""
    d = VEH
    assert S >= 16 and 300 <= T <= 600
    dirs = {tuple(int(x) for x in r) for r in d["group_dirs"]}
    assert (1, 1, 1, 1) in dirs and (1, 1, -1, -1) in dirs and len(dirs) >= 3
    ang = (d["frames"][..., 0].astype(np.int32) << 8) | d["frames"][..., 1]
    assert (ang >= 8192).any() and (ang >= 32768).any()          # top bits set, negative words
    assert not d["frames"][..., 6:].any()                         # the reserved bytes
    st = d["stamps"].astype(np.int64)
    dl = np.diff(st, axis=1)
    assert (dl < 0).any() and (np.abs(dl) > 0x7FFF).any()         # wraps at 15 and at 16 bits
    assert (d["present"] == 0).any() and ((d["present"] != 0) & (d["present"] != 15)).any()
    assert d["angle_sum"].max() > 2 ** 15 and d["angle_sum"].min() < -2 ** 15
    # both delta wraps disagree somewhere: the int32 path and the int16 path of rx_callback
    a = d["st_i16"][..., 1].astype(np.int64)
    da = np.diff(a, axis=1)
    assert (np.abs(da) > 4096).any() and (np.abs(da) > 32767).any()
    y = d["yaw_deg"]
    for v in (-180.0, 0.0, 179.99):
        assert (y == np.float32(v)).any(), v
    assert (np.abs(np.diff(y.astype(np.float64), axis=1)) > 300).any()   # across +-180
    moved = np.diff(d["angle_sum"], axis=1)
    assert (moved == 0).all(axis=2).any()                         # a tick where no wheel moved
    c = d["curr"].astype(np.int64)
    g0 = d["group"] == 0
    assert (np.abs(c[g0]) == 3000).any()                          # the current limit saturates
    assert (np.abs(c[d["group"] == 2]) > 3000).any()              # the high limit lets more through
    assert {int(on) for _, _, on in d["power_ev"]} == {0, 1}
    acl = {float(v[1][0]) for v in d["target_val"]}
    assert acl == {1000.0, 2000.0}                                # the MOVE and the STOP sets
    k = list(d["gain_keys"])
    assert (d["group_gains"][:, k.index("dg")] > 0).any() and (d["group_gains"][:, k.index("c_freq")] == 1000).any()
    names = [n for n, _ in gr.imu_streams(IMU)]
    assert len(names) >= 6
    assert IMU["latch"].sum() > len(names) and IMU["is_error"].any()
    # a latching poll that begins inside a frame (the rest of one split across the poll before)
    first = [p[0][0] for _, polls in gr.imu_streams(IMU) for p in polls if p[1]]
    assert sum(b != 0x55 for b in first) >= 2
    roll = IMU["data"][:, 9]
    assert (roll < -1).any() and (roll > 1).any() and (roll == -180.0).any()


def test_fixture_retargets_in_every_phase(orc):
    """the interpolator is retargeted in its jerk-up, constant-acceleration and jerk-down phases
    (acl_ini != 0) and after the end of a move, read off the oracle's interpolator state of the x
    axis, which the tests below hold to the fixture"""
    d = VEH
    seen = set()
    for s in range(S):
        cb = orc.CtrlBatch(1, orc.ctrl_params(**gr.group_gains(d, int(d["group"][s]))))
        pw, tg = gr.power_events(d, s), gr.target_events(d, s)
        ts = float(cb.p.ts)
        for t in range(T):
            if t in pw:
                cb.set_power(pw[t])
            if t in tg:
                a = cb.c[0].ax[0]
                ph = 1 if a.dt <= a.dt1 + ts else 2 if a.dt <= a.dt1 + a.dt2 + ts else 3 if a.dt <= a.dt1 + a.dt2 + a.dt3 + ts else 4
                seen.add((ph, a.acl_now != 0.0))
                cb.set_target_vel(*(tg[t][k][:, None] for k in range(3)))
            cb.step(np.zeros((1, 4), np.int16))
    assert {(1, True), (2, True), (3, True), (4, False)} <= seen, seen


def test_fixture_saturates_the_controller(orc):
    """the feed-forward limit, the integrator limit and the int16 narrowing are reached: read off
    the oracle's FF_PI_D state (which the tests below hold to the fixture's currents).  Under the
    32767 limit of the custom group a raw command amp * 1000 lies between 32768 and 2^31, so
    set_CurrA_tgt's (int16_t) cast keeps its low 16 bits."""
    d = VEH
    seen = {}
    for s in range(S):
        g = int(d["group"][s])
        kw = gr.group_gains(d, g)
        dirs = [int(x) for x in d["group_dirs"][g]]
        mb, cb = orc.MotorBatch(1, dirs), orc.CtrlBatch(1, orc.ctrl_params(**kw), dirs)
        pw, tg = gr.power_events(d, s), gr.target_events(d, s)
        for t in range(T):
            if t in pw:
                cb.set_power(pw[t])
            if t in tg:
                cb.set_target_vel(*(tg[t][k][:, None] for k in range(3)))
            mb.rx(d["frames"][s, t][None], d["stamps"][s, t][None], d["present"][s, t:t + 1])
            cb.step(mb.field("rpm"))
            raw = np.abs(cb.wheel("ctrl").astype(np.float64)) * 1000.0
            hit = seen.setdefault(g, dict(ff=0, integ=0, narrow=0))
            hit["ff"] += int((np.abs(cb.wheel("tgt").astype(np.float64) * kw["ff"]) >= kw["fflim"]).any())
            hit["integ"] += int((np.abs(cb.wheel("integ")) == np.float32(kw["ilim"])).any())
            hit["narrow"] += int(((raw >= 32768.0) & (raw < 2.0 ** 31)).any())
            assert (raw < 2.0 ** 31).all()
    for g in (0, 2):  # the firmware's gains and the custom set
        assert seen[g]["ff"] > 10 and seen[g]["integ"] > 10, (g, seen[g])
    assert seen[2]["narrow"] > 100 and int(gr.group_gains(d, 2)["clim"]) == 32767, seen[2]


def _replay_single(orc, s):
    """scenario s through one robot's M2006 x4, rs_tick, CtrlBatch(1) and can_tx"""
    d = VEH
    g = int(d["group"][s])
    dirs = [int(x) for x in d["group_dirs"][g]]
    m = [orc.M2006(dr) for dr in dirs]
    cb = orc.CtrlBatch(1, orc.ctrl_params(**gr.group_gains(d, g)), dirs)
    pos, vel, prev = np.zeros((3, 1), np.float32), np.zeros((3, 1), np.float32), np.zeros((4, 1), np.int64)
    pw, tg = gr.power_events(d, s), gr.target_events(d, s)
    name = str(d["name"][s])
    for t in range(T):
        if t in pw:
            cb.set_power(pw[t])
        if t in tg:
            cb.set_target_vel(*(tg[t][k][:, None] for k in range(3)))
        for w in range(4):
            if (int(d["present"][s, t]) >> w) & 1:
                m[w].rx(d["frames"][s, t, w], int(d["stamps"][s, t, w]))
        where = f"{name} tick {t}"
        for w in range(4):
            got_i = np.array([getattr(m[w].s, f) for f in ST_I16], np.int16)
            np.testing.assert_array_equal(got_i, d["st_i16"][s, t, w], err_msg=f"{where} wheel {w} status")
            got_f = np.array([getattr(m[w].s, f) for f in ST_F32], np.float32)
            np.testing.assert_array_equal(bits(got_f), bits(d["st_f32"][s, t, w]), err_msg=f"{where} wheel {w} {ST_F32}")
            assert m[w].s.angle_sum == d["angle_sum"][s, t, w], f"{where} wheel {w} angle sum"
        sums = np.array([[m[w].s.angle_sum] for w in range(4)], np.int64)
        rpm = np.array([[m[w].s.rpm for w in range(4)]], np.int16)
        orc.rs_tick(pos, vel, prev, d["yaw_deg"][s, t:t + 1].copy(), sums, rpm)
        cb.step(rpm)
        np.testing.assert_array_equal(bits(pos[:, 0]), bits(d["pose"][s, t]), err_msg=f"{where} pose")
        np.testing.assert_array_equal(bits(vel[:, 0]), bits(d["vel"][s, t]), err_msg=f"{where} velocity")
        np.testing.assert_array_equal(bits(cb.vel_tgt()[:, 0]), bits(d["vel_tgt"][s, t]), err_msg=f"{where} velocity target")
        np.testing.assert_array_equal(cb.curr()[0], d["curr"][s, t], err_msg=f"{where} raw currents")
        np.testing.assert_array_equal(orc.can_tx(cb.curr())[0], gr.tx_frames(d["curr"][s, t]), err_msg=f"{where} 0x200 frame")


@pytest.mark.parametrize("s", range(S), ids=[str(n) for n in VEH["name"]])
def test_vehicle_fixture_oracle(orc, s):
    """one scenario, one robot: every recorded output at every tick"""
    _replay_single(orc, s)


@pytest.mark.parametrize("g", range(len(VEH["group_dirs"])))
def test_vehicle_fixture_oracle_batched(orc, g):
    """a config group's scenarios as one batch through MotorBatch (orc_can_ingest_batch with the
    present masks), rs_tick and CtrlBatch over n robots, each scenario three times"""
    d = VEH
    idx = np.tile(np.flatnonzero(d["group"] == g), 3)
    n = idx.size
    dirs = [int(x) for x in d["group_dirs"][g]]
    mb = orc.MotorBatch(n, dirs)
    cb = orc.CtrlBatch(n, orc.ctrl_params(**gr.group_gains(d, g)), dirs)
    pos, vel, prev = np.zeros((3, n), np.float32), np.zeros((3, n), np.float32), np.zeros((4, n), np.int64)
    pw = [gr.power_events(d, s) for s in idx]
    tg = [gr.target_events(d, s) for s in idx]
    on = np.zeros(n, np.uint8)
    for t in range(T):
        for i in range(n):
            if t in pw[i]:
                on[i] = pw[i][t]
        cb.set_power(on)
        mask = np.array([t in tg[i] for i in range(n)])
        if mask.any():
            val = np.zeros((3, 3, n), np.float32)
            for i in np.flatnonzero(mask):
                val[:, :, i] = tg[i][t]
            cb.set_target_vel(val[0], val[1], val[2], mask)
        mb.rx(d["frames"][idx, t], d["stamps"][idx, t], d["present"][idx, t])
        for k, f in enumerate(ST_I16):
            np.testing.assert_array_equal(mb.field(f), d["st_i16"][idx, t, :, k], err_msg=f"tick {t} {f}")
        for k, f in enumerate(ST_F32):
            np.testing.assert_array_equal(bits(mb.field(f)), bits(d["st_f32"][idx, t, :, k]), err_msg=f"tick {t} {f}")
        np.testing.assert_array_equal(mb.field("angle_sum"), d["angle_sum"][idx, t], err_msg=f"tick {t} sums")
        orc.rs_tick(pos, vel, prev, np.ascontiguousarray(d["yaw_deg"][idx, t]),
                    np.ascontiguousarray(mb.field("angle_sum").T), mb.field("rpm"))
        cb.step(mb.field("rpm"))
        np.testing.assert_array_equal(bits(pos.T), bits(d["pose"][idx, t]), err_msg=f"tick {t} pose")
        np.testing.assert_array_equal(bits(vel.T), bits(d["vel"][idx, t]), err_msg=f"tick {t} velocity")
        np.testing.assert_array_equal(bits(cb.vel_tgt().T), bits(d["vel_tgt"][idx, t]), err_msg=f"tick {t} targets")
        np.testing.assert_array_equal(cb.curr(), d["curr"][idx, t], err_msg=f"tick {t} currents")
    np.testing.assert_array_equal(orc.can_tx(cb.curr()), gr.tx_frames(d["curr"][idx, T - 1]))


def test_imu_fixture_oracle(orc):
    """every stream through Wt901 (one instance) and, stream against stream, through Wt901Batch:
    the Data page and is_error after every poll"""
    streams = list(gr.imu_streams(IMU))
    for name, polls in streams:
        w = orc.Wt901()
        for k, (b, latch, data, err) in enumerate(polls):
            w.update(b, latch_qinit=latch)
            np.testing.assert_array_equal(bits(w.data), bits(data), err_msg=f"{name} poll {k} Data page")
            assert int(w.is_error) == err, f"{name} poll {k} is_error (latch {latch})"
    # batched: streams that latch on the same polls share a Wt901Batch (one latch flag per call);
    # a stream that has ended sends empty polls and is no longer compared
    groups = {}
    for name, polls in streams:
        groups.setdefault(tuple(k for k, p in enumerate(polls) if p[1]), []).append((name, polls))
    assert len(groups) >= 3 and sum(len(k) > 1 for k in groups) >= 3   # second latches are among them
    for latches, members in groups.items():
        n = len(members)
        wb = orc.Wt901Batch(n)
        for k in range(max(len(p) for _, p in members)):
            buf, lens = np.zeros((n, 48), np.uint8), np.zeros(n, np.uint32)
            for i, (_, polls) in enumerate(members):
                if k < len(polls):
                    buf[i, :polls[k][0].size], lens[i] = polls[k][0], polls[k][0].size
            wb.update(buf, lens, latch_qinit=k in latches)
            page, err = wb.data, wb.is_error
            for i, (name, polls) in enumerate(members):
                if k < len(polls):
                    np.testing.assert_array_equal(bits(page[:, i]), bits(polls[k][2]), err_msg=f"batched {name} poll {k}")
                    assert int(err[i]) == polls[k][3], f"batched {name} poll {k} is_error"


def _generator(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(gr.GOLDEN, name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_fixtures_regenerate(orc):
    """where the reference's own files were built (oracle/_ref), the two generators give the
    committed fixtures again, array for array"""
    if not (os.path.exists(orc.REF_VEHICLE_PATH) and os.path.exists(orc.REF_IMU_PATH)):
        pytest.skip("oracle/_ref/libvehicle_ref.so and libimu_ref.so are built only where the reference exists")
    for name, have in (("make_golden_vehicle", VEH), ("make_golden_imu", IMU)):
        new = _generator(name).generate()
        assert sorted(new) == sorted(have), name
        for k in have:
            a, b = np.asarray(new[k]), have[k]
            assert a.dtype == b.dtype and a.shape == b.shape, (name, k, a.dtype, b.dtype, a.shape, b.shape)
            np.testing.assert_array_equal(bits(a) if a.dtype == np.float32 else a, bits(b) if b.dtype == np.float32 else b,
                                          err_msg=f"{name}: {k}")
