"""The library against the firmware's own VEHICLE_CTRL, MOTOR_IF_M2006, VelInterpConstJerk and
IMU_IF_WT901C (GPU).

tests/golden/vehicle_ref.npz and imu_ref.npz hold what the reference's own files answered,
compiled against the stand-in headers of oracle/ref_standin/ (generators: tests/golden/
make_golden_vehicle.py, make_golden_imu.py; tests/test_vehicle_golden_cpu.py holds the oracle to
the same files).  Here a handle of n = 1037 robots replays them, robot i scenario i % S, so
every scenario also sits in the ragged last block; a handle holds the motor directions and the
controller gains once, so the scenarios of one config group share a handle.

Call shapes, each against the fixture bit for bit (the 0x200 frames every tick; pose, velocity,
velocity targets, raw currents, fmskf_get_motors and fmskf_get_motor_status every 8th tick and
at the end):
  split    fmskf_ingest_can (with the present mask on the ticks that have one, k_can4 on the
           others) + fmskf_tick + fmskf_control + fmskf_can_tx
  isr      fmskf_ingest_can + fmskf_isr_tick on the ingested state
  isr_can  fmskf_isr_tick_can (one kernel), the scenarios without masks
KF6 and EKF9 handles run the same CAN and control scenarios (isr, isr_can); their motor state,
currents and frames are compared, their estimator state has no firmware counterpart.

IMU: fmskf_ingest_wt901 at strides 48 (the vector kernel) and 96 (the byte-load kernel) with the
fixture's latches; fmskf_get_imu gives the fixture's pages and is_error after every poll, and an
RS handle's fmskf_correct with no yaw plane gives theta = deg2rad(page.angle[2]).

As for the CPU test, the CMSIS sine table stays pinned by the project's restatement alone
(the stand-in arm_sin_f32 / arm_cos_f32 forward to it).
"""
import numpy as np
import pytest

import golden_replay as gr
from fmskf import Engine
from golden_replay import bits

pytestmark = pytest.mark.gpu

VEH = gr.load(gr.VEHICLE_NPZ)
IMU = gr.load(gr.IMU_NPZ)
N = 1037
S, T = VEH["frames"].shape[:2]
GROUPS = range(len(VEH["group_dirs"]))


def _scenarios(g, masked):
    """the scenarios of config group g; masked=False: those whose wheels never miss a frame"""
    idx = np.flatnonzero(VEH["group"] == g)
    if not masked:
        idx = np.array([s for s in idx if (VEH["present"][s] == 15).all()])
    return idx


def _tick_inputs(model, yaw):
    if model == "rs":
        return dict(yaw_deg=yaw)
    if model == "kf6":
        return dict(yaw_deg=yaw, gyro_z_dps=np.zeros_like(yaw))
    raw = np.zeros((yaw.size, 8), np.int16)  # yaw, gz, ax, ay words; the wheels come from the motor state
    raw[:, 0] = np.clip(np.rint(yaw / 180.0 * 32768.0), -32768, 32767).astype(np.int16)
    return dict(raw=raw)


def _compare_state(e, model, d, idx, t):
    where = f"tick {t}"
    if model == "rs":
        np.testing.assert_array_equal(bits(e.get_pose()), bits(d["pose"][idx, t].T), err_msg=f"{where} pose")
        np.testing.assert_array_equal(bits(e.get_vel()), bits(d["vel"][idx, t].T), err_msg=f"{where} velocity")
    c = e.get_ctrl()
    np.testing.assert_array_equal(bits(c["vel_tgt"]), bits(d["vel_tgt"][idx, t].T), err_msg=f"{where} velocity targets")
    np.testing.assert_array_equal(c["curr"], d["curr"][idx, t], err_msg=f"{where} raw currents")
    m = e.get_motors()
    st_i, st_f = d["st_i16"][idx, t], d["st_f32"][idx, t]
    np.testing.assert_array_equal(m["angle"], st_i[..., 1], err_msg=f"{where} motors angle")
    np.testing.assert_array_equal(m["rpm"], st_i[..., 2], err_msg=f"{where} motors rpm")
    np.testing.assert_array_equal(m["curr"], st_i[..., 3], err_msg=f"{where} motors current")
    np.testing.assert_array_equal(m["angle_sum"], d["angle_sum"][idx, t].T, err_msg=f"{where} angle sums")
    np.testing.assert_array_equal(bits(m["speed_radps"]), bits(np.ascontiguousarray(st_f[..., 1].T)), err_msg=f"{where} motors speed")
    s = e.get_motor_status()
    for k, f in enumerate(("microsec_id", "angle", "rpm", "curr")):
        np.testing.assert_array_equal(s[f], st_i[..., k], err_msg=f"{where} status {f}")
    for k, f in enumerate(("dlt_out_angle_rad", "speed_radps")):
        np.testing.assert_array_equal(bits(s[f]), bits(np.ascontiguousarray(st_f[..., k])), err_msg=f"{where} status {f}")


def _run(model, g, shape):
    d = VEH
    scen = _scenarios(g, masked=shape != "isr_can")
    assert scen.size >= 2
    idx = scen[np.arange(N) % scen.size]
    pw = {s: gr.power_events(d, s) for s in scen}
    tg = {s: gr.target_events(d, s) for s in scen}
    want_frames = gr.tx_frames(d["curr"])  # [S][T][8]
    masked_ticks = 0
    with Engine(model, N, motor_dir=[int(x) for x in d["group_dirs"][g]]) as e:
        e.set_ctrl_params(**gr.engine_ctrl_params(d, g))
        on = np.zeros(N, np.uint8)  # isPowerOn starts false on the firmware
        e.set_power(on)
        for t in range(T):
            ev = [s for s in scen if t in pw[s]]
            if ev:
                for s in ev:
                    on[idx == s] = pw[s][t]
                e.set_power(on)
            ev = [s for s in scen if t in tg[s]]
            if ev:
                val, mask = np.zeros((3, 3, N), np.float32), np.zeros(N, np.uint8)
                for s in ev:
                    val[:, :, idx == s] = tg[s][t][:, :, None]
                    mask[idx == s] = 1
                e.set_target_vel(val[0], val[1], val[2], mask)
            f = np.ascontiguousarray(d["frames"][idx, t])
            st = np.ascontiguousarray(d["stamps"][idx, t])
            pres = np.ascontiguousarray(d["present"][idx, t])
            kw = _tick_inputs(model, np.ascontiguousarray(d["yaw_deg"][idx, t]))
            if shape == "isr_can":
                fr = e.isr_tick_can(f, st, **kw)
            else:
                if (pres != 15).any():
                    masked_ticks += 1
                    e.ingest_can(f, st, present=pres)
                else:
                    e.ingest_can(f, st)
                if shape == "isr":
                    fr = e.isr_tick(**kw)
                else:
                    e.tick(**kw)
                    e.control()
                    fr = e.can_tx()
            np.testing.assert_array_equal(fr, want_frames[idx, t], err_msg=f"0x200 frames at tick {t}")
            if t % 8 == 7 or t == T - 1:
                _compare_state(e, model, d, idx, t)
    if shape != "isr_can":
        assert 0 < masked_ticks < T  # both CAN RX kernels ran


@pytest.mark.parametrize("shape", ["split", "isr", "isr_can"])
@pytest.mark.parametrize("g", GROUPS)
def test_rs_replays_firmware_fixture(g, shape):
    _run("rs", g, shape)


@pytest.mark.parametrize("shape", ["isr", "isr_can"])
@pytest.mark.parametrize("g", GROUPS)
@pytest.mark.parametrize("model", ["kf6", "ekf9"])
def test_kf_handles_replay_firmware_can_and_control(model, g, shape):
    _run(model, g, shape)


def _latch_groups():
    """streams that latch on the same polls share a handle (the latch flag is one per call)"""
    groups = {}
    for name, polls in gr.imu_streams(IMU):
        key = tuple(k for k, p in enumerate(polls) if p[1])
        groups.setdefault(key, []).append((name, polls))
    return groups


@pytest.mark.parametrize("stride", [48, 96])
def test_imu_replays_firmware_fixture(orc, stride):
    groups = _latch_groups()
    assert len(groups) >= 3 and max(len(v) for v in groups.values()) >= 4
    for latches, streams in groups.items():
        which = np.arange(N) % len(streams)
        npoll = max(len(p) for _, p in streams)
        with Engine("rs", N) as e:
            for k in range(npoll):
                buf, lens = np.zeros((N, stride), np.uint8), np.zeros(N, np.uint32)
                want, werr, live = np.zeros((16, N), np.float32), np.zeros(N, np.uint8), np.zeros(N, bool)
                for j, (_, polls) in enumerate(streams):
                    if k < len(polls):  # a stream that has ended sends empty polls and is not compared
                        b, _, data, err = polls[k]
                        buf[which == j, :b.size], lens[which == j] = b, b.size
                        want[:, which == j], werr[which == j], live[which == j] = data[:, None], err, True
                e.ingest_wt901(buf, lens, latch_qinit=k in latches)
                data, err = e.get_imu()
                where = f"streams {[n for n, _ in streams]} poll {k}"
                np.testing.assert_array_equal(bits(data[:, live]), bits(want[:, live]), err_msg=f"{where} Data page")
                np.testing.assert_array_equal(err[live], werr[live], err_msg=f"{where} is_error")
                e.correct()  # no yaw plane: set_now_yaw_world(deg2rad(getYawDate()))
                th = np.array([orc.deg2rad(float(v)) for v in want[11]], np.float32)
                np.testing.assert_array_equal(bits(e.get_pose()[2][live]), bits(th[live]), err_msg=f"{where} theta")
