"""What a firmware-side caller reads -- fmskf_get_pose, fmskf_get_vel (k_readout) and
fmskf_export_vehicle_info (k_readout + k_vehicle_info) -- against tests/readout_ref.py, a numpy
reference of the state that was set (pinned on the CPU by tests/test_readout_cpu.py), for every
model, across tile boundaries of the tiled state, on the export's edge conversions, and through
device outputs and NULL pointers.  Every case but the frame-convention one is a set_state of
chosen values followed by a readout: no tick runs in between."""
import ctypes as C

import numpy as np
import pytest

import fmskf
import readout_ref as ref
from fmskf import Engine, synth
from fmskf._lib import CFG_COMP_POS, EINVAL, MEM_DEVICE, MEM_HOST, load

pytestmark = pytest.mark.gpu

NX = {"rs": 6, "kf6": 6, "ekf9": 9, "kf12d": 12}
TILE = {"rs": 2048, "kf6": 2048, "ekf9": 2048, "kf12d": 4096}  # robots per tile row (RS: planar)
ROTATED = ("kf6", "kf12d")  # world-frame velocity state, rotated by -theta at readout


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _assert_records_equal(got, want, what):
    """VehicleInfo records byte for byte; a mismatch names the field and the robots"""
    if got.tobytes() == want.tobytes():
        return
    for f in got.dtype.names:
        g, w = (np.ascontiguousarray(a[f]).reshape(len(a), -1) for a in (got, want))
        bad = np.flatnonzero((bits(g) != bits(w)).any(axis=1))
        if bad.size:
            i = int(bad[0])
            raise AssertionError(f"{what}: {f} differs on {bad.size} robots, first {bad[:8].tolist()}: "
                                 f"robot {i} got {g[i].tolist()}, want {w[i].tolist()}")
    raise AssertionError(f"{what}: records differ outside the named fields")


def _state(model, n, seed=0):
    """A dense state x [nx, n] in the model's element type, random per (row, robot) with a
    distinct scale per row, so that a wrong row, tile or robot index cannot return a matching
    value.  theta is spread over +-1e4 rad and includes exact 0, +-pi as float32 and values just
    beyond +-pi; velocities reach a few m/s."""
    rng = np.random.default_rng([seed, n, NX[model], ref.MODELS.index(model)])
    nx = NX[model]
    x = rng.normal(size=(nx, n)) * (3.0 * 1.7 ** np.arange(nx))[:, None]
    x[2] = rng.uniform(-1e4, 1e4, n)
    pi32 = float(np.float32(np.pi))
    special = [pi32, -pi32, 3.1415930, -3.1415930, 3.5, -3.5, 6.2831855, -100.25, 1.5707964, 0.0]
    for j, v in enumerate(special):
        x[2, (j * 23) % n] = v  # n = 1: the last one, exact 0
    x[3] = rng.uniform(-4.0, 4.0, n)
    x[4] = rng.uniform(-2.5, 2.5, n)
    if model == "rs":
        x[3:5] *= 1000.0  # RS keeps mm/s
    return np.ascontiguousarray(x.astype(np.float64 if model == "kf12d" else np.float32))


def _check_pose_vel(model, x, pose, vel, what):
    """Pose bit for bit; velocity bit for bit (RS, EKF9, every model's omega) or within the derived
    bound of the unrounded longdouble reference (KF6 / KF12D vbx, vby), on every lane.
    Returns the worst observed |got - ref| / bound."""
    assert pose.dtype == np.float32 and vel.dtype == np.float32
    np.testing.assert_array_equal(bits(pose), bits(ref.pose(model, x)), err_msg=f"{what}: pose")
    want = ref.vel(model, x)
    if model not in ROTATED:
        np.testing.assert_array_equal(bits(vel), bits(want), err_msg=f"{what}: vel")
        return 0.0
    np.testing.assert_array_equal(bits(vel[2]), bits(want[2].astype(np.float32)), err_msg=f"{what}: omega")
    assert np.isfinite(vel[:2]).all(), what
    err = np.abs(vel[:2].astype(np.longdouble) - want[:2]).astype(np.float64)
    bound = ref.body_vel_bound(want[:2], x[3], x[4])
    ratio = err / bound
    worst = float(ratio.max())
    k = np.unravel_index(int(ratio.argmax()), ratio.shape)
    # the narrowing alone brings the ratio close to 1 on some lane of thousands; whether the
    # allowance for the double arithmetic is used at all shows in the lanes that are not the
    # float nearest to the reference
    off = int((bits(vel[:2]) != bits(want[:2].astype(np.float32))).sum())
    print(f"{what}: worst |got - ref| / bound = {worst:.4f} (axis {k[0]}, robot {k[1]}, theta {x[2, k[1]]!r}); "
          f"{off} of {err.size} values are not the float nearest to the reference")
    assert (err <= bound).all(), f"{what}: {int((err > bound).sum())} lanes past the bound, worst ratio {worst}"
    return worst


# ----------------------------------------------------------------------------- (a)
A_CASES = [("rs", n, "") for n in (1, 257, 2049)] + \
          [("kf6", n, f) for n in (1, 255, 2047, 2049, 4099) for f in ("", "comp")] + \
          [("ekf9", n, "") for n in (1, 255, 2047, 2049, 4099)] + [("ekf9", 4099, "lo")] + \
          [("kf12d", n, "") for n in (1, 257, 4095, 4097, 8195)]


@pytest.mark.parametrize("model,n,variant", A_CASES)
def test_pose_vel_against_reference(model, n, variant):
    """get_pose / get_vel of a state set with set_state, against readout_ref, at sizes on both
    sides of one and two tile boundaries with a ragged tail.  KF6 also with FMSKF_CFG_COMP_POS
    and EKF9 once with a heading low part, both set non-zero: the pose is the hi rows.

    Bound of the KF6 / KF12D body velocity (readout_ref.body_vel_bound, derived, not measured):
    1/2 ulp_f32(ref) + 2^-48 * 1000 (|vx| + |vy|).  Measured on an MI355X (printed with -s): the
    worst ratio to it is 1.0000 (KF6 n = 2049, KF12D n = 4095 and 4097; 0.9997 - 0.9999 at the
    other sizes past one robot), which is the half ulp of the narrowing met on one lane of
    thousands: all 67,094 values are the float nearest to the reference, so the allowance for
    the double arithmetic is not drawn on."""
    x = _state(model, n)
    rng = np.random.default_rng(n)
    with Engine(model, n, flags=CFG_COMP_POS if variant == "comp" else 0) as e:
        e.set_state(x)
        if variant:  # low parts of the size of a rounding error of their hi rows, none zero
            rows = 5 if variant == "comp" else 1
            lo = (rng.uniform(0.25, 1.0, (rows, n)) * 2.0**-24).astype(np.float32)
            e.set_state_lo(lo)
            np.testing.assert_array_equal(bits(e.get_state_lo()), bits(lo))
        pose = e.get_pose()
        vel = e.get_vel()
    _check_pose_vel(model, x, pose, vel, f"{model} n={n} {variant}".strip())


# ----------------------------------------------------------------------------- (b)
def _motion(n):
    """constant inputs of n robots: one yaw each, spread over (-180, 180) degrees, and constant
    rpm of three patterns: forward, sideways, and turning while moving diagonally"""
    yaw = np.linspace(-179.0, 179.0, n).astype(np.float32)
    pat = np.arange(n) % 3
    fwd = np.where(pat == 0, 300.0, np.where(pat == 1, 0.0, 150.0))  # body mm/s
    left = np.where(pat == 0, 0.0, np.where(pat == 1, 250.0, -100.0))
    turn = np.where(pat == 2, 1.0, 0.0)  # rad/s
    wheel = synth.vdir_to_mdir(fwd, left, turn) * synth.GEAR / float(synth.RPM_TO_RADPS)
    rpm = np.ascontiguousarray(np.clip(np.rint(wheel), -32768, 32767).astype(np.int16))
    return yaw, rpm


def _kf12d_z(yaw, body_mmps):
    """kf12d measurements of the same motion: heading, no rotation, the body velocity turned
    into the world frame (m/s), an arm tip at rest"""
    th = np.radians(yaw.astype(np.float64))
    c, s = np.cos(th), np.sin(th)
    z = np.zeros((8, yaw.size))
    z[0] = th
    z[2] = (body_mmps[0] * c - body_mmps[1] * s) * 1e-3
    z[3] = (body_mmps[0] * s + body_mmps[1] * c) * 1e-3
    z[4], z[5], z[6] = 0.30, 0.05, 0.20
    return z


@pytest.mark.parametrize("model,T", [("kf6", 50), ("kf12d", 100)])
def test_body_frame_agrees_with_firmware_model(orc, model, T):
    """The frame convention of the KF6 / KF12D readout against the firmware-exact model.  An RS
    handle and a KF6 (KF12D) handle are driven with the same constant rpm and yaw for T ticks
    (KF12D: with z built from the RS body velocity turned into the world frame by the yaw).  RS's
    get_vel is the firmware's body velocity (VD_vehicle_controller.cpp:21-33, bit-exact against
    the reference binaries elsewhere); the filter's get_vel must agree with it in vx and vy.

    The bound comes from the CPU oracle alone: 10 x the largest |readout_ref rotation of the
    oracle's filter state - orc.rs_tick velocity| over robots and both axes.
    Measured (CPU oracle, deterministic): KF6, T = 50: residual 5.65e-3 mm/s (the 512-entry
    table's error in the measurement rotation), bound 5.65e-2 mm/s = 0.031 % of the slowest
    robot's 180.3 mm/s.  KF12D, T = 100: residual 1.24e-4 mm/s (the filter still converging),
    bound 1.24e-3 mm/s = 0.0007 %.  A sign or frame error is of the order of the speed."""
    n = 257
    yaw, rpm = _motion(n)
    gz = np.zeros(n, np.float32)
    sums = np.zeros((4, n), np.int64)
    # the oracle's side: RS velocity, the filter's state, their residual
    pos, rs_vel, prev = np.zeros((3, n), np.float32), np.zeros((3, n), np.float32), np.zeros((4, n), np.int64)
    orc.rs_tick(pos, rs_vel, prev, yaw, sums, rpm)
    cfg = fmskf.default_config(model, n)
    np_ = NX[model] * (NX[model] + 1) // 2
    if model == "kf6":
        prm = orc.kf6_params(cfg.dt, np.array(cfg.q[:21]), np.array(cfg.r[:10]))
        xo = np.zeros((6, n), np.float32)
        Po = np.repeat(np.float32(np.array(cfg.p0[:np_]))[:, None], n, 1).copy()
        kw = dict(yaw_deg=yaw, gyro_z_dps=gz, rpm=rpm)
        for _ in range(T):
            orc.kf6_tick(xo, Po, yaw, gz, rpm, None, prm)
    else:
        z = _kf12d_z(yaw, rs_vel)
        prm = orc.kf12d_params(cfg.dt, np.array(cfg.q[:78]), np.array(cfg.r[:36]))
        xo = np.zeros((12, n))
        Po = np.repeat(np.array(cfg.p0[:np_])[:, None], n, 1).copy()
        kw = dict(z=z)
        for _ in range(T):
            orc.kf12d_tick(xo, Po, z, None, prm, nthreads=0)
    speed = float(np.hypot(rs_vel[0], rs_vel[1]).min())
    residual = float(np.abs(ref.vel_f32(model, xo)[:2].astype(np.float64) - rs_vel[:2]).max())
    bound = 10.0 * residual
    print(f"{model} T={T}: oracle residual {residual:.3e} mm/s, bound {bound:.3e} mm/s, "
          f"slowest robot {speed:.1f} mm/s ({100 * bound / speed:.4f} %)")
    assert 0.0 < bound < 0.01 * speed
    with Engine("rs", n) as r, Engine(model, n) as e:
        for _ in range(T):
            r.tick(yaw_deg=yaw, angle_sum=sums, rpm=rpm)
            e.tick(**kw)
        fw = r.get_vel()
        got = e.get_vel()
    np.testing.assert_array_equal(bits(fw), bits(rs_vel))  # RS: the firmware's velocity, as ever
    diff = np.abs(got[:2].astype(np.float64) - fw[:2])
    print(f"{model} T={T}: largest |filter get_vel - RS get_vel| = {diff.max():.3e} mm/s")
    assert (diff <= bound).all(), (float(diff.max()), bound)


# ----------------------------------------------------------------------------- (c)
def _table_state(model, n):
    """(x, table lanes [n] bool): random state whose first lanes of every tile and last lane
    carry the edge table in px, py and, one row at a time, in the two velocity rows (so a
    non-finite neighbour cannot mask a value through the rotation).  theta = 0 on those lanes
    of KF6 / KF12D: the body velocity is the stored one times 1000."""
    x = _state(model, n, seed=1).astype(np.float64)
    tp = ref.EDGE_TABLE.astype(np.float64)
    tv = np.concatenate([ref.EDGE_TABLE, ref.EDGE_VEL_EXTRA]).astype(np.float64)
    if model == "kf12d":
        tp = np.concatenate([tp, ref.EDGE_F64_EXTRA])
        tv = np.concatenate([tv, ref.EDGE_F64_EXTRA])
    tab = np.zeros(n, bool)
    for t0 in range(0, n, TILE[model]):
        for j in range(2 * tv.size):
            i = t0 + j
            if i >= n:
                break
            k = j + 5 * (t0 // TILE[model])  # another table phase in every tile
            x[0, i] = tp[k % tp.size]
            x[1, i] = tp[(k + 3) % tp.size]
            x[3 + j // tv.size, i] = tv[k % tv.size]
            tab[i] = True
    i = n - 1  # the last lane overall: both int32 limits and NaN
    x[0, i], x[1, i], x[3, i], x[4, i] = -2147483.75, np.nan, 2.0**31, -3e9
    tab[i] = True
    if model in ROTATED:
        x[2, tab] = 0.0
    with np.errstate(over="ignore"):
        return np.ascontiguousarray(x.astype(np.float64 if model == "kf12d" else np.float32)), tab


@pytest.mark.parametrize("model,n", [("rs", 2049), ("kf6", 2049), ("ekf9", 2049), ("kf12d", 4097)])
def test_vehicle_info_against_reference(model, n):
    """The exported records against readout_ref.vehicle_info of readout_ref.pose / vel of the
    state that was set (not of get_pose / get_vel), with the edge table of the ARM conversion in
    the converted fields; the imu fields from get_imu.  Before any WT901 poll and after a poll in
    which every seventh robot gets no bytes; with floor, cam_pitch and fault given and all NULL.
    RS, EKF9: whole records byte for byte.  KF6, KF12D: everything byte for byte except vel_x /
    vel_y off the table lanes, which may differ by 1 where the unrounded velocity lies within
    the bound of test_pose_vel_against_reference of an integer (the count is printed); on the
    table lanes they are exact.  Measured on an MI355X: 0 lanes off by one for KF6 (no velocity
    of 4024 lies that close to an integer) and 0 for KF12D (2 of 8108 do).

    What the table can and cannot tell apart: a conversion that wraps (through int64) fails on
    the table lanes of all four models.  A plain C++ cast `(int32_t)f` in k_vehicle_info does
    not: for gfx950 the compiler lowers it to the same v_cvt_i32_f32 that f2i32_arm issues, so
    the two builds convert every input alike and no test on this target can separate them."""
    x, tab = _table_state(model, n)
    rng = np.random.default_rng(3)
    floor = rng.integers(0, 2, (n, 8)).astype(np.uint8)
    cam = rng.uniform(-30, 30, n).astype(np.float32)
    fault = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    buf, lens = synth.Trajectory(n, 1, seed=23).wt901_poll_rows(0)
    lens[::7] = 0  # no bytes this poll -> is_error, exported as imu.fault 0xFF
    pose = ref.pose(model, x)
    full = ref.vel(model, x)
    with np.errstate(over="ignore", invalid="ignore"):
        vel = full.astype(np.float32)
    assert arm_table_is_exercised(pose, vel, tab)
    off = ~tab
    if model in ROTATED:  # where a velocity within the bound of `full` may truncate otherwise
        bound = ref.body_vel_bound(full[:2, off], x[3, off], x[4, off])
        near = (np.abs(full[:2, off] - np.rint(full[:2, off])).astype(np.float64) <= bound)
    plus_minus_one = 0
    with Engine(model, n) as e:
        e.set_state(x)
        for step, args in (("before a poll", (floor, cam, fault)), ("poll", None),
                           ("after a poll", (floor, cam, fault)), ("after a poll, NULL", (None, None, None))):
            if args is None:
                e.ingest_wt901(buf, lens, latch_qinit=True)
                continue
            rec = e.export_vehicle_info(*args)
            data, err = e.get_imu()
            if step != "before a poll":
                assert err[::7].all() and not err[1::7].any() and np.abs(data[:, 1]).max() > 0
            want = ref.vehicle_info(pose, vel, data, err, *args)
            what = f"{model} {step}"
            if model not in ROTATED:
                _assert_records_equal(rec, want, what)
                continue
            a, b = rec.copy(), want.copy()
            for f, k in (("vel_x", 0), ("vel_y", 1)):
                np.testing.assert_array_equal(rec[f][tab], want[f][tab], err_msg=f"{what}: {f}, table lanes")
                d = rec[f][off].astype(np.int64) - want[f][off]
                bad = d != 0
                assert (np.abs(d) <= 1).all() and not (bad & ~near[k]).any(), f"{what}: {f}"
                plus_minus_one += int(bad.sum())
                a[f][off] = 0
                b[f][off] = 0
            _assert_records_equal(a, b, what)
    if model in ROTATED:
        print(f"{model} n={n}: {plus_minus_one} vel_x / vel_y lanes off by one over three exports "
              f"({int(near.sum())} of {near.size} lie within the bound of an integer)")


def arm_table_is_exercised(pose, vel, tab):
    """the expected records reach both saturations, NaN and a fraction truncated toward zero in
    the position and in the velocity fields"""
    with np.errstate(over="ignore", invalid="ignore"):
        p = pose[:2, tab] * ref.F32_1000
    v = vel[:2, tab]
    for a in (p, v):
        if not ((a >= 2.0**31).any() and (a <= -2.0**31).any() and np.isnan(a).any()
                and ((a < 0) & (a > -1)).any() and np.isinf(a).any()):
            return False
    return True


# ----------------------------------------------------------------------------- (d)
SENTINEL = np.array([0x7FC12345], np.uint32).view(np.float32)[0]  # a NaN no readout produces
D_CASES = [("rs", 257), ("kf6", 2049), ("ekf9", 2049), ("kf12d", 4097)]


@pytest.mark.parametrize("model,n", D_CASES)
def test_readout_device_outputs_and_null_pointers(model, n):
    """FMSKF_MEM_DEVICE outputs of get_pose / get_vel equal the host outputs bit for bit; a call
    with one pointer and two NULLs fills exactly that plane, with what the all-pointer call
    gives, on the host and on the device."""
    import torch
    x = _state(model, n, seed=2)
    with Engine(model, n) as e:
        e.set_state(x)
        for get in (e.get_pose, e.get_vel):
            host = get()
            dev = torch.full((3, n), float("nan"), dtype=torch.float32, device="cuda")
            assert get(out=dev) is dev
            torch.cuda.synchronize()
            np.testing.assert_array_equal(bits(dev.cpu().numpy()), bits(host))
            for k in range(3):
                planes = tuple(j == k for j in range(3))
                h1 = np.full((3, n), SENTINEL, np.float32)
                d1 = torch.from_numpy(h1).cuda()
                assert get(out=h1, planes=planes) is h1
                get(out=d1, planes=planes)
                torch.cuda.synchronize()
                for got in (h1, d1.cpu().numpy()):
                    for j in range(3):
                        want = host[j] if j == k else np.full(n, SENTINEL, np.float32)
                        np.testing.assert_array_equal(bits(got[j]), bits(want), err_msg=f"plane {j} of call {k}")
            np.testing.assert_array_equal(bits(get(planes=(False, True, False))[1]), bits(host[1]))
            rc = load().fmskf_get_pose(e.h, None, None, None, MEM_HOST)  # every pointer NULL: no-op
            assert rc == 0
        with pytest.raises(TypeError):
            e.get_pose(out=np.zeros((3, n), np.float64))
        with pytest.raises(ValueError):
            e.get_vel(out=np.zeros((3, n + 1), np.float32))


@pytest.mark.parametrize("model,n", [("kf6", 2049), ("kf12d", 4097)])
def test_vehicle_info_device_out_and_null_out(model, n):
    """A device `out` of fmskf_export_vehicle_info (device floor / cam_pitch / fault, or NULL)
    holds the bytes of the host record; out = NULL is FMSKF_EINVAL in either memory space."""
    import torch
    x, _ = _table_state(model, n)
    rng = np.random.default_rng(4)
    floor = rng.integers(0, 2, (n, 8)).astype(np.uint8)
    cam = rng.uniform(-30, 30, n).astype(np.float32)
    fault = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    buf, lens = synth.Trajectory(n, 1, seed=29).wt901_poll_rows(0)
    lens[::7] = 0
    with Engine(model, n) as e:
        e.set_state(x)
        e.ingest_wt901(buf, lens, latch_qinit=True)
        host = e.export_vehicle_info(floor, cam, fault)
        host0 = e.export_vehicle_info()
        assert host.tobytes() != host0.tobytes()
        dfl, dcam = torch.from_numpy(floor).cuda(), torch.from_numpy(cam).cuda()
        dfault = torch.from_numpy(fault.view(np.int32)).cuda()
        out = torch.zeros((n, 84), dtype=torch.uint8, device="cuda")
        assert e.export_vehicle_info(dfl, dcam, dfault, out=out) is out
        new = e.export_vehicle_info(dfl, dcam, dfault)  # device inputs: a new device tensor
        out0 = e.export_vehicle_info(out=torch.zeros((n, 84), dtype=torch.uint8, device="cuda"))
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == host.tobytes()
        assert new.cpu().numpy().tobytes() == host.tobytes()
        assert out0.cpu().numpy().tobytes() == host0.tobytes()
        with pytest.raises(ValueError):  # one mem flag covers the call
            e.export_vehicle_info(floor, cam, fault, out=out)
        with pytest.raises(TypeError):
            e.export_vehicle_info(out=torch.zeros((n, 21), dtype=torch.int32, device="cuda"))
        L = load()
        for mem, ptrs in ((MEM_HOST, (None, None, None)),
                          (MEM_DEVICE, tuple(C.c_void_p(t.data_ptr()) for t in (dfl, dcam, dfault)))):
            assert L.fmskf_export_vehicle_info(e.h, None, *ptrs, mem) == EINVAL
        assert e.export_vehicle_info(floor, cam, fault).tobytes() == host.tobytes()  # handle still good
