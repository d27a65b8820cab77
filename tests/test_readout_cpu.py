"""tests/readout_ref.py pinned on the CPU before tests/test_gpu_readout.py lets it judge
k_readout / k_vehicle_info: its int32 conversion and record against the oracle's C functions
(themselves pinned by tests/test_oracle_ctrl.py), and its longdouble body velocity against a
float64 evaluation."""
import numpy as np

import readout_ref as ref

# every fp32 value the GPU test puts through the conversion, times 1000 too (the pose path)
with np.errstate(over="ignore", invalid="ignore"):
    _TABLE = np.concatenate([ref.EDGE_TABLE, ref.EDGE_VEL_EXTRA, ref.EDGE_TABLE * ref.F32_1000,
                             ref.EDGE_F64_EXTRA.astype(np.float32)])


def test_arm_i32_equals_oracle_on_the_edge_table(orc):
    got = ref.arm_i32(_TABLE)
    want = np.array([orc.f2i32_arm(v) for v in _TABLE], np.int64)
    np.testing.assert_array_equal(got, want)
    # known answers, so that two wrong conversions cannot agree
    ka = {0.9999: 0, -0.9999: 0, 1999.5: 1999, -1999.5: -1999, 2147483520.0: 2147483520,
          2147483648.0: 2**31 - 1, -2147483648.0: -2**31, 3e9: 2**31 - 1, -3e9: -2**31,
          float("inf"): 2**31 - 1, float("-inf"): -2**31, float("nan"): 0, -0.0: 0, 1e-45: 0}
    for f, i in ka.items():
        assert ref.arm_i32(np.float32(f)) == i, f
    rng = np.random.default_rng(11)
    r = (rng.normal(size=4096) * 10.0 ** rng.uniform(-3, 11, 4096)).astype(np.float32)
    np.testing.assert_array_equal(ref.arm_i32(r), [orc.f2i32_arm(v) for v in r])


def _inputs(rng, n):
    d = rng.normal(size=(16, n)).astype(np.float32)
    err = (rng.random(n) < 0.3).astype(np.uint8)
    floor = rng.integers(0, 2, (n, 8)).astype(np.uint8)
    cam = rng.uniform(-30, 30, n).astype(np.float32)
    fault = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    return d, err, floor, cam, fault


def test_vehicle_info_equals_oracle_bytes(orc):
    rng = np.random.default_rng(12)
    n = 512
    pose = (rng.normal(size=(3, n)) * [[30.0], [2000.0], [4.0]]).astype(np.float32)
    vel = (rng.normal(size=(3, n)) * [[1500.0], [40.0], [3.0]]).astype(np.float32)
    d, err, floor, cam, fault = _inputs(rng, n)
    got = ref.vehicle_info(pose, vel, d, err, floor, cam, fault)
    want = orc.vehicle_info(*pose, *vel, d, err, floor=floor, cam_pitch=cam, fault=fault)
    assert got.dtype == want.dtype and got.itemsize == 84
    assert got.tobytes() == want.tobytes()
    got = ref.vehicle_info(pose, vel, d, err)  # floor, cam_pitch, fault NULL: zero
    assert got.tobytes() == orc.vehicle_info(*pose, *vel, d, err).tobytes()
    # the edge table in every converted field (theta rows stay finite: NaN payloads of a float
    # passed through ctypes as double are not what this compares)
    t = _TABLE
    m = t.size
    pose = np.stack([t, np.roll(t, 5), rng.normal(size=m).astype(np.float32)])
    vel = np.stack([np.roll(t, 9), np.roll(t, 14), rng.normal(size=m).astype(np.float32)])
    d, err, floor, cam, fault = _inputs(rng, m)
    got = ref.vehicle_info(pose, vel, d, err, floor, cam, fault)
    want = orc.vehicle_info(*pose, *vel, d, err, floor=floor, cam_pitch=cam, fault=fault)
    assert got.tobytes() == want.tobytes()
    with np.errstate(over="ignore"):
        assert np.isinf(np.float32(1e36) * ref.F32_1000)  # the case the table names
    k = int(np.flatnonzero(t == np.float32(1e36))[0])
    assert got["pos_x"][k] == 2**31 - 1


def test_pose_and_vel_layout():
    """rows, units and types of pose() / vel() on values chosen by hand"""
    x = np.arange(1, 7, dtype=np.float32)[:, None] * np.float32([[1.0, -2.0]])
    np.testing.assert_array_equal(ref.pose("rs", x), x[:3])
    np.testing.assert_array_equal(ref.vel("rs", x), x[3:6])
    x9 = np.concatenate([x, x[:3] * 7])
    np.testing.assert_array_equal(ref.pose("ekf9", x9), x[:3])
    np.testing.assert_array_equal(ref.vel("ekf9", x9), [[4000, -8000], [5000, -10000], [6, -12]])
    assert ref.vel("ekf9", x9).dtype == np.float32
    # KF6: heading +90 deg, world velocity (0, 1) m/s is 1000 mm/s straight ahead; world (1, 0)
    # is 1000 mm/s to the robot's right (body y points left)
    for model, dt in (("kf6", np.float32), ("kf12d", np.float64)):
        nx = 6 if model == "kf6" else 12
        s = np.zeros((nx, 2), dt)
        s[2] = np.pi / 2
        s[3] = [0.0, 1.0]
        s[4] = [1.0, 0.0]
        s[5] = [0.25, -0.5]
        v = ref.vel(model, s)
        assert v.dtype == np.longdouble
        np.testing.assert_allclose(v.astype(np.float64), [[1000, 0], [0, -1000], [0.25, -0.5]], atol=1e-4)
        np.testing.assert_array_equal(ref.pose(model, s), s[:3].astype(np.float32))


def test_longdouble_body_velocity_vs_float64_and_float32():
    """2^20 random lanes: the longdouble reference narrowed to float equals a float64
    evaluation narrowed to float on every lane and either axis (so the GPU bound, which allows
    the double arithmetic 2^-48 of the magnitudes, is not hiding a disagreement of the
    reference with itself), while an fp32 evaluation misses that bound on a large share of the
    lanes (so the bound separates a rotation done in float)."""
    rng = np.random.default_rng(13)
    n = 1 << 20
    x = np.zeros((6, n), np.float32)
    x[2] = rng.uniform(-np.pi, np.pi, n)
    x[3:5] = rng.normal(0, 1.5, (2, n))
    full = ref.vel("kf6", x)[:2]
    want = full.astype(np.float32)
    th, vx, vy = (x[k].astype(np.float64) for k in (2, 3, 4))
    c, s = np.cos(th), np.sin(th)
    f64 = np.stack([(vx * c + vy * s) * 1000.0, (-vx * s + vy * c) * 1000.0])
    bad = (f64.astype(np.float32).view(np.uint32) != want.view(np.uint32)).sum(axis=1)
    print(f"float64 vs longdouble, narrowed: {bad.tolist()} mismatches of {n}")
    assert bad.tolist() == [0, 0]
    bound = ref.body_vel_bound(full, x[3], x[4])
    assert (np.abs(f64 - full).astype(np.float64) <= bound).all()
    c32, s32 = np.cos(x[2]), np.sin(x[2])
    k32 = np.float32(1000)
    f32 = np.stack([(x[3] * c32 + x[4] * s32) * k32, (-x[3] * s32 + x[4] * c32) * k32])
    assert f32.dtype == np.float32
    miss = (np.abs(f32.astype(np.longdouble) - full).astype(np.float64) > bound).mean(axis=1)
    print(f"fp32 evaluation outside the bound: {miss.round(3).tolist()} of the lanes")
    assert (miss > 0.25).all()


def test_ulp_f32():
    for v in (1.0, 1.5, -3.0, 1000.25, 2.0**-130, 1e-45, 3.4e38):
        f = np.float32(v)
        assert ref.ulp_f32(f) == float(np.spacing(np.abs(f))), v
    assert ref.ulp_f32(0.0) == 2.0**-149
