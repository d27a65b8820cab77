"""The premise of the KF6 kernels' conditional write-back (csrc/kf6_lane.hpp kKf6SkipMask), on the
oracle alone: with the default tuning (block-diagonal Q, R and P0) the covariance between the
heading pair (theta, omega) and the translation quad (px, py, vx, vy) is touched by neither the
update nor the predict, so those eight packed planes stay +0.0 bit for bit; one Q entry that
couples the two blocks makes them move."""
import numpy as np

import fmskf
from fmskf.synth import Trajectory

import param_cases
from param_cases import pk

N, T = 64, 500
# P20 P21 P32 P42 P50 P51 P53 P54: (theta | omega) x (px | py | vx | vy)
CROSS = sorted(pk(i, j) for i, j in ((2, 0), (2, 1), (3, 2), (4, 2), (5, 0), (5, 1), (5, 3), (5, 4)))


def _run(orc, prm):
    """the cross planes' bits after each of T ticks of random yaw / gyro / rpm: [T, 8, N] uint32"""
    rng = np.random.default_rng(20)
    yaw = rng.uniform(-180.0, 180.0, (T, N)).astype(np.float32)
    gz = rng.uniform(-500.0, 500.0, (T, N)).astype(np.float32)
    rpm = rng.integers(-8000, 8001, (T, N, 4)).astype(np.int16)
    op = param_cases.orc_params(orc, prm)
    x, P = param_cases.fresh(prm, N)
    out = np.empty((T, len(CROSS), N), np.uint32)
    for t in range(T):
        orc.kf6_tick(x, P, yaw[t], gz[t], np.ascontiguousarray(rpm[t]), None, op)
        out[t] = P[CROSS].view(np.uint32)
    assert np.isfinite(x).all() and np.isfinite(P).all()
    return out


def test_cross_planes_are_the_packed_indices_the_kernels_mask():
    assert CROSS == [3, 4, 8, 12, 15, 16, 18, 19]


def test_cross_planes_stay_plus_zero_with_the_default_tuning(orc):
    bits = _run(orc, param_cases.default_params("kf6"))
    assert not bits.any(), "a cross plane left +0.0 (bitwise) under the default KF6 tuning"


def test_cross_planes_move_when_q_couples_theta_and_vx(orc):
    base = param_cases.default_params("kf6")
    q = base.q.astype(np.float64)
    q[pk(3, 2)] = 0.3 * np.sqrt(q[pk(2, 2)] * q[pk(3, 3)])
    assert q[pk(3, 2)] != 0.0
    bits = _run(orc, base._replace(q=q.astype(np.float32)))
    assert bits.any(), "an off-block Q entry left every cross plane at +0.0"


def test_trajectory_inputs_keep_them_zero_too(orc):
    """the synthetic trajectory the GPU tests and the bench feed, not only white inputs"""
    yaw, gz, rpm = Trajectory(N, 200, seed=3).kf6_inputs()
    prm = param_cases.default_params("kf6")
    op = param_cases.orc_params(orc, prm)
    x, P = param_cases.fresh(prm, N)
    for t in range(200):
        orc.kf6_tick(x, P, yaw[t], gz[t], np.ascontiguousarray(rpm[t]), None, op)
        assert not P[CROSS].view(np.uint32).any(), t
    assert fmskf.default_config("kf6", N).dt == prm.dt
