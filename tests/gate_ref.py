"""The float64 reference of the KF6 innovation gate (fmskf_set_gate) and the shared inputs of its
tests (test_gate_cpu.py, test_gpu_gate.py).  Built from what the oracle exports: orc.kf6_measure
is the kernel's fp32 z, orc.kf6_tick with a `valid` mask is "skip the update for these robots";
NIS and the decision are float64 here: y = z - H x with the heading wrapped, S = H P H^T + R,
np.linalg.solve, on the pre-tick state."""
import numpy as np

import fmskf
from fmskf.synth import Trajectory, inject_outliers

H = (2, 5, 3, 4)         # KF6: z = (theta, omega, vx, vy)
NIS_MAX = 18.47          # chi-square, 4 degrees of freedom, 0.999
BAND = 1e-3              # |NIS - nis_max| <= BAND * nis_max: the decision is not compared there


def pk(i, j):
    return i * (i + 1) // 2 + j if i >= j else j * (j + 1) // 2 + i


# `prm` (optional, everywhere below): a param_cases.Params of KF6; omitted: fmskf.default_config
def params(orc, n, trig=fmskf.TRIG_TABLE512, prm=None):
    otrig = orc.TRIG_LIBM if trig == fmskf.TRIG_LIBM else orc.TRIG_TABLE512
    if prm is not None:
        return orc.kf6_params(prm.dt, prm.q, prm.r, otrig)
    cfg = fmskf.default_config("kf6", n)
    return orc.kf6_params(cfg.dt, np.array(cfg.q[:21]), np.array(cfg.r[:10]), otrig)


def r_packed(n=1, prm=None):
    """the filter's R: the fp32 values the kernels receive"""
    if prm is not None:
        return np.float32(prm.r).astype(np.float64)
    return np.float32(np.array(fmskf.default_config("kf6", n).r[:10])).astype(np.float64)


def fresh(n, prm=None):
    if prm is not None:
        return np.zeros((6, n), np.float32), np.repeat(np.float32(prm.p0)[:, None], n, 1).copy()
    cfg = fmskf.default_config("kf6", n)
    return np.zeros((6, n), np.float32), np.repeat(np.float32(np.array(cfg.p0[:21]))[:, None], n, 1).copy()


def nis_f64(orc, x, P, yaw, gz, rpm, trig=fmskf.TRIG_TABLE512, prm=None):
    """NIS [n] in float64 of the measurement (yaw, gz, rpm) against the fp32 state (x, P)"""
    z = orc.kf6_measure(np.ascontiguousarray(yaw, np.float32), np.ascontiguousarray(gz, np.float32),
                        np.ascontiguousarray(rpm, np.int16),
                        orc.TRIG_LIBM if trig == fmskf.TRIG_LIBM else orc.TRIG_TABLE512).astype(np.float64)
    x = x.astype(np.float64)
    P = P.astype(np.float64)
    y = z - x[list(H)]
    y[0] = np.where(y[0] > np.pi, y[0] - 2 * np.pi, np.where(y[0] < -np.pi, y[0] + 2 * np.pi, y[0]))
    n = x.shape[1]
    R = r_packed(prm=prm)
    S = np.empty((n, 4, 4))
    for a in range(4):
        for b in range(4):
            S[:, a, b] = P[pk(H[a], H[b])] + R[pk(a, b)]
    yt = np.ascontiguousarray(y.T)
    sol = np.linalg.solve(S, yt[:, :, None])[:, :, 0]
    return np.einsum("na,na->n", yt, sol)


def gate_inputs(n, T, seed, start=20):
    """(yaw [T,n], gz [T,n], rpm [T,n,4], kind [T,n]): a synthetic trajectory with the 5 % + 5 %
    outlier mix from tick `start` on"""
    yaw, gz, rpm = Trajectory(n, T, seed=seed).kf6_inputs()
    yaw, rpm, kind = inject_outliers(yaw, rpm, seed=seed, start=start)
    return yaw, gz, rpm, kind


def decide(nis, run, nis_max, max_consecutive):
    """(status, run', rejected) of fmskf.h's rule for robots that have a measurement"""
    forced = (max_consecutive > 0) & (run >= max_consecutive)
    apply = forced | (nis <= nis_max)
    status = np.where(forced, fmskf.GATE_FORCED, np.where(apply, fmskf.GATE_ACCEPTED, fmskf.GATE_REJECTED))
    return status.astype(np.uint8), np.where(apply, 0, np.minimum(run.astype(np.int64) + 1, 255)).astype(np.uint8), ~apply
