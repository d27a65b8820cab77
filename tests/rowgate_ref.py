"""The float64 reference of the EKF9 per-row innovation gate (fmskf_set_row_gate) and the oracle
driver its tests share (test_rowgate_cpu.py, test_gpu_rowgate.py).

The reference is the sequential scalar update in float64 on oracle.kf_ref's H: the heading taken
as hi + lo, the heading innovation wrapped, per row d2 = y^2 / s and fmskf.h's decision rule (or
decisions handed in), an applied row updating x, the later innovations and P, a rejected row
nothing.  orc.ekf9_measure is the kernel's fp32 z.

The oracle driver rests on the identity the header states: a tick whose rejected rows are R is
the ungated sequential tick with R[a][a] = +inf on the rows in R (1 / inf = 0 makes every term of
such a row an exact zero), so orc.ekf9_tick on the robots that share a pattern, with such
parameters, is the row-gated tick value for value."""
import numpy as np

import fmskf
from fmskf.synth import Trajectory, inject_outliers_ekf9
from oracle import kf_ref

ROWS = 6
D2_MAX = 10.83           # chi-square, 1 degree of freedom, 0.999
BAND = 1e-3              # |d2 - d2_max| <= BAND * d2_max: the decision is not compared there (gate_ref.py)
ALL = (1 << ROWS) - 1    # the pattern with every row applied
H = kf_ref.ekf9_H()
NONE, ACC, REJ, FRC = fmskf.GATE_NONE, fmskf.GATE_ACCEPTED, fmskf.GATE_REJECTED, fmskf.GATE_FORCED


def _cfg(n=1):
    return fmskf.default_config("ekf9", n)


def r_diag():
    """the default R's diagonal: the fp32 values the kernels receive"""
    r = np.float32(np.array(_cfg().r[:21]))
    return np.array([r[a * (a + 1) // 2 + a] for a in range(ROWS)], np.float64)


def params(orc, trig=fmskf.TRIG_TABLE512, rejected=0):
    """oracle parameters of the default EKF9 with R[a][a] = +inf on the rows in the bit mask
    `rejected`"""
    cfg = _cfg()
    r = np.array(cfg.r[:21])
    for a in range(ROWS):
        if (rejected >> a) & 1:
            r[a * (a + 1) // 2 + a] = np.inf
    return orc.ekf9_params(cfg.dt, np.array(cfg.q[:45]), r,
                           orc.TRIG_LIBM if trig == fmskf.TRIG_LIBM else orc.TRIG_TABLE512)


def fresh(n):
    """the oracle's start state: x [10, n] (row 9: the heading's low part), P [45, n]"""
    cfg = _cfg(n)
    return np.zeros((10, n), np.float32), np.repeat(np.float32(np.array(cfg.p0[:45]))[:, None], n, 1).copy()


def inputs(n, T, seed, start=20):
    """(raw [T,n,8], kind [T,n], trajectory): the 5 % + 5 % + 5 % outlier recipe from `start` on"""
    tr = Trajectory(n, T, seed=seed)
    raw, kind = inject_outliers_ekf9(tr.ekf9_raw(), seed=seed, start=start)
    return raw, kind, tr


def _dense(P):
    n = P.shape[1]
    D = np.empty((n, 9, 9))
    k = 0
    for i in range(9):
        for j in range(i + 1):
            D[:, i, j] = D[:, j, i] = P[k]
            k += 1
    return D


def decide(d2, run, d2_max, max_consecutive):
    """fmskf.h's rule for one row: (apply, forced)"""
    forced = np.full(d2.shape, max_consecutive > 0) & (run >= max_consecutive)
    with np.errstate(invalid="ignore"):
        return forced | (d2 <= d2_max), forced


def update64(orc, x10, P, raw, d2_max, max_consecutive=0, run=None, apply=None):
    """The float64 gated sequential update of the fp32 state (x10 [10,n], P [45,n]) with the raw
    records [n,8].  run [6,n]: the rows' runs before the update (zeros by default).  apply [6,n]
    bool or None: decisions handed in for every row (d2 is then each row's value on the state those
    decisions leave), else fmskf.h's rule.  Returns dict(d2, apply, forced [6,n], x [9,n], P
    [n,9,9]) after the update."""
    n = x10.shape[1]
    d2_max = np.broadcast_to(np.asarray(d2_max, np.float64), (ROWS,))
    run = np.zeros((ROWS, n), np.int64) if run is None else run.astype(np.int64)
    z = orc.ekf9_measure(np.ascontiguousarray(raw, np.int16)).astype(np.float64)
    x = x10[:9].astype(np.float64)
    x[2] += x10[9].astype(np.float64)
    D = _dense(P.astype(np.float64))
    y = z - H @ x
    y[0] = np.where(y[0] > np.pi, y[0] - 2 * np.pi, np.where(y[0] < -np.pi, y[0] + 2 * np.pi, y[0]))
    R = r_diag()
    out = dict(d2=np.zeros((ROWS, n)), apply=np.zeros((ROWS, n), bool), forced=np.zeros((ROWS, n), bool))
    for a in range(ROWS):
        hp = D @ H[a]                       # [n, 9]
        s = hp @ H[a] + R[a]
        d2 = y[a] * y[a] / s
        ap, forced = decide(d2, run[a], d2_max[a], max_consecutive)
        if apply is not None:
            ap = apply[a]
        g = np.where(ap, y[a] / s, 0.0)
        x += (hp * g[:, None]).T
        for b in range(a + 1, ROWS):
            y[b] -= (hp @ H[b]) * g
        D -= np.where(ap, 1.0 / s, 0.0)[:, None, None] * hp[:, :, None] * hp[:, None, :]
        out["d2"][a], out["apply"][a], out["forced"][a] = d2, ap, forced
    out["x"], out["P"] = x, D
    return out


def predict64_x(x, dt):
    """f(x) of the EKF9 in float64 on x [9,n] (the heading wrapped to [-pi, pi))"""
    x = x.copy()
    c, s = np.cos(x[2]), np.sin(x[2])
    vwx, vwy = x[3] * c - x[4] * s, x[3] * s + x[4] * c
    x[0] += vwx * dt
    x[1] += vwy * dt
    x[2] = x[2] + x[5] * dt
    x[2] = np.where(x[2] >= np.pi, x[2] - 2 * np.pi, np.where(x[2] < -np.pi, x[2] + 2 * np.pi, x[2]))
    x[3] += x[7] * dt
    x[4] += x[8] * dt
    return x


def status_run(apply, forced, run, has=None):
    """(status, run') [6,n] of fmskf.h from the decisions; robots without a measurement (has ==
    False) read NONE and keep their runs"""
    status = np.where(forced, FRC, np.where(apply, ACC, REJ)).astype(np.uint8)
    nrun = np.where(apply, 0, np.minimum(run.astype(np.int64) + 1, 255)).astype(np.uint8)
    if has is not None:
        status = np.where(has[None, :], status, NONE).astype(np.uint8)
        nrun = np.where(has[None, :], nrun, run).astype(np.uint8)
    return status, nrun


def pattern(apply):
    """[n] bit masks of the applied rows"""
    return (apply.astype(np.int64) << np.arange(ROWS)[:, None]).sum(axis=0)


def oracle_tick(orc, x10, P, raw, apply, has=None, trig=fmskf.TRIG_TABLE512, do_predict=True):
    """One row-gated tick of the oracle state in place: orc.ekf9_tick on the robots sharing an
    applied pattern, with +inf on the rejected rows' R; robots without a measurement through
    valid = 0."""
    n = x10.shape[1]
    pat = pattern(apply)
    if has is not None:
        pat = np.where(has, pat, -1)
    for p in np.unique(pat):
        idx = np.nonzero(pat == p)[0]
        xs, Ps = np.ascontiguousarray(x10[:, idx]), np.ascontiguousarray(P[:, idx])
        rs = np.ascontiguousarray(raw[idx])
        if p < 0:
            orc.ekf9_tick(xs, Ps, rs, np.zeros(idx.size, np.uint8), params(orc, trig), do_predict=do_predict)
        else:
            orc.ekf9_tick(xs, Ps, rs, None, params(orc, trig, ALL & ~int(p)), do_predict=do_predict)
        x10[:, idx], P[:, idx] = xs, Ps
