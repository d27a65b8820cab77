"""The float64 reference of the absolute pose-fix update (fmskf_correct_pose) and the shared inputs
of its tests (test_fix_cpu.py, test_gpu_fix.py).  Built from what the oracle exports: the filters
are oracle.kf_ref's Kf6Batch / Ekf9Batch driven with the kernels' fp32 z (orc.kf6_measure /
orc.ekf9_measure), the fix update is kf_ref.kf_update_batch with H = the first m rows of the
identity, NIS and the decision are float64 here (np.linalg.solve)."""
import numpy as np

import fmskf
from fmskf.synth import Trajectory, pose_fixes
from oracle import kf_ref

BAND = 1e-3                      # |NIS - nis_max| <= BAND * nis_max: the decision is not compared there
NIS_MAX = {2: 13.82, 3: 16.27}   # chi-square 0.999 at 2 and 3 degrees of freedom
R_FIX = 1e-4                     # R = diag(1e-4, 1e-4, 1e-4): 1 cm, 1 cm, 0.01 rad
N_LOOP, T_LOOP, SEED_LOOP = 4096, 400, 4096   # the closed-loop recipe
NX = {"kf6": 6, "ekf9": 9}


def wrap_innov(a):
    return np.where(a > np.pi, a - 2 * np.pi, np.where(a < -np.pi, a + 2 * np.pi, a))


def fix_update_f64(x, P, z, m, nis_max):
    """One fix update of every row: x [K, n], P [K, n, n] float64, z [K, m].  Returns (x', P', nis
    [K], apply [K]); rows that are not applied come back unchanged."""
    n = x.shape[1]
    H = np.eye(n)[:m]
    R = np.eye(m) * R_FIX
    y = z - x[:, :m]
    if m == 3:
        y[:, 2] = wrap_innov(y[:, 2])
    S = P[:, :m, :m] + R
    nis = np.einsum("ka,ka->k", y, np.linalg.solve(S, y[:, :, None])[:, :, 0])
    apply = nis <= nis_max
    xn, Pn = kf_ref.kf_update_batch(x, P, H, R, y, apply)
    return xn, Pn, nis, apply


def unpack_state(x, P):
    """the engine's planes (x [n, K], P packed [n(n+1)/2, K]) -> x [K, n], P [K, n, n] float64"""
    n = x.shape[0]
    i, j = np.tril_indices(n)
    Pm = np.zeros((x.shape[1], n, n))
    Pm[:, i, j] = P.T
    Pm[:, j, i] = P.T
    return x.T.astype(np.float64), Pm


def pack_P(Pm):
    i, j = np.tril_indices(Pm.shape[1])
    return Pm[:, i, j].T


def model_inputs(orc, model, tr):
    """per tick the engine's tick keywords and the kernels' fp32 z [m, N] as float64"""
    if model == "kf6":
        yaw, gz, rpm = tr.kf6_inputs()
        kw = [dict(yaw_deg=yaw[t], gyro_z_dps=gz[t], rpm=rpm[t]) for t in range(tr.ticks)]
        z = [orc.kf6_measure(yaw[t], gz[t], rpm[t]).astype(np.float64) for t in range(tr.ticks)]
    else:
        raw = tr.ekf9_raw()
        kw = [dict(raw=raw[t]) for t in range(tr.ticks)]
        z = [orc.ekf9_measure(raw[t]).astype(np.float64) for t in range(tr.ticks)]
    return kw, z


def fresh_filter(model, n):
    """the float64 filter with the noise the kernels receive (the config narrowed to fp32)"""
    cfg = fmskf.default_config(model, n)
    nx = NX[model]
    npk, m = nx * (nx + 1) // 2, (4 if model == "kf6" else 6)
    f32 = lambda a: np.float32(np.array(a)).astype(np.float64)
    cls = kf_ref.Kf6Batch if model == "kf6" else kf_ref.Ekf9Batch
    return cls(n, np.zeros(nx), f32(cfg.p0[:npk]), f32(cfg.q[:npk]), f32(cfg.r[:m * (m + 1) // 2]), float(np.float32(cfg.dt)))


_LOOPS = {}


def closed_loop(orc, model, m, n=N_LOOP, T=T_LOOP, seed=SEED_LOOP):
    """The closed-loop recipe in float64, computed once per (model, m) and shared: before tick t
    the fixes of pose_fixes(traj, t) (defaults), gated at NIS_MAX[m], then the tick.  Returns a
    dict: traj, kw (tick keywords per tick), fixes (per tick: robot, x, y, theta, outlier), nis and
    apply (per tick, float64), err (final position error [n] against the truth), p00 (final)."""
    key = (model, m, n, T, seed)
    if key in _LOOPS:
        return _LOOPS[key]
    tr = Trajectory(n, T, seed=seed)
    kw, z = model_inputs(orc, model, tr)
    f = fresh_filter(model, n)
    out = dict(traj=tr, kw=kw, fixes=[], nis=[], apply=[])
    for t in range(T):
        fx = pose_fixes(tr, t, seed=seed)
        out["fixes"].append(fx)
        robot = fx[0].astype(np.int64)
        if robot.size:
            zf = np.stack([a.astype(np.float64) for a in fx[1:1 + m]], axis=1)
            f.x[robot], f.P[robot], nis, apply = fix_update_f64(f.x[robot], f.P[robot], zf, m, NIS_MAX[m])
        else:
            nis, apply = np.zeros(0), np.zeros(0, bool)
        out["nis"].append(nis)
        out["apply"].append(apply)
        f.step(z[t])
    out["err"] = np.hypot(f.x[:, 0] - tr.px[T - 1], f.x[:, 1] - tr.py[T - 1])
    out["p00"] = f.P[:, 0, 0].copy()
    _LOOPS[key] = out
    return out


def in_band(nis, m):
    return np.abs(nis - NIS_MAX[m]) <= BAND * NIS_MAX[m]
