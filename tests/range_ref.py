"""The float64 reference of the range update against surveyed anchors (fmskf_correct_range), a
float32 numpy restatement of the same formulas in the kernel's operation order, the run loop over
a non-descending list, and the shared inputs of test_range_cpu.py and test_gpu_range.py.

The float64 update builds H explicitly (three coefficients on px, py, theta) and takes sin / cos of
the heading as inputs, so a caller decides the trig policy: np.sin / np.cos here, Engine.eval_trig
in the GPU tests.  cross_check() compares its gain and covariance update with
oracle.kf_ref.kf_update_batch given that H.

Tolerance of the GPU tests (nothing fixed in advance): both the kernel and range_update_f32 are
fp32 roundings of the same ~100 operations; the kernel's deviation from the float64 update of the
same fp32 pre-state must stay within MARGIN = 8 times the restatement's deviation from that same
reference, per quantity (x; P, compensated entries as hi + lo; d2 relative to max(d2, 1)), the
maximum taken over the listed robots (deviations())."""
import numpy as np

import fmskf
from fmskf.synth import Trajectory, range_fixes
from oracle import kf_ref

import fix_ref

ACC, REJ, IGN, NEAR = fmskf.GATE_ACCEPTED, fmskf.GATE_REJECTED, fmskf.FIX_IGNORED, 5
MARGIN = 8.0
BAND = 1e-3                # |d2 - d2_max| <= BAND * d2_max: the decision is not compared there
D2_MAX = 10.83             # chi-square 0.999 at one degree of freedom
ANCHORS = np.array([[6.0, 6.1, 2.5], [-6.2, 5.9, 2.4], [-5.9, -6.0, 2.6], [6.1, -6.2, 2.5]], np.float32)
TAG = (0.15, 0.05, 0.30)
SIGMA = 0.05               # range noise of synth.range_fixes (its default), var = SIGMA^2
VAR = SIGMA * SIGMA
D_MIN = 0.5
N_LOOP, T_LOOP, SEED_LOOP = 1024, 400, 1024   # the closed-loop recipe


def _geometry(px, py, sn, cs, anc, tag):
    """dx, dy, dz, rx, ry in the arrays' own precision (operation order of include/fmskf.h)"""
    lx, ly, lz = tag
    rx = cs * lx - sn * ly
    ry = sn * lx + cs * ly
    dx = (px - anc[:, 0]) + rx
    dy = (py - anc[:, 1]) + ry
    dz = lz - anc[:, 2]
    return dx, dy, dz, rx, ry


def range_update_f64(x, P, sn, cs, anc, rho, r, tag, d2_max, d_min):
    """One range per row in float64: x [K, n], P [K, n, n], sn / cs [K] the heading's sin / cos,
    anc [K, 3], rho [K] the measured ranges, r [K] their variances.  Returns (x', P', d2 [K],
    status [K], d [K] the predicted distances, H [K, n], y [K]); rows that are NEAR or rejected
    come back unchanged, NEAR rows with d2 = 0."""
    x, P = np.asarray(x, np.float64), np.asarray(P, np.float64)
    tag = tuple(float(np.float32(v)) for v in tag)
    dx, dy, dz, rx, ry = _geometry(x[:, 0], x[:, 1], sn, cs, anc.astype(np.float64), tag)
    d = np.sqrt(dx * dx + dy * dy + dz * dz)
    near = ~(d >= d_min)
    ds = np.where(near, 1.0, d)
    H = np.zeros_like(x)
    H[:, 0], H[:, 1], H[:, 2] = dx / ds, dy / ds, (dy * rx - dx * ry) / ds
    hp = np.einsum("ki,kij->kj", H, P)
    S = np.einsum("kj,kj->k", H, hp) + r
    y = rho - d
    with np.errstate(invalid="ignore"):
        d2 = np.where(near, 0.0, y * y / S)
        apply = (d2 <= d2_max) & ~near
    K = hp / S[:, None]
    xn = np.where(apply[:, None], x + K * y[:, None], x)
    Pn = P - K[:, :, None] * hp[:, None, :]
    Pn = np.where(apply[:, None, None], 0.5 * (Pn + Pn.transpose(0, 2, 1)), P)
    status = np.where(near, NEAR, np.where(apply, ACC, REJ)).astype(np.uint8)
    return xn, Pn, d2, status, d, H, y


def cross_check(x, P, H, y, r, rows):
    """largest difference of the reference's gain / covariance form (P - hp hp^T / S) from
    kf_ref.kf_update_batch (Joseph form) with the same H, over `rows`; relative to the entries'
    scale"""
    worst = 0.0
    for k in rows:
        xa, Pa = kf_ref.kf_update_batch(x[k:k + 1], P[k:k + 1], H[k:k + 1], np.array([[r[k]]]), y[k:k + 1, None])
        hp = H[k] @ P[k]
        S = H[k] @ hp + r[k]
        xb = x[k] + hp / S * y[k]
        Pb = P[k] - np.outer(hp, hp) / S
        worst = max(worst, np.abs(xa[0] - xb).max() / max(1.0, np.abs(xb).max()),
                    np.abs(Pa[0] - Pb).max() / max(1e-12, np.abs(P[k]).max()))
    return worst


def range_update_f32(x, P, sn, cs, anc, rho, r, tag, d2_max, d_min):
    """range_update_f64's formulas in float32 numpy arithmetic in the kernel's operation order
    (csrc/range_lane.hpp; plain fp32 state, no compensated pairs): every product and sum rounded on
    its own.  x [K, n] float32, P [K, n, n] float32 (symmetric)."""
    f = np.float32
    x, P = np.array(x, f), np.array(P, f)
    sn, cs, rho, r, anc = (np.asarray(a, f) for a in (sn, cs, rho, r, anc))
    tag = tuple(f(v) for v in tag)
    n = x.shape[1]
    dx, dy, dz, rx, ry = _geometry(x[:, 0], x[:, 1], sn, cs, anc, tag)
    d = np.sqrt((dx * dx + dy * dy) + dz * dz)
    near = ~(d >= f(d_min))
    with np.errstate(divide="ignore", invalid="ignore"):
        di = f(1.0) / d
        H0, H1, H2 = dx * di, dy * di, (dy * rx - dx * ry) * di
        hp = np.stack([(H0 * P[:, 0, j] + H1 * P[:, 1, j]) + H2 * P[:, 2, j] for j in range(n)], axis=1)
        S = ((H0 * hp[:, 0] + H1 * hp[:, 1]) + H2 * hp[:, 2]) + r
        si = f(1.0) / S
        y = rho - d
        g = y * si
        d2 = np.where(near, f(0.0), y * g)
        apply = (d2 <= f(d2_max)) & ~near
        xn = x + hp * g[:, None]
        u = hp * si[:, None]
        T = u[:, :, None] * hp[:, None, :]            # T[i][j] = (hp[i] si) hp[j]
        T = np.tril(T) + np.tril(T, -1).transpose(0, 2, 1)
        Pn = P - T
    xn = np.where(apply[:, None], xn, x)
    Pn = np.where(apply[:, None, None], Pn, P)
    status = np.where(near, NEAR, np.where(apply, ACC, REJ)).astype(np.uint8)
    assert xn.dtype == f and Pn.dtype == f and d2.dtype == f
    return xn, Pn, d2, status, d


def run_positions(robot):
    """position of every entry in its run (0 for a run's first entry) of a non-descending list"""
    robot = np.asarray(robot).astype(np.int64)
    k = np.arange(robot.size)
    head = np.ones(robot.size, bool)
    head[1:] = robot[1:] != robot[:-1]
    return k - np.maximum.accumulate(np.where(head, k, 0))


def apply_list(update, x, P, robot, anchor, rho, var, anchors, trig, tag=TAG, var_default=VAR, d2_max=np.inf,
               d_min=D_MIN):
    """The run loop on a well-formed list: the entries of every robot in list order, each on the
    state the one before left.  update: range_update_f64 or range_update_f32; x [N, n], P [N, n, n]
    of the whole fleet (not modified); trig(theta [K]) -> (sin, cos).  Returns (x', P', d2 [count],
    status [count], d [count] the predicted distances)."""
    x, P = x.copy(), P.copy()
    r = robot.astype(np.int64)
    pos = run_positions(r)
    var = np.full(r.size, var_default) if var is None else np.where(np.asarray(var) > 0, var, var_default)
    d2, dist = np.zeros(r.size, x.dtype), np.zeros(r.size, x.dtype)
    status = np.zeros(r.size, np.uint8)
    for j in range(int(pos.max()) + 1 if r.size else 0):
        sel = np.flatnonzero(pos == j)
        rr = r[sel]
        sn, cs = trig(x[rr, 2])
        out = update(x[rr], P[rr], np.asarray(sn, x.dtype), np.asarray(cs, x.dtype), anchors[anchor[sel]],
                     rho[sel].astype(x.dtype), var[sel].astype(x.dtype), tag, d2_max, d_min)
        x[rr], P[rr], d2[sel], status[sel], dist[sel] = out[:5]
    return x, P, d2, status, dist


def trig64(th):
    return np.sin(th), np.cos(th)


def deviations(got, ref):
    """largest deviations of (x [K, n], P [K, n, n], d2 [K]) from the float64 (x, P, d2): x and P
    absolute, d2 relative to max(d2, 1)"""
    return dict(x=float(np.abs(got[0] - ref[0]).max()), P=float(np.abs(got[1] - ref[1]).max()),
                d2=float((np.abs(got[2] - ref[2]) / np.maximum(ref[2], 1.0)).max()))


def in_band(d2, d2_max=D2_MAX):
    return np.abs(d2 - d2_max) <= BAND * d2_max


_LOOPS = {}


def start_offsets(n, seed):
    """the filters' start: N(0, 0.5 m) off the truth (0, 0) in px, py, as fp32"""
    return np.random.default_rng([seed, 0x6F6666]).normal(0.0, 0.5, (2, n)).astype(np.float32)


def closed_loop(orc, model, n=N_LOOP, T=T_LOOP, seed=SEED_LOOP):
    """The closed-loop recipe in float64, computed once per model and shared: the filter started
    N(0, 0.5 m) off the truth; before tick t the ranges of range_fixes(traj, t, ANCHORS, TAG)
    (defaults: a burst of 3 for 1 / 32 of the fleet, sigma 0.05 m, 5 % lengthened by 0.5 - 2 m
    from tick 40 on) gated at D2_MAX, then the tick; and the same run without the ranges.  Returns
    a dict: traj, kw (tick keywords per tick), x0 [2, n] the start offsets, fixes (per tick: robot,
    anchor, range, outlier), d2 / status (per tick, float64), dmin (smallest predicted distance),
    err / err_plain (final position error [n] against the truth, with and without the ranges),
    p00 / p00_plain (final)."""
    key = (model, n, T, seed)
    if key in _LOOPS:
        return _LOOPS[key]
    tr = Trajectory(n, T, seed=seed)
    kw, z = fix_ref.model_inputs(orc, model, tr)
    x0 = start_offsets(n, seed)
    f, plain = fix_ref.fresh_filter(model, n), fix_ref.fresh_filter(model, n)
    for flt in (f, plain):
        flt.x[:, 0], flt.x[:, 1] = x0[0], x0[1]
    out = dict(traj=tr, kw=kw, x0=x0, fixes=[], d2=[], status=[], dmin=np.inf)
    anchors = ANCHORS.astype(np.float64)
    for t in range(T):
        fx = range_fixes(tr, t, ANCHORS, TAG, seed=seed)
        out["fixes"].append(fx)
        if fx[0].size:
            f.x, f.P, d2, status, dist = apply_list(range_update_f64, f.x, f.P, fx[0], fx[1], fx[2], None, anchors,
                                                    trig64, d2_max=D2_MAX)
            out["dmin"] = min(out["dmin"], float(dist.min()))
        else:
            d2, status = np.zeros(0), np.zeros(0, np.uint8)
        out["d2"].append(d2)
        out["status"].append(status)
        f.step(z[t])
        plain.step(z[t])
    truth = (tr.px[T - 1], tr.py[T - 1])
    out["err"] = np.hypot(f.x[:, 0] - truth[0], f.x[:, 1] - truth[1])
    out["err_plain"] = np.hypot(plain.x[:, 0] - truth[0], plain.x[:, 1] - truth[1])
    out["p00"], out["p00_plain"] = f.P[:, 0, 0].copy(), plain.P[:, 0, 0].copy()
    _LOOPS[key] = out
    return out
