"""References of the KF6 fixed-interval smoother (fmskf_tick_many_smooth) and the shared inputs of
test_smooth_cpu.py and test_gpu_smooth.py.

rts_f64: the definition in include/fmskf.h, the textbook Rauch-Tung-Striebel pass in float64,
batched over robots.  Its forward pass is oracle.kf_ref's: Kf6Batch.step advances the filter, and
the filtered state of every tick is kf_ref.kf_update_batch on the prior with the innovation formed
as Kf6Batch.step forms it.  z is the kernels' fp32 measurement (orc.kf6_measure) as float64.

smooth_form: the form the kernels use (csrc/smooth_lane.hpp: with Pi = (P-[t+1])^-1 through an LDL^T
factor, x_s[t] = x+[t] + F^-1 (I - Q Pi)(x_s[t+1] - x-[t+1]) and P_s[t] = F^-1 (Q - Q Pi Q +
(I - Q Pi) P_s[t+1] (I - Q Pi)^T) F^-T), restated in numpy in the kernels' operation order, in the
precision asked for.  smooth_f32 is that in float32: every product and sum rounded on its own
(numpy has no fused multiply-add, the kernels use it throughout: the two are fp32 roundings of the
same operations, not the same bits).

Tolerance of the GPU tests (nothing fixed in advance): per quantity -- the 6 rows of x_s, the 21
packed planes of P_s -- the kernels' largest deviation from rts_f64 over robots and ticks must
stay within range_ref.MARGIN (8, reasoned there) times the larger of smooth_f32's own deviation
from rts_f64 and one fp32 ulp of the quantity's largest reference magnitude (bounds()): where the
restatement happens to hit the reference exactly, a correctly rounded result may still be an ulp
off.  Heading differences are taken mod 2 pi."""
import numpy as np

import fmskf
from fmskf.synth import Trajectory
from oracle import kf_ref

import fix_ref
from range_ref import MARGIN

N, T, WARM = 4113, 37, 50    # three 2048-wide tiles, no multiple of 256; an odd window; plain ticks first
SEED = 37
H1 = (2, 5, 3, 4)            # the state every measurement row reads (MdKF6::h1)
PI_F = np.float32(3.14159265358979)
TRI = np.tril_indices(6)


def pk(i, j):
    return i * (i + 1) // 2 + j if i >= j else j * (j + 1) // 2 + i


def wrap_pi_f32(a):
    """fmskf_device.hpp wrap_pi on float32 arrays: what the smoothed heading goes through"""
    a = np.asarray(a, np.float32)
    two_pi = np.float32(2.0) * PI_F
    return np.where(a >= PI_F, a - two_pi, np.where(a < -PI_F, a + two_pi, a)).astype(np.float32)


def params(n=1):
    """(dt, q [21], r [10]) as the kernels receive them: the default config narrowed to fp32"""
    cfg = fmskf.default_config("kf6", n)
    f = np.float32
    return f(cfg.dt), np.array(cfg.q[:21]).astype(f), np.array(cfg.r[:10]).astype(f)


def measure(orc, yaw, gz, rpm):
    """z [T, 4, N] float32: the kernels' measurement of every tick"""
    return np.stack([orc.kf6_measure(yaw[t], gz[t], rpm[t]) for t in range(yaw.shape[0])]).astype(np.float32)


def reset_state(n):
    """the state reset() leaves, in the engine's planes: x = 0, P = P0 (fp32)"""
    cfg = fmskf.default_config("kf6", n)
    return np.zeros((6, n), np.float32), np.repeat(np.float32(np.array(cfg.p0[:21]))[:, None], n, 1)


# ----------------------------------------------------------------------------- float64 RTS
def rts_f64(x0, P0, z, valid=None):
    """x0 [6, N], P0 packed [21, N] (the engine's planes), z [T, 4, N], valid [T, N] or None.
    Returns a dict: xs [T, 6, N], Ps [T, 21, N] the smoothed estimates; xf, Pf the filtered ones;
    pred_x [T, N, 6], pred_P [T, N, 6, 6] the predict of every filtered state formed here (what
    Kf6Batch.step must have left: test_smooth_cpu.py compares); x_end, P_end the final state."""
    Tn, n = z.shape[0], z.shape[2]
    f = fix_ref.fresh_filter("kf6", n)
    f.x, f.P = fix_ref.unpack_state(np.asarray(x0), np.asarray(P0))
    F, H, R, Q = f.F, f.H, f.R, f.Q
    xp, Pp, xf, Pf, qx, qP = [], [], [], [], [], []
    for t in range(Tn):
        xp.append(f.x.copy())
        Pp.append(f.P.copy())
        zt = z[t].astype(np.float64)
        y = zt.T - f.x @ H.T
        y[:, 0] = kf_ref._wrap_innov_v(y[:, 0])
        m = None if valid is None else np.asarray(valid[t]).astype(bool)
        a, b = kf_ref.kf_update_batch(f.x, f.P, H, R, y, m)
        xf.append(a)
        Pf.append(b)
        px = a @ F.T
        px[:, 2] = kf_ref._wrap_state_v(px[:, 2])
        qx.append(px)
        qP.append(F @ b @ F.T + Q)
        f.step(zt, None if valid is None else valid[t])
    xs, Ps = [None] * Tn, [None] * Tn
    xs[-1] = xf[-1].copy()
    xs[-1][:, 2] = kf_ref._wrap_state_v(xs[-1][:, 2])
    Ps[-1] = Pf[-1].copy()
    for t in range(Tn - 2, -1, -1):
        C = np.linalg.solve(Pp[t + 1], F @ Pf[t]).transpose(0, 2, 1)   # P+ F^T (P-[t+1])^-1
        dx = xs[t + 1] - xp[t + 1]
        dx[:, 2] = kf_ref._wrap_innov_v(dx[:, 2])
        x = xf[t] + np.einsum("nij,nj->ni", C, dx)
        x[:, 2] = kf_ref._wrap_state_v(x[:, 2])
        xs[t] = x
        Ps[t] = Pf[t] + C @ (Ps[t + 1] - Pp[t + 1]) @ C.transpose(0, 2, 1)
    planes = lambda xl, Pl: (np.stack([a.T for a in xl]), np.stack([b[:, TRI[0], TRI[1]].T for b in Pl]))
    out = dict(zip(("xs", "Ps"), planes(xs, Ps)))
    out["xf"], out["Pf"] = planes(xf, Pf)
    out.update(pred_x=np.stack(qx), pred_P=np.stack(qP), x_end=f.x.copy(), P_end=f.P.copy())
    return out


# ----------------------------------------------------------------------------- the kernels' form
def _wrap(a, hi_closed, pi, two_pi):
    return np.where(a >= pi if hi_closed else a > pi, a - two_pi, np.where(a < -pi, a + two_pi, a))


def _factor(P, y, r):
    """kf_update_factor: U = L^-1 H P, 1 / D, w = L^-1 y, L (unit lower; S = H P H^T + R = L D L^T)"""
    U = [[P[pk(H1[a], j)] for j in range(6)] for a in range(4)]
    L = [[None] * 4 for _ in range(4)]
    E = [[None] * 4 for _ in range(4)]
    dinv = [None] * 4
    for a in range(4):
        for b in range(a + 1):
            s = U[a][H1[b]] + r[pk(a, b)]
            for k in range(b):
                s = s - L[a][k] * E[b][k]
            if a == b:
                dinv[a] = 1 / s
            else:
                E[a][b] = s
                L[a][b] = s * dinv[b]
    w = [None] * 4
    for a in range(4):
        for j in range(6):
            s = U[a][j]
            for k in range(a):
                s = s - L[a][k] * U[k][j]
            U[a][j] = s
        s = y[a]
        for k in range(a):
            s = s - L[a][k] * w[k]
        w[a] = s
    return U, dinv, w, L


def _apply(x, P, U, dinv, w):
    """kf_update_apply: x += U^T D^-1 w, P -= U^T D^-1 U"""
    vw = [w[a] * dinv[a] for a in range(4)]
    V = [[U[a][j] * dinv[a] for j in range(6)] for a in range(4)]
    xn, Pn = list(x), list(P)
    for j in range(6):
        t = U[0][j] * vw[0]
        for a in range(1, 4):
            t = t + U[a][j] * vw[a]
        xn[j] = x[j] + t
    for i in range(6):
        for j in range(i + 1):
            t = U[0][i] * V[0][j]
            for a in range(1, 4):
                t = t + U[a][i] * V[a][j]
            Pn[pk(i, j)] = P[pk(i, j)] - t
    return xn, Pn


def _predict(x, P, dt, q, pi, two_pi):
    xn = list(x)
    xn[0] = dt * x[3] + x[0]
    xn[1] = dt * x[4] + x[1]
    xn[2] = _wrap(dt * x[5] + x[2], True, pi, two_pi)
    Tm = [[P[pk(i, j)] + (dt * P[pk(i + 3, j)] if i < 3 else 0) for j in range(6)] for i in range(6)]
    Pn = list(P)
    for i in range(6):
        for j in range(i + 1):
            t = Tm[i][j] + (dt * Tm[i][j + 3] if j < 3 else 0)
            Pn[pk(i, j)] = t + q[pk(i, j)]
    return xn, Pn


def _select(m, new, old):
    return [np.where(m, a, b) for a, b in zip(new, old)]


def _ldl6(P):
    """P = L D L^T of a packed 6 x 6 (smooth_ldl6): L unit lower, 1 / D"""
    L = [[None] * 6 for _ in range(6)]
    E = [[None] * 6 for _ in range(6)]
    dinv = [None] * 6
    for i in range(6):
        for j in range(i + 1):
            s = P[pk(i, j)]
            for k in range(j):
                s = s - L[i][k] * E[j][k]
            if i == j:
                dinv[i] = 1 / s
            else:
                E[i][j] = s
                L[i][j] = s * dinv[j]
    return L, dinv


def _solve6(L, dinv, v):
    """P^-1 v (smooth_solve6): forward substitution, the scaling, back substitution"""
    u = [None] * 6
    for i in range(6):
        s = v[i]
        for k in range(i):
            s = s - L[i][k] * u[k]
        u[i] = s
    u = [u[i] * dinv[i] for i in range(6)]
    for i in range(4, -1, -1):
        s = u[i]
        for k in range(i + 1, 6):
            s = s - L[k][i] * u[k]
        u[i] = s
    return u


def _filtered_x(x, P, zt, r, m, f, pi, two_pi):
    """x+ of a tick: the forward update's x (the prior where valid == 0)"""
    y = [zt[a].astype(f) - x[H1[a]] for a in range(4)]
    y[0] = _wrap(y[0], False, pi, two_pi)
    xu, Pu = _apply(x, P, *_factor(P, y, r)[:3])
    if m is not None:
        xu, Pu = _select(m, xu, x), _select(m, Pu, P)
    return xu, Pu


def smooth_form(x0, P0, z, valid=None, dtype=np.float32, with_P=True):
    """The kernels' form in `dtype`, in their operation order (module docstring).  Arguments as
    rts_f64; returns (xs [T, 6, N], Ps [T, 21, N] or None, x_end [6, N], P_end [21, N])."""
    f = dtype
    dt, q, r = (f(v) if np.ndim(v) == 0 else v.astype(f) for v in params())
    pi = f(PI_F) if dtype == np.float32 else f(np.pi)
    two_pi = f(2.0) * pi
    Tn, n = z.shape[0], z.shape[2]
    mask = lambda t: None if valid is None else np.asarray(valid[t]).astype(bool)
    x = [np.array(x0[k], f) for k in range(6)]
    P = [np.array(P0[k], f) for k in range(21)]
    hist = []
    for t in range(Tn):                                   # forward: the ticks, every prior kept
        hist.append((x, P))
        xu, Pu = _filtered_x(x, P, z[t], r, mask(t), f, pi, two_pi)
        x, P = _predict(xu, Pu, dt, q, pi, two_pi)
    x_end, P_end = np.stack(x), np.stack(P)
    xs, Ps = [None] * Tn, [None] * Tn
    # the last tick: the filtered state itself
    xc, Pc = _filtered_x(*hist[-1], z[-1], r, mask(Tn - 1), f, pi, two_pi)
    xc[2] = _wrap(xc[2], True, pi, two_pi)
    xs[-1], Ps[-1] = np.stack(xc), np.stack(Pc)
    one = np.ones(n, f)
    for t in range(Tn - 2, -1, -1):                       # backward
        x1, P1 = hist[t + 1]
        L, dinv = _ldl6(P1)
        d = [xc[i] - x1[i] for i in range(6)]
        d[2] = _wrap(d[2], False, pi, two_pi)
        pd = _solve6(L, dinv, d)
        e = []
        for i in range(6):                                # e = (I - Q Pi) d
            s = q[pk(i, 0)] * pd[0]
            for k in range(1, 6):
                s = s + q[pk(i, k)] * pd[k]
            e.append(d[i] - s)
        if with_P:
            X = [[None] * 6 for _ in range(6)]            # Pi Q, column by column
            for j in range(6):
                c = _solve6(L, dinv, [q[pk(k, j)] * one for k in range(6)])
                for k in range(6):
                    X[k][j] = c[k]
            A = [[(one if i == j else 0) - X[j][i] for j in range(6)] for i in range(6)]
            M = [[None] * 6 for _ in range(6)]            # A P_s[t+1]
            for i in range(6):
                for l in range(6):
                    s = A[i][0] * Pc[pk(0, l)]
                    for k in range(1, 6):
                        s = s + A[i][k] * Pc[pk(k, l)]
                    M[i][l] = s
            G = [None] * 21                               # Q - Q Pi Q + A P_s[t+1] A^T
            for i in range(6):
                for j in range(i + 1):
                    s = q[pk(i, 0)] * X[0][j]
                    for k in range(1, 6):
                        s = s + q[pk(i, k)] * X[k][j]
                    s = q[pk(i, j)] - s
                    for l in range(6):
                        s = s + M[i][l] * A[j][l]
                    G[pk(i, j)] = s
            T1 = [[G[pk(i, j)] - (dt * G[pk(i + 3, j)] if i < 3 else 0) for j in range(6)] for i in range(6)]
            Pc = [None] * 21
            for i in range(6):
                for j in range(i + 1):
                    Pc[pk(i, j)] = T1[i][j] - (dt * T1[i][j + 3] if j < 3 else 0)
            Ps[t] = np.stack(Pc)
        xu, _ = _filtered_x(*hist[t], z[t], r, mask(t), f, pi, two_pi)
        xc = [xu[i] + (e[i] - dt * e[i + 3] if i < 3 else e[i]) for i in range(6)]
        xc[2] = _wrap(xc[2], True, pi, two_pi)
        xs[t] = np.stack(xc)
    xs = np.stack(xs)
    assert xs.dtype == f and x_end.dtype == f
    return xs, (np.stack(Ps) if with_P else None), x_end, P_end


def smooth_f32(x0, P0, z, valid=None, with_P=True):
    return smooth_form(x0, P0, z, valid, np.float32, with_P)


# ----------------------------------------------------------------------------- comparing
def deviations(xs, Ps, ref):
    """(dx [6], dP [21]): per row of x and per packed plane of P the largest absolute difference
    from ref["xs"], ref["Ps"] over robots and ticks, heading differences taken mod 2 pi"""
    d = np.abs(np.asarray(xs, np.float64) - ref["xs"])
    d[:, 2] = np.abs((d[:, 2] + np.pi) % (2 * np.pi) - np.pi)
    dP = np.abs(np.asarray(Ps, np.float64) - ref["Ps"]).max(axis=(0, 2)) if Ps is not None else None
    return d.max(axis=(0, 2)), dP


def bounds(dev32, ref):
    """the bound of the module docstring for each of the 6 + 21 quantities, from smooth_f32's
    deviations (dx, dP) and the reference's magnitudes"""
    ulp = lambda a: np.spacing(np.abs(a).max(axis=(0, 2)).astype(np.float32)).astype(np.float64)
    return (MARGIN * np.maximum(dev32[0], ulp(ref["xs"])), MARGIN * np.maximum(dev32[1], ulp(ref["Ps"])))


def crossings(th):
    """robots whose true heading th [T, N] crosses +-pi between two ticks of the window"""
    return np.flatnonzero((np.abs(np.diff(th, axis=0)) > np.pi).any(axis=0))


def random_valid(Tn, n, seed, share=0.7):
    """valid [T, N] uint8 at `share`; tick 0 invalid for the robots with i % 5 == 1 (and valid for
    the others with i % 5 == 0), tick T-1 invalid for i % 7 == 2: both ends of the window see both"""
    v = (np.random.default_rng([seed, 0x76616C]).random((Tn, n)) < share).astype(np.uint8)
    i = np.arange(n)
    v[0, i % 5 == 1] = 0
    v[0, i % 5 == 0] = 1
    v[-1, i % 7 == 2] = 0
    v[-1, i % 7 == 3] = 1
    return v


_WINDOWS = {}


def window(orc, n=N, Tn=T, warm=WARM, seed=SEED):
    """The shared inputs, computed once and never written: a Trajectory of warm + Tn ticks; yaw,
    gz, rpm, rec (records) of all ticks; z [warm + Tn, 4, N]; valid [Tn, N] (random_valid)."""
    key = (n, Tn, warm, seed)
    if key not in _WINDOWS:
        tr = Trajectory(n, warm + Tn, seed=seed)
        yaw, gz, rpm = tr.kf6_inputs()
        w = dict(tr=tr, yaw=yaw, gz=gz, rpm=rpm, rec=fmskf.kf6_records(yaw, gz, rpm), z=measure(orc, yaw, gz, rpm),
                 valid=random_valid(Tn, n, seed), warm=warm, T=Tn, n=n)
        for v in w.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _WINDOWS[key] = w
    return _WINDOWS[key]
