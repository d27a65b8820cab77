"""References of the KF6 EM sufficient statistics (fmskf_tick_many_em) for test_em_cpu.py and
test_gpu_em.py; the shared inputs are smooth_ref.window's.

definition: the float64 definition of include/fmskf.h in the textbook lag-one form, built on
smooth_ref.rts_f64 -- its xs, Ps, its priors (x0 / pred_x, P0 / pred_P), its filtered xf, Pf, its
wraps and the valid mask.  Per step t -> t+1, with C = P+[t] F^T (P-[t+1])^-1 and the lag-one
covariance P_{t,t+1} = C P_s[t+1]:
    E[w w^T | all] = s s^T + P_s[t+1] - F P_{t,t+1} - P_{t,t+1}^T F^T + F P_s[t] F^T,
    s = x_s[t+1] - F x_s[t]   (heading difference wrapped as the innovation is)
and per measured tick v v^T + H P_s[t] H^T, v = z - H x_s[t] (heading wrapped); each of the 21 + 10
packed entries summed per robot with math.fsum.

em_form: the kernels' scheme (csrc/em_lane.hpp on csrc/smooth_lane.hpp's recursion) restated in
numpy in their operation order, in the precision asked for: the transition term as
s s^T + (Q - Q Pi Q) + X^T P_s[t+1] X with Pi = (P-[t+1])^-1 through the LDL^T factor, X = Pi Q,
s = Q Pi (x_s[t+1] - x-[t+1]); every tick's terms formed in that precision and added to float64
accumulators in the kernels' order (s s^T + X^T P_s X, then Q - Q Pi Q; then the tick's measurement
term).  restate_f32 is that in float32 (numpy has no fused multiply-add, the kernels use it
throughout: fp32 roundings of the same operations, not the same bits); form_f64 the same form in
float64, the cancellation-free form test_em_cpu.py holds against `definition`.

Tolerance of the GPU tests (smooth_ref's rule, nothing fixed in advance): per quantity -- the 21
planes of sq, the 10 of sr -- the kernels' largest deviation from `definition` over the robots must
stay within range_ref.MARGIN (8) times the larger of restate_f32's own deviation from `definition`
and one fp32 ulp of the quantity's largest reference magnitude (bounds())."""
import math

import numpy as np

import fmskf

import fix_ref
import loglik_ref as lr
import smooth_ref as sr
from range_ref import MARGIN  # noqa: F401  (the tests take it from here)
from smooth_ref import pk

H = sr.H1
QUANTITIES = ("sq", "sr")
TOTAL_LEN = 34
DIAG_Q = [pk(i, i) for i in range(6)]
DIAG_R = [pk(a, a) for a in range(4)]


def _wrap_innov(a):
    return np.where(a > np.pi, a - 2 * np.pi, np.where(a < -np.pi, a + 2 * np.pi, a))


def _fsum_cols(terms):
    """terms: a list of [N] float64 arrays (possibly empty) -> per robot math.fsum"""
    if not terms:
        return None
    a = np.stack(terms)
    return np.array([math.fsum(a[:, i]) for i in range(a.shape[1])])


# ----------------------------------------------------------------------------- float64 definition
def definition(x0, P0, z, valid=None, ref=None):
    """x0 [6, N], P0 packed [21, N], z [T, 4, N], valid [T, N] or None (rts_f64's arguments; ref: its
    result when the caller has it).  Returns a dict: n_meas [N] uint32, sq [21, N], sr [10, N]."""
    ref = sr.rts_f64(x0, P0, z, valid) if ref is None else ref
    Tn, n = z.shape[0], z.shape[2]
    f = fix_ref.fresh_filter("kf6", n)
    F, Hm = f.F, f.H
    unp = lambda xa, Pa: fix_ref.unpack_state(xa, Pa)
    xs, Ps = zip(*(unp(ref["xs"][t], ref["Ps"][t]) for t in range(Tn)))
    _, Pf = zip(*(unp(ref["xf"][t], ref["Pf"][t]) for t in range(Tn)))
    m = np.ones((Tn, n), bool) if valid is None else np.asarray(valid).astype(bool)
    tq = [[] for _ in range(21)]
    for t in range(Tn - 1):
        Pp1 = ref["pred_P"][t]                                        # P-[t+1]
        C = np.linalg.solve(Pp1, F @ Pf[t]).transpose(0, 2, 1)        # P+ F^T (P-[t+1])^-1
        s = xs[t + 1] - xs[t] @ F.T
        s[:, 2] = _wrap_innov(s[:, 2])
        Pl = C @ Ps[t + 1]                                            # P_{t,t+1}
        FP = F @ Pl
        E = np.einsum("ni,nj->nij", s, s) + Ps[t + 1] - FP - FP.transpose(0, 2, 1) + F @ Ps[t] @ F.T
        for i in range(6):
            for j in range(i + 1):
                tq[pk(i, j)].append(E[:, i, j])
    tr = [[] for _ in range(10)]
    for t in range(Tn):
        v = z[t].astype(np.float64).T - xs[t] @ Hm.T
        v[:, 0] = _wrap_innov(v[:, 0])
        E = np.einsum("na,nb->nab", v, v) + Hm @ Ps[t] @ Hm.T
        for a in range(4):
            for b in range(a + 1):
                tr[pk(a, b)].append(np.where(m[t], E[:, a, b], 0.0))
    zero = np.zeros(n)
    return dict(n_meas=m.sum(axis=0).astype(np.uint32),
                sq=np.stack([zero if not c else _fsum_cols(c) for c in tq]),
                sr=np.stack([_fsum_cols(c) for c in tr]))


# ----------------------------------------------------------------------------- the kernels' form
def em_form(x0, P0, z, valid=None, dtype=np.float32, q=None, r=None):
    """The kernels' scheme in `dtype` (module docstring).  Arguments as definition's; q [21], r [10]:
    the filter's packed Q and R in float64 (default: the default config's), narrowed as the
    library narrows them.  Returns definition's dict plus bad [N] (the robots the kernel leaves
    out: their sq and sr are NaN) and x_end, P_end (the forward pass's final state)."""
    f = dtype
    dt, qd, rd = sr.params()
    dt = f(dt)
    q = qd.astype(f) if q is None else np.float32(np.asarray(q, np.float64)).astype(f)
    r = rd.astype(f) if r is None else np.float32(np.asarray(r, np.float64)).astype(f)
    pi = f(sr.PI_F) if dtype == np.float32 else f(np.pi)
    two_pi = f(2.0) * pi
    Tn, n = z.shape[0], z.shape[2]
    mask = lambda t: None if valid is None else np.asarray(valid[t]).astype(bool)
    x = [np.array(x0[k], f) for k in range(6)]
    P = [np.array(P0[k], f) for k in range(21)]
    hist = []
    acc = np.zeros((31, n), np.float64)
    n_meas = np.zeros(n, np.uint32)
    one = np.ones(n, f)
    with np.errstate(all="ignore"):
        for t in range(Tn):                                   # forward: the ticks, every prior kept
            hist.append((x, P))
            xu, Pu = sr._filtered_x(x, P, z[t], r, mask(t), f, pi, two_pi)
            x, P = sr._predict(xu, Pu, dt, q, pi, two_pi)
        x_end, P_end = np.stack(x), np.stack(P)

        def measured(t, xc, Pc):
            m = np.ones(n, bool) if valid is None else mask(t)
            v = [z[t][a].astype(f) - xc[H[a]] for a in range(4)]
            v[0] = sr._wrap(v[0], False, pi, two_pi)
            for a in range(4):
                for b in range(a + 1):
                    term = v[a] * v[b] + Pc[pk(H[a], H[b])]
                    assert term.dtype == f
                    acc[21 + pk(a, b)] += np.where(m, term.astype(np.float64), 0.0)
            n_meas[:] += m.astype(np.uint32)

        # the last tick: the filtered state itself
        xc, Pc = sr._filtered_x(*hist[-1], z[-1], r, mask(Tn - 1), f, pi, two_pi)
        xc[2] = sr._wrap(xc[2], True, pi, two_pi)
        measured(Tn - 1, xc, Pc)
        for t in range(Tn - 2, -1, -1):                       # backward (smooth_ref.smooth_form)
            x1, P1 = hist[t + 1]
            L, dinv = sr._ldl6(P1)
            d = [xc[i] - x1[i] for i in range(6)]
            d[2] = sr._wrap(d[2], False, pi, two_pi)
            pd = sr._solve6(L, dinv, d)
            s, e = [], []
            for i in range(6):                                # s = Q Pi d, e = (I - Q Pi) d
                u = q[pk(i, 0)] * pd[0]
                for k in range(1, 6):
                    u = u + q[pk(i, k)] * pd[k]
                s.append(u)
                e.append(d[i] - u)
            X = [[None] * 6 for _ in range(6)]                # Pi Q, column by column
            for j in range(6):
                c = sr._solve6(L, dinv, [q[pk(k, j)] * one for k in range(6)])
                for k in range(6):
                    X[k][j] = c[k]
            for j in range(6):                                # EmTap::gain: s s^T + X^T P_s[t+1] X
                y = []
                for l in range(6):
                    u = Pc[pk(l, 0)] * X[0][j]
                    for k in range(1, 6):
                        u = u + Pc[pk(l, k)] * X[k][j]
                    y.append(u)
                for i in range(j, 6):
                    u = s[i] * s[j]
                    for l in range(6):
                        u = u + X[l][i] * y[l]
                    assert u.dtype == f
                    acc[pk(i, j)] += u.astype(np.float64)
            A = [[(one if i == j else 0) - X[j][i] for j in range(6)] for i in range(6)]
            M = [[None] * 6 for _ in range(6)]                # A P_s[t+1]
            for i in range(6):
                for l in range(6):
                    u = A[i][0] * Pc[pk(0, l)]
                    for k in range(1, 6):
                        u = u + A[i][k] * Pc[pk(k, l)]
                    M[i][l] = u
            G = [None] * 21                                   # Q - Q Pi Q + A P_s[t+1] A^T
            for i in range(6):
                for j in range(i + 1):
                    u = q[pk(i, 0)] * X[0][j]
                    for k in range(1, 6):
                        u = u + q[pk(i, k)] * X[k][j]
                    u = q[pk(i, j)] - u
                    acc[pk(i, j)] += u.astype(np.float64)     # EmTap::noise
                    for l in range(6):
                        u = u + M[i][l] * A[j][l]
                    G[pk(i, j)] = u
            T1 = [[G[pk(i, j)] - (dt * G[pk(i + 3, j)] if i < 3 else 0) for j in range(6)] for i in range(6)]
            Pc = [None] * 21
            for i in range(6):
                for j in range(i + 1):
                    Pc[pk(i, j)] = T1[i][j] - (dt * T1[i][j + 3] if j < 3 else 0)
            xu, _ = sr._filtered_x(*hist[t], z[t], r, mask(t), f, pi, two_pi)
            xc = [xu[i] + (e[i] - dt * e[i + 3] if i < 3 else e[i]) for i in range(6)]
            xc[2] = sr._wrap(xc[2], True, pi, two_pi)
            measured(t, xc, Pc)
    bad = ~np.isfinite(acc).all(axis=0)
    acc[:, bad] = np.nan
    return dict(n_meas=n_meas, sq=acc[:21], sr=acc[21:], bad=bad, x_end=x_end, P_end=P_end)


def restate_f32(x0, P0, z, valid=None, q=None, r=None):
    return em_form(x0, P0, z, valid, np.float32, q, r)


def form_f64(x0, P0, z, valid=None):
    return em_form(x0, P0, z, valid, np.float64)


# ----------------------------------------------------------------------------- comparing
def deviations(got, ref):
    """per quantity the largest absolute difference from ref over the robots: sq [21], sr [10]"""
    return {k: np.abs(np.asarray(got[k], np.float64) - ref[k]).max(axis=-1) for k in QUANTITIES}


def bounds(dev32, ref):
    """the bound of the module docstring for every quantity, from restate_f32's deviations and the
    reference's magnitudes"""
    ulp = lambda a: np.spacing(np.abs(a).max(axis=-1).astype(np.float32)).astype(np.float64)
    return {k: MARGIN * np.maximum(dev32[k], ulp(ref[k])) for k in QUANTITIES}


def fleet_fold(d, Tn):
    """total [34] of a per-robot result (n_meas [N], sq [21, N], sr [10, N]) of a window of Tn
    ticks: the kernels' fixed tree (csrc/em_lane.hpp em_store, window_lane.hpp k_window_fold), which is
    loglik_ref.fleet_fold's, over each of the 34 rows {n_trans, n_meas, left out, sq, sr}, the
    robots left out (a NaN in their sums) as zeros in every row but the third -- the same bits."""
    sq, sr_ = np.asarray(d["sq"], np.float64), np.asarray(d["sr"], np.float64)
    n = sq.shape[-1]
    bad = ~(np.isfinite(sq).all(axis=0) & np.isfinite(sr_).all(axis=0))
    rows = [np.full(n, float(Tn - 1)), np.asarray(d["n_meas"]).astype(np.float64)[:n], None, *sq, *sr_]
    out = np.empty(TOTAL_LEN)
    for k, v in enumerate(rows):
        out[k] = lr.fleet_fold(bad.astype(np.float64) if k == 2 else np.where(bad, 0.0, v))
    return out


def mstep(total):
    """(Q [6, 6], R [4, 4], q [21], r [10]) of a fleet total, in float64"""
    q, r = np.asarray(total[3:24]) / total[0], np.asarray(total[24:34]) / total[1]
    Q, R = np.zeros((6, 6)), np.zeros((4, 4))
    for M, p, k in ((Q, q, 6), (R, r, 4)):
        i, j = np.tril_indices(k)
        M[i, j] = p
        M[j, i] = p
    return Q, R, q, r


def priors_qr(orc, x0, P0, yaw, gz, rpm, valid, q, r):
    """loglik_ref.priors for a filter with the packed Q [21] and R [10] (float64)"""
    cfg = fmskf.default_config("kf6", 1)
    prm = orc.kf6_params(cfg.dt, np.asarray(q, np.float64), np.asarray(r, np.float64))
    x, P = np.array(x0, np.float32), np.array(P0, np.float32)
    xs, Ps = [], []
    for t in range(yaw.shape[0]):
        xs.append(x.copy())
        Ps.append(P.copy())
        orc.kf6_tick(x, P, np.ascontiguousarray(yaw[t]), np.ascontiguousarray(gz[t]), np.ascontiguousarray(rpm[t]),
                     None if valid is None else np.ascontiguousarray(valid[t], np.uint8), prm)
    return np.stack(xs), np.stack(Ps)


def host(r):
    """a result dict as numpy arrays (n_meas as uint32), the device drained first"""
    import torch
    torch.cuda.synchronize()
    out = {k: (v.cpu().numpy() if not isinstance(v, np.ndarray) else v) for k, v in r.items()}
    if "n_meas" in out:
        out["n_meas"] = out["n_meas"].view(np.uint32)
    return out
