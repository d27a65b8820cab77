"""References of the KF6 innovation log-likelihood (fmskf_tick_many_loglik) for test_loglik_cpu.py
and test_gpu_loglik.py; the shared inputs are smooth_ref.window's.

priors: orc.kf6_tick tick by tick gives the fp32 state before every tick -- the GPU's own bits --
for any R (the oracle takes the filter's parameters).

definition: the float64 definition of include/fmskf.h, built as gate_ref.nis_f64 is.  From every
prior, in float64: y = z - H x with the heading wrapped (z the kernels' fp32 measurement,
orc.kf6_measure), S = H P H^T + R, NIS by np.linalg.solve, log det S by np.linalg.slogdet, y and
y y^T; each summed per robot over the measured ticks with math.fsum.

restate_f32: the kernels' accumulation scheme (csrc/loglik_lane.hpp) on smooth_ref._factor's
float32 values from the same priors: NIS as kf_nis forms it, summed as a compensated fp32 pair
(TwoSum); log det S through np.frexp of every dinv[a], the mantissas multiplied as
((m0 m1) m2) m3, that into the running mantissa, frexp again, the exponents in an integer, one
float64 log at the end; y[a] and the fp32 products y[i] y[j] as compensated pairs.  numpy has no
fused multiply-add, the kernels use it throughout: another fp32 rounding of the same operations,
not the same bits.

Tolerance of the GPU tests (smooth_ref's rule, nothing fixed in advance): per quantity -- nis_sum,
logdet_sum, the 4 rows of innov_sum, the 10 of innov_outer -- the kernels' largest deviation from
`definition` over the robots must stay within range_ref.MARGIN (8) times the larger of
restate_f32's own deviation and one fp32 ulp of the quantity's largest reference magnitude
(bounds()).

The accumulation's own share (test_loglik_cpu.py): against the float64 sum of -log dinv[a] over
the restatement's own fp32 dinv, logdet_sum is off by at most 4 * n_meas * 2^-24 (four fp32
roundings per measured tick, each at most 2^-24 relative to a factor of the product, so at most
2^-24 / (1 - 2^-24) in the log domain: LOGDET_SLACK covers the second order) plus the final
float64 operations."""
import math

import numpy as np

import fmskf

import smooth_ref as sr
from range_ref import MARGIN

H = sr.H1
U24 = 2.0 ** -24
LOGDET_SLACK = 1.0 + 1e-6
QUANTITIES = ("nis_sum", "logdet_sum", "innov_sum", "innov_outer")
LOG_2PI = math.log(2.0 * math.pi)


def r_default():
    """the filter's packed R [10] in float64, before the kernels narrow it"""
    return np.array(fmskf.default_config("kf6", 1).r[:10])


def orc_params(orc, r=None):
    cfg = fmskf.default_config("kf6", 1)
    return orc.kf6_params(cfg.dt, np.array(cfg.q[:21]), r_default() if r is None else np.asarray(r, np.float64))


def priors(orc, x0, P0, yaw, gz, rpm, valid=None, r=None):
    """(xs [T, 6, N], Ps [T, 21, N] float32: the state before every tick; x_end, P_end)"""
    prm = orc_params(orc, r)
    x, P = np.array(x0, np.float32), np.array(P0, np.float32)
    xs, Ps = [], []
    for t in range(yaw.shape[0]):
        xs.append(x.copy())
        Ps.append(P.copy())
        orc.kf6_tick(x, P, np.ascontiguousarray(yaw[t]), np.ascontiguousarray(gz[t]), np.ascontiguousarray(rpm[t]),
                     None if valid is None else np.ascontiguousarray(valid[t], np.uint8), prm)
    return np.stack(xs), np.stack(Ps), x, P


def _r32(r):
    return np.float32(r_default() if r is None else np.asarray(r, np.float64))


def _fsum_rows(a, m):
    """a [T, N] float64, m [T, N] bool: per robot math.fsum over the ticks where m"""
    return np.array([math.fsum(a[m[:, i], i]) for i in range(a.shape[1])])


def definition(xs, Ps, z, valid=None, r=None):
    """The float64 sums from the fp32 priors (xs, Ps) and z [T, 4, N] float32.  Returns a dict:
    n_meas [N] uint32, nis_sum [N], logdet_sum [N], innov_sum [4, N], innov_outer [10, N]."""
    Tn, _, n = xs.shape
    R = _r32(r).astype(np.float64)
    m = np.ones((Tn, n), bool) if valid is None else np.asarray(valid).astype(bool)
    nis, ld = np.empty((Tn, n)), np.empty((Tn, n))
    ys = np.empty((Tn, 4, n))
    for t in range(Tn):
        x, P = xs[t].astype(np.float64), Ps[t].astype(np.float64)
        y = z[t].astype(np.float64) - x[list(H)]
        y[0] = np.where(y[0] > np.pi, y[0] - 2 * np.pi, np.where(y[0] < -np.pi, y[0] + 2 * np.pi, y[0]))
        S = np.empty((n, 4, 4))
        for a in range(4):
            for b in range(4):
                S[:, a, b] = P[sr.pk(H[a], H[b])] + R[sr.pk(a, b)]
        yt = np.ascontiguousarray(y.T)
        nis[t] = np.einsum("na,na->n", yt, np.linalg.solve(S, yt[:, :, None])[:, :, 0])
        sign, ld[t] = np.linalg.slogdet(S)
        assert (sign > 0).all()
        ys[t] = y
    out = dict(n_meas=m.sum(axis=0).astype(np.uint32), nis_sum=_fsum_rows(nis, m), logdet_sum=_fsum_rows(ld, m))
    out["innov_sum"] = np.stack([_fsum_rows(ys[:, a], m) for a in range(4)])
    out["innov_outer"] = np.stack([_fsum_rows(ys[:, i] * ys[:, j], m) for i in range(4) for j in range(i + 1)])
    return out


def _two_sum(hi, lo, d, m):
    """kf_generic.hpp th_add on float32 arrays, for the robots in m"""
    s = hi + d
    bp = s - hi
    e = (hi - (s - bp)) + (d - bp)
    return np.where(m, s, hi), np.where(m, lo + e, lo)


def restate_f32(xs, Ps, z, valid=None, r=None):
    """The kernels' scheme in float32 (module docstring).  Returns definition's dict, plus dinv
    [T, 4, N] float32 (the restatement's own) and bad [N] (the robots the kernel would leave out)."""
    f = np.float32
    Tn, _, n = xs.shape
    R = _r32(r)
    pi, two_pi = f(sr.PI_F), f(2.0) * f(sr.PI_F)
    m_all = np.ones((Tn, n), bool) if valid is None else np.asarray(valid).astype(bool)
    zero = lambda k=None: np.zeros(n if k is None else (k, n), f)
    nis_hi, nis_lo, pm, E = zero(), zero(), np.ones(n, f), np.zeros(n, np.int64)
    s_hi, s_lo, o_hi, o_lo = zero(4), zero(4), zero(10), zero(10)
    bad = np.zeros(n, bool)
    dinvs = np.empty((Tn, 4, n), f)
    with np.errstate(all="ignore"):
        for t in range(Tn):
            m = m_all[t]
            x, P = xs[t], [Ps[t][k] for k in range(21)]
            y = [z[t][a].astype(f) - x[H[a]] for a in range(4)]
            y[0] = sr._wrap(y[0], False, pi, two_pi)
            _, dinv, w, _ = sr._factor(P, y, R)
            v = w[0] * (w[0] * dinv[0])
            for a in range(1, 4):
                v = v + w[a] * (w[a] * dinv[a])
            assert v.dtype == f
            nis_hi, nis_lo = _two_sum(nis_hi, nis_lo, v, m)
            bad |= m & np.isnan(v)
            mant, ex = zip(*(np.frexp(dinv[a]) for a in range(4)))
            for a in range(4):
                bad |= m & ~((dinv[a] > 0) & np.isfinite(dinv[a]))
                dinvs[t, a] = dinv[a]
            prod = pm * (((mant[0] * mant[1]) * mant[2]) * mant[3])
            assert prod.dtype == f
            pm2, e2 = np.frexp(prod)
            pm = np.where(m, pm2, pm)
            E = np.where(m, E + sum(e.astype(np.int64) for e in ex) + e2, E)
            for a in range(4):
                s_hi[a], s_lo[a] = _two_sum(s_hi[a], s_lo[a], y[a], m)
            for i in range(4):
                for j in range(i + 1):
                    k = sr.pk(i, j)
                    o_hi[k], o_lo[k] = _two_sum(o_hi[k], o_lo[k], y[i] * y[j], m)
        d = np.float64
        out = dict(n_meas=m_all.sum(axis=0).astype(np.uint32),
                   nis_sum=np.where(bad, np.nan, nis_hi.astype(d) + nis_lo.astype(d)),
                   logdet_sum=np.where(bad, np.nan, -(E.astype(d) * math.log(2.0) + np.log(pm.astype(d)))),
                   innov_sum=s_hi.astype(d) + s_lo.astype(d), innov_outer=o_hi.astype(d) + o_lo.astype(d),
                   dinv=dinvs, bad=bad)
    return out


def deviations(got, ref):
    """per quantity the largest absolute difference from ref over the robots: nis_sum, logdet_sum
    scalars, innov_sum [4], innov_outer [10]"""
    return {k: np.abs(np.asarray(got[k], np.float64) - ref[k]).max(axis=-1) for k in QUANTITIES}


def bounds(dev32, ref):
    """the bound of the module docstring for every quantity, from restate_f32's deviations and the
    reference's magnitudes"""
    ulp = lambda a: np.spacing(np.abs(a).max(axis=-1).astype(np.float32)).astype(np.float64)
    return {k: MARGIN * np.maximum(dev32[k], ulp(ref[k])) for k in QUANTITIES}


def model_log(n, Tn, seed, yaw_sigma=0.0):
    """A synthetic log drawn from the filter's own model, so that the default Q and R are its
    true parameters: x0 ~ N(0, P0) (the velocities at a third of P0's deviation, or the fastest
    robots' wheels would pass the int16 rpm: the first tick's innovation alone is smaller than the
    filter expects), x[t+1] = F x[t] + N(0, Q), z[t] = H x[t] + N(0, R), in float64;
    then the inputs that make the kernels' frontend measure z: yaw = z0 in degrees, gyro z = -z1
    in degrees per second, the wheel rpm of the world velocity (z2, z3) turned into the body frame
    by that yaw (the Trajectory's kinematics; the int16 rpm quantise z2, z3 to ~1e-4 m/s against a
    noise of 2e-2).  yaw_sigma: extra Gaussian yaw noise (rad) on top, from its own stream -- the
    same log otherwise.  Returns (yaw [T, N] float32, gz [T, N] float32, rpm [T, N, 4] int16)."""
    from fmskf import synth
    import fix_ref
    f = fix_ref.fresh_filter("kf6", n)
    rng = np.random.default_rng([seed, 0])
    extra = np.random.default_rng([seed, 1]).normal(size=(Tn, n)) * yaw_sigma
    Lq, Lr = np.linalg.cholesky(f.Q), np.linalg.cholesky(f.R)
    x = rng.normal(size=(n, 6)) @ np.linalg.cholesky(f.P[0]).T
    x[:, 3:5] /= 3.0
    yaw, gz, rpm = np.empty((Tn, n), np.float32), np.empty((Tn, n), np.float32), np.empty((Tn, n, 4), np.int16)
    for t in range(Tn):
        z = x @ f.H.T + rng.normal(size=(n, 4)) @ Lr.T
        yaw[t] = np.degrees((z[:, 0] + extra[t] + np.pi) % (2 * np.pi) - np.pi)
        gz[t] = -np.degrees(z[:, 1])
        th = np.radians(yaw[t].astype(np.float64))
        c, s = np.cos(th), np.sin(th)
        wheels = synth.vdir_to_mdir((z[:, 2] * c + z[:, 3] * s) * 1e3, (z[:, 3] * c - z[:, 2] * s) * 1e3, np.zeros(n))
        mrpm = wheels * synth.GEAR / float(synth.RPM_TO_RADPS)
        assert np.abs(mrpm).max() < 32000, "a drawn velocity saturates the int16 rpm"
        rpm[t] = synth._i16(mrpm)
        x = x @ f.F.T + rng.normal(size=(n, 6)) @ Lq.T
    return yaw, gz, rpm


def fleet_loglik(d):
    """the fleet's log-likelihood of a dict of sums, by math.fsum over the robots"""
    return -0.5 * (math.fsum(d["nis_sum"]) + math.fsum(d["logdet_sum"]) + 4.0 * LOG_2PI * int(d["n_meas"].sum()))


# ----------------------------------------------------------------------------- GPU test helpers
def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def kw_of(w, form, valid, lo=None, hi=None):
    """the keyword inputs of ticks lo .. hi-1 of a smooth_ref.window (default: the window behind
    the warm-up), as records or as the three planes, with the mask when given"""
    lo = w["warm"] if lo is None else lo
    hi = w["warm"] + w["T"] if hi is None else hi
    if form == "rec":
        kw = dict(kf6_rec=np.ascontiguousarray(w["rec"][lo:hi]))
    else:
        kw = dict(yaw_deg=np.ascontiguousarray(w["yaw"][lo:hi]), gyro_z_dps=np.ascontiguousarray(w["gz"][lo:hi]),
                  rpm=np.ascontiguousarray(w["rpm"][lo:hi]))
    if valid is not None:
        kw["valid"] = np.ascontiguousarray(valid)
    return kw


def to_device(kw):
    import torch
    out = {}
    for k, v in kw.items():
        if k == "kf6_rec":
            v = v.view(np.int32).reshape(v.shape + (4,))
        out[k] = torch.from_numpy(np.array(v)).cuda()   # a copy: the shared inputs are read-only
    return out


def warmed(w, warm=True, n=None):
    """an engine behind the window's plain warm-up ticks (or fresh from reset())"""
    e = fmskf.Engine("kf6", w["n"] if n is None else n)
    if warm:
        e.tick_many(w["warm"], **kw_of(w, "rec", None, 0, w["warm"]))
    return e


def snapshot(e, gate=False):
    x, P = e.get_state()
    s = [x, P, np.array(e.get_counters(), np.uint64)]
    if gate:
        s += list(e.get_gate().values())
    return s


def same(a, b, what):
    for k, (u, v) in enumerate(zip(a, b)):
        u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
        assert u.tobytes() == v.tobytes(), f"{what}: element {k} of the snapshot changed"


def fleet_fold(v):
    """The kernels' fixed tree over a per-robot float64 array (csrc/window_lane.hpp block_partials,
    k_window_fold): zeros for the lanes past N, inside every 64-lane wave the
    butterfly v[i] + v[i ^ d] for d = 1, 2, .. 32, the four waves of a 256-robot block added in
    order, the blocks added in order from 0.0 -- every addition an IEEE one, so the same bits."""
    v = np.asarray(v, np.float64)
    nb = (v.size + 255) // 256
    w = np.zeros(nb * 256)
    w[:v.size] = v
    w = w.reshape(nb * 4, 64)
    idx = np.arange(64)
    for d in (1, 2, 4, 8, 16, 32):
        w = w + w[:, idx ^ d]
    w = w[:, 0].reshape(nb, 4)
    blocks = ((w[:, 0] + w[:, 1]) + w[:, 2]) + w[:, 3]
    s = np.float64(0.0)
    for b in blocks:
        s = s + b
    return float(s)
