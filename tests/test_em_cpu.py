"""The references of the KF6 EM sufficient statistics (tests/em_ref.py) against each other, the
host M-step, and what the statistics are for; no GPU.  The float64 lag-one sums are the definition
(include/fmskf.h); em_form is the kernels' cancellation-free scheme (csrc/em_lane.hpp)."""
import ctypes as C
import json

import numpy as np
import pytest

import fmskf
from fmskf.synth import Trajectory

import em_ref as er
import loglik_ref as lr
import smooth_ref as sr

T_LONG, N_LONG = 300, 96


# ----------------------------------------------------------------------------- the host M-step
def test_mstep_divides_and_refuses():
    total = np.arange(1.0, 35.0)
    total[0], total[1] = 7.0, 3.0
    q, r = fmskf.em_mstep(total)
    assert q.shape == (21,) and r.shape == (10,)
    assert np.array_equal(q, total[3:24] / 7.0) and np.array_equal(r, total[24:34] / 3.0)
    assert np.array_equal(er.mstep(total)[2], q) and np.array_equal(er.mstep(total)[3], r)
    L = fmskf.load()
    qq, rr = np.full(21, -1.0), np.full(10, -1.0)
    ptr = lambda a: a.ctypes.data
    EINVAL = fmskf._lib.EINVAL
    for k, v in ((0, 0.0), (1, 0.0), (0, -2.0), (1, -1.0), (0, np.nan), (2, np.nan), (5, np.inf), (33, -np.inf)):
        bad = total.copy()
        bad[k] = v
        assert L.fmskf_em_mstep(ptr(bad), ptr(qq), ptr(rr)) == EINVAL, (k, v)
        with pytest.raises(fmskf.FmskfError) as ei:
            fmskf.em_mstep(bad)
        assert ei.value.code == EINVAL
    assert L.fmskf_em_mstep(None, ptr(qq), ptr(rr)) == EINVAL
    assert L.fmskf_em_mstep(ptr(total), None, ptr(rr)) == EINVAL
    assert L.fmskf_em_mstep(ptr(total), ptr(qq), None) == EINVAL
    assert (qq == -1.0).all() and (rr == -1.0).all(), "a refused call wrote its outputs"
    assert L.fmskf_em_mstep(ptr(total), ptr(qq), ptr(rr)) == 0 and np.array_equal(qq, q) and np.array_equal(rr, r)
    assert C.sizeof(fmskf._lib.EmOut) == 48 and fmskf._lib.EM_TOTAL_LEN == 34 == er.TOTAL_LEN


# ----------------------------------------------------------------------------- the two forms
@pytest.fixture(scope="module")
def long_window(orc):
    """test_smooth_cpu.py's window: T = 300 from the reset state, default tuning, 70 % valid"""
    tr = Trajectory(N_LONG, T_LONG, seed=11)
    z = sr.measure(orc, *tr.kf6_inputs())
    valid = sr.random_valid(T_LONG, N_LONG, 11)
    x0, P0 = sr.reset_state(N_LONG)
    return z, valid, sr.rts_f64(x0, P0, z, valid), x0, P0


def test_forms_agree_in_float64(long_window):
    """The cancellation-free form in float64 is the lag-one definition.  The yardstick is the
    definition's own float64 noise: its forward pass (oracle Kf6Batch.step) and the same filter run
    in the kernels' operation order in float64 (em_form's forward pass, smooth_ref's) are two
    float64 roundings of one recursion, and their final covariances differ by `fwd`, taken as
    matrices: the largest entry of the difference over the largest entry of the covariance.  Both
    EM forms are a backward pass on top of such a forward pass, so two roundings of them cannot be
    expected to agree better than that; the sums of sq and of sr, as matrices in the same sense,
    are held to MARGIN times it.  (Matrix-wise, not entry by entry: the lag-one form subtracts
    covariances whose largest entries -- the unobservable position's variance, near 1 -- are nine
    orders above the position entries of sq, so its own error is relative to the matrix.)"""
    z, valid, ref, x0, P0 = long_window
    d = er.definition(x0, P0, z, valid, ref)
    g = er.form_f64(x0, P0, z, valid)
    assert not g["bad"].any() and np.array_equal(d["n_meas"], g["n_meas"])
    Pe = sr.fix_ref.pack_P(ref["P_end"])
    fwd = float(np.abs(Pe - g["P_end"]).max() / np.abs(Pe).max())
    dev = er.deviations(g, d)
    rel = {k: float(dev[k].max() / np.abs(d[k]).max()) for k in er.QUANTITIES}
    entry = {k: (dev[k] / np.abs(d[k]).max(axis=-1)).tolist() for k in er.QUANTITIES}
    print("EM_FORM64 " + json.dumps(dict(forward_rel=fwd, bound=er.MARGIN * fwd, rel=rel, rel_per_entry=entry)))
    assert fwd > 0
    for k in er.QUANTITIES:
        assert rel[k] <= er.MARGIN * fwd, (k, rel[k], fwd)


def test_f32_from_reset_keeps_diagonals(orc):
    """restate_f32 straight from reset() with tick 0 invalid for one robot in five -- the diffuse
    P0, the case that broke the adjoint smoother form: every diagonal entry of sq and sr is >= 0,
    and the sums track the definition"""
    n, Tn = 96, 37
    tr = Trajectory(n, Tn, seed=13)
    z = sr.measure(orc, *tr.kf6_inputs())
    valid = sr.random_valid(Tn, n, 13)
    assert (valid[0] == 0).sum() >= n // 6
    x0, P0 = sr.reset_state(n)
    r32, d = er.restate_f32(x0, P0, z, valid), er.definition(x0, P0, z, valid)
    assert not r32["bad"].any() and np.array_equal(r32["n_meas"], valid.sum(axis=0))
    assert (r32["sq"][er.DIAG_Q] >= 0).all() and (r32["sr"][er.DIAG_R] >= 0).all()
    assert (d["sq"][er.DIAG_Q] >= 0).all() and (d["sr"][er.DIAG_R] >= 0).all()
    dev = er.deviations(r32, d)
    print("EM_F32 " + json.dumps({k: (v / np.abs(d[k]).max(axis=-1)).tolist() for k, v in dev.items()}))
    # fp32 roundings of a few hundred operations per term, each relative to the term's matrix (an
    # off-diagonal sum of signed terms is itself orders below its terms): 1e-4 of the matrix's
    # largest entry is three orders above them and four below the matrix
    for k in er.QUANTITIES:
        assert dev[k].max() <= 1e-4 * np.abs(d[k]).max(), k


# ----------------------------------------------------------------------------- what it is for
N_FIT, T_FIT, SEED_FIT = 256, 50, 21     # test_loglik_cpu.py's log
SIGMA = 0.025                            # rad: R00 starts at default + 4 SIGMA^2, 100 x too large


def test_em_raises_the_likelihood(orc):
    """A log drawn from the filter's own model (lr.model_log: the default Q and R are its true
    parameters), the filter started on the default Q and R00 inflated by 4 SIGMA^2 as
    test_loglik_cpu.py inflates it: each of three M-steps from restate_f32's fleet sums does not
    lower the float64 fleet likelihood (EM's guarantee), the first raises it (the start is no
    stationary point), and R00 moves towards the truth."""
    yaw, gz, rpm = lr.model_log(N_FIT, T_FIT, SEED_FIT)
    z = sr.measure(orc, yaw, gz, rpm)
    x0, P0 = sr.reset_state(N_FIT)
    cfg = fmskf.default_config("kf6", 1)
    q_true, r_true = np.array(cfg.q[:21]), lr.r_default()

    def ll(q, r):
        xs, Ps = er.priors_qr(orc, x0, P0, yaw, gz, rpm, None, q, r)
        return lr.fleet_loglik(lr.definition(xs, Ps, z, None, r))

    q, r = q_true.copy(), r_true.copy()
    r[0] += 4.0 * SIGMA ** 2
    lls = [ll(q, r)]
    for _ in range(3):
        s = er.restate_f32(x0, P0, z, None, q, r)
        assert not s["bad"].any()
        q, r = fmskf.em_mstep(er.fleet_fold(s, T_FIT))
        lls.append(ll(q, r))
    truth = ll(q_true, r_true)
    print("EM_LOGLIK " + json.dumps(dict(loglik=lls, at_true_parameters=truth, r00=[r_true[0] + 4.0 * SIGMA ** 2, r[0]])))
    for a, b in zip(lls, lls[1:]):
        assert b >= a, lls
    assert lls[1] > lls[0] and r[0] < r_true[0] + 4.0 * SIGMA ** 2, (lls, r[0])
