"""The references of the KF6 innovation log-likelihood (tests/loglik_ref.py) against each other,
and what the number is for; no GPU.  The float64 sums are the definition (include/fmskf.h); the
fp32 restatement is the kernels' accumulation scheme (csrc/loglik_lane.hpp)."""
import math

import numpy as np
import pytest

import loglik_ref as lr
import smooth_ref as sr

N_ACC, T_ACC = 96, 300


@pytest.fixture(scope="module")
def acc_window(orc):
    """T = 300 from the reset state (the diffuse P0: log det S moves over orders of magnitude),
    70 % valid: the priors, z, the mask"""
    from fmskf.synth import Trajectory
    tr = Trajectory(N_ACC, T_ACC, seed=12)
    yaw, gz, rpm = tr.kf6_inputs()
    valid = sr.random_valid(T_ACC, N_ACC, 12)
    xs, Ps, _, _ = lr.priors(orc, *sr.reset_state(N_ACC), yaw, gz, rpm, valid)
    return xs, Ps, sr.measure(orc, yaw, gz, rpm), valid


def test_restatement_within_its_derived_bound(acc_window):
    """The mantissa-product accumulation costs at most 4 * n_meas * 2^-24 in logdet_sum: held
    against the float64 sum of -log dinv[a] over the restatement's OWN fp32 dinv (math.fsum), so
    that dinv's error is on neither side."""
    xs, Ps, z, valid = acc_window
    r = lr.restate_f32(xs, Ps, z, valid)
    m = valid.astype(bool)
    assert not r["bad"].any()
    worst = 0.0
    for i in range(N_ACC):
        exact = -math.fsum(np.log(r["dinv"][m[:, i], :, i].astype(np.float64)).ravel())
        n = int(r["n_meas"][i])
        assert n == m[:, i].sum()
        bound = 4 * n * lr.U24 * lr.LOGDET_SLACK + 4 * np.spacing(abs(exact))
        err = abs(r["logdet_sum"][i] - exact)
        worst = max(worst, err / bound)
        assert err <= bound, (i, err, bound)
    print("LOGLIK_ACC", dict(worst_share_of_bound=worst, n_meas_max=int(r["n_meas"].max())))
    assert r["n_meas"].max() > 200


def test_restatement_tracks_the_definition(acc_window):
    """restate_f32 and the float64 definition are roundings of one quantity: the likelihood sums
    agree to fp32 accuracy of their terms (relative to the sum of the terms' magnitudes, T of
    them), the innovation sums likewise"""
    xs, Ps, z, valid = acc_window
    ref, r = lr.definition(xs, Ps, z, valid), lr.restate_f32(xs, Ps, z, valid)
    assert np.array_equal(ref["n_meas"], r["n_meas"])
    dev = lr.deviations(r, ref)
    print("LOGLIK_F32", {k: np.max(v).item() for k, v in dev.items()})
    # per term: dinv and w carry a few hundred fp32 roundings of the factorisation; 1e-4 relative
    # per term is three orders above that and three below the quantities themselves
    assert dev["nis_sum"] <= 1e-4 * np.abs(ref["nis_sum"]).max()
    assert dev["logdet_sum"] <= 1e-4 * T_ACC
    assert (dev["innov_sum"] <= 1e-4 * np.abs(ref["innov_sum"]).max(axis=-1) + 1e-6).all()
    assert (dev["innov_outer"] <= 1e-4 * np.abs(ref["innov_outer"]).max(axis=-1) + 1e-9).all()


def test_loglik_formula():
    import fmskf
    d = dict(nis_sum=np.array([8.0, 3.0]), logdet_sum=np.array([-20.0, -9.5]), n_meas=np.array([2, 1], np.uint32))
    got = fmskf.loglik(d["nis_sum"], d["logdet_sum"], d["n_meas"])
    want = [-0.5 * (8.0 - 20.0 + 8 * math.log(2 * math.pi)), -0.5 * (3.0 - 9.5 + 4 * math.log(2 * math.pi))]
    assert np.allclose(got, want, rtol=1e-15)
    assert math.isclose(lr.fleet_loglik(d), sum(want), rel_tol=1e-14)


# ----------------------------------------------------------------------------- what it is for
N_FIT, T_FIT, SEED_FIT = 256, 50, 21   # the model's velocity random walk (0.06 m/s per tick) stays inside the int16 rpm
SIGMA = 0.025     # rad: sigma^2 = 6.25e-4 = 25 x the default R[0][0] of 2.5e-5
SCALES = (0.25, 1.0, 4.0)


def test_likelihood_ranks_the_yaw_noise(orc):
    """One log drawn from the filter's own model (lr.model_log: the default Q and R are its true
    parameters) and a copy whose yaw carries extra noise of SIGMA.  Candidates: R00 = default +
    SIGMA^2 * {1/4, 1, 4}.  The float64 fleet likelihood of the noisy copy peaks at the middle one;
    that of the clean log at none of them but at the default; and the noisy copy's mean NIS at the
    matching candidate is nearer 4 (its expectation for four rows) than at the other two."""
    r0 = lr.r_default()
    assert SIGMA ** 2 >= 16 * r0[0]
    x0, P0 = sr.reset_state(N_FIT)
    res = {}
    for name, sigma in (("clean", 0.0), ("noisy", SIGMA)):
        yaw, gz, rpm = lr.model_log(N_FIT, T_FIT, SEED_FIT, sigma)
        z = sr.measure(orc, yaw, gz, rpm)
        for c in (0.0,) + SCALES:
            r = r0.copy()
            r[0] += c * SIGMA ** 2
            xs, Ps, _, _ = lr.priors(orc, x0, P0, yaw, gz, rpm, None, r)
            d = lr.definition(xs, Ps, z, None, r)
            res[name, c] = (lr.fleet_loglik(d), math.fsum(d["nis_sum"]) / int(d["n_meas"].sum()))
    print("LOGLIK_FIT", {f"{k[0]}:{k[1]}": v for k, v in res.items()})
    ll = lambda name, c: res[name, c][0]
    nis = lambda name, c: res[name, c][1]
    assert ll("noisy", 1.0) > max(ll("noisy", 0.25), ll("noisy", 4.0))
    assert ll("clean", 0.0) > max(ll("clean", c) for c in SCALES)
    assert abs(nis("noisy", 1.0) - 4) < min(abs(nis("noisy", 0.25) - 4), abs(nis("noisy", 4.0) - 4))
    # and the clean log is consistent at the default: 4 within 5 standard errors of the mean of
    # N T chi-square(4) values (variance 8 each)
    assert abs(nis("clean", 0.0) - 4) < 5 * math.sqrt(8.0 / (N_FIT * T_FIT))
