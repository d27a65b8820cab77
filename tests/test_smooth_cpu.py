"""The references of the KF6 fixed-interval smoother (tests/smooth_ref.py) against each other and
against the synthetic truth; no GPU.  The float64 Rauch-Tung-Striebel pass is the definition
(include/fmskf.h); the kernels' adjoint form must be the same quantity, and smoothing must be
worth having with the default tuning."""
import numpy as np
import pytest

from fmskf.synth import Trajectory

import fix_ref
import smooth_ref as sr

T_LONG, N_LONG = 300, 96


@pytest.fixture(scope="module")
def long_window(orc):
    """T = 300 from the reset state, default tuning, 70 % valid: (z, valid, ref, x0, P0)"""
    tr = Trajectory(N_LONG, T_LONG, seed=11)
    z = sr.measure(orc, *tr.kf6_inputs())
    valid = sr.random_valid(T_LONG, N_LONG, 11)
    x0, P0 = sr.reset_state(N_LONG)
    return z, valid, sr.rts_f64(x0, P0, z, valid), x0, P0


def test_forms_agree_in_float64(long_window):
    """the textbook RTS and the kernels' adjoint form, both in float64, are roundings of one
    quantity: within 1e-10 in every row of x_s and every plane of P_s (measured: ~1e-13)"""
    z, valid, ref, x0, P0 = long_window
    xs, Ps, x_end, P_end = sr.smooth_form(x0, P0, z, valid, np.float64)
    dx, dP = sr.deviations(xs, Ps, ref)
    print("SMOOTH_FORM64", dict(x=float(dx.max()), P=float(dP.max())))
    assert dx.max() <= 1e-10 and dP.max() <= 1e-10, (dx, dP)
    # and its forward pass is the same filter
    assert np.abs(x_end.T - ref["x_end"])[:, [0, 1, 3, 4, 5]].max() <= 1e-10
    assert np.abs(fix_ref.pack_P(ref["P_end"]) - P_end).max() <= 1e-10


def test_reference_forward_is_kf6batch(long_window):
    """the reference's forward pass is oracle.kf_ref.Kf6Batch's: the predict of every filtered
    state it forms equals, exactly, the state an independent Kf6Batch holds after that tick"""
    z, valid, ref, x0, P0 = long_window
    f = fix_ref.fresh_filter("kf6", N_LONG)
    f.x, f.P = fix_ref.unpack_state(x0, P0)
    for t in range(T_LONG):
        f.step(z[t].astype(np.float64), valid[t])
        assert np.array_equal(f.x, ref["pred_x"][t]) and np.array_equal(f.P, ref["pred_P"][t]), t
    assert np.array_equal(f.x, ref["x_end"]) and np.array_equal(f.P, ref["P_end"])


def test_smoothed_variances(long_window):
    """every smoothed variance is positive and at most the filtered one"""
    ref = long_window[2]
    diag = [sr.pk(i, i) for i in range(6)]
    vs, vf = ref["Ps"][:, diag], ref["Pf"][:, diag]
    assert (vs > 0).all()
    assert (vs <= vf * (1 + 1e-12)).all(), float((vs / vf).max())
    assert np.array_equal(ref["Ps"][-1], ref["Pf"][-1])


def test_f32_form_tracks_the_reference(long_window):
    """smooth_f32 (the kernels' form in float32) does not cancel while the prior is diffuse.  The
    window starts from P0 (heading variance 1) with tick 0 invalid for one robot in five: there a
    form that subtracts from the filtered covariance (P+ - P+ Lambda P+, or the textbook
    P+ + C (P_s - P-) C^T) loses the smoothed heading variance of 4e-7 to the rounding of numbers
    near 1 (6e-8 each) and returns negative variances.  This form must keep every variance positive
    and the heading variance within one such rounding, 6e-8, of the reference (measured: 2e-10)"""
    z, valid, ref, x0, P0 = long_window
    assert (valid[0] == 0).sum() >= N_LONG // 6
    xs, Ps, _, _ = sr.smooth_f32(x0, P0, z, valid)
    dx, dP = sr.deviations(xs, Ps, ref)
    print("SMOOTH_F32", dict(x=dx.tolist(), P_heading=float(dP[sr.pk(2, 2)]),
                             var_heading=float(ref["Ps"][:, sr.pk(2, 2)].min())))
    assert (Ps[:, [sr.pk(i, i) for i in range(6)]] > 0).all()
    assert dP[sr.pk(2, 2)] <= float(np.spacing(np.float32(0.75)))


def test_smoothing_beats_filtering_on_the_trajectory(orc):
    """Trajectory(512, 160, seed=5) with one tick in 10 measured: the smoothed RMS error of
    heading, vx and vy against the truth over ticks 40 .. T-2 is below the filtered one.  No
    assertion on omega: the truth holds it constant, which the white-acceleration Q does not
    describe."""
    n, Tn = 512, 160
    tr = Trajectory(n, Tn, seed=5)
    assert sr.crossings(tr.th).size >= 1, "no robot's heading crosses +-pi inside the window"
    z = sr.measure(orc, *tr.kf6_inputs())
    valid = np.zeros((Tn, n), np.uint8)
    valid[::10] = 1
    ref = sr.rts_f64(*sr.reset_state(n), z, valid)
    sl = slice(40, Tn - 1)
    wrap = lambda a: (a + np.pi) % (2 * np.pi) - np.pi
    ratios = {}
    for name, row, truth, w in (("heading", 2, tr.th, wrap), ("vx", 3, tr.vx_w, None), ("vy", 4, tr.vy_w, None)):
        es, ef = ref["xs"][sl, row] - truth[sl], ref["xf"][sl, row] - truth[sl]
        if w:
            es, ef = w(es), w(ef)
        rs, rf = np.sqrt(np.mean(es ** 2)), np.sqrt(np.mean(ef ** 2))
        ratios[name] = float(rs / rf)
        assert rs < rf, (name, rs, rf)
    print("SMOOTH_RATIOS", ratios, "crossing robots", int(sr.crossings(tr.th).size))
