"""The range call's ABI surface (fmskf_set_anchors / fmskf_get_anchors / fmskf_correct_range; no
compute calls), the synthetic range lists, the float64 reference against kf_ref.kf_update_batch and
against its float32 restatement, and a check of the shared closed-loop inputs on the float64
reference alone: the GPU test compares every accept / reject decision with float64 outside a narrow
band around d2_max, which is only a test if few ranges fall into the band, the lengthened ranges
are rejected and the good ones are not.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import range_ref
from range_ref import ACC, NEAR, REJ

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_range_abi_surface(tmp_path):
    import fmskf
    from fmskf import _lib
    src = open(os.path.join(ROOT, "include", "fmskf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    L = fmskf.load()
    for name in ("fmskf_set_anchors", "fmskf_get_anchors", "fmskf_correct_range"):
        assert re.search(r"\b%s\s*\(" % name, code)
        assert name in _lib.SIGNATURES and hasattr(L, name)
    assert re.search(r"#define\s+FMSKF_ABI_VERSION\s+3u", code)
    assert L.fmskf_abi_version() == 3 == fmskf.ABI_VERSION
    prm = _lib.RangeParams()
    assert L.fmskf_correct_range(None, None, 0, C.byref(prm), None, None, _lib.MEM_HOST) == _lib.EINVAL
    assert L.fmskf_set_anchors(None, None, 0) == _lib.EINVAL
    assert L.fmskf_get_anchors(None, None, 0, None) == _lib.EINVAL
    # the C compiler's layout of both structs and the constants against the Python mirror
    c = tmp_path / "rng.c"
    F = ("robot", "anchor", "range_m", "var_m2")
    G = ("tag", "var_m2", "d2_max", "d_min", "flags", "reserved")
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fmskf.h"\nint main(void){'
                 'printf("%zu ' + "%zu " * len(F) + '%zu ' + "%zu " * len(G) + '%u %u %d %d\\n", sizeof(fmskf_range_fix), ' +
                 "".join(f"offsetof(fmskf_range_fix, {k}), " for k in F) + "sizeof(fmskf_range_params), " +
                 "".join(f"offsetof(fmskf_range_params, {k}), " for k in G) +
                 "FMSKF_RANGE_ANCHORS_MAX, FMSKF_RANGE_RUN_MAX, FMSKF_RANGE_NEAR, FMSKF_FIX_IGNORED); return 0;}\n")
    exe = tmp_path / "rng"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    Fx, Pm = _lib.RangeFix, _lib.RangeParams
    assert got == [C.sizeof(Fx)] + [getattr(Fx, k).offset for k in F] + [C.sizeof(Pm)] + \
        [getattr(Pm, k).offset for k in G] + [fmskf.RANGE_ANCHORS_MAX, fmskf.RANGE_RUN_MAX, fmskf.RANGE_NEAR,
                                              fmskf.FIX_IGNORED]
    # 16 bytes a range; the parameters are six floats and two words, 32 bytes
    assert got[:5] == [16, 0, 4, 8, 12] and got[5:12] == [32, 0, 12, 16, 20, 24, 28]
    assert got[12:] == [1024, 8, 5, 4]
    assert fmskf.RANGE_FIX_DTYPE.itemsize == 16
    assert [fmskf.RANGE_FIX_DTYPE.fields[k][1] for k in F] == [0, 4, 8, 12]
    rec = fmskf.range_fix_records(np.array([3, 3, 9]), np.array([0, 1, 2]), np.array([1.5, 2.5, 3.5]))
    assert rec.dtype == fmskf.RANGE_FIX_DTYPE and rec["robot"].tolist() == [3, 3, 9] and np.all(rec["var_m2"] == 0)
    assert rec.view(np.uint32).reshape(-1, 4)[1].tolist() == [3, 1, np.float32(2.5).view(np.uint32), 0]


def test_synth_range_fixes():
    """the synthetic range lists: none before `start`; the robots (i + t) % every == 0, each with a
    burst of `run` entries to the anchors (t // every + k + i) % A, non-descending; no outlier
    before `outlier_start`; outliers only lengthen, by 0.5 - 2 m; the rest within noise of the
    distance from the antenna at the truth (px[t - 1], py[t - 1], th[t]) to the anchor"""
    from fmskf.synth import Trajectory, range_fixes
    tr = Trajectory(300, 60, seed=5)
    A, tag = range_ref.ANCHORS, range_ref.TAG
    assert range_fixes(tr, 7, A, tag)[0].size == 0
    seen = np.zeros(300, int)
    for t in range(8, 60):
        robot, anchor, rho, out = range_fixes(tr, t, A, tag, seed=5, outlier_share=0.3)
        assert robot.dtype == np.uint32 and anchor.dtype == np.uint32 and rho.dtype == np.float32
        i = np.flatnonzero((np.arange(300) + t) % 32 == 0)
        assert np.array_equal(robot, np.repeat(i, 3)) and np.all(np.diff(robot.astype(np.int64)) >= 0)
        k = np.tile(np.arange(3), i.size)
        assert np.array_equal(anchor, (t // 32 + k + robot) % 4)
        assert np.array_equal(range_ref.run_positions(robot), k)
        np.add.at(seen, robot, 1)
        if t == 39:
            assert seen.min() >= 3  # every robot has had a burst before the first outlier
        r = robot.astype(np.int64)
        th = tr.th[t, r]
        p = np.stack([tr.px[t - 1, r] + np.cos(th) * tag[0] - np.sin(th) * tag[1],
                      tr.py[t - 1, r] + np.sin(th) * tag[0] + np.cos(th) * tag[1], np.full(r.size, tag[2])], axis=1)
        e = rho - np.linalg.norm(p - A[anchor].astype(np.float64), axis=1)
        assert not out.any() or t >= 40
        assert np.all(np.abs(e[~out]) < 0.3) and np.all((e[out] > 0.2) & (e[out] < 2.3))
        again = range_fixes(tr, t, A, tag, seed=5, outlier_share=0.3)
        assert all(np.array_equal(a, b) for a, b in zip((robot, anchor, rho, out), again))
    r1 = range_fixes(tr, 20, A, tag, run=1, every=4)
    assert np.array_equal(r1[0], np.flatnonzero((np.arange(300) + 20) % 4 == 0))


def _random_states(n, K, seed):
    rng = np.random.default_rng(seed)
    x = rng.normal(0, 0.5, (K, n))
    M = rng.normal(0, 0.3, (K, n, n))
    P = M @ M.transpose(0, 2, 1) + 0.05 * np.eye(n)
    return x.astype(np.float32), P.astype(np.float32), rng


@pytest.mark.parametrize("n", [6, 9])
def test_reference_update(n):
    """the float64 update: H is the gradient of the predicted distance in (px, py, theta)
    (finite differences), gain and covariance equal kf_ref.kf_update_batch with that H, NEAR and a
    NaN range leave the row alone, and the float32 restatement agrees to fp32 accuracy"""
    K = 200
    x, P, rng = _random_states(n, K, 11 + n)
    P = 0.5 * (P + P.transpose(0, 2, 1))
    anc = range_ref.ANCHORS[rng.integers(0, 4, K)]
    th = x[:, 2].astype(np.float64)
    rho = (np.linalg.norm(anc[:, :2] - x[:, :2], axis=1) + rng.normal(0, 0.3, K)).astype(np.float32)
    r = np.full(K, range_ref.VAR)
    tag = range_ref.TAG
    xn, Pn, d2, st, d, H, y = range_ref.range_update_f64(x, P, np.sin(th), np.cos(th), anc, rho, r, tag, np.inf, 0.5)
    assert np.all(st == ACC) and np.all(d2 >= 0) and np.all(H[:, 3:] == 0)
    eps = 1e-6
    for j in range(3):
        xp = x.astype(np.float64)
        xp[:, j] += eps
        tp = xp[:, 2]
        dp = range_ref.range_update_f64(xp, P, np.sin(tp), np.cos(tp), anc, rho, r, tag, np.inf, 0.5)[4]
        assert np.abs((dp - d) / eps - H[:, j]).max() < 1e-5, j
    assert range_ref.cross_check(x.astype(np.float64), P.astype(np.float64), H, y, r, range(0, K, 3)) < 1e-9
    # rows the gate rejects, NEAR rows and NaN ranges come back unchanged
    far = rho.copy()
    far[::2] += np.float32(5.0)
    far[5] = np.nan
    a2 = anc.copy()
    a2[7] = (x[7, 0], x[7, 1], tag[2])   # an anchor within the lever arm of the antenna
    for fn, dt in ((range_ref.range_update_f64, np.float64), (range_ref.range_update_f32, np.float32)):
        o = fn(x.astype(dt), P.astype(dt), np.sin(th).astype(dt), np.cos(th).astype(dt), a2, far, r, tag, 10.83, 0.5)
        assert o[3][7] == NEAR and o[2][7] == 0 and o[3][5] == REJ and np.isnan(o[2][5])
        same = (o[3] != ACC)
        assert np.array_equal(o[0][same], x[same].astype(dt)) and np.array_equal(o[1][same], P[same].astype(dt))
        assert np.all(o[3][np.arange(0, K, 2)] != ACC)
    f32 = range_ref.range_update_f32(x, P, np.sin(th), np.cos(th), anc, rho, r, tag, np.inf, 0.5)
    dev = range_ref.deviations((f32[0].astype(np.float64), f32[1].astype(np.float64), f32[2].astype(np.float64)),
                               (xn, Pn, d2))
    print(f"n = {n}: float32 restatement against float64: {dev}")
    assert 0 < dev["x"] < 1e-4 and 0 < dev["P"] < 1e-4 and 0 < dev["d2"] < 1e-3


def test_run_loop_is_sequential():
    """apply_list on a list with runs equals the calls that carry every robot's j-th entry"""
    x, P, rng = _random_states(6, 40, 3)
    x, P = x.astype(np.float64), P.astype(np.float64)
    robot = np.repeat(np.arange(0, 40, 2), np.arange(20) % 4 + 1).astype(np.uint32)
    anchor = rng.integers(0, 4, robot.size).astype(np.uint32)
    rho = rng.uniform(7.0, 10.0, robot.size).astype(np.float32)
    A = range_ref.ANCHORS.astype(np.float64)
    a = range_ref.apply_list(range_ref.range_update_f64, x, P, robot, anchor, rho, None, A, range_ref.trig64, d2_max=50.0)
    xs, Ps = x, P
    pos = range_ref.run_positions(robot)
    d2 = np.zeros(robot.size)
    for j in range(4):
        s = pos == j
        xs, Ps, d2[s], _, _ = range_ref.apply_list(range_ref.range_update_f64, xs, Ps, robot[s], anchor[s], rho[s], None,
                                                   A, range_ref.trig64, d2_max=50.0)
    assert np.array_equal(a[0], xs) and np.array_equal(a[1], Ps) and np.array_equal(a[2], d2)
    assert np.any(a[3] == ACC) and np.any(a[3] == REJ)
    untouched = np.arange(1, 40, 2)
    assert np.array_equal(a[0][untouched], x[untouched])


@pytest.mark.parametrize("model", ["kf6", "ekf9"])
def test_range_inputs_on_the_reference(orc, model):
    """The closed-loop recipe on the float64 reference alone (1024 robots x 400 ticks, the filter
    started N(0, 0.5 m) off the truth, range_fixes defaults, gate 10.83): at least 30 000
    decisions, at most 0.5 % of them within 1e-3 d2_max of the threshold, at least 95 % of the
    lengthened ranges rejected, at most 1 % of the good ones rejected, every predicted distance
    above 1 m, and the median final position error below a tenth of the same run's without
    ranges."""
    r = range_ref.closed_loop(orc, model)
    d2 = np.concatenate(r["d2"])
    st = np.concatenate(r["status"])
    outlier = np.concatenate([f[3] for f in r["fixes"]])
    band = int(np.count_nonzero(range_ref.in_band(d2)))
    bad_rej = int(np.count_nonzero(st[outlier] == REJ))
    good_rej = int(np.count_nonzero(st[~outlier] == REJ))
    print(f"{model}: decisions {d2.size}; in the band {band}; lengthened ranges rejected {bad_rej} of "
          f"{np.count_nonzero(outlier)}; good ranges rejected {good_rej} of {np.count_nonzero(~outlier)}; smallest "
          f"predicted distance {r['dmin']:.2f} m; median final error {np.median(r['err']):.4f} m with, "
          f"{np.median(r['err_plain']):.4f} m without; P00 max {r['p00'].max():.3e} with, min "
          f"{r['p00_plain'].min():.3e} without")
    assert not np.any(st == NEAR)
    assert d2.size >= 30000
    assert band <= 0.005 * d2.size
    assert bad_rej >= 0.95 * np.count_nonzero(outlier) and np.count_nonzero(outlier) > 1000
    assert good_rej <= 0.01 * np.count_nonzero(~outlier)
    assert r["dmin"] > 1.0
    assert np.median(r["err"]) < 0.1 * np.median(r["err_plain"])
    assert np.all(r["p00"] < r["p00_plain"])
