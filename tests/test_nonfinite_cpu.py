"""tests/nonfinite_ref.py on the CPU: the plant patterns reach every row of x and P at every fleet
size the GPU tests use, the lane pair is a real pair, and bad_robots is the plain loop."""
import numpy as np
import pytest

import nonfinite_ref as nf

CASES = [(m, n) for m in nf.DIMS for n in nf.SIZES[m]]


@pytest.mark.parametrize("model,n", CASES)
def test_patterns_inside_fleet_and_cover_every_row(model, n):
    sets = {p: nf.plant_set(p, model, n) for p in nf.PATTERNS}
    for p, s in sets.items():
        assert s.dtype == np.int64 and np.all(np.diff(s) > 0), p
        assert s.size == 0 or (s[0] >= 0 and s[-1] < n), p
    assert sets["none"].size == 0
    assert sets["last_only"].tolist() == [n - 1]
    assert n - 1 in sets["dense"] and n - 1 in sets["edges"] and 0 in sets["edges"]
    for k in (1, 63, 64, 255, 256) + tuple(range(128, 192)):
        assert (k in sets["edges"]) == (k < n)
    if n >= 10:  # about 30 %: the per-row minimum of one robot adds at most R robots
        assert 0.2 * n <= sets["dense"].size <= 0.3 * n + nf.rows(model) + 1
    if n >= 257:
        both = np.union1d(sets["edges"], sets["dense"])
        hit = {nf.poison_of(model, int(i))[0] for i in both}
        assert hit == set(range(nf.rows(model)))
        vals = {(r, repr(v)) for r, v in (nf.poison_of(model, int(i)) for i in range(n))}
        if n >= 3 * nf.rows(model):  # every row meets NaN, +Inf and -Inf somewhere in the fleet
            assert len(vals) == 3 * nf.rows(model)


@pytest.mark.parametrize("model,n", CASES)
def test_lane_pair(model, n):
    g, pair = nf.lane_stride(model, n), nf.lane_pair(model, n)
    if model == "kf12d":
        assert g is None and pair is None
        return
    assert g % 256 == 0 and g >= 256 and 2 * g >= n  # two robots per lane cover the fleet
    if n <= g:
        assert pair is None
        return
    i, j = pair
    assert 0 <= i < j < n and j - i == g and i < g
    assert i in nf.plant_set("edges", model, n) and j in nf.plant_set("edges", model, n)
    if n == 257:  # lane 0 serves robots 0 and 256; every other lane's second robot is dead
        assert pair == (0, 256)


def test_lane_stride_restated():
    assert [nf.lane_stride("kf6", n) for n in (1, 257, 512, 513, 700, 1025)] == [256, 256, 256, 512, 512, 768]
    assert [nf.lane_stride("ekf9", n) for n in (1, 257, 513, 2049)] == [256, 256, 512, 1280]


@pytest.mark.parametrize("model", list(nf.DIMS))
def test_bad_robots_is_the_plain_loop(model):
    nx, np_ = nf.DIMS[model]
    n = 300
    rng = np.random.default_rng(5)
    x = rng.normal(size=(nx, n))
    P = rng.normal(size=(np_, n))
    planted = nf.plant_set("dense", model, n)
    xp, Pp = nf.plant(model, x, P, planted)
    want = []
    for i in range(n):
        ok = all(np.isfinite(float(xp[k, i])) for k in range(nx)) and \
            all(np.isfinite(float(Pp[k, i])) for k in range(np_))
        if not ok:
            want.append(i)
    assert nf.bad_robots(xp, Pp).tolist() == want == planted.tolist()
    assert nf.bad_robots(x, P).size == 0 and nf.bad_robots(xp, None).tolist() == nf.x_only(model, planted).tolist()
    # one element per robot, the planted one, and nothing else moved
    changed = (np.concatenate([xp, Pp]) != np.concatenate([x, P])) | ~np.isfinite(np.concatenate([xp, Pp]))
    assert changed.sum() == planted.size
    for i in planted:
        r, v = nf.poison_of(model, int(i))
        got = np.concatenate([xp, Pp])[r, i]
        assert (np.isnan(v) and np.isnan(got)) or got == v


def test_assert_small():
    x = np.array([[1.0, np.nan, -np.inf]])
    nf.assert_small(x, None)
    with pytest.raises(AssertionError):
        nf.assert_small(np.array([[2e30]]), None)
    assert 90 * nf.FINITE_MAX < np.finfo(np.float32).max
