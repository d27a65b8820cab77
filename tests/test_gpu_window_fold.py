"""The fold of the fleet total (csrc/window_lane.hpp k_window_fold) across a chunk boundary: at
N = 257 * 256 + 1 = 65793 robots the grid has 258 blocks, so the fold's chunk loop runs more than
once and ends on a ragged tail of two partials, for the log-likelihood's chunk (256) and for EM's
(128).  T = 2 from reset(), the masked inputs of the suites' test_small_shapes.  The total must be
the fixed tree of the call's own per-robot outputs bit for bit, and a second, accumulating call
must double the counts exactly.  No oracle filter run."""
import numpy as np
import pytest

from fmskf import Engine

import em_ref as er
import loglik_ref as lr
import smooth_ref as sr

pytestmark = pytest.mark.gpu

N, T = 257 * 256 + 1, 2


def b64(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("call", ["loglik", "em"])
def test_fold_across_chunks(orc, call):
    wd = sr.window(orc, n=N, Tn=T, warm=0, seed=100 + N)
    valid = wd["valid"]
    kw = lr.kw_of(wd, "rec", valid, 0, T)
    assert 0 < int(valid.sum()) < T * N
    with Engine("kf6", N) as e:
        if call == "loglik":
            got = e.tick_many_loglik(T, total=True, **kw)
            tree = np.array([lr.fleet_fold(got[k]) for k in ("n_meas", "nis_sum", "logdet_sum")] + [0.0])
            counts = [0, 3]
        else:
            got = e.tick_many_em(T, per_robot=True, total=True, **kw)
            tree = er.fleet_fold(got, T)
            counts = [0, 1, 2]
            assert got["total"][0] == (T - 1) * N
        assert np.array_equal(got["n_meas"], valid.sum(axis=0)), "n_meas is not the mask's column sums"
        assert np.array_equal(b64(got["total"]), b64(tree)), "total is not the fixed tree of the per-robot sums"
        assert got["total"][1 if call == "em" else 0] == int(valid.sum())
        first = {k: v.copy() for k, v in got.items()}
        again = (e.tick_many_loglik if call == "loglik" else e.tick_many_em)(T, accumulate_into=got, **kw)
        assert again is got
    assert np.array_equal(got["n_meas"], 2 * first["n_meas"])
    for k in counts:
        assert got["total"][k] == 2 * first["total"][k], k
