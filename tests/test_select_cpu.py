"""The numpy reference of fmskf_select (tests/select_ref.py) on hand-made cases (no GPU)."""
import numpy as np

import select_ref
from select_ref import GATE_RUN, NONFINITE, POS_VAR


def _state(n, nx=6):
    x = np.zeros((nx, n), np.float32)
    P = np.zeros((nx * (nx + 1) // 2, n), np.float32)
    P[0], P[2] = 1.0, 2.0
    return x, P


def test_threshold_is_strict():
    x, P = _state(4)             # P[0] + P[2] = 1 + 2: exactly the threshold
    P[2, 1] = 2.0 + 2.0 ** -22   # just above: 3 + 2^-22 is a float32
    P[2, 2] = 2.0 - 2.0 ** -22   # just below: 3 - 2^-22 is a float32
    # one float32 addition: 1 + 2^-23 and 2 sum to 3 + 2^-23 in float64, above the threshold, and
    # to 3 in float32 (a tie, rounded to even), which is not
    P[0, 3] = 1.0 + 2.0 ** -23
    assert float(P[0, 3]) + float(P[2, 3]) > 3.0
    robots, reason, count = select_ref.select(x, P, pos_var_min=3.0)
    assert robots.tolist() == [1] and reason.tolist() == [POS_VAR] and count == 1


def test_nan_sum_selects_only_nonfinite():
    x, P = _state(5)
    P[0, 1] = np.nan
    P[2, 2] = np.inf       # an infinite sum is above every finite threshold
    P[0, 3], P[2, 3] = np.inf, -np.inf   # inf - inf: a NaN sum from two non-NaN rows
    x[4, 4] = -np.inf      # x only: the sum is finite
    r = select_ref.reasons(x, P, pos_var_min=10.0)
    assert r.tolist() == [0, 0, POS_VAR, 0, 0]
    r = select_ref.reasons(x, P, nonfinite=True)
    assert r.tolist() == [0, NONFINITE, NONFINITE, NONFINITE, NONFINITE]
    r = select_ref.reasons(x, P, nonfinite=True, pos_var_min=10.0)
    assert r.tolist() == [0, NONFINITE, NONFINITE | POS_VAR, NONFINITE, NONFINITE]


def test_reasons_combine_by_or():
    x, P = _state(6)
    run = np.array([0, 3, 0, 3, 1, 3], np.uint8)
    P[0, 2:4] = 100.0
    x[0, 5] = np.nan
    P[2, 5] = 100.0
    robots, reason, count = select_ref.select(x, P, run, nonfinite=True, pos_var_min=50.0, run_min=3)
    assert robots.tolist() == [1, 2, 3, 5] and count == 4
    assert reason.tolist() == [GATE_RUN, POS_VAR, POS_VAR | GATE_RUN, NONFINITE | POS_VAR | GATE_RUN]
    # a criterion that was not asked for leaves no bit
    robots, reason, count = select_ref.select(x, P, run, run_min=1)
    assert robots.tolist() == [1, 3, 4, 5] and set(reason.tolist()) == {GATE_RUN}


def test_row_mask_picks_rows():
    x, P = _state(4, 9)
    run = np.zeros((6, 4), np.uint8)
    run[0, 1] = 3   # heading row
    run[4, 2] = 2   # vbx row
    run[5, 3] = 5   # vby row
    assert select_ref.select(x, P, run, run_min=3, row_mask=0x01)[0].tolist() == [1]
    assert select_ref.select(x, P, run, run_min=3, row_mask=0x30)[0].tolist() == [3]
    assert select_ref.select(x, P, run, run_min=2, row_mask=0x30)[0].tolist() == [2, 3]
    assert select_ref.select(x, P, run, run_min=1, row_mask=0x3F)[0].tolist() == [1, 2, 3]


def test_capacity_truncates_the_list_not_the_count():
    x, P = _state(100)
    P[0, ::3] = 50.0
    full = select_ref.select(x, P, pos_var_min=10.0)
    assert full[2] == 34 and full[0].tolist() == list(range(0, 100, 3))
    robots, reason, count = select_ref.select(x, P, pos_var_min=10.0, capacity=5)
    assert count == 34 and robots.tolist() == [0, 3, 6, 9, 12] and reason.tolist() == [POS_VAR] * 5
    robots, reason, count = select_ref.select(x, P, pos_var_min=10.0, capacity=0)
    assert count == 34 and robots.size == 0 and reason.size == 0
    assert np.all(np.diff(full[0].astype(np.int64)) > 0)


def test_binding_declares_the_select_entry_points():
    """the ctypes mirror of fmskf_select_params is the header's 16 bytes and the three entry points
    are bound"""
    import ctypes as C
    from fmskf import _lib
    assert C.sizeof(_lib.SelectParams) == 16
    assert [f[0] for f in _lib.SelectParams._fields_] == ["criteria", "pos_var_min", "run_min", "row_mask"]
    assert {"fmskf_select", "fmskf_get_state_subset", "fmskf_set_state_subset"} <= set(_lib.SIGNATURES)
    assert (_lib.SEL_NONFINITE, _lib.SEL_POS_VAR, _lib.SEL_GATE_RUN) == (NONFINITE, POS_VAR, GATE_RUN)
