"""numpy reference of fmskf_select (include/fmskf.h): the ascending list of the robots for which
any requested criterion holds, their reason bytes and the uncapped count, from a handle's own
readouts.  The arithmetic is the header's: an element-wise isfinite over x and packed P, one
float32 addition of packed rows 0 and 2 with a strict `>`, an integer compare of the runs."""
import numpy as np

NONFINITE, POS_VAR, GATE_RUN = 1, 2, 4
ROWS = 6


def reasons(x, P, run=None, nonfinite=False, pos_var_min=None, run_min=None, row_mask=0x3F):
    """the reason byte of every robot ([N] uint8, 0: not selected).  x [n, N], P [n(n+1)/2, N]
    float32; run [N] (KF6 gate) or [6, N] (EKF9 row gate) for run_min."""
    x, P = np.asarray(x), np.asarray(P)
    assert x.dtype == np.float32 and P.dtype == np.float32
    r = np.zeros(x.shape[1], np.uint8)
    if nonfinite:
        bad = ~np.isfinite(x).all(axis=0) | ~np.isfinite(P).all(axis=0)
        r[bad] |= NONFINITE
    if pos_var_min is not None:
        with np.errstate(invalid="ignore", over="ignore"):
            s = P[0] + P[2]  # one float32 addition
            assert s.dtype == np.float32
            r[s > np.float32(pos_var_min)] |= POS_VAR  # a NaN sum compares false
    if run_min is not None:
        run = np.asarray(run)
        if run.ndim == 1:
            hit = run >= run_min
        else:
            rows = [a for a in range(ROWS) if (row_mask >> a) & 1]
            hit = (run[rows] >= run_min).any(axis=0)
        r[hit] |= GATE_RUN
    return r


def select(x, P, run=None, capacity=None, **prm):
    """(robots [min(count, capacity)] uint32 ascending, reason uint8, count)"""
    r = reasons(x, P, run, **prm)
    robots = np.flatnonzero(r).astype(np.uint32)
    count = int(robots.size)
    if capacity is not None:
        robots = robots[:capacity]
    return robots, r[robots], count
