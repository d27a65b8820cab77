"""Reference for the non-finite guard (fmskf_get_counters [0]; nan_guard, csrc/kf_generic.hpp) and
the plant patterns of tests/test_gpu_nonfinite.py.  numpy only.

What a launch must count is read off the state it stored: bad_robots(x, P) of get_state() after the
launch, the robots with any element of x or packed P that is not finite (np.isfinite is exact).

Condition (the guard tests the *sum* of a robot's x and P, not every element): every finite state
element of a test stays below FINITE_MAX = 1e30 in magnitude.  A robot's sum has at most 12 + 78 =
90 terms (KF12D), so a sum of finite elements stays below 9e31, far inside the fp32 range (3.4e38):
it cannot overflow, and "the sum is not finite" is the same as "some element is not finite".  The
planted finite values, every Q, R, P0 and every input of the tests are chosen accordingly, and
assert_small() holds the twin's state (and the finite part of the poisoned handle's) to it.
"""
import numpy as np

FINITE_MAX = 1e30
POISON = (np.nan, np.inf, -np.inf)

# (nx, np) of the models with a covariance
DIMS = {"kf6": (6, 21), "ekf9": (9, 45), "kf12d": (12, 78)}
# the fleet sizes of the GPU tests: one lane; a second block / tile of one robot (KF6 lane 0 then
# serves robots 0 and 256, every other lane's second robot is dead); ragged rows of tiles
SIZES = {"kf6": (1, 257, 700), "ekf9": (1, 257, 2049), "kf12d": (1, 257, 4097)}
PATTERNS = ("edges", "last_only", "dense", "none")
BLOCK = 256


def rows(model):
    nx, np_ = DIMS[model]
    return nx + np_


def bad_robots(x, P):
    """the robots (ascending) with any element of x[:, i] or P[:, i] not finite"""
    bad = ~np.isfinite(x).all(axis=0)
    if P is not None:
        bad |= ~np.isfinite(P).all(axis=0)
    return np.nonzero(bad)[0]


def assert_small(x, P, what=""):
    """the condition above on the finite elements of a state"""
    for name, a in (("x", x), ("P", P)):
        if a is None:
            continue
        f = np.isfinite(a)
        big = np.abs(np.where(f, a, 0.0)).max() if a.size else 0.0
        assert big < FINITE_MAX, f"{what}: finite {name} element of magnitude {big} (limit {FINITE_MAX})"


def lane_stride(model, n):
    """G of the two-robots-per-lane tick kernels, which serve robots i and i + G in one lane; None
    for a model with one robot per lane.
    KF6 (launch_o / launch_ens_o, kernels_kf6.hip): a grid of ceil(N / 512) blocks, G = grid * 256.
    EKF9 (k_ekf9p, kernels_kf.hip): chunks b and b + g2 of 256 robots, g2 = (ceil(N / 256) + 1) / 2
    (integer division), G = g2 * 256."""
    if model == "kf6":
        return ((n + 2 * BLOCK - 1) // (2 * BLOCK)) * BLOCK
    if model == "ekf9":
        return (((n + BLOCK - 1) // BLOCK + 1) // 2) * BLOCK
    return None


def lane_pair(model, n):
    """(i, i + G): two robots that one lane of the two-per-lane kernel serves, or None when the
    fleet has no such pair (N <= G, or one robot per lane).  Robot 0's lane where its partner is the
    fleet's last robot, else lane 70 (outside the planted wave and the other edges)."""
    g = lane_stride(model, n)
    if g is None or n <= g:
        return None
    i = 70 if 70 + g < n else 0
    return i, i + g


def plant_set(pattern, model, n, seed=0):
    """the robots (ascending, int64) a pattern poisons"""
    if pattern == "none":
        return np.zeros(0, np.int64)
    if pattern == "last_only":
        return np.array([n - 1], np.int64)
    if pattern == "edges":
        s = {0, 1, 63, 64, 255, 256, n - 1} | set(range(128, 192))
        pair = lane_pair(model, n)
        if pair:
            s |= set(pair)
        return np.array(sorted(k for k in s if 0 <= k < n), np.int64)
    if pattern == "dense":
        # a seeded 30 % of the robots, drawn per poisoned row (the robots r, r + R, r + 2 R, ... that
        # poison row r, R = nx + np) so that every row that has a robot gets at least one: of each
        # such class 30 % with the remainder rounded at random, but no fewer than one.  Plus N - 1.
        rng = np.random.default_rng(1000 + seed)
        R = rows(model)
        s = {n - 1}
        for r in range(min(R, n)):
            cls = np.arange(r, n, R)
            k = max(1, int(np.floor(0.3 * cls.size + rng.random())))
            s |= set(rng.choice(cls, min(k, cls.size), replace=False).tolist())
        return np.array(sorted(s), np.int64)
    raise ValueError(pattern)


def poison_of(model, robot):
    """(row, value) planted in `robot`: the row rotates with the robot index over all rows of x and
    then P (row = robot mod (nx + np); a row >= nx is P row `row - nx` of a robot whose x stays
    finite); the value rotates over NaN, +Inf, -Inf so that every row meets all three as the robot
    index grows by nx + np"""
    R = rows(model)
    return robot % R, POISON[(robot // R + robot % R) % 3]


def plant(model, x, P, robots):
    """copies of x, P with poison_of() written into the listed robots"""
    x, P = x.copy(), P.copy()
    nx = DIMS[model][0]
    for i in robots:
        r, v = poison_of(model, int(i))
        if r < nx:
            x[r, i] = v
        else:
            P[r - nx, i] = v
    return x, P


def x_only(model, robots):
    """the listed robots whose poison sits in x (their P is planted finite)"""
    nx = DIMS[model][0]
    return np.array([i for i in robots if poison_of(model, int(i))[0] < nx], np.int64)
