"""The launch regimes of the tick launchers (csrc/launch_regime.hpp) on the CPU: the stand-alone host
program tests/native/regime_table.cpp, built here with g++ from that header alone, prints the regime
of every form on both sides of every boundary; the expected values restate the launchers'
decisions here, with the bytes per robot written out as literals (nothing is imported from the
header under test).  Boundaries are floor(2^28 / bytes) for
the 256 MiB Infinity Cache and floor(2^27 / bytes) for its half.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CACHE, HALF, K = 1 << 28, 1 << 27, 1024

# bytes per robot: KF6 plain / gated / COMP, EKF9 plain / row-gated /
# COMP, KF12D, RS state, the RS tick, one KF6 tick's inputs
KF6 = {(0, 0): 108, (0, 1): 116, (1, 0): 128}  # (comp, gated)
EKF9 = {(0, 0): 220, (0, 1): 228, (1, 0): 240}
KF12D, RS_STATE, RS_TICK, KF6_IN = 90 * 8, 56, 124, 16

ENVS = [{}, {"FMSKF_STATE_NT": "0"}, {"FMSKF_STATE_NT": "1"}, {"FMSKF_KF6_VARIANT": "12"},
        {"FMSKF_KF6_VARIANT": "15"}, {"FMSKF_KF6_VARIANT": "3"}, {"FMSKF_EKF9_VARIANT": "2"},
        {"FMSKF_EKF9_VARIANT": "4"}, {"FMSKF_EKF9_VARIANT": "3"}, {"FMSKF_KF6_SKIP_WIDE": "0"},
        {"FMSKF_KF6_SKIP_WIDE": "1"}, {"FMSKF_KF6_SKIP_WIDE": "2"}]


# ---- the decisions, restated (env: the knobs set in the child process) ----
def state_nt(nbytes, env):
    force = int(env.get("FMSKF_STATE_NT", -1))
    return force != 0 if force >= 0 else nbytes > CACHE


def kf6_regime(n, comp, gated, rec, env):
    v = int(env.get("FMSKF_KF6_VARIANT", 0))
    v = v if v in (12, 15) else 0
    sb = KF6[comp, gated]
    rb = sb + KF6_IN
    nt = state_nt(n * sb, env)
    if (not gated or not nt) and (v == 12 or (v == 0 and n * rb <= CACHE)):
        if v == 12:
            return 1, int(nt), 0
        return 1, int(nt), (48 if rec and n * rb <= HALF else 32) * K
    return 0, int(nt), 48 * K if nt else 0


def kf6_ens_regime(n, comp, env):  # (FMSKF_KF6_VARIANT is not consulted)
    sb = KF6[comp, 0]
    nt = state_nt(n * sb, env)
    if n * (sb + KF6_IN) <= CACHE:
        return 1, int(nt), 32 * K
    return 0, int(nt), 32 * K if nt else 0


def kf6_wide(n, env):
    force = int(env.get("FMSKF_KF6_SKIP_WIDE", -1))
    return int(force == 1 if force in (0, 1) else n * (108 + KF6_IN) <= HALF)


def ekf9_regime(n, comp, gated, libm, env):
    sb = EKF9[comp, gated]
    nt = state_nt(n * sb, env)
    var = int(env.get("FMSKF_EKF9_VARIANT", 0))
    v = var if var in (2, 4) else (2 if n * sb <= CACHE else 4)
    if not libm and v == 2:
        return 1, int(nt), 64 * K
    if libm:
        return 0, int(nt), 0
    return 0, int(nt), 64 * K if nt else 0


def ekf9_ens_regime(n, comp, libm, env):  # (FMSKF_EKF9_VARIANT is not consulted)
    sb = EKF9[comp, 0]
    nt = state_nt(n * sb, env)
    if not libm and n * sb <= CACHE:
        return 1, int(nt), 64 * K
    return 0, int(nt), 0 if libm or not nt else 32 * K


def around(*nbytes):
    """N on both sides of the cache and half-cache boundary of every byte count, and a small N"""
    ns = {4113, 1 << 20, 1 << 21, 1 << 22, 1 << 24}
    for b in nbytes:
        for cap in (CACHE, HALF):
            ns |= {cap // b, cap // b + 1}
    return sorted(ns)


def queries(env):
    """(query line, expected answer line) for every form"""
    q = []
    reg = lambda r: "%d %d %d" % r  # noqa: E731
    for (comp, gated), sb in KF6.items():
        for rec in (0, 1):
            for n in around(sb, sb + KF6_IN):
                q.append((f"kf6 {comp} {gated} {rec} {n}", reg(kf6_regime(n, comp, gated, rec, env))))
    for comp in (0, 1):
        for n in around(KF6[comp, 0], KF6[comp, 0] + KF6_IN):
            q.append((f"kf6_ens {comp} {n}", reg(kf6_ens_regime(n, comp, env))))
    for n in around(108 + KF6_IN):
        q.append((f"kf6_wide {n}", str(kf6_wide(n, env))))
    for (comp, gated), sb in EKF9.items():
        for libm in (0, 1):
            for n in around(sb):
                q.append((f"ekf9 {comp} {gated} {libm} {n}", reg(ekf9_regime(n, comp, gated, libm, env))))
    for comp in (0, 1):
        for libm in (0, 1):
            for n in around(EKF9[comp, 0]):
                q.append((f"ekf9_ens {comp} {libm} {n}", reg(ekf9_ens_regime(n, comp, libm, env))))
    for n in around(KF12D):
        q.append((f"kf12d {n}", reg((0, int(state_nt(n * KF12D, env)), 0))))
    for n in around(RS_TICK):
        nt = state_nt(n * RS_TICK, env)
        q.append((f"rs {n}", reg((1, int(nt), 64 * K if nt else 0))))
    # est_state_bytes per model (FMSKF_MODEL_RS, KF6, EKF9, KF12D = 0..3), plain and COMP
    for model, comp, b in ((0, 0, RS_STATE), (0, 1, RS_STATE), (1, 0, 108), (1, 1, 128), (2, 0, 220),
                           (2, 1, 240), (3, 0, KF12D), (3, 1, KF12D)):
        q.append((f"bytes {model} {comp}", str(b)))
    return q


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("regime") / "regime_table")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "regime_table.cpp"),
                    "-o", exe], check=True)

    def run(env, lines):
        base = {k: v for k, v in os.environ.items() if not k.startswith("FMSKF_")}
        out = subprocess.run([exe], input="\n".join(lines) + "\n", env={**base, **env}, capture_output=True,
                             text=True, check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


@pytest.mark.parametrize("env", ENVS, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "unset")
def test_regime_table(table, env):
    q = queries(env)
    got = table(env, [line for line, _ in q])
    bad = [(line, want, g) for (line, want), g in zip(q, got) if g != want]
    assert not bad, bad[:10]


def test_known_boundaries(table):
    """the boundaries as numbers: plain KF6 state leaves the cache above N = 2 485 513 (108 B), its
    two-per-lane regime ends above 2 164 802 (124 B), plain EKF9 above 1 220 161 (220 B); COMP KF6
    (128 B) is still resident at exactly 2^21, the test there being `>`"""
    assert (CACHE // 108, CACHE // 124, CACHE // 220) == (2485513, 2164802, 1220161)
    got = table({}, ["kf6 0 0 0 2485513", "kf6 0 0 0 2485514", "kf6 0 0 0 2164802", "kf6 0 0 0 2164803",
                     "ekf9 0 0 0 1220161", "ekf9 0 0 0 1220162", "kf6 1 0 0 %d" % (1 << 21),
                     "kf6 1 0 0 %d" % ((1 << 21) + 1), "kf6_wide 1082401", "kf6_wide 1082402"])
    assert got == ["0 0 0", "0 1 49152", "1 0 32768", "0 0 0", "1 0 65536", "0 1 65536", "0 0 0", "0 1 49152",
                   "1", "0"]


def test_forced_values(table):
    """each knob forces what it is documented to force; out-of-range values are ignored"""
    big, small = "kf6 0 0 0 %d" % (1 << 24), "kf6 0 0 0 4113"
    assert table({"FMSKF_KF6_VARIANT": "12"}, [big, small]) == ["1 1 0", "1 0 0"]
    assert table({"FMSKF_KF6_VARIANT": "15"}, [big, small]) == ["0 1 49152", "0 0 0"]
    assert table({"FMSKF_KF6_VARIANT": "3"}, [big, small]) == table({}, [big, small]) == ["0 1 49152", "1 0 32768"]
    # the gated family has no streamed two-per-lane kernel, forced or not
    assert table({"FMSKF_KF6_VARIANT": "12", "FMSKF_STATE_NT": "1"}, ["kf6 0 1 0 4113", small]) == ["0 1 49152", "1 1 0"]
    ebig, esmall = "ekf9 0 0 0 %d" % (1 << 22), "ekf9 0 0 0 4113"
    assert table({"FMSKF_EKF9_VARIANT": "2"}, [ebig, esmall]) == ["1 1 65536", "1 0 65536"]
    assert table({"FMSKF_EKF9_VARIANT": "4"}, [ebig, esmall]) == ["0 1 65536", "0 0 0"]
    assert table({"FMSKF_EKF9_VARIANT": "3"}, [ebig, esmall]) == table({}, [ebig, esmall]) == ["0 1 65536", "1 0 65536"]
    assert table({"FMSKF_STATE_NT": "1"}, [small, esmall, "kf12d 4113", "rs 4113"]) == \
        ["1 1 32768", "1 1 65536", "0 1 0", "1 1 65536"]
    assert table({"FMSKF_STATE_NT": "0"}, [big, ebig]) == ["0 0 0", "0 0 0"]
    wide = ["kf6_wide 4113", "kf6_wide %d" % (1 << 24)]
    assert table({"FMSKF_KF6_SKIP_WIDE": "0"}, wide) == ["0", "0"]
    assert table({"FMSKF_KF6_SKIP_WIDE": "1"}, wide) == ["1", "1"]
    assert table({"FMSKF_KF6_SKIP_WIDE": "2"}, wide) == table({}, wide) == ["1", "0"]
