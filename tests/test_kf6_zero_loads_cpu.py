"""Where the two-per-lane full KF6 tick leaves out the loads of cross planes known to hold zero
(csrc/launch_regime.hpp kf6_zero_loads), on the CPU: the stand-alone host program
tests/native/zero_loads_table.cpp, built here with g++ from that header alone.  The expected values
restate the decision with the bytes written out as literals: state + one tick's inputs (108 + 16 B
per robot) within half the 256 MiB Infinity Cache, i.e. N <= floor(2^27 / 124) = 1 082 401, the
regime of the wide write-back mask; FMSKF_KF6_ZERO_LOADS = 0 / 1 forces it, any other value is
ignored, and the knob leaves kf6_wide alone.  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HALF = 1 << 27
EDGE = HALF // 124
NS = [1, 63, 64, 65, 549, 1 << 20, EDGE, EDGE + 1, 1 << 21, 1 << 24]


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("zero_loads") / "zero_loads_table")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror",
                    os.path.join(ROOT, "tests", "native", "zero_loads_table.cpp"), "-o", exe], check=True)

    def run(env):
        base = {k: v for k, v in os.environ.items() if not k.startswith("FMSKF_")}
        out = subprocess.run([exe], input="\n".join(map(str, NS)) + "\n", env={**base, **env},
                             capture_output=True, text=True, check=True).stdout.splitlines()
        assert len(out) == len(NS)
        return [tuple(int(w) for w in line.split()) for line in out]
    return run


def test_boundary_is_half_the_cache(table):
    assert EDGE == 1082401
    got = table({})
    assert [z for z, _ in got] == [int(n * 124 <= HALF) for n in NS]
    assert got[NS.index(EDGE)] == (1, 1) and got[NS.index(EDGE + 1)] == (0, 0)
    assert got[NS.index(1 << 20)] == (1, 1) and got[NS.index(1 << 21)] == (0, 0)


@pytest.mark.parametrize("value,want", [("0", 0), ("1", 1)])
def test_knob_forces_both_sides(table, value, want):
    got = table({"FMSKF_KF6_ZERO_LOADS": value})
    assert [z for z, _ in got] == [want] * len(NS)
    assert [w for _, w in got] == [w for _, w in table({})]  # the mask's regime is not the knob's


def test_other_values_are_ignored(table):
    assert table({"FMSKF_KF6_ZERO_LOADS": "2"}) == table({}) == table({"FMSKF_KF6_ZERO_LOADS": "-1"})


def test_wide_knob_does_not_move_it(table):
    """the function answers for the regime; the launcher asks it only where the wide mask is taken"""
    assert [z for z, _ in table({"FMSKF_KF6_SKIP_WIDE": "0"})] == [z for z, _ in table({})]
