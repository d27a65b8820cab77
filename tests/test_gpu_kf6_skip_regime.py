"""The write-back mask of a KF6 tick is a property of its launch regime (csrc/kernels_kf6.hip
kf6_wide): the two-per-lane full tick stores the eight cross-covariance planes only where their bits
changed while state + inputs fill at most half the Infinity Cache, their position half otherwise,
and FMSKF_KF6_SKIP_WIDE forces either.  Memory must hold what an unconditional write-back leaves
under every choice: test_gpu_kf6_skip_store.run_all() (bit for bit the oracle's x and P after every
call: from reset, with lanes of one wave disagreeing, with -0.0 planted in all eight cross planes,
with a Q and R under which every masked plane changes on every tick; N = 2 * 256 + 37) runs in a
child process with the mask forced narrow and forced wide on the two-per-lane kernels, and forced
wide on the one-per-lane kernels (which have no wide form, so the switch must change nothing).
test_gpu_kf6_skip_store itself covers the regime's own choice for each variant."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("variant,wide", [("12", "0"), ("12", "1"), ("15", "1")])
def test_write_back_bitexact_with_the_mask_forced(variant, wide):
    path = os.pathsep.join([ROOT, os.path.join(ROOT, "roboken-fmskf-robot-controller_amd"),
                            os.path.join(ROOT, "tests")] + [p for p in [os.environ.get("PYTHONPATH")] if p])
    env = dict(os.environ, FMSKF_KF6_VARIANT=variant, FMSKF_KF6_SKIP_WIDE=wide, PYTHONPATH=path)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "test_gpu_kf6_skip_store.py")],
                         capture_output=True, text=True, timeout=240, env=env)
    assert out.returncode == 0, (out.stdout[-1500:] + out.stderr[-3000:])
    assert "skip store ok" in out.stdout
