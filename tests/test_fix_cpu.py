"""The pose-fix call's ABI surface (fmskf_correct_pose; no compute calls) and a check of the shared
closed-loop inputs on the float64 reference alone: the GPU test compares every accept / reject
decision with float64 outside a narrow band around nis_max, which is only a test if few fixes fall
into the band and the outlier share is rejected at a rate worth testing.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import fix_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fix_abi_surface(tmp_path):
    import fmskf
    from fmskf import _lib
    src = open(os.path.join(ROOT, "include", "fmskf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bfmskf_correct_pose\s*\(", code)
    assert "fmskf_correct_pose" in _lib.SIGNATURES
    assert hasattr(fmskf.load(), "fmskf_correct_pose")
    assert re.search(r"#define\s+FMSKF_ABI_VERSION\s+3u", code)
    assert fmskf.load().fmskf_abi_version() == 3 == fmskf.ABI_VERSION
    L = fmskf.load()
    prm = _lib.PoseFixParams()
    assert L.fmskf_correct_pose(None, None, 0, C.byref(prm), None, None, _lib.MEM_HOST) == _lib.EINVAL
    # the C compiler's layout of both structs and the constants against the Python mirror
    c = tmp_path / "fix.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fmskf.h"\nint main(void){'
                 'printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %u %d %d %d\\n", sizeof(fmskf_pose_fix), '
                 'offsetof(fmskf_pose_fix, robot), offsetof(fmskf_pose_fix, x_m), offsetof(fmskf_pose_fix, y_m), '
                 'offsetof(fmskf_pose_fix, theta_rad), sizeof(fmskf_pose_fix_params), '
                 'offsetof(fmskf_pose_fix_params, r), offsetof(fmskf_pose_fix_params, nis_max), '
                 'offsetof(fmskf_pose_fix_params, flags), FMSKF_FIX_HEADING, FMSKF_FIX_IGNORED, '
                 'FMSKF_GATE_ACCEPTED, FMSKF_GATE_REJECTED); return 0;}\n')
    exe = tmp_path / "fix"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    F, Pm = _lib.PoseFix, _lib.PoseFixParams
    assert got == [C.sizeof(F), F.robot.offset, F.x_m.offset, F.y_m.offset, F.theta_rad.offset,
                   C.sizeof(Pm), Pm.r.offset, Pm.nis_max.offset, Pm.flags.offset,
                   fmskf.FIX_HEADING, fmskf.FIX_IGNORED, fmskf.GATE_ACCEPTED, fmskf.GATE_REJECTED]
    # 16 bytes a fix; the parameters are six doubles and two words, 56 bytes as C lays them out
    assert got[:9] == [16, 0, 4, 8, 12, 56, 0, 48, 52]
    assert fmskf.POSE_FIX_DTYPE.itemsize == 16
    assert [fmskf.POSE_FIX_DTYPE.fields[k][1] for k in ("robot", "x_m", "y_m", "theta_rad")] == [0, 4, 8, 12]


def test_synth_pose_fixes():
    """the synthetic fix lists: none before `start`, robots (i + t) % every == 0 ascending, no
    outlier before `outlier_start`, outliers displaced by 0.5 - 2 m, the rest within noise"""
    from fmskf.synth import Trajectory, pose_fixes
    tr = Trajectory(300, 60, seed=5)
    assert pose_fixes(tr, 7)[0].size == 0
    seen = np.zeros(300, int)
    for t in range(8, 60):
        robot, x, y, th, out = pose_fixes(tr, t, seed=5, outlier_share=0.3)
        assert robot.dtype == np.uint32 and np.all(np.diff(robot.astype(np.int64)) > 0)
        assert np.array_equal(robot, np.flatnonzero((np.arange(300) + t) % 32 == 0))
        seen[robot] += 1
        if t == 39:
            assert seen.min() >= 1  # every robot has had a fix before the first outlier
        d = np.hypot(x - tr.px[t - 1, robot], y - tr.py[t - 1, robot])
        assert not out.any() or t >= 40
        assert np.all(d[~out] < 0.08) and np.all((d[out] > 0.4) & (d[out] < 2.1))
        assert np.all(np.abs(th - tr.th[t, robot]) < 0.08)
        again = pose_fixes(tr, t, seed=5, outlier_share=0.3)
        assert all(np.array_equal(a, b) for a, b in zip((robot, x, y, th, out), again))


@pytest.mark.parametrize("m", [2, 3])
def test_fix_inputs_on_the_reference(orc, m):
    """4096 robots x 400 ticks, seed 4096, the pose_fixes defaults, default KF6 noise, gated in
    float64 at 13.82 (m = 2) / 16.27 (m = 3): at most 0.1 % of the fixes lie within 1e-3 * nis_max
    of the threshold, between 3 % and 8 % are rejected, and the reference's final position error
    against the truth is finite.  Measured here: m = 2: 50 176 fixes, 2 in the band, 4.68 % rejected,
    final error <= 11.3 mm; m = 3: 50 176 fixes, 1 in the band, 4.66 % rejected, <= 10.8 mm."""
    r = fix_ref.closed_loop(orc, "kf6", m)
    nis = np.concatenate(r["nis"])
    apply = np.concatenate(r["apply"])
    outlier = np.concatenate([f[4] for f in r["fixes"]])
    band = int(np.count_nonzero(fix_ref.in_band(nis, m)))
    rejected = np.count_nonzero(~apply) / nis.size
    print(f"m = {m}: fixes {nis.size}; in the band {band}; rejected {rejected:.4f}; outliers injected "
          f"{np.count_nonzero(outlier) / nis.size:.4f}; final position error max {r['err'].max():.3e} m; "
          f"final P00 max {r['p00'].max():.3e}")
    assert nis.size == 50176
    assert band <= 1e-3 * nis.size
    assert 0.03 <= rejected <= 0.08
    assert np.all(np.isfinite(r["err"]))
