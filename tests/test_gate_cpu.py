"""The innovation gate's ABI surface (fmskf_set_gate / fmskf_get_gate; no compute calls) and a
check of the shared test inputs on the float64 reference alone: the GPU tests compare the gate's
decision with float64 outside a narrow band around nis_max, which is only a test if few
robot-ticks fall into the band and the outlier mix is rejected at a rate worth testing.  No GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import gate_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_gate_abi_surface(tmp_path):
    import fmskf
    from fmskf import _lib
    src = open(os.path.join(ROOT, "include", "fmskf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in ("fmskf_set_gate", "fmskf_get_gate"):
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES
        assert hasattr(fmskf.load(), name)
    assert re.search(r"#define\s+FMSKF_ABI_VERSION\s+3u", code)
    L = fmskf.load()
    g = _lib.Gate(gate_ref.NIS_MAX, 3)
    assert L.fmskf_set_gate(None, C.byref(g)) == _lib.EINVAL
    assert L.fmskf_set_gate(None, None) == _lib.EINVAL
    assert L.fmskf_get_gate(None, None, None, None, None, _lib.MEM_HOST) == _lib.EINVAL
    # the C compiler's layout of fmskf_gate and the status values against the Python mirror
    c = tmp_path / "gate.c"
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fmskf.h"\nint main(void){'
                 'printf("%zu %zu %zu %d %d %d %d\\n", sizeof(fmskf_gate), offsetof(fmskf_gate, nis_max), '
                 'offsetof(fmskf_gate, max_consecutive), FMSKF_GATE_NONE, FMSKF_GATE_ACCEPTED, '
                 'FMSKF_GATE_REJECTED, FMSKF_GATE_FORCED); return 0;}\n')
    exe = tmp_path / "gate"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == [C.sizeof(_lib.Gate), _lib.Gate.nis_max.offset, _lib.Gate.max_consecutive.offset,
                   fmskf.GATE_NONE, fmskf.GATE_ACCEPTED, fmskf.GATE_REJECTED, fmskf.GATE_FORCED]
    assert got[:3] == [8, 0, 4]


def test_gate_inputs_on_the_reference(orc):
    """4096 robots x 200 ticks, default KF6 noise, nis_max = 18.47, the 5 % + 5 % outlier mix from
    tick 20 on, gated in float64 (rejected robots skip the update through the oracle's `valid`):
    at most 0.1 % of the robot-ticks lie within 1e-3 * nis_max of the threshold, and between 3 %
    and 15 % are rejected"""
    n, T = 4096, 200
    yaw, gz, rpm, kind = gate_ref.gate_inputs(n, T, seed=4096)
    prm = gate_ref.params(orc, n)
    x, P = gate_ref.fresh(n)
    band = rejected = 0
    for t in range(T):
        nis = gate_ref.nis_f64(orc, x, P, yaw[t], gz[t], rpm[t])
        band += int(np.count_nonzero(np.abs(nis - gate_ref.NIS_MAX) <= gate_ref.BAND * gate_ref.NIS_MAX))
        apply = nis <= gate_ref.NIS_MAX
        rejected += int(np.count_nonzero(~apply))
        orc.kf6_tick(x, P, yaw[t], gz[t], np.ascontiguousarray(rpm[t]), apply.astype(np.uint8), prm)
    assert np.all(np.isfinite(x)) and np.all(np.isfinite(P))
    print(f"in the band: {band} of {n * T}; rejected: {rejected / (n * T):.4f}; outliers injected: "
          f"{np.count_nonzero(kind) / (n * T):.4f}")
    assert band <= 1e-3 * n * T
    assert 0.03 <= rejected / (n * T) <= 0.15
