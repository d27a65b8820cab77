"""fmskf_tick_many_trace without a GPU: the ABI surface (struct layout, header, export, binding) and
a check of the shared test inputs on the float64 gate reference alone -- the GPU tests ask that
every status occurs in the traced window, which is only a test if the inputs produce them."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

import trace_ref as tr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ("mem", "reserved", "pitch", "every", "reserved2", "nis", "status", "applied", "x", "P")


def test_trace_abi_surface(tmp_path):
    import fmskf
    from fmskf import _lib
    src = open(os.path.join(ROOT, "include", "fmskf.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bfmskf_tick_many_trace\s*\(", code)
    assert "fmskf_tick_many_trace" in _lib.SIGNATURES
    assert hasattr(fmskf.load(), "fmskf_tick_many_trace")
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert any(ln.split()[-1] == "fmskf_tick_many_trace" and " T " in ln for ln in out.splitlines())
    assert re.search(r"#define\s+FMSKF_ABI_VERSION\s+3u", code), "the call does not bump the ABI version"
    assert fmskf.load().fmskf_tick_many_trace(None, None, 1, 1, None) == _lib.EINVAL
    assert callable(fmskf.Engine.tick_many_trace)
    # the C compiler's layout of fmskf_trace_out against the ctypes mirror
    c = tmp_path / "trace.c"
    offs = ", ".join(f"offsetof(fmskf_trace_out, {f})" for f in FIELDS)
    c.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "fmskf.h"\nint main(void){'
                 'printf("%zu' + " %zu" * len(FIELDS) + '\\n", sizeof(fmskf_trace_out), ' + offs + '); return 0;}\n')
    exe = tmp_path / "trace"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(c), "-o", str(exe)], check=True)
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert [n for n, _ in _lib.TraceOut._fields_] == list(FIELDS)
    assert got == [C.sizeof(_lib.TraceOut)] + [getattr(_lib.TraceOut, f).offset for f in FIELDS]
    assert got == [64, 0, 4, 8, 16, 20, 24, 32, 40, 48, 56]


def test_trace_inputs_on_the_reference(orc):
    """the main window on the float64 gate reference (NIS_MAX = 18.47, max_consecutive = 2): each of
    NONE, ACCEPTED, REJECTED and FORCED occurs on at least 64 robot-ticks, and at least one FORCED
    directly follows two REJECTED.  A condition on the inputs, not a measurement."""
    w = tr.window()
    st = tr.reference_statuses(orc, w)
    counts = {s: int(np.count_nonzero(st == s)) for s in (tr.NONE, tr.ACC, tr.REJ, tr.FRC)}
    print(f"statuses of {tr.N} x {tr.T} robot-ticks: {counts}")
    for s, c in counts.items():
        assert c >= 64, (s, c)
    chain = (st[2:] == tr.FRC) & (st[1:-1] == tr.REJ) & (st[:-2] == tr.REJ)
    assert chain.any(), "no FORCED directly behind two REJECTED"
