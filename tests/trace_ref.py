"""Shared inputs and helpers of the tests of fmskf_tick_many_trace (test_trace_cpu.py,
test_gpu_trace.py).

The window: gate_ref.gate_inputs(N, WARM + T, SEED, start=WARM) -- a synthetic trajectory with the
5 % + 5 % outlier mix from the first tick behind the warm-up on -- plus a persistent +20 degree yaw
offset on every third robot from tick WARM + 5 on (test_gpu_gate.py's construction: REJECTED until
the run reaches max_consecutive, then FORCED), and a smooth_ref.random_valid mask of share 0.7.
The gate: NIS_MAX = 18.47, max_consecutive = 2.  N = 4113 (no multiple of 256), T = 37 (odd: the
loop unrolled by two ends on its tail), WARM = 50.

reference_statuses: the float64 gate over the oracle (gate_ref.nis_f64 + decide, orc.kf6_tick with
the apply mask, as test_gate_cpu.py runs it).

The GPU's reference is the existing API: a twin handle that runs the window as T calls of
tick_many(1), read out after each (twin_run).  An ungated handle's twin carries a monitor-only
gate (nis_max = +inf, max_consecutive = 0), whose state is the ungated one bit for bit and whose
NIS is what the trace must report."""
import numpy as np

import fmskf

import gate_ref
import smooth_ref as sr
from gate_ref import NIS_MAX
from loglik_ref import bits, kw_of

N, T, WARM, SEED = sr.N, sr.T, sr.WARM, 41
MAXC = 2
OFFSET_FROM, OFFSET_DEG = 5, 20.0
NONE, ACC, REJ, FRC = fmskf.GATE_NONE, fmskf.GATE_ACCEPTED, fmskf.GATE_REJECTED, fmskf.GATE_FORCED
NO_NIS = 0x7FC00000     # the quiet NaN of a tick without a measurement
SMALL = [(n, Tn) for n in (1, 65, 257) for Tn in (1, 2)]

_WINDOWS = {}


def window(n=N, Tn=T, warm=WARM, seed=SEED):
    """The shared inputs, computed once and never written: yaw, gz, rpm, rec of warm + Tn ticks,
    valid [Tn, n]; the keys loglik_ref.kw_of reads."""
    key = (n, Tn, warm, seed)
    if key not in _WINDOWS:
        yaw, gz, rpm, _ = gate_ref.gate_inputs(n, warm + Tn, seed, start=warm)
        yaw = yaw.copy()
        yaw[warm + OFFSET_FROM:, ::3] += np.float32(OFFSET_DEG)
        w = dict(yaw=yaw, gz=gz, rpm=rpm, rec=fmskf.kf6_records(yaw, gz, rpm), valid=sr.random_valid(Tn, n, seed),
                 warm=warm, T=Tn, n=n)
        for v in w.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _WINDOWS[key] = w
    return _WINDOWS[key]


def reference_statuses(orc, w, nis_max=NIS_MAX, max_consecutive=MAXC):
    """status [T, n] of the window's ticks from the float64 gate reference, the warm-up gated by the
    same rule (every warm-up tick measured)"""
    n, warm, Tn = w["n"], w["warm"], w["T"]
    prm = gate_ref.params(orc, n)
    x, P = gate_ref.fresh(n)
    run = np.zeros(n, np.uint8)
    out = np.zeros((Tn, n), np.uint8)
    for t in range(warm + Tn):
        has = np.ones(n, bool) if t < warm else w["valid"][t - warm] != 0
        nis = gate_ref.nis_f64(orc, x, P, w["yaw"][t], w["gz"][t], w["rpm"][t])
        status, run_new, rejected = gate_ref.decide(nis, run, nis_max, max_consecutive)
        status = np.where(has, status, NONE).astype(np.uint8)
        run = np.where(has, run_new, run).astype(np.uint8)
        orc.kf6_tick(x, P, w["yaw"][t], w["gz"][t], np.ascontiguousarray(w["rpm"][t]),
                     (has & ~rejected).astype(np.uint8), prm)
        if t >= warm:
            out[t - warm] = status
    return out


# ----------------------------------------------------------------------------- GPU test helpers
def engine(w, gated, warm=True, monitor=False):
    """an engine of the window's size: gated (NIS_MAX, MAXC), monitor-only, or ungated; behind the
    warm-up ticks (run with that gate), or fresh from reset()"""
    e = fmskf.Engine("kf6", w["n"])
    if gated:
        e.set_gate(NIS_MAX, MAXC)
    elif monitor:
        e.set_gate(float("inf"), 0)
    if warm and w["warm"]:
        e.tick_many(w["warm"], **kw_of(w, "rec", None, 0, w["warm"]))
    return e


def twin_run(w, gated, valid, warm=True):
    """The window as T calls of tick_many(1) on a twin (gated, or monitor-only for an ungated
    handle), read out after each: status, nis [T, n], xs [T, 6, n], Ps [T, 21, n], and the
    snapshot's x, P and counters behind the last tick."""
    n, Tn, lo = w["n"], w["T"], w["warm"]
    r = dict(status=np.zeros((Tn, n), np.uint8), nis=np.zeros((Tn, n), np.float32),
             xs=np.zeros((Tn, 6, n), np.float32), Ps=np.zeros((Tn, 21, n), np.float32))
    with engine(w, gated, warm, monitor=not gated) as e:
        for t in range(Tn):
            e.tick_many(1, **kw_of(w, "rec", None if valid is None else valid[t:t + 1], lo + t, lo + t + 1))
            g = e.get_gate()
            r["status"][t], r["nis"][t] = g["status"], g["nis"]
            r["xs"][t], r["Ps"][t] = e.get_state()
        r["gate"] = e.get_gate()
        r["counters"] = np.array(e.get_counters(), np.uint64)
    return r


def host(r):
    """a result dict as numpy arrays, the device drained first"""
    if all(isinstance(v, np.ndarray) for v in r.values()):
        return r
    import torch
    torch.cuda.synchronize()
    return {k: (v if isinstance(v, np.ndarray) else v.cpu().numpy()) for k, v in r.items()}


def check_against_twin(r, tw, valid, gated, every, what):
    """the trace r (host arrays, N columns) against the twin's per-tick readouts, bit for bit"""
    Tn, n = tw["status"].shape
    has = np.ones((Tn, n), bool) if valid is None else np.asarray(valid[:Tn, :n]) != 0
    st = r["status"][:Tn, :n]
    assert np.array_equal(st, tw["status"]), f"{what}: status"
    assert np.array_equal(st != NONE, has), f"{what}: NONE exactly where valid == 0"
    if not gated:
        assert np.array_equal(st, np.where(has, ACC, NONE)), f"{what}: an ungated tick is ACCEPTED"
    nis = bits(r["nis"][:Tn, :n])
    assert np.array_equal(nis[has], bits(tw["nis"])[has]), f"{what}: nis"
    assert (nis[~has] == NO_NIS).all(), f"{what}: nis of an unmeasured tick"
    assert np.array_equal(r["applied"][:Tn, :n], np.isin(st, (ACC, FRC)).astype(np.uint8)), f"{what}: applied"
    if every:
        rows = Tn // every
        for j in range(rows):
            t = (j + 1) * every - 1
            if "x" in r:
                assert np.array_equal(bits(r["x"][j, :, :n]), bits(tw["xs"][t])), f"{what}: x row {j}"
            if "P" in r:
                assert np.array_equal(bits(r["P"][j, :, :n]), bits(tw["Ps"][t])), f"{what}: P row {j}"
