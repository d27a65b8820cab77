"""The KF6 kernels write a masked covariance plane (csrc/kf6_lane.hpp kKf6SkipMask) and the gate
word back only where the bits changed.  Memory must hold what an unconditional write-back leaves:
every case here is bit for bit the oracle's x and P after every call, with all masked planes
unchanged (from reset: no lane of any wave stores them), with lanes of one wave disagreeing (a
random SPD P on every third robot), with -0.0 planted in the cross planes, and with a Q and R that
couple the heading and the translation blocks so every masked plane changes on every tick.

n = 2 * 256 + 37: full waves, a partial wave, clamped lanes, and both robots of a two-per-lane
kernel's lane.  Both single-tick kernels are forced (FMSKF_KF6_VARIANT 12 and 15) in a child
process, as test_gpu_parity does; the child runs this file's run_all()."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 2 * 256 + 37
T = 12
CROSS = (3, 4, 8, 12, 15, 16, 18, 19)
MAXC = 2


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same(e, xo, Po, what, lo=None):
    x, P = e.get_state()
    assert np.array_equal(_bits(x), _bits(xo)), f"{what}: x"
    bad = [k for k in range(21) if not np.array_equal(_bits(P[k]), _bits(Po[k]))]
    assert not bad, f"{what}: P planes {bad}"
    if lo is not None:
        assert np.array_equal(_bits(e.get_state_lo()), _bits(lo)), f"{what}: lo"


def _coupled():
    """default dt and P0, Q and R with every entry non-zero (param_cases.dense)"""
    import param_cases
    d = param_cases.case("kf6", "all_dense")
    return param_cases.default_params("kf6")._replace(q=d.q, r=d.r)


def _spd(rng, count):
    """packed lower triangles [21, count] of random SPD 6 x 6 matrices of the filter's scale,
    every entry non-zero, condition number below ten"""
    A = rng.normal(size=(count, 6, 6))
    M = 1e-3 * (A @ A.transpose(0, 2, 1) / 6.0 + np.eye(6))
    return np.stack([M[:, i, j] for i in range(6) for j in range(i + 1)]).astype(np.float32)


def _phases(e, xo, Po, lo=None):
    """yields the phase name after preparing the engine's and the oracle's state for it"""
    yield "reset"
    rng = np.random.default_rng(5)
    Po[:, ::3] = _spd(rng, len(range(0, N, 3)))
    e.set_state(xo, Po)
    if lo is not None:
        e.set_state_lo(lo)
    yield "spd_every_third"
    for k in CROSS:
        Po[k, 1::5] = np.float32(-0.0)
    assert np.signbit(Po[3, 1])
    e.set_state(xo, Po)
    if lo is not None:
        e.set_state_lo(lo)
    yield "minus_zero"


def _inputs(seed):
    from fmskf.synth import Trajectory
    import fmskf
    yaw, gz, rpm = Trajectory(N, 3 * T, seed=seed).kf6_inputs()
    return yaw, gz, rpm, fmskf.kf6_records(yaw, gz, rpm)


def _plain(orc, prm, form, comp=False):
    """one ungated engine through the three phases, T ticks each, in one input form"""
    import fmskf
    import param_cases
    yaw, gz, rpm, rec = _inputs(31)
    op = param_cases.orc_params(orc, prm)
    xo, Po = param_cases.fresh(prm, N)
    lo = np.zeros((5, N), np.float32) if comp else None

    def ref(t, upd=True, pred=True):
        r = np.ascontiguousarray(rpm[t])
        if comp:
            orc.kf6_tick_comp(xo, Po, lo, yaw[t], gz[t], r, None, op, upd, pred)
        else:
            orc.kf6_tick(xo, Po, yaw[t], gz[t], r, None, op, upd, pred)

    kw = param_cases.engine_kw(prm)
    with fmskf.Engine("kf6", N, flags=fmskf.CFG_COMP_POS if comp else 0, **kw) as e:
        t = 0
        for phase in _phases(e, xo, Po, lo):
            what = f"{form} comp={comp} {phase}"
            if form == "tick_many":
                for cnt in (5, 5, 2):
                    e.tick_many(cnt, kf6_rec=rec[t:t + cnt])
                    for k in range(cnt):
                        ref(t + k)
                    t += cnt
                    _same(e, xo, Po, f"{what} t={t}", lo)
                continue
            for _ in range(T):
                planes = dict(yaw_deg=yaw[t], gyro_z_dps=gz[t], rpm=rpm[t])
                if form == "records":
                    e.tick(kf6_rec=rec[t])
                    ref(t)
                elif form == "planes":
                    e.tick(**planes)
                    ref(t)
                elif form == "isr":
                    e.isr_tick(frames=False, **planes)
                    ref(t)
                else:  # correct, then predict, each checked on its own
                    e.correct(kf6_rec=rec[t]) if t % 2 else e.correct(**planes)
                    ref(t, True, False)
                    _same(e, xo, Po, f"{what} t={t} correct", lo)
                    e.predict()
                    ref(t, False, True)
                _same(e, xo, Po, f"{what} t={t}", lo)
                t += 1
        assert e.get_counters()[0] == 0
    if prm is not None and form == "records" and not comp:
        return Po
    return None


def _gated(orc, prm):
    """a gated engine: some robots reject (their gate word changes), most accept with the word
    they had.  State bit for bit the oracle's fed the applied robots; the word's fields follow from
    the status history; status and NIS against float64 (gate_ref: there is no bitwise gate oracle;
    the decision is compared outside gate_ref.BAND around nis_max, and the fp32 NIS, which
    test_gpu_gate holds to 3e-6 on the default run, to that same 1e-3, the width the decision
    check already grants it); tick_many(5) against the single ticks, state and gate readout bit
    for bit"""
    import fmskf
    import gate_ref
    import param_cases
    from gate_ref import NIS_MAX, BAND
    ACC, REJ, FRC = fmskf.GATE_ACCEPTED, fmskf.GATE_REJECTED, fmskf.GATE_FORCED
    yaw, gz, rpm, _ = gate_ref.gate_inputs(N, 3 * T, seed=4100, start=3)
    rec = fmskf.kf6_records(yaw, gz, rpm)
    op = param_cases.orc_params(orc, prm)
    xo, Po = param_cases.fresh(prm, N)
    kw = param_cases.engine_kw(prm)
    with fmskf.Engine("kf6", N, **kw) as e, fmskf.Engine("kf6", N, **kw) as m:
        for h in (e, m):
            h.set_gate(NIS_MAX, MAXC)
        run = np.zeros(N, np.int64)
        rej = np.zeros(N, np.int64)
        t = 0
        seen = set()
        kept = 0
        for phase in _phases(e, xo, Po):
            m.set_state(xo, Po)
            t0 = t
            for _ in range(T):
                x, P = e.get_state()
                nis64 = gate_ref.nis_f64(orc, x, P, yaw[t], gz[t], rpm[t], prm=prm)
                if t % 3 == 0:
                    e.tick(kf6_rec=rec[t])
                elif t % 3 == 1:
                    e.tick(yaw_deg=yaw[t], gyro_z_dps=gz[t], rpm=rpm[t])
                else:
                    e.correct(kf6_rec=rec[t])
                    e.predict()
                g = e.get_gate()
                st = g["status"]
                what = f"gated {phase} t={t}"
                forced = run >= MAXC
                assert np.array_equal(st == FRC, forced), f"{what}: forced"
                band = ~forced & (np.abs(nis64 - NIS_MAX) <= BAND * NIS_MAX)
                cmp = ~forced & ~band
                assert np.array_equal(st[cmp] == REJ, nis64[cmp] > NIS_MAX), f"{what}: decision"
                assert np.all(np.isin(st, (ACC, REJ, FRC)))
                applied = st != REJ
                kept += int(np.count_nonzero(applied & (run == 0) & (t > t0)))
                run = np.where(applied, 0, np.minimum(run + 1, 255))
                rej = rej + ~applied
                assert np.array_equal(g["run"], run), f"{what}: run"
                assert np.array_equal(g["rejects"], rej), f"{what}: rejects"
                mid = (nis64 > NIS_MAX / 4) & (nis64 < 4 * NIS_MAX)
                assert np.all(np.abs(g["nis"][mid] - nis64[mid]) <= BAND * nis64[mid]), f"{what}: nis"
                seen.update(np.unique(st).tolist())
                orc.kf6_tick(xo, Po, yaw[t], gz[t], np.ascontiguousarray(rpm[t]), applied.astype(np.uint8), op)
                _same(e, xo, Po, what)
                t += 1
            for cnt in (5, 5, 2):
                m.tick_many(cnt, kf6_rec=rec[t0:t0 + cnt])
                t0 += cnt
            _same(m, xo, Po, f"gated tick_many {phase}")
            ge, gm = e.get_gate(), m.get_gate()
            for k in ("status", "run", "nis"):
                assert np.array_equal(_bits(ge[k]) if ge[k].dtype == np.float32 else ge[k],
                                      _bits(gm[k]) if gm[k].dtype == np.float32 else gm[k]), f"tick_many {phase}: {k}"
        assert {ACC, REJ, FRC} <= seen and kept > 0


def _graph(orc, prm):
    """two record ticks captured once, the graph launched three times"""
    import torch
    import fmskf
    import param_cases
    yaw, gz, rpm, rec = _inputs(33)
    op = param_cases.orc_params(orc, prm)
    xo, Po = param_cases.fresh(prm, N)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st), fmskf.Engine("kf6", N, **param_cases.engine_kw(prm)) as e:
        e.set_stream(st)
        dy, dg, dr = (torch.from_numpy(a[:2]).cuda() for a in (yaw, gz, rpm))
        d0, d1 = fmskf.kf6_records(dy, dg, dr)  # the two ticks' 16-byte records on the device
        st.synchronize()
        e.graph_begin()
        e.tick(kf6_rec=d0)
        e.tick(kf6_rec=d1)
        e.graph_end()
        for k in range(3):
            e.graph_launch(1)
            for t in (0, 1):
                orc.kf6_tick(xo, Po, yaw[t], gz[t], np.ascontiguousarray(rpm[t]), None, op)
        st.synchronize()
        _same(e, xo, Po, "graph")


def run_all():
    import param_cases
    from oracle import oracle as orc
    orc.build()
    for prm in (param_cases.default_params("kf6"), _coupled()):
        coupled = prm.q[3] != 0
        for form in ("records", "planes", "correct_predict", "tick_many", "isr"):
            Po = _plain(orc, prm, form)
            if Po is not None and coupled:  # the premise of this half: every masked plane is live
                assert all(np.all(Po[k] != 0) for k in CROSS)
        _plain(orc, prm, "records", comp=True)
        _plain(orc, prm, "tick_many", comp=True)
        _gated(orc, prm)
        _graph(orc, prm)


@pytest.mark.parametrize("variant", ["12", "15"])
def test_conditional_write_back_bitexact(variant):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = os.pathsep.join([root, os.path.join(root, "roboken-fmskf-robot-controller_amd"),
                            os.path.join(root, "tests")] + [p for p in [os.environ.get("PYTHONPATH")] if p])
    env = dict(os.environ, FMSKF_KF6_VARIANT=variant, PYTHONPATH=path)
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True,
                         timeout=240, env=env)
    assert out.returncode == 0, (out.stdout[-1500:] + out.stderr[-3000:])
    assert "skip store ok" in out.stdout


if __name__ == "__main__":
    run_all()
    print("skip store ok")
