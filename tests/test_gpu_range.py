"""Range updates against surveyed anchors (fmskf_correct_range; csrc/kernels_range.hip) on the GPU:
one call of KF6, KF6 + FMSKF_CFG_COMP_POS and EKF9 against the float64 run loop on the same fp32
pre-state (tests/range_ref.py) within a bound formed in the test from the float32 restatement's own
deviation, the robots a call must not touch bit for bit, runs against the sequence of single-entry
calls, the closed loop against the float64 reference, every calling form against every other bit
for bit, malformed lists, the error cases, and that nothing else of a handle moves."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import fmskf
from fmskf import Engine
from fmskf.synth import Trajectory

import fix_ref
import range_ref
from range_ref import ACC, ANCHORS, D2_MAX, D_MIN, IGN, NEAR, REJ, TAG, VAR

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 4113      # not a multiple of 256, three 2048-wide tiles
WARM = 50     # ticks before the calls
MODELS = {"kf6": ("kf6", 0), "kf6comp": ("kf6", fmskf.CFG_COMP_POS), "ekf9": ("ekf9", 0)}
KEYS = list(MODELS)
KW = dict(tag=TAG, var_default=VAR, d_min=D_MIN)
EINVAL, ENOTSUP = fmskf._lib.EINVAL, fmskf._lib.ENOTSUP


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _snapshot(e):
    x, P = e.get_state()
    return x, P, e.get_state_lo()


def _same(a, b, what, cols=None):
    for name, u, v in zip(("x", "P", "lo"), a, b):
        if u is None and v is None:
            continue
        if cols is not None:
            u, v = u[:, cols], v[:, cols]
        assert np.array_equal(_bits(u), _bits(v)), f"{what}: {name}"


def _engine(key, n=N, **kw):
    model, flags = MODELS[key]
    return Engine(model, n, flags=flags, **kw)


_TRAJ = {}


def _warm(key, n=N, T=WARM, seed=78):
    """(trajectory, tick keywords) of the warm-up run, shared"""
    model = MODELS[key][0]
    k = (model, n, T, seed)
    if k not in _TRAJ:
        tr = Trajectory(n, T + 1, seed=seed)
        if model == "kf6":
            yaw, gz, rpm = tr.kf6_inputs()
            tk = [dict(yaw_deg=yaw[t], gyro_z_dps=gz[t], rpm=rpm[t]) for t in range(T + 1)]
        else:
            raw = tr.ekf9_raw()
            tk = [dict(raw=raw[t]) for t in range(T + 1)]
        _TRAJ[k] = (tr, tk)
    return _TRAJ[k]


def _warmed(key, n=N, T=WARM, anchors=ANCHORS, **kw):
    """an engine after T warm-up ticks with the anchor table set"""
    tr, tk = _warm(key, n, T)
    e = _engine(key, n, **kw)
    for t in range(T):
        e.tick(**tk[t])
    if anchors is not None:
        e.set_anchors(anchors)
    return e, tr


def _list129(n=N):
    """129 robots ascending, the tile edges among them"""
    rng = np.random.default_rng(129)
    must = np.array([0, 2047, 2048, n - 1])
    rest = rng.choice(np.setdiff1d(np.arange(n), must), 125, replace=False)
    return np.sort(np.concatenate([must, rest])).astype(np.uint32)


def _truth_range(tr, r, anchor, anchors=ANCHORS, t=WARM):
    th = tr.th[t, r]
    dx = tr.px[t - 1, r] + np.cos(th) * TAG[0] - np.sin(th) * TAG[1] - anchors[anchor, 0]
    dy = tr.py[t - 1, r] + np.sin(th) * TAG[0] + np.cos(th) * TAG[1] - anchors[anchor, 1]
    return np.sqrt(dx * dx + dy * dy + (TAG[2] - anchors[anchor, 2]) ** 2)


def _ranges129(tr, sigma=0.05, seed=3):
    """the 129 robots of _list129 with runs of 1, 2, 3, 4, 1, ... entries, the entries of a run to
    different anchors: (robot, anchor, range_m) -- the truth with Gaussian noise sigma"""
    robots = _list129()
    runs = np.arange(robots.size) % 4 + 1
    robot = np.repeat(robots, runs)
    pos = range_ref.run_positions(robot)
    anchor = ((robot + pos) % 4).astype(np.uint32)
    rng = np.random.default_rng(seed)
    rho = _truth_range(tr, robot.astype(np.int64), anchor) + rng.normal(0.0, sigma, robot.size)
    return robot, anchor, rho.astype(np.float32)


def _f64_state(snap, model):
    """x [N, n], P [N, n, n] float64 of a snapshot, compensated entries as hi + lo"""
    x, P, lo = snap
    x64, P64 = x.astype(np.float64), P.astype(np.float64)
    if lo is not None:
        lo = lo.astype(np.float64)
        if model == "ekf9":
            x64[2] += lo[0]
        else:  # px, py, P00, P10, P11
            x64[0] += lo[0]
            x64[1] += lo[1]
            P64[0] += lo[2]
            P64[1] += lo[3]
            P64[2] += lo[4]
    return fix_ref.unpack_state(x64, P64)


def _trig_of(e):
    """the handle's own sin / cos of fp32 headings, for the references"""
    def trig(th):
        s, c = e.eval_trig(np.asarray(th, np.float32))
        return s, c
    return trig


# ---------------------------------------------------------------------------- 1
def single_call(key):
    """One call of the 129 robots' runs after WARM ticks, no gate: the largest deviations of the
    GPU and of the float32 restatement from the float64 run loop on the same fp32 pre-state"""
    model = MODELS[key][0]
    e, tr = _warmed(key)
    with e:
        robot, anchor, rho = _ranges129(tr, sigma=0.3)
        pre = _snapshot(e)
        d2, status = e.correct_range(robot, anchor, rho, out=True, **KW)
        post = _snapshot(e)
        assert e.get_counters()[0] == 0 and e.get_counters()[5] == 0
        assert np.all(status == ACC)
        r = np.unique(robot).astype(np.int64)
        x0, P0 = _f64_state(pre, model)
        A = ANCHORS.astype(np.float64)
        ref = range_ref.apply_list(range_ref.range_update_f64, x0, P0, robot, anchor, rho, None, A, _trig_of(e))
        f32 = range_ref.apply_list(range_ref.range_update_f32, x0.astype(np.float32), P0.astype(np.float32), robot,
                                   anchor, rho, None, ANCHORS, _trig_of(e))
    assert np.all(ref[3] == ACC) and np.all(f32[3] == ACC)
    xg, Pg = _f64_state(post, model)
    _same(pre, post, f"{key}: robots not listed", np.setdiff1d(np.arange(N), r))
    assert not np.array_equal(_bits(pre[1][:, r]), _bits(post[1][:, r]))
    want = (ref[0][r], ref[1][r], ref[2])
    gpu = range_ref.deviations((xg[r], Pg[r], d2.astype(np.float64)), want)
    rst = range_ref.deviations((f32[0][r].astype(np.float64), f32[1][r].astype(np.float64), f32[2].astype(np.float64)),
                               want)
    return gpu, rst


@pytest.mark.parametrize("key", KEYS)
def test_single_call_against_float64(key):
    """x, P and d2 of the 129 listed robots (0, 2047, 2048 and N - 1 among them; runs of 1 to 4
    entries) after one ungated call against the float64 run loop on the same fp32 pre-state, fed
    Engine.eval_trig of the headings: within 8 times the deviation of the float32 restatement from
    that same reference, per quantity (range_ref's docstring has the reasoning; the GPU's own
    deviations on an MI355X are recorded in profiles/range_fix.json).  Every status is ACCEPTED
    and every robot that is not listed is bit-identical."""
    gpu, rst = single_call(key)
    print("RANGE_DEV " + json.dumps({"key": key, "gpu": gpu, "float32_restatement": rst}))
    for k in ("x", "P", "d2"):
        assert rst[k] > 0 and gpu[k] <= range_ref.MARGIN * rst[k], (k, gpu[k], rst[k])


# ---------------------------------------------------------------------------- 2
@pytest.mark.parametrize("key", KEYS)
def test_untouched_robots(key):
    """bit-identical in x, P and low parts: the robots that are not listed, those whose ranges are
    all rejected (+5 m at d2_max = 10.83 after a first accepted pass) and NEAR robots (an anchor
    placed at their antenna); and a run whose middle entry is rejected equals the call without
    that entry"""
    e, tr = _warmed(key)
    f, _ = _warmed(key)
    with e, f:
        robot, anchor, rho = _ranges129(tr)
        r = np.unique(robot).astype(np.int64)
        others = np.setdiff1d(np.arange(N), r)
        s0 = _snapshot(e)
        for h in (e, f):
            _, st = h.correct_range(robot, anchor, rho, out=True, **KW)
            assert np.all(st == ACC)
        s1 = _snapshot(e)
        _same(s0, s1, "not listed", others)
        d2, st = e.correct_range(robot, anchor, rho + np.float32(5.0), d2_max=D2_MAX, out=True, **KW)
        assert np.all(st == REJ) and np.all(d2 > D2_MAX)
        _same(s1, _snapshot(e), "every range rejected")
        # NEAR: five robots get an anchor of their own at their antenna (d = 0 up to rounding)
        near = r[[0, 1, 40, 127, 128]]
        sn, cs = e.eval_trig(s1[0][2, near])
        own = np.stack([s1[0][0, near] + cs * np.float32(TAG[0]) - sn * np.float32(TAG[1]),
                        s1[0][1, near] + sn * np.float32(TAG[0]) + cs * np.float32(TAG[1]),
                        np.full(near.size, TAG[2], np.float32)], axis=1)
        e.set_anchors(np.concatenate([ANCHORS, own]))
        a2 = anchor.copy()
        for k, rb in enumerate(near):
            a2[robot == rb] = 4 + k
        d2, st = e.correct_range(robot, a2, rho, d2_max=D2_MAX, out=True, **KW)
        is_near = np.isin(robot, near)
        assert np.all(st[is_near] == NEAR) and np.all(d2[is_near] == 0) and np.all(st[~is_near] == ACC)
        s2 = _snapshot(e)
        _same(s1, s2, "NEAR robots and robots not listed", np.concatenate([others, near]))
        assert not np.array_equal(_bits(s1[1][:, r]), _bits(s2[1][:, r]))
        assert e.get_counters()[5] == 0 and e.get_counters()[0] == 0
        # f: the runs of 3 and 4 with their second entry 5 m long against the list without it
        pos = range_ref.run_positions(robot)
        runlen = np.repeat(np.arange(129) % 4 + 1, np.arange(129) % 4 + 1)
        mid = (pos == 1) & (runlen >= 3)
        g, _ = _warmed(key)
        with g:
            g.correct_range(robot, anchor, rho, **KW)
            _same(_snapshot(f), _snapshot(g), "two engines after the same calls")
            bad = np.where(mid, rho + np.float32(5.0), rho).astype(np.float32)
            d2f, stf = f.correct_range(robot, anchor, bad, d2_max=1e3, out=True, **KW)
            d2g, stg = g.correct_range(robot[~mid], anchor[~mid], rho[~mid], d2_max=1e3, out=True, **KW)
            assert np.all(stf[mid] == REJ) and np.all(stf[~mid] == ACC) and np.all(stg == ACC)
            assert np.array_equal(_bits(d2f[~mid]), _bits(d2g))
            _same(_snapshot(f), _snapshot(g), "a run with its middle entry rejected")


# ---------------------------------------------------------------------------- 3
@pytest.mark.parametrize("key", KEYS)
def test_runs_against_single_entry_calls(key):
    """a call with runs equals, bit for bit (state, d2, status), the sequence of four calls that
    carry every robot's j-th entry, j = 0, 1, 2, 3; a fifth of the ranges are 5 m long, so both
    decisions occur"""
    e, tr = _warmed(key)
    f, _ = _warmed(key)
    with e, f:
        robot, anchor, rho = _ranges129(tr)
        for h in (e, f):
            h.correct_range(robot, anchor, rho, **KW)   # covariance down
        robot, anchor, rho = _ranges129(tr, seed=4)
        rho = np.where(np.arange(rho.size) % 5 == 2, rho + np.float32(5.0), rho).astype(np.float32)
        d2, st = e.correct_range(robot, anchor, rho, d2_max=D2_MAX, out=True, **KW)
        pos = range_ref.run_positions(robot)
        d2s, sts = np.zeros_like(d2), np.zeros_like(st)
        for j in range(4):
            s = pos == j
            d2s[s], sts[s] = f.correct_range(robot[s], anchor[s], rho[s], d2_max=D2_MAX, out=True, **KW)
        assert np.any(st == REJ) and np.any(st == ACC)
        assert np.array_equal(st, sts) and np.array_equal(_bits(d2), _bits(d2s))
        _same(_snapshot(e), _snapshot(f), "runs against single-entry calls")


# ---------------------------------------------------------------------------- 4
@pytest.mark.parametrize("key", KEYS)
def test_closed_loop_against_float64(orc, key):
    """the closed loop of the CPU recipe (1024 robots x 400 ticks, the state started N(0, 0.5 m)
    off the truth through set_state): every decision outside the band equals the float64
    reference's, the final position error is at most twice the reference's own maximum, and P00
    is below that of the same run without the calls for every robot"""
    ref = range_ref.closed_loop(orc, MODELS[key][0])
    tr, n, T = ref["traj"], range_ref.N_LOOP, range_ref.T_LOOP
    differ = compared = 0
    with _engine(key, n) as e, _engine(key, n) as plain:
        for h in (e, plain):
            x, P = h.get_state()
            x[0], x[1] = ref["x0"][0], ref["x0"][1]
            h.set_state(x, P)
        e.set_anchors(ANCHORS)
        for t in range(T):
            robot, anchor, rho, _ = ref["fixes"][t]
            if robot.size:
                d2, st = e.correct_range(robot, anchor, rho, d2_max=D2_MAX, out=True, **KW)
                assert not np.any((st == IGN) | (st == NEAR))
                cmp_ = ~range_ref.in_band(ref["d2"][t])
                differ += int(np.count_nonzero(st[cmp_] != ref["status"][t][cmp_]))
                compared += int(np.count_nonzero(cmp_))
            e.tick(**ref["kw"][t])
            plain.tick(**ref["kw"][t])
        x, P = e.get_state()
        _, Pp = plain.get_state()
        assert e.get_counters()[0] == 0 and e.get_counters()[5] == 0
    err = np.hypot(x[0] - tr.px[T - 1], x[1] - tr.py[T - 1])
    print(f"{key}: decisions compared {compared}, different {differ}; final position error max {err.max():.3e} m "
          f"(float64 reference {ref['err'].max():.3e} m); P00 max {P[0].max():.3e} with, min {Pp[0].min():.3e} without")
    assert compared >= 30000 and differ == 0
    assert err.max() <= 2 * ref["err"].max()
    assert np.all(Pp[0] > P[0])


# ---------------------------------------------------------------------------- 5
FORMS = ("host", "device", "device_null", "host_null", "split", "graph")


def form_result(key, form):
    """The state, d2 and status after the same two calls -- a first accepted pass, then a list
    with a third of the ranges 5 m long at d2_max = 10.83 -- the second in calling form `form`"""
    e, tr = _warmed(key)
    with e:
        robot, anchor, rho = _ranges129(tr)
        e.correct_range(robot, anchor, rho, **KW)
        robot, anchor, rho = _ranges129(tr, seed=5)
        rho = np.where(np.arange(rho.size) % 3 == 0, rho + np.float32(5.0), rho).astype(np.float32)
        kw = dict(d2_max=D2_MAX, **KW)
        out = None
        if form == "host":
            out = e.correct_range(robot, anchor, rho, out=True, **kw)
        elif form == "host_null":
            assert e.correct_range(robot, anchor, rho, **kw) is None
        else:
            import torch
            e.set_stream(torch.cuda.current_stream())   # the stream torch's own work is on
            rec = torch.from_numpy(fmskf.range_fix_records(robot, anchor, rho).view(np.int32).reshape(-1, 4)).cuda()
            if form == "device":
                out = e.correct_range(fixes=rec, out=True, **kw)
            elif form == "device_null":
                assert e.correct_range(fixes=rec, **kw) is None
            elif form == "split":
                k = int(np.flatnonzero(range_ref.run_positions(robot) == 0)[60])   # a run boundary
                a = e.correct_range(fixes=rec[:k].contiguous(), out=True, **kw)
                b = e.correct_range(fixes=rec[k:].contiguous(), out=True, **kw)
                out = (torch.cat([a[0], b[0]]), torch.cat([a[1], b[1]]))
            elif form == "graph":
                d2 = torch.zeros(rec.shape[0], dtype=torch.float32, device="cuda")
                st = torch.zeros(rec.shape[0], dtype=torch.uint8, device="cuda")
                e.graph_begin()
                e.correct_range(fixes=rec, out=(d2, st), **kw)
                e.graph_end()
                e.graph_launch(1)
                e.sync()
                out = (d2, st)
            else:
                raise ValueError(form)
            if out is not None:
                out = (out[0].cpu().numpy(), out[1].cpu().numpy())
        assert e.get_counters()[5] == 0
        return _snapshot(e), out


def _check_forms(results):
    base, out0 = results["host"]
    assert np.any(out0[1] == REJ) and np.any(out0[1] == ACC)
    for form, (snap, out) in results.items():
        _same(base, snap, form)
        if out is not None:
            assert np.array_equal(_bits(out[0]), _bits(out0[0])), f"{form}: d2"
            assert np.array_equal(out[1], out0[1]), f"{form}: status"


@pytest.mark.parametrize("key", KEYS)
def test_forms_agree_bit_for_bit(key):
    """host list, device list, outputs requested or NULL, two calls split at a run boundary, and
    a captured-and-replayed call: the same state, d2 and status bits"""
    import torch
    st_ = torch.cuda.Stream()
    with torch.cuda.stream(st_):
        _check_forms({form: form_result(key, form) for form in FORMS})


def child_main(path):
    """the host form of every key in this process, saved to `path` (the env-variable forms)"""
    out = {}
    for key in KEYS:
        snap, (d2, st) = form_result(key, "host")
        for name, a in zip(("x", "P", "lo"), snap):
            if a is not None:
                out[f"{key}_{name}"] = a
        out[f"{key}_d2"], out[f"{key}_st"] = d2, st
    np.savez(path, **out)
    print("range forms ok")


@pytest.mark.parametrize("var", ["FMSKF_STATE_NT", "FMSKF_LIST_BIG"])
def test_forms_in_a_fresh_process(tmp_path, var):
    """the same calls with FMSKF_STATE_NT=1 (the streamed-state cache policy) and with
    FMSKF_LIST_BIG=1 (64-bit lane addresses, the form an array past 4 GiB takes), each in a fresh
    process (the variables are read once, at the first launch): bit for bit the host form's state,
    d2 and status, for every key"""
    path = str(tmp_path / "forms.npz")
    code = ("import sys; sys.path[:0] = %r\nimport test_gpu_range as t\nt.child_main(%r)\n"
            % ([os.path.join(ROOT, "tests"), ROOT, os.path.join(ROOT, "roboken-fmskf-robot-controller_amd")], path))
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, **{var: "1"}))
    assert out.returncode == 0 and "range forms ok" in out.stdout, out.stdout + out.stderr
    got = np.load(path)
    for key in KEYS:
        snap, (d2, st) = form_result(key, "host")
        for name, a in zip(("x", "P", "lo"), snap):
            if a is not None:
                assert np.array_equal(_bits(a), _bits(got[f"{key}_{name}"])), f"{var} {key}: {name}"
        assert np.array_equal(_bits(d2), _bits(got[f"{key}_d2"])) and np.array_equal(st, got[f"{key}_st"])


# ---------------------------------------------------------------------------- 6
def _malformed(tr):
    """a device list with every kind of ignored entry: (robot, anchor, want status)"""
    runs = [(3, [0, 1], [ACC, ACC]),
            (70, [k % 4 for k in range(fmskf.RANGE_RUN_MAX + 3)], [ACC] * fmskf.RANGE_RUN_MAX + [IGN] * 3),
            (2048, [0, 4, 2], [ACC, IGN, ACC]),          # anchor 4 of a table of 4: that entry alone
            (100, [0, 1], [IGN, IGN]),                   # a run head below its predecessor: the whole run
            (2049, [1], [ACC]),
            (N + 5, [0, 1], [IGN, IGN]),                 # robot >= N
            (0xFFFFFFFF, [0], [IGN])]
    robot = np.concatenate([np.full(len(a), r, np.uint32) for r, a, _ in runs])
    anchor = np.concatenate([np.array(a, np.uint32) for _, a, _ in runs])
    want = np.concatenate([np.array(w, np.uint8) for _, _, w in runs])
    idx = np.minimum(robot.astype(np.int64), N - 1)
    rng = np.random.default_rng(6)
    rho = (_truth_range(tr, idx, np.minimum(anchor, 3)) + rng.normal(0, 0.05, idx.size)).astype(np.float32)
    return robot, anchor, rho, want


@pytest.mark.parametrize("key", KEYS)
def test_malformed_device_lists(key):
    """robot >= N, a descending run head (the whole run), a bad anchor (that entry alone) and a
    run of FMSKF_RANGE_RUN_MAX + 3: each is reported IGNORED with d2 0, counted in counter [5],
    leaves its robot untouched (unless listed well formed elsewhere) and leaves the rest of the
    list applied as if listed alone; the same lists from host memory are FMSKF_EINVAL with
    nothing changed"""
    import torch
    a, tr = _warmed(key)
    b, _ = _warmed(key)
    with a, b:
        robot, anchor, rho, want = _malformed(tr)
        good = want == ACC
        s0 = _snapshot(a)
        with pytest.raises(fmskf.FmskfError) as ei:
            a.correct_range(robot, anchor, rho, **KW)
        assert ei.value.code == EINVAL
        # each kind alone: the run of RUN_MAX + 3, the bad anchor, the descending head, robot >= N
        for sl in (slice(2, 13), slice(13, 16), slice(15, 18), slice(19, 21), slice(21, 22)):
            with pytest.raises(fmskf.FmskfError) as ei:
                a.correct_range(robot[sl], anchor[sl], rho[sl], **KW)
            assert ei.value.code == EINVAL, sl
        _same(s0, _snapshot(a), "host lists refused")
        assert a.get_counters()[5] == 0
        rec = torch.from_numpy(fmskf.range_fix_records(robot, anchor, rho).view(np.int32).reshape(-1, 4)).cuda()
        d2, st = a.correct_range(fixes=rec, out=True, **KW)
        d2, st = d2.cpu().numpy(), st.cpu().numpy()
        assert np.array_equal(st, want)
        assert np.all(d2[~good] == 0) and np.all(d2[good] > 0)
        nbad = int(np.count_nonzero(~good))
        assert a.get_counters()[5] == nbad == 9
        d2b, stb = b.correct_range(robot[good], anchor[good], rho[good], out=True, **KW)
        assert np.array_equal(_bits(d2[good]), _bits(d2b)) and np.all(stb == ACC)
        sa = _snapshot(a)
        _same(sa, _snapshot(b), "the well-formed entries alone")
        _same(s0, sa, "robots of ignored entries", np.setdiff1d(np.arange(N), robot[good].astype(np.int64)))
        a.correct_range(fixes=rec, **KW)
        assert a.get_counters()[5] == 2 * nbad and a.get_counters()[3] == 0 and a.get_counters()[4] == 0
        a.reset()
        assert a.get_counters()[5] == 0


# ---------------------------------------------------------------------------- 7
def test_error_cases():
    """every FMSKF_EINVAL case of fmskf_set_anchors and fmskf_correct_range, with nothing changed"""
    import torch
    e, tr = _warmed("kf6", anchors=None)
    st_ = torch.cuda.Stream()
    with e, torch.cuda.stream(st_):
        e.set_stream(st_)   # a capture needs a stream
        robot, anchor, rho = _ranges129(tr)
        s0 = _snapshot(e)
        with pytest.raises(fmskf.FmskfError) as ei:   # no anchors set
            e.correct_range(robot, anchor, rho, **KW)
        assert ei.value.code == EINVAL
        L = fmskf.load()
        big = np.zeros((fmskf.RANGE_ANCHORS_MAX + 1, 3), np.float32)
        assert L.fmskf_set_anchors(e.h, big.ctypes.data, fmskf.RANGE_ANCHORS_MAX + 1) == EINVAL
        assert L.fmskf_set_anchors(e.h, None, 2) == EINVAL
        for bad in (np.nan, np.inf):
            a = ANCHORS.copy()
            a[2, 1] = bad
            with pytest.raises(fmskf.FmskfError) as ei:
                e.set_anchors(a)
            assert ei.value.code == EINVAL
        assert e.get_anchors().shape == (0, 3)
        e.set_anchors(big[:fmskf.RANGE_ANCHORS_MAX] + ANCHORS[0])   # the full table is fine
        assert e.get_anchors().shape == (fmskf.RANGE_ANCHORS_MAX, 3)
        e.set_anchors(ANCHORS)
        inf = float("inf")
        for bad in (dict(var_default=0.0), dict(var_default=-1.0), dict(var_default=np.nan), dict(var_default=inf),
                    dict(d2_max=0.0), dict(d2_max=-1.0), dict(d2_max=np.nan), dict(d_min=0.0), dict(d_min=-0.5),
                    dict(d_min=np.nan), dict(d_min=inf), dict(tag=(np.nan, 0, 0)), dict(tag=(0, inf, 0)),
                    dict(tag=(0, 0, -inf))):
            with pytest.raises(fmskf.FmskfError) as ei:
                e.correct_range(robot, anchor, rho, **{**KW, **bad})
            assert ei.value.code == EINVAL, bad
        rec = fmskf.range_fix_records(robot, anchor, rho)
        p = rec.ctypes.data
        prm = fmskf._lib.RangeParams()
        prm.tag[0], prm.tag[1], prm.tag[2] = TAG
        prm.var_m2, prm.d2_max, prm.d_min = VAR, inf, D_MIN
        H, D = fmskf.MEM_HOST, fmskf.MEM_DEVICE
        assert L.fmskf_correct_range(e.h, p, rec.size, None, None, None, H) == EINVAL
        assert L.fmskf_correct_range(e.h, None, rec.size, prm, None, None, H) == EINVAL
        assert L.fmskf_correct_range(e.h, p, rec.size, prm, None, None, 7) == EINVAL
        assert L.fmskf_correct_range(e.h, p, fmskf.RANGE_RUN_MAX * N + 1, prm, None, None, D) == EINVAL
        prm.flags = 1
        assert L.fmskf_correct_range(e.h, p, rec.size, prm, None, None, H) == EINVAL
        prm.flags, prm.reserved = 0, 1
        assert L.fmskf_correct_range(e.h, p, rec.size, prm, None, None, H) == EINVAL
        prm.reserved = 0
        dev = torch.from_numpy(rec.view(np.int32).reshape(-1, 4)).cuda()
        assert L.fmskf_correct_range(e.h, dev.data_ptr() + 4, 8, prm, None, None, D) == EINVAL   # misaligned
        for mem in (H, D):   # count == 0: FMSKF_OK with no launch
            assert L.fmskf_correct_range(e.h, None, 0, prm, None, None, mem) == 0
        e.graph_begin()
        assert L.fmskf_correct_range(e.h, p, rec.size, prm, None, None, H) == EINVAL   # a host list in a capture
        assert L.fmskf_set_anchors(e.h, ANCHORS.ctypes.data, 4) == EINVAL
        e.correct_range(fixes=dev, **KW)   # a device list is captured (and not replayed here)
        e.graph_end()
        _same(s0, _snapshot(e), "refused calls")
        assert np.array_equal(e.get_anchors(), ANCHORS)
        assert L.fmskf_correct_range(e.h, p, rec.size, prm, None, None, H) == 0
        assert not np.array_equal(_bits(s0[1]), _bits(_snapshot(e)[1]))


@pytest.mark.parametrize("model,flags", [("rs", 0), ("kf12d", 0), ("ekf9", fmskf.CFG_COMP_POS)])
def test_unsupported_models(model, flags):
    with Engine(model, 300, flags=flags) as e:
        e.set_anchors(ANCHORS)
        for cnt in (1, 0):   # whatever the count
            with pytest.raises(fmskf.FmskfError) as ei:
                e.correct_range(np.zeros(cnt, np.uint32), np.zeros(cnt, np.uint32), np.ones(cnt, np.float32), **KW)
            assert ei.value.code == ENOTSUP


@pytest.mark.parametrize("key", KEYS)
def test_nan_inputs(key):
    """a NaN range is REJECTED with a NaN d2 and the robot untouched, also in the middle of a run;
    a NaN in P00 gives a NaN d2: REJECTED, untouched and not counted in counter [0]; a NaN px gives
    a NaN predicted distance, which is below every d_min: NEAR with d2 0, untouched, not counted"""
    e, tr = _warmed(key)
    with e:
        x, P = e.get_state()
        P[0, 7] = np.nan
        x[0, 9] = np.nan
        e.set_state(x, P)
        robot = np.array([3, 5, 5, 5, 7, 7, 9, 11], np.uint32)
        anchor = np.array([0, 0, 1, 2, 0, 1, 2, 3], np.uint32)
        rho = _truth_range(tr, robot.astype(np.int64), anchor).astype(np.float32)
        rho[0] = rho[2] = np.nan
        s0 = _snapshot(e)
        d2, st = e.correct_range(robot, anchor, rho, out=True, **KW)
        assert st.tolist() == [REJ, ACC, REJ, ACC, REJ, REJ, NEAR, ACC]
        assert np.all(np.isnan(d2[[0, 2, 4, 5]])) and d2[6] == 0 and np.all(d2[[1, 3, 7]] >= 0)
        s1 = _snapshot(e)
        _same(s0, s1, "NaN range, NaN P00, NaN px", np.setdiff1d(np.arange(N), [5, 11]))
        assert np.all(np.isfinite(s1[0][:, [5, 11]])) and np.all(np.isfinite(s1[1][:, [5, 11]]))
        assert e.get_counters()[0] == 0 and e.get_counters()[5] == 0
        # the run of robot 5 with its NaN entry equals the run without it
        f, _ = _warmed(key)
        with f:
            f.set_state(x, P)
            keep = np.array([1, 3, 7])
            d2f, _ = f.correct_range(robot[keep], anchor[keep], rho[keep], out=True, **KW)
            assert np.array_equal(_bits(d2[keep]), _bits(d2f))
            _same(s1, _snapshot(f), "a NaN range in the middle of a run", [5, 11])


# ---------------------------------------------------------------------------- 8
def test_anchor_table(tmp_path):
    """the anchors round-trip, are replaced and are cleared; fmskf_reset keeps them; a later
    table is what a later call reads"""
    e, tr = _warmed("kf6", anchors=None)
    with e:
        assert e.get_anchors().shape == (0, 3)
        e.set_anchors(ANCHORS)
        assert np.array_equal(_bits(e.get_anchors()), _bits(ANCHORS))
        cnt = fmskf._lib.C.c_uint32()
        two = np.zeros((2, 3), np.float32)
        assert fmskf.load().fmskf_get_anchors(e.h, two.ctypes.data, 2, fmskf._lib.C.byref(cnt)) == 0
        assert cnt.value == 4 and np.array_equal(two, ANCHORS[:2])
        assert fmskf.load().fmskf_get_anchors(e.h, None, 0, fmskf._lib.C.byref(cnt)) == 0 and cnt.value == 4
        robot, anchor, rho = _ranges129(tr)
        d2a, _ = e.correct_range(robot, anchor, rho, d2_max=1e-30, out=True, **KW)   # evaluates, applies nothing
        moved = ANCHORS[::-1].copy()
        e.set_anchors(moved)   # replaced: the same indices now name other anchors
        assert np.array_equal(e.get_anchors(), moved)
        d2b, _ = e.correct_range(robot, (3 - anchor).astype(np.uint32), rho, d2_max=1e-30, out=True, **KW)
        assert np.array_equal(_bits(d2a), _bits(d2b))
        d2c, _ = e.correct_range(robot, anchor, rho, d2_max=1e-30, out=True, **KW)
        assert not np.array_equal(_bits(d2a), _bits(d2c))
        e.reset()
        assert np.array_equal(e.get_anchors(), moved)
        e.correct_range(robot, anchor, rho, **KW)   # and the device table is still there
        e.set_anchors(np.zeros((0, 3), np.float32))
        assert e.get_anchors().shape == (0, 3)
        with pytest.raises(fmskf.FmskfError) as ei:
            e.correct_range(robot, anchor, rho, **KW)
        assert ei.value.code == EINVAL


def test_checkpoint_without_anchors(tmp_path):
    """checkpoints neither write nor read the anchors: the file of a handle with anchors is byte
    for byte that of one without, and loading it leaves the table alone"""
    tr, tk = _warm("kf6")
    files = []
    for anchors in (None, ANCHORS):
        e, _ = _warmed("kf6", anchors=anchors)
        with e:
            p = tmp_path / f"{0 if anchors is None else 1}.ckpt"
            e.save_state(p)
            files.append(p.read_bytes())
            e.load_state(p)
            assert e.get_anchors().shape[0] == (0 if anchors is None else 4)
    assert files[0] == files[1]


def test_gate_state_and_other_counters_untouched():
    """a KF6 handle with a persistent gate (fmskf_set_gate) has the same gate state before and
    after range calls, the call's own d2_max is what decides, and counters [3] and [4] stay"""
    e, tr = _warmed("kf6")
    with e:
        e.set_gate(18.47, 3)
        e.tick(**_warm("kf6")[1][WARM])
        g0 = e.get_gate()
        c0 = e.get_counters()
        robot, anchor, rho = _ranges129(tr)
        e.correct_range(robot, anchor, rho, **KW)
        _, st = e.correct_range(robot, anchor, rho + np.float32(5.0), d2_max=D2_MAX, out=True, **KW)
        assert np.all(st == REJ)
        g1 = e.get_gate()
        for k in g0:
            assert np.array_equal(_bits(g0[k]), _bits(g1[k])), k
        assert list(e.get_counters()) == list(c0)
