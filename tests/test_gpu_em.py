"""fmskf_tick_many_em on the GPU: the forward pass is fmskf_tick_many, the per-robot sums against
the float64 definition within the bound of tests/em_ref.py, short and empty windows, the
deterministic fleet total, the call forms, accumulation over windows, lane isolation, the closed
fit loop with fmskf_tick_many_loglik as its monitor, the error cases.

Shapes (smooth_ref): N = 4113 robots (no multiple of 256, three 2048-wide tiles), windows of
T = 37 ticks (odd: the loop unrolled by two ends on its tail) behind 50 plain ticks or straight
from reset(); T = 1 and 2 on 257 robots; the closed loop on 1024 robots and 64 ticks of
loglik_ref.model_log."""
import ctypes as C
import json

import numpy as np
import pytest

import fmskf
from fmskf import Engine
from fmskf import _lib

import em_ref as er
import loglik_ref as lr
import smooth_ref as sr
from em_ref import host
from loglik_ref import kw_of, same, snapshot, to_device, warmed

pytestmark = pytest.mark.gpu

N, T, WARM = sr.N, sr.T, sr.WARM
EINVAL, ENOMEM, ENOTSUP = _lib.EINVAL, _lib.ENOMEM, _lib.ENOTSUP
ROBOT = ("n_meas", "sq", "sr")
ALL = ROBOT + ("total",)
SENT = -12345.5


def b64(a):
    return np.ascontiguousarray(a).view(np.uint64 if np.asarray(a).dtype.itemsize == 8 else np.uint32)


def same_sums(a, b, keys, what):
    for k in keys:
        assert np.array_equal(b64(a[k]), b64(b[k])), f"{what}: {k} differs"


@pytest.fixture(scope="module")
def w(orc):
    return sr.window(orc)


@pytest.fixture(scope="module")
def clean(w):
    """the masked window behind the warm-up, everything asked for, host memory: computed once"""
    with warmed(w) as e:
        r = e.tick_many_em(T, per_robot=True, total=True, **kw_of(w, "rec", w["valid"]))
    for v in r.values():
        v.setflags(write=False)
    return r


def raw_out(arrays, flags=0, pitch=0):
    """a fmskf_em_out over numpy arrays or torch device tensors"""
    eo = _lib.EmOut()
    dev = any(not isinstance(v, np.ndarray) for v in arrays.values())
    eo.mem, eo.flags, eo.pitch = (_lib.MEM_DEVICE if dev else _lib.MEM_HOST), flags, pitch
    for k, v in arrays.items():
        setattr(eo, k, v.data_ptr() if dev else v.ctypes.data)
    return eo


def raw_call(e, ti, n_ticks, stride, eo):
    return fmskf.load().fmskf_tick_many_em(e.h, C.byref(ti) if ti is not None else None, n_ticks, stride,
                                           C.byref(eo) if eo is not None else None)


def check_against_float64(wd, e, Tn, valid, tag, n):
    """run the window on e, and hold every per-robot sum to the rule of em_ref"""
    lo = wd["warm"]
    x0, P0 = e.get_state()
    got = e.tick_many_em(Tn, per_robot=True, total=True, **kw_of(wd, "rec", valid, lo, lo + Tn))
    z = wd["z"][lo:lo + Tn]
    ref, r32 = er.definition(x0, P0, z, valid), er.restate_f32(x0, P0, z, valid)
    assert not r32["bad"].any()
    assert np.array_equal(got["n_meas"], ref["n_meas"]), "n_meas is not the mask's column sums"
    assert np.array_equal(got["n_meas"], np.asarray(valid[:Tn], np.uint32).sum(axis=0))
    dev32, dev = er.deviations(r32, ref), er.deviations(got, ref)
    bound = er.bounds(dev32, ref)
    tol = lambda d: {k: np.asarray(v).tolist() for k, v in d.items()}
    print("EM_DEV " + json.dumps(dict(case=tag, n=n, T=Tn, gpu=tol(dev), f32=tol(dev32), bound=tol(bound))))
    for k in er.QUANTITIES:
        assert np.isfinite(got[k]).all(), k
        assert (dev[k] <= bound[k]).all(), (k, dev[k], bound[k])
    assert (got["sq"][er.DIAG_Q] >= 0).all() and (got["sr"][er.DIAG_R] >= 0).all(), "a negative diagonal sum"
    assert np.array_equal(b64(got["total"]), b64(er.fleet_fold(got, Tn))), "total is not the fixed tree"
    assert got["total"][0] == (Tn - 1) * n and got["total"][1] == int(got["n_meas"].sum()) and got["total"][2] == 0
    return got


# ----------------------------------------------------------------------------- 1. forward identity
@pytest.mark.parametrize("masked", [False, True], ids=["all", "valid"])
@pytest.mark.parametrize("form", ["rec", "planes"])
def test_forward_is_tick_many(w, form, masked):
    kw = kw_of(w, form, w["valid"] if masked else None)
    with warmed(w) as e, warmed(w) as c:
        r = e.tick_many_em(T, per_robot=masked, total=True, **kw)
        c.tick_many(T, **kw)
        same(snapshot(e), snapshot(c), f"{form} masked={masked}")
    assert np.isfinite(r["total"]).all() and r["total"][0] == (T - 1) * N
    assert r["total"][1] == (int(w["valid"].sum()) if masked else T * N)


# ----------------------------------------------------------------------------- 2. values
@pytest.mark.parametrize("start", ["warm", "reset"])
def test_against_float64(w, start):
    """`warm`: behind 50 plain ticks; `reset`: straight from reset(), the diffuse prior P0 with tick 0
    invalid for one robot in five, the case that broke the adjoint smoother form"""
    valid = w["valid"]
    assert (valid[0] == 0).sum() > N // 6 and (valid[-1] == 0).sum() > N // 8
    with warmed(w, warm=start == "warm") as e:
        check_against_float64(w, e, T, valid, start, N)


# ----------------------------------------------------------------------------- 3. short and empty
@pytest.mark.parametrize("Tn", [1, 2])
def test_short_windows(orc, Tn):
    """T = 1: no transition, sq all +0 and total[0] = 0; T = 2: one; 257 robots from reset(), masked"""
    n = 257
    wd = sr.window(orc, n=n, Tn=2, warm=0, seed=100 + n)
    with Engine("kf6", n) as e:
        got = check_against_float64(wd, e, Tn, wd["valid"][:Tn], f"short-{Tn}", n)
    if Tn == 1:
        assert not b64(got["sq"]).any() and not b64(got["total"][3:24]).any() and got["total"][0] == 0
    else:
        assert got["total"][0] == n and (got["sq"][er.DIAG_Q] > 0).all()


def test_no_measurement_gives_zeros(w):
    """robots without a measured tick: n_meas = 0 and sr = +0, sq as ever"""
    valid = w["valid"].copy()
    quiet = np.arange(N) % 3 == 1
    valid[:, quiet] = 0
    with warmed(w) as e, warmed(w) as c:
        r = e.tick_many_em(T, per_robot=True, total=True, **kw_of(w, "rec", valid))
        c.tick_many(T, **kw_of(w, "rec", valid))
        same(snapshot(e), snapshot(c), "a third of the robots unmeasured")
    assert not r["n_meas"][quiet].any() and not b64(r["sr"][:, quiet]).any()
    assert (r["n_meas"][~quiet] > 0).all() and (r["sr"][er.DIAG_R][:, ~quiet] > 0).all()
    assert np.isfinite(r["sq"]).all() and (r["sq"][er.DIAG_Q] > 0).all()
    assert r["total"][2] == 0 and r["total"][1] == int(valid.sum())


# ----------------------------------------------------------------------------- 4. the total
def test_total_is_the_fixed_tree_and_deterministic(w, clean):
    with warmed(w) as e:
        again = e.tick_many_em(T, per_robot=True, total=True, **kw_of(w, "rec", w["valid"]))
    same_sums(again, clean, ALL, "two calls on the same state and inputs")
    assert np.array_equal(b64(clean["total"]), b64(er.fleet_fold(clean, T)))
    assert clean["total"][0] == (T - 1) * N and clean["total"][1] == int(w["valid"].sum()) and clean["total"][2] == 0


# ----------------------------------------------------------------------------- 5. call forms
@pytest.mark.parametrize("form", ["device-out", "device-in", "padded-host", "padded-device"])
def test_call_forms_agree(w, clean, form):
    import torch
    kw = kw_of(w, "rec", w["valid"])
    pitch = N + 59 if form.startswith("padded") else N
    dev = form in ("device-out", "padded-device")
    arrays = dict(n_meas=np.zeros(N, np.uint32), sq=np.full((21, pitch), SENT), sr=np.full((10, pitch), SENT),
                  total=np.full(34, SENT))
    if dev:
        arrays = {k: torch.from_numpy(v.view(np.int32) if k == "n_meas" else v).cuda() for k, v in arrays.items()}
    with warmed(w) as e:
        if form == "device-in":
            r = e.tick_many_em(T, per_robot=True, total=True, **to_device(kw))
            assert not isinstance(r["sq"], np.ndarray)
        else:
            ti, _keep = e._inputs(kw, T, N)
            assert raw_call(e, ti, T, N, raw_out(arrays, pitch=0 if pitch == N else pitch)) == 0
            r = arrays
        r = host(r)
    for k in ("sq", "sr"):
        assert (r[k][:, N:] == SENT).all(), k + " padding"
        assert not (r[k][:, :N] == SENT).any()
    same_sums({k: (v[:, :N] if v.ndim == 2 else v) for k, v in r.items()}, clean, ALL, form)


@pytest.mark.parametrize("which", ["per-robot", "total"])
def test_output_subsets_agree(w, clean, which):
    with warmed(w) as e:
        r = e.tick_many_em(T, per_robot=which == "per-robot", total=which == "total", **kw_of(w, "rec", w["valid"]))
    assert set(r) == (set(ROBOT) if which == "per-robot" else {"total"})
    same_sums(r, clean, tuple(r), which + " only")


# ----------------------------------------------------------------------------- 6. accumulation
def test_accumulate_over_windows(w):
    """two windows (18 and 19 ticks, each smoothed on its own) into one set of arrays: every element
    is the fp64 sum of the two single calls' results, bit for bit; the 36 transitions of a 37-tick
    log cut in two become 17 + 18"""
    valid = w["valid"]
    cut = 18
    k1, k2 = kw_of(w, "rec", valid[:cut], WARM, WARM + cut), kw_of(w, "rec", valid[cut:], WARM + cut, WARM + T)
    with warmed(w) as e, warmed(w) as s, warmed(w) as c:
        acc = e.tick_many_em(cut, per_robot=True, total=True, **k1)
        first = {k: v.copy() for k, v in acc.items()}
        assert e.tick_many_em(T - cut, accumulate_into=acc, **k2) is acc
        r1 = s.tick_many_em(cut, per_robot=True, total=True, **k1)
        r2 = s.tick_many_em(T - cut, per_robot=True, total=True, **k2)
        c.tick_many(T, **kw_of(w, "rec", valid))
        same(snapshot(e), snapshot(c), "18 + 19 ticks against 37")
        same(snapshot(s), snapshot(c), "18 + 19 ticks, separate results")
        ti, _keep = s._inputs(k2, T - cut, N)
    same_sums(first, r1, ALL, "the first window")
    assert np.array_equal(acc["n_meas"], r1["n_meas"] + r2["n_meas"]) and np.array_equal(acc["n_meas"], valid.sum(axis=0))
    for k in ("sq", "sr", "total"):
        assert np.array_equal(b64(acc[k]), b64(r1[k] + r2[k])), f"{k}: not one fp64 addition of the windows' results"
    assert acc["total"][0] == (T - 2) * N
    # without the flag a call overwrites what the arrays hold
    with warmed(w) as o:
        o.tick_many(cut, **k1)
        over = {k: v.copy() for k, v in r1.items()}
        assert raw_call(o, ti, T - cut, N, raw_out(over)) == 0
    same_sums(over, r2, ALL, "overwritten without FMSKF_EM_ACCUMULATE")


# ----------------------------------------------------------------------------- 7. isolation
def test_lane_isolation(w):
    """a NaN yaw for robot 2049 at tick 20 of the window (data, not a fault): its sums are NaN and
    its n_meas the count, total[2] counts it and the other totals leave it out, every other robot's
    bytes are the clean run's, and the forward pass is still fmskf_tick_many's"""
    bad, tick = 2049, 20
    kw = kw_of(w, "planes", None)
    with warmed(w) as e:
        ok = e.tick_many_em(T, per_robot=True, total=True, **kw)
    dirty_kw = dict(kw, yaw_deg=kw["yaw_deg"].copy())
    dirty_kw["yaw_deg"][tick, bad] = np.nan
    with warmed(w) as p, warmed(w) as c:
        dirty = p.tick_many_em(T, per_robot=True, total=True, **dirty_kw)
        c.tick_many(T, **dirty_kw)
        same(snapshot(p), snapshot(c), "poisoned forward pass")
        assert p.get_counters()[0] == 1
    others = np.setdiff1d(np.arange(N), [bad])
    for k in ROBOT:
        assert np.array_equal(b64(ok[k][..., others]), b64(dirty[k][..., others])), k
    assert np.isnan(dirty["sq"][:, bad]).all() and np.isnan(dirty["sr"][:, bad]).all() and dirty["n_meas"][bad] == T
    assert np.isfinite(ok["sq"]).all() and np.isfinite(ok["sr"]).all() and ok["total"][2] == 0
    assert dirty["total"][2] == 1 and dirty["total"][0] == (T - 1) * (N - 1) and dirty["total"][1] == T * (N - 1)
    holed = {k: v.copy() for k, v in ok.items()}
    holed["sq"][:, bad] = np.nan
    assert np.array_equal(b64(dirty["total"]), b64(er.fleet_fold(holed, T))), "the totals do not leave the robot out"


# ----------------------------------------------------------------------------- 8. the closed loop
N_FIT, T_FIT, SEED_FIT, SIGMA = 1024, 64, 21, 0.025


def test_closed_loop_raises_the_likelihood():
    """lr.model_log (the default Q and R are its true parameters), the filter started on the default
    Q and R00 inflated by 4 SIGMA^2 as test_em_cpu.py starts it: one M-step from the GPU's total,
    a new Engine on the fitted Q and R, and fmskf_tick_many_loglik's fleet likelihood of the same
    window is not lower than before"""
    yaw, gz, rpm = lr.model_log(N_FIT, T_FIT, SEED_FIT)
    kw = dict(kf6_rec=fmskf.kf6_records(yaw, gz, rpm))
    r0 = lr.r_default()
    r0[0] += 4.0 * SIGMA ** 2

    def fleet(e):
        t = e.tick_many_loglik(T_FIT, total=True, **kw)["total"]
        assert t[3] == 0 and t[0] == N_FIT * T_FIT
        return float(fmskf.loglik(t[1], t[2], t[0]))

    with Engine("kf6", N_FIT, r=r0) as e:
        total = e.tick_many_em(T_FIT, **kw)["total"]
        e.reset()
        before = fleet(e)
    assert total[0] == (T_FIT - 1) * N_FIT and total[1] == T_FIT * N_FIT and total[2] == 0
    q1, r1 = fmskf.em_mstep(total)
    with Engine("kf6", N_FIT, q=q1, r=r1) as e:
        after = fleet(e)
    print("EM_LOOP " + json.dumps(dict(before=before, after=after, r00=[float(r0[0]), float(r1[0])])))
    assert after >= before, (before, after)


# ----------------------------------------------------------------------------- 9. errors
def test_errors_change_nothing(w):
    import torch
    kw = kw_of(w, "rec", None)
    st_ = torch.cuda.Stream()
    with warmed(w) as e, torch.cuda.stream(st_):
        e.set_stream(st_)   # a capture needs a stream
        s0 = snapshot(e)
        ti, keep = e._inputs(kw, T, N)
        nm, sq, sr_, tot = np.zeros(N, np.uint32), np.zeros((21, N)), np.zeros((10, N)), np.zeros(34)

        def out(**f):
            eo = raw_out(dict(n_meas=nm, sq=sq, sr=sr_, total=tot))
            for k, v in f.items():
                setattr(eo, k, v)
            return eo

        assert raw_call(e, ti, T, N, None) == EINVAL
        assert raw_call(e, ti, T, N, out(n_meas=None, sq=None, sr=None, total=None)) == EINVAL
        assert raw_call(e, ti, T, N, out(flags=2)) == EINVAL
        assert raw_call(e, ti, T, N, out(flags=_lib.EM_ACCUMULATE | 0x80000000)) == EINVAL
        assert raw_call(e, ti, T, N, out(mem=7)) == EINVAL
        assert raw_call(e, ti, T, N, out(pitch=N - 1)) == EINVAL
        assert raw_call(e, ti, 0, N, out()) == EINVAL
        dev = torch.zeros(34 + 1, dtype=torch.float64, device="cuda")
        assert raw_call(e, ti, T, N, out(mem=_lib.MEM_DEVICE, n_meas=None, sq=None, sr=None,
                                         total=dev.data_ptr() + 4)) == EINVAL    # misaligned device doubles
        # everything fmskf_tick_many refuses
        assert raw_call(e, None, T, N, out()) == EINVAL
        assert raw_call(e, ti, T, N - 1, out()) == EINVAL
        for bad in (dict(kw, yaw_deg=np.ascontiguousarray(w["yaw"][:T])),       # records and a plane
                    dict(yaw_deg=np.ascontiguousarray(w["yaw"][:T]))):          # planes missing
            with pytest.raises(fmskf.FmskfError) as ei:
                e.tick_many_em(T, **bad)
            assert ei.value.code == EINVAL
        # the host staging cannot be allocated (31 rows of 2^44 doubles): before any launch
        assert raw_call(e, ti, T, N, out(pitch=1 << 44)) == ENOMEM
        assert raw_call(e, ti, T, N, out(pitch=1 << 62)) == ENOMEM
        same(s0, snapshot(e), "refused calls")
        assert not nm.any() and not sq.any() and not sr_.any() and not tot.any()
        # inside a graph capture
        dti, dkeep = e._inputs(to_device(kw), T, N)
        darr = dict(total=torch.zeros(34, dtype=torch.float64, device="cuda"))
        e.graph_begin()
        assert raw_call(e, dti, T, N, raw_out(darr)) == EINVAL
        e.predict()          # captured, never replayed
        e.graph_end()
        same(s0, snapshot(e), "refused in a capture")
        r = e.tick_many_em(T, per_robot=True, **kw)   # and the handle still works
        e.sync()
    with warmed(w) as c:
        same_sums(c.tick_many_em(T, per_robot=True, **kw), r, ALL, "after the refused calls")


@pytest.mark.parametrize("model,flags,gate", [("rs", 0, False), ("ekf9", 0, False), ("kf12d", 0, False),
                                              ("kf6", fmskf.CFG_COMP_POS, False), ("kf6", 0, True)])
def test_unsupported_handles(w, model, flags, gate):
    n = 300
    kw = dict(kf6_rec=np.ascontiguousarray(w["rec"][:3, :n])) if model == "kf6" else \
        dict(yaw_deg=np.ascontiguousarray(w["yaw"][:3, :n]), rpm=np.ascontiguousarray(w["rpm"][:3, :n]))

    def snap(e):
        x, P = e.get_state()
        return [x] + ([P] if P is not None else []) + [np.array(e.get_counters(), np.uint64)] + \
            (list(e.get_gate().values()) if gate else [])

    with Engine(model, n, flags=flags) as e:
        if gate:
            e.set_gate(25.0, 3)
        if model == "kf6":
            e.tick(kf6_rec=kw["kf6_rec"][0])
        s0 = snap(e)
        with pytest.raises(fmskf.FmskfError) as ei:
            e.tick_many_em(3, per_robot=True, total=True, **kw)
        assert ei.value.code == ENOTSUP
        same(s0, snap(e), model)
