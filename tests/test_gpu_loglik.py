"""fmskf_tick_many_loglik on the GPU: the forward pass is fmskf_tick_many, the window's sums against
the float64 definition within the bound of tests/loglik_ref.py, the NIS of one tick against the
monitor-only gate bit for bit, the deterministic fleet total, chunked accumulation, lane isolation,
the error cases.

Shapes (smooth_ref): N = 4113 robots (no multiple of 256, three 2048-wide tiles), windows of
T = 37 ticks (odd: the loop unrolled by two ends on its tail) behind 50 plain ticks; and
N in (1, 65, 257) with T in (1, 2) from reset()."""
import ctypes as C
import json
import math

import numpy as np
import pytest

import fmskf
from fmskf import Engine
from fmskf import _lib

import loglik_ref as lr
import smooth_ref as sr
from loglik_ref import bits, kw_of, same, snapshot, to_device, warmed

pytestmark = pytest.mark.gpu

N, T, WARM = sr.N, sr.T, sr.WARM
EINVAL, ENOMEM, ENOTSUP = _lib.EINVAL, _lib.ENOMEM, _lib.ENOTSUP
LIK = ("n_meas", "nis_sum", "logdet_sum")
MOM = ("innov_sum", "innov_outer")
SENT = -12345.5


def b64(a):
    return np.ascontiguousarray(a).view(np.uint64 if np.asarray(a).dtype.itemsize == 8 else np.uint32)


def host(r):
    """a result dict as numpy arrays (n_meas as uint32), the device drained first"""
    import torch
    torch.cuda.synchronize()
    out = {k: (v.cpu().numpy() if not isinstance(v, np.ndarray) else v) for k, v in r.items()}
    out["n_meas"] = out["n_meas"].view(np.uint32)
    return out


def same_sums(a, b, keys, what):
    for k in keys:
        assert np.array_equal(b64(a[k]), b64(b[k])), f"{what}: {k} differs"


@pytest.fixture(scope="module")
def w(orc):
    return sr.window(orc)


def check_against_float64(orc, wd, e, Tn, valid, tag, n=N):
    """run the window on e (moments and total), and hold every sum to the rule of loglik_ref"""
    lo = wd["warm"]
    x0, P0 = e.get_state()
    got = e.tick_many_loglik(Tn, moments=True, total=True, **kw_of(wd, "rec", valid, lo, lo + Tn))
    xs, Ps, x_end, P_end = lr.priors(orc, x0, P0, wd["yaw"][lo:lo + Tn], wd["gz"][lo:lo + Tn], wd["rpm"][lo:lo + Tn], valid)
    x1, P1 = e.get_state()
    assert np.array_equal(bits(x1), bits(x_end)) and np.array_equal(bits(P1), bits(P_end)), "the state is not the oracle's"
    z = wd["z"][lo:lo + Tn]
    ref, r32 = lr.definition(xs, Ps, z, valid), lr.restate_f32(xs, Ps, z, valid)
    assert not r32["bad"].any()
    assert np.array_equal(got["n_meas"], ref["n_meas"]), "n_meas is not the mask's column sums"
    if valid is not None:
        assert np.array_equal(got["n_meas"], np.asarray(valid[:Tn], np.uint32).sum(axis=0))
    dev32, dev = lr.deviations(r32, ref), lr.deviations(got, ref)
    bound = lr.bounds(dev32, ref)
    tol = lambda d: {k: np.asarray(v).tolist() for k, v in d.items()}
    print("LOGLIK_DEV " + json.dumps(dict(case=tag, n=n, T=Tn, gpu=tol(dev), f32=tol(dev32), bound=tol(bound))))
    for k in lr.QUANTITIES:
        assert np.isfinite(got[k]).all(), k
        assert (dev[k] <= bound[k]).all(), (k, dev[k], bound[k])
    # the total: the kernels' fixed tree, bit for bit, and exact in its count
    for k, name in enumerate(LIK):
        assert got["total"][k] == lr.fleet_fold(got[name]), name
    assert got["total"][0] == int(got["n_meas"].sum()) and got["total"][3] == 0
    return got


# ----------------------------------------------------------------------------- 1. forward identity
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "valid"])
@pytest.mark.parametrize("form", ["rec", "planes"])
def test_forward_is_tick_many(w, form, masked, mem):
    kw = kw_of(w, form, w["valid"] if masked else None)
    if mem == "device":
        kw = to_device(kw)
    with warmed(w) as e, warmed(w) as c:
        r = e.tick_many_loglik(T, moments=masked, total=not masked, **kw)
        c.tick_many(T, **kw)
        assert (mem == "device") == (not isinstance(r["nis_sum"], np.ndarray))
        r = host(r)
        same(snapshot(e), snapshot(c), f"{form} masked={masked} {mem}")
    assert np.isfinite(r["nis_sum"]).all() and (r["n_meas"] == (w["valid"].sum(axis=0) if masked else T)).all()


# ----------------------------------------------------------------------------- 2. values
@pytest.mark.parametrize("start", ["warm", "reset"])
def test_against_float64(orc, w, start):
    """`warm`: behind 50 plain ticks; `reset`: straight from reset(), the diffuse prior P0, where
    log det S falls by orders of magnitude inside the window"""
    valid = w["valid"]
    assert (valid[0] == 0).sum() > N // 6 and (valid[-1] == 0).sum() > N // 8
    with warmed(w, warm=start == "warm") as e:
        got = check_against_float64(orc, w, e, T, valid, start)
    # the likelihood-only kernel: the same likelihood bytes
    with warmed(w, warm=start == "warm") as e:
        lik = e.tick_many_loglik(T, total=True, **kw_of(w, "rec", valid))
    assert set(lik) == set(LIK) | {"total"}
    same_sums(lik, got, LIK + ("total",), "likelihood-only against the innovation-sum variant")


@pytest.mark.parametrize("Tn", [1, 2])
@pytest.mark.parametrize("n", [1, 65, 257])
def test_small_shapes(orc, n, Tn):
    """one lane, one block and a bit, two blocks; one tick and the unrolled pair: from reset(), masked"""
    wd = sr.window(orc, n=n, Tn=2, warm=0, seed=100 + n)
    with Engine("kf6", n) as e:
        check_against_float64(orc, wd, e, Tn, wd["valid"][:Tn], f"small-{n}-{Tn}", n)


def test_no_measurement_gives_zeros(w):
    valid = np.zeros((T, N), np.uint8)
    with warmed(w) as e, warmed(w) as c:
        r = e.tick_many_loglik(T, moments=True, total=True, **kw_of(w, "rec", valid))
        c.tick_many(T, **kw_of(w, "rec", valid))
        same(snapshot(e), snapshot(c), "no measurement")
    for k, v in r.items():
        assert not b64(v).any(), f"{k} is not all +0"


# ----------------------------------------------------------------------------- 3. the gate's NIS
def test_one_tick_is_the_gates_nis(w):
    """T = 1 against a monitor-only gated twin: nis_sum is (double)nis of fmskf_get_gate bit for bit"""
    valid = w["valid"][:1]
    kw = kw_of(w, "rec", valid, WARM, WARM + 1)
    with warmed(w) as e, warmed(w) as g:
        g.set_gate(float("inf"), 0)
        r = e.tick_many_loglik(1, **kw)
        g.tick_many(1, **kw)
        gate = g.get_gate()
        same(snapshot(e), snapshot(g), "monitor-only twin")
    m = valid[0].astype(bool)
    assert m.any() and (~m).any()
    assert np.array_equal(b64(r["nis_sum"][m]), b64(gate["nis"][m].astype(np.float64)))
    assert not b64(r["nis_sum"][~m]).any() and np.array_equal(r["n_meas"], valid[0])


# ----------------------------------------------------------------------------- 4. the total
def test_total_is_deterministic_and_close(w):
    kw = kw_of(w, "rec", w["valid"])
    runs = []
    for _ in range(2):
        with warmed(w) as e:
            runs.append(e.tick_many_loglik(T, moments=True, total=True, **kw))
    a, b = runs
    same_sums(a, b, LIK + MOM + ("total",), "two calls on the same state and inputs")
    for k, name in enumerate(LIK):
        v = a[name].astype(np.float64)
        assert abs(a["total"][k] - math.fsum(v)) <= N * 2.0 ** -52 * math.fsum(np.abs(v)), name
        assert a["total"][k] == lr.fleet_fold(a[name]), f"{name}: the total is not the fixed tree of the per-robot sums"
    assert a["total"][0] == int(a["n_meas"].sum()) and a["total"][3] == 0


# ----------------------------------------------------------------------------- 5. accumulation
def raw_out(arrays, flags=0, pitch=0):
    """a fmskf_loglik_out over numpy arrays or torch device tensors"""
    lo = _lib.LoglikOut()
    dev = any(not isinstance(v, np.ndarray) for v in arrays.values())
    lo.mem, lo.flags, lo.pitch = (_lib.MEM_DEVICE if dev else _lib.MEM_HOST), flags, pitch
    for k, v in arrays.items():
        setattr(lo, k, v.data_ptr() if dev else v.ctypes.data)
    return lo


def raw_call(e, ti, n_ticks, stride, lo):
    return fmskf.load().fmskf_tick_many_loglik(e.h, C.byref(ti) if ti is not None else None, n_ticks, stride,
                                               C.byref(lo) if lo is not None else None)


def test_accumulate_over_chunks(w):
    valid = w["valid"]
    cut = 18
    k1, k2 = kw_of(w, "rec", valid[:cut], WARM, WARM + cut), kw_of(w, "rec", valid[cut:], WARM + cut, WARM + T)
    with warmed(w) as e, warmed(w) as s, warmed(w) as c:
        acc = e.tick_many_loglik(cut, moments=True, total=True, **k1)
        first = {k: v.copy() for k, v in acc.items()}
        assert e.tick_many_loglik(T - cut, accumulate_into=acc, **k2) is acc
        r1 = s.tick_many_loglik(cut, moments=True, total=True, **k1)
        r2 = s.tick_many_loglik(T - cut, moments=True, total=True, **k2)
        c.tick_many(T, **kw_of(w, "rec", valid))
        same(snapshot(e), snapshot(c), "18 + 19 ticks against 37")
        same(snapshot(s), snapshot(c), "18 + 19 ticks, separate results")
        # without the flag a call overwrites what the arrays hold: the second chunk again, on a twin
        # state, into arrays that hold the first chunk's sums
        ti, _keep = s._inputs(k2, T - cut, N)
    same_sums(first, r1, LIK + MOM + ("total",), "the first chunk")
    assert np.array_equal(acc["n_meas"], r1["n_meas"] + r2["n_meas"]) and np.array_equal(acc["n_meas"], valid.sum(axis=0))
    for k in ("nis_sum", "logdet_sum") + MOM + ("total",):
        assert np.array_equal(acc[k], r1[k] + r2[k]), f"{k}: not one fp64 addition of the chunks' results"
    with warmed(w) as o:
        o.tick_many(cut, **k1)
        over = {k: v.copy() for k, v in r1.items()}
        assert raw_call(o, ti, T - cut, N, raw_out(over)) == 0
    same_sums(over, r2, LIK + MOM + ("total",), "overwritten without FMSKF_LL_ACCUMULATE")


# ----------------------------------------------------------------------------- 6. isolation
@pytest.mark.parametrize("mem", ["host", "device"])
def test_lane_isolation_and_pitch(w, mem):
    """one robot's state set to NaN: its sums are NaN and its n_meas true, it is counted in
    total[3] and left out of the rest, every other robot's bytes are the clean run's; the padded
    innovation planes keep their elements past N"""
    import torch
    bad, pitch = 2049, N + 59
    valid = w["valid"]
    kw = kw_of(w, "rec", valid)

    def arrays():
        a = dict(n_meas=np.zeros(N, np.uint32), nis_sum=np.zeros(N), logdet_sum=np.zeros(N),
                 innov_sum=np.full((4, pitch), SENT), innov_outer=np.full((10, pitch), SENT), total=np.zeros(4))
        if mem == "device":
            a = {k: torch.from_numpy(v.view(np.int32) if k == "n_meas" else v).cuda() for k, v in a.items()}
        return a

    with warmed(w) as e, warmed(w) as p, warmed(w) as c:
        nan = np.full((6, 1), np.nan, np.float32)
        for h in (p, c):
            h.set_state_subset([bad], x=nan)
        ti, _keep = e._inputs(kw, T, N)
        clean, dirty = arrays(), arrays()
        assert raw_call(e, ti, T, N, raw_out(clean, pitch=pitch)) == 0
        assert raw_call(p, ti, T, N, raw_out(dirty, pitch=pitch)) == 0
        c.tick_many(T, **kw)
        clean, dirty = host(clean), host(dirty)
        same(snapshot(p), snapshot(c), "poisoned forward pass")
        assert p.get_counters()[0] == 1 and e.get_counters()[0] == 0
    others = np.setdiff1d(np.arange(N), [bad])
    for k in LIK + MOM:
        assert np.array_equal(b64(clean[k][..., others]), b64(dirty[k][..., others])), k
    for k in MOM:
        assert (clean[k][:, N:] == SENT).all() and (dirty[k][:, N:] == SENT).all(), k + " padding"
        assert not (clean[k][:, :N] == SENT).any()
    assert np.isnan(dirty["nis_sum"][bad]) and np.isnan(dirty["logdet_sum"][bad])
    assert dirty["n_meas"][bad] == valid[:, bad].sum() > 0
    assert dirty["total"][3] == 1 and clean["total"][3] == 0
    for k, name in enumerate(LIK):
        v = clean[name].astype(np.float64)
        v[bad] = 0.0
        assert dirty["total"][k] == lr.fleet_fold(v), name
    assert dirty["total"][0] == int(dirty["n_meas"][others].sum())


# ----------------------------------------------------------------------------- 7. errors
def test_errors_change_nothing(w):
    import torch
    kw = kw_of(w, "rec", None)
    st_ = torch.cuda.Stream()
    with warmed(w) as e, torch.cuda.stream(st_):
        e.set_stream(st_)   # a capture needs a stream
        s0 = snapshot(e)
        ti, keep = e._inputs(kw, T, N)
        nis, ld, nm = np.zeros(N), np.zeros(N), np.zeros(N, np.uint32)
        mom = np.zeros((4, N))

        def out(**f):
            lo = raw_out(dict(n_meas=nm, nis_sum=nis, logdet_sum=ld))
            for k, v in f.items():
                setattr(lo, k, v)
            return lo

        assert raw_call(e, ti, T, N, None) == EINVAL
        assert raw_call(e, ti, T, N, out(n_meas=None, nis_sum=None, logdet_sum=None)) == EINVAL
        assert raw_call(e, ti, T, N, out(flags=2)) == EINVAL
        assert raw_call(e, ti, T, N, out(flags=_lib.LL_ACCUMULATE | 0x80000000)) == EINVAL
        assert raw_call(e, ti, T, N, out(mem=7)) == EINVAL
        assert raw_call(e, ti, T, N, out(pitch=N - 1)) == EINVAL
        assert raw_call(e, ti, 0, N, out()) == EINVAL
        dev = torch.zeros(N + 1, dtype=torch.float64, device="cuda")
        assert raw_call(e, ti, T, N, out(mem=_lib.MEM_DEVICE, n_meas=None, logdet_sum=None,
                                         nis_sum=dev.data_ptr() + 4)) == EINVAL    # misaligned device doubles
        # everything fmskf_tick_many refuses
        assert raw_call(e, None, T, N, out()) == EINVAL
        assert raw_call(e, ti, T, N - 1, out()) == EINVAL
        for bad in (dict(kw, yaw_deg=np.ascontiguousarray(w["yaw"][:T])),       # records and a plane
                    dict(yaw_deg=np.ascontiguousarray(w["yaw"][:T]))):          # planes missing
            with pytest.raises(fmskf.FmskfError) as ei:
                e.tick_many_loglik(T, **bad)
            assert ei.value.code == EINVAL
        # the host staging cannot be allocated (14 rows of 2^44 doubles): before any launch
        assert raw_call(e, ti, T, N, out(innov_sum=mom.ctypes.data, pitch=1 << 44)) == ENOMEM
        assert raw_call(e, ti, T, N, out(innov_sum=mom.ctypes.data, pitch=1 << 62)) == ENOMEM
        same(s0, snapshot(e), "refused calls")
        assert not nis.any() and not ld.any() and not nm.any() and not mom.any()
        # inside a graph capture
        dti, dkeep = e._inputs(to_device(kw), T, N)
        darr = dict(nis_sum=torch.zeros(N, dtype=torch.float64, device="cuda"))
        e.graph_begin()
        assert raw_call(e, dti, T, N, raw_out(darr)) == EINVAL
        e.predict()          # captured, never replayed
        e.graph_end()
        same(s0, snapshot(e), "refused in a capture")
        r = e.tick_many_loglik(T, total=True, **kw)   # and the handle still works
        e.sync()
    with warmed(w) as c:
        same_sums(c.tick_many_loglik(T, total=True, **kw), r, LIK + ("total",), "after the refused calls")


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
            e.tick_many_loglik(3, moments=True, total=True, **kw)
        assert ei.value.code == ENOTSUP
        same(s0, snap(e), model)
