"""fmskf_tick_many_trace on the GPU: the forward pass is fmskf_tick_many (on a gated handle the
gate state too), every per-tick value and state row against a twin that runs the window as T
single ticks and reads out after each, the bridge (an ungated handle fed the `applied` plane
repeats the gated trajectory and takes the other window calls), sentinels and bounds, lane
isolation, determinism, small shapes, the refusals.

Shapes (trace_ref): N = 4113 robots (no multiple of 256, three 2048-wide tiles), a window of T = 37
ticks (odd: the loop unrolled by two ends on its tail) behind 50 warm-up ticks; and N in
(1, 65, 257) with T in (1, 2) from reset()."""
import ctypes as C

import numpy as np
import pytest

import fmskf
from fmskf import Engine
from fmskf import _lib

import trace_ref as tr
from loglik_ref import bits, kw_of, same, snapshot, to_device
from trace_ref import ACC, FRC, N, NONE, REJ, T, WARM, host

pytestmark = pytest.mark.gpu

EINVAL, ENOMEM, ENOTSUP = _lib.EINVAL, _lib.ENOMEM, _lib.ENOTSUP
PLANES = ("nis", "status", "applied")
SENT_F, SENT_B = np.float32(-12345.5), np.uint8(0xA5)
GATED = pytest.mark.parametrize("gated", [False, True], ids=["ungated", "gated"])


@pytest.fixture(scope="module")
def w():
    return tr.window()


_TWINS = {}


def twin(w, gated, masked=True):
    """the twin's run of the main window, computed once per case and never written"""
    key = (gated, masked)
    if key not in _TWINS:
        _TWINS[key] = tr.twin_run(w, gated, w["valid"] if masked else None)
    return _TWINS[key]


def raw_out(arrays, **fields):
    """a fmskf_trace_out over a dict of arrays (numpy: host, torch: device)"""
    to = _lib.TraceOut()
    dev = any(not isinstance(v, np.ndarray) for v in arrays.values())
    to.mem = _lib.MEM_DEVICE if dev else _lib.MEM_HOST
    for k, v in arrays.items():
        setattr(to, k, v.ctypes.data if isinstance(v, np.ndarray) else v.data_ptr())
    for k, v in fields.items():
        setattr(to, k, v)
    return to


def raw_call(e, ti, n_ticks, stride, to):
    return fmskf.load().fmskf_tick_many_trace(e.h, C.byref(ti) if ti is not None else None, n_ticks, stride,
                                              C.byref(to) if to is not None else None)


def sentinels(rows, pitch, Tn=T, extra=2, device=False, odd=False):
    """output arrays prefilled with a sentinel: Tn + extra rows of the per-tick planes, rows + extra
    state rows; on the device the byte planes one byte off any alignment when `odd`"""
    a = dict(nis=np.full((Tn + extra, pitch), SENT_F, np.float32), status=np.full((Tn + extra, pitch), SENT_B, np.uint8),
             applied=np.full((Tn + extra, pitch), SENT_B, np.uint8), x=np.full((rows + extra, 6, pitch), SENT_F, np.float32),
             P=np.full((rows + extra, 21, pitch), SENT_F, np.float32))
    if device:
        import torch
        for k, v in a.items():
            if odd and v.dtype == np.uint8:
                buf = torch.full((v.size + 1,), int(SENT_B), dtype=torch.uint8, device="cuda")
                a[k] = buf[1:].view(v.shape)
                assert a[k].data_ptr() % 2 == 1 and a[k].is_contiguous()
            else:
                a[k] = torch.from_numpy(v).cuda()
    return a


def check_untouched(r, n, Tn, rows, what):
    """columns [n, pitch) and the rows past the declared ones still hold the sentinel"""
    for k in PLANES:
        s = SENT_F if k == "nis" else SENT_B
        assert (r[k][:, n:] == s).all() and (r[k][Tn:] == s).all(), f"{what}: {k} written outside its rows / columns"
    for k in ("x", "P"):
        if k in r:
            assert (r[k][:, :, n:] == SENT_F).all() and (r[k][rows:] == SENT_F).all(), f"{what}: {k} outside"
            assert not (bits(r[k][:rows, :, :n]) == bits(np.array([SENT_F]))[0]).all()


# ----------------------------------------------------------------------------- 1. forward identity
@GATED
@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "valid"])
@pytest.mark.parametrize("form", ["rec", "planes"])
def test_forward_is_tick_many(w, form, masked, mem, gated):
    kw = kw_of(w, form, w["valid"] if masked else None)
    if mem == "device":
        kw = to_device(kw)
    with tr.engine(w, gated) as e, tr.engine(w, gated) as c:
        r = e.tick_many_trace(T, every=5, want_P=masked, **kw)
        c.tick_many(T, **kw)
        assert (mem == "device") == (not isinstance(r["nis"], np.ndarray))
        assert set(r) == set(PLANES) | {"x"} | ({"P"} if masked else set())
        r = host(r)
        same(snapshot(e, gate=gated), snapshot(c, gate=gated), f"{form} masked={masked} {mem} gated={gated}")
    assert r["x"].shape == (T // 5, 6, N) and np.isfinite(r["x"]).all()


# ----------------------------------------------------------------------------- 2. per-tick values
@GATED
@pytest.mark.parametrize("every", [1, 2, 5, 37])
def test_values_against_single_ticks(w, gated, every):
    """status, nis, applied of every tick and the state rows against the twin's readouts behind T
    single ticks, bit for bit; 5 does not divide 37: 7 rows"""
    tw = twin(w, gated)
    with tr.engine(w, gated) as e:
        r = host(e.tick_many_trace(T, every=every, want_P=True, **kw_of(w, "rec", w["valid"])))
        x, P = e.get_state()
        assert np.array_equal(bits(x), bits(tw["xs"][-1])) and np.array_equal(bits(P), bits(tw["Ps"][-1]))
    assert r["x"].shape == (T // every, 6, N) and r["P"].shape == (T // every, 21, N)
    assert every != 5 or r["x"].shape[0] == 7
    tr.check_against_twin(r, tw, w["valid"], gated, every, f"every={every} gated={gated}")
    if gated:
        st = r["status"]
        for s in (NONE, ACC, REJ, FRC):
            assert (st == s).any(), f"status {s} does not occur in the GPU's trace"
        assert ((st[2:] == FRC) & (st[1:-1] == REJ) & (st[:-2] == REJ)).any()


def test_every_is_not_read_without_state_rows(w):
    tw = twin(w, True)
    for every in (0, 0xFFFFFFFF):
        st = np.zeros((T, N), np.uint8)
        with tr.engine(w, True) as e:
            ti, keep = e._inputs(kw_of(w, "rec", w["valid"]), T, N)
            assert raw_call(e, ti, T, N, raw_out(dict(status=st), every=every)) == 0
        assert np.array_equal(st, tw["status"])


@GATED
def test_values_unmasked_planes_device(w, gated):
    """the same without a mask, from device planes into device outputs"""
    tw = twin(w, gated, masked=False)
    with tr.engine(w, gated) as e:
        r = host(e.tick_many_trace(T, every=2, **to_device(kw_of(w, "planes", None))))
    assert "P" not in r
    tr.check_against_twin(r, tw, None, gated, 2, f"unmasked gated={gated}")


# ----------------------------------------------------------------------------- 3. the bridge
def test_applied_plane_replays_the_gated_log(w):
    """a gated handle traced with pitch = tick_stride = N + 3; an ungated handle set to the same
    start and fed valid = applied ends with the gated handle's x and P bit for bit, and takes
    tick_many_loglik and tick_many_smooth"""
    S = N + 3
    lo = w["warm"]
    rec = np.zeros((T, S), w["rec"].dtype)
    rec[:, :N] = w["rec"][lo:lo + T]
    valid = np.zeros((T, S), np.uint8)
    valid[:, :N] = w["valid"]
    with tr.engine(w, True) as g:
        x0, P0 = g.get_state()
        out = dict(applied=np.zeros((T, S), np.uint8), status=np.zeros((T, S), np.uint8))
        g.tick_many_trace(T, tick_stride=S, pitch=S, out=out, kf6_rec=rec, valid=valid)
        xg, Pg = g.get_state()
    applied = out["applied"]
    assert not applied[:, N:].any()
    assert 0 < applied.sum() < valid.sum(), "the gate rejected nothing, or everything"
    assert np.array_equal(applied, np.isin(out["status"], (ACC, FRC)).astype(np.uint8))
    with Engine("kf6", N) as u, Engine("kf6", N) as ll, Engine("kf6", N) as sm:
        for e in (u, ll, sm):
            e.set_state(x0, P0)
        u.tick_many(T, tick_stride=S, kf6_rec=rec, valid=applied)
        xu, Pu = u.get_state()
        assert np.array_equal(bits(xu), bits(xg)) and np.array_equal(bits(Pu), bits(Pg))
        r = ll.tick_many_loglik(T, tick_stride=S, kf6_rec=rec, valid=applied)
        assert np.array_equal(r["n_meas"], applied[:, :N].sum(axis=0).astype(np.uint32))
        xs = sm.tick_many_smooth(T, tick_stride=S, kf6_rec=rec, valid=applied)
        assert xs.shape == (T, 6, N) and np.isfinite(xs).all()
        for e in (ll, sm):
            xe, Pe = e.get_state()
            assert np.array_equal(bits(xe), bits(xg)) and np.array_equal(bits(Pe), bits(Pg))


# ----------------------------------------------------------------------------- 4. sentinels, bounds
@GATED
@pytest.mark.parametrize("mem", ["host", "device"])
def test_sentinels_and_bounds(w, mem, gated):
    """prefilled outputs at an odd pitch (device byte planes at an odd address): unmeasured ticks are
    exactly (0x7FC00000, NONE, 0), columns [N, pitch) and rows past T // every are untouched"""
    every, pitch = 5, N + 4
    rows = T // every
    tw = twin(w, gated)
    a = sentinels(rows, pitch, device=mem == "device", odd=True)
    with tr.engine(w, gated) as e:
        r = e.tick_many_trace(T, every=every, pitch=pitch, out=a, **kw_of(w, "rec", w["valid"]))
        assert r is a
        r = host(r)
    check_untouched(r, N, T, rows, f"{mem} gated={gated}")
    un = w["valid"] == 0
    assert (bits(r["nis"][:T, :N])[un] == tr.NO_NIS).all()
    assert (r["status"][:T, :N][un] == NONE).all() and (r["applied"][:T, :N][un] == 0).all()
    tr.check_against_twin(r, tw, w["valid"], gated, every, f"sentinels {mem} gated={gated}")


@GATED
def test_no_measurement_is_all_none(w, gated):
    zero = np.zeros((T, N), np.uint8)
    kw = kw_of(w, "rec", zero)
    with tr.engine(w, gated) as e, tr.engine(w, gated) as c:
        r = e.tick_many_trace(T, **kw)
        c.tick_many(T, **kw)
        same(snapshot(e, gate=gated), snapshot(c, gate=gated), "all-zero valid")
    assert not r["status"].any() and not r["applied"].any() and (bits(r["nis"]) == tr.NO_NIS).all()


# ----------------------------------------------------------------------------- 5. isolation, guard
@GATED
def test_lane_isolation_and_guard(w, gated):
    """one robot's state set to NaN: every other robot's outputs and state are the clean run's byte
    for byte, and counter [0] moves as tick_many's does"""
    bad = 2049
    kw = kw_of(w, "rec", w["valid"])
    nan = np.full((6, 1), np.nan, np.float32)
    with tr.engine(w, gated) as e, tr.engine(w, gated) as p, tr.engine(w, gated) as c:
        for h in (p, c):
            h.set_state_subset([bad], x=nan)
        clean = e.tick_many_trace(T, every=5, want_P=True, **kw)
        dirty = p.tick_many_trace(T, every=5, want_P=True, **kw)
        c.tick_many(T, **kw)
        same(snapshot(p, gate=gated), snapshot(c, gate=gated), "poisoned forward pass")
        assert p.get_counters()[0] == c.get_counters()[0] == 1 and e.get_counters()[0] == 0
        se, sp = snapshot(e, gate=gated), snapshot(p, gate=gated)
    others = np.setdiff1d(np.arange(N), [bad])
    for k in clean:
        assert np.ascontiguousarray(clean[k][..., others]).tobytes() == \
            np.ascontiguousarray(dirty[k][..., others]).tobytes(), k
    for k, (u, v) in enumerate(zip(se, sp)):
        if k != 2:   # the counters
            assert np.ascontiguousarray(u[..., others]).tobytes() == np.ascontiguousarray(v[..., others]).tobytes(), k
    assert np.isnan(dirty["x"][:, :, bad]).any()


# ----------------------------------------------------------------------------- 6. determinism
@GATED
def test_two_calls_write_the_same_bytes(w, gated):
    pitch, rows = N + 4, T // 2
    kw = to_device(kw_of(w, "rec", w["valid"]))
    res = []
    for _ in range(2):
        with tr.engine(w, gated) as e:
            a = sentinels(rows, pitch, device=True)
            e.tick_many_trace(T, every=2, pitch=pitch, out=a, **kw)
            res.append((host(a), snapshot(e, gate=gated)))
    for k in res[0][0]:
        assert res[0][0][k].tobytes() == res[1][0][k].tobytes(), k
    same(res[0][1], res[1][1], "two calls")


# ----------------------------------------------------------------------------- 7. small shapes
@GATED
@pytest.mark.parametrize("n,Tn", tr.SMALL)
def test_small_shapes(n, Tn, gated):
    ws = tr.window(n, Tn, warm=0, seed=100 + n)
    tw = tr.twin_run(ws, gated, ws["valid"], warm=False)
    for every in sorted({1, Tn}):
        a = sentinels(Tn // every, n + 1, Tn=Tn)
        with tr.engine(ws, gated, warm=False) as e:
            e.tick_many_trace(Tn, every=every, pitch=n + 1, out=a, **kw_of(ws, "rec", ws["valid"]))
            x, P = e.get_state()
            assert np.array_equal(bits(x), bits(tw["xs"][-1])) and np.array_equal(bits(P), bits(tw["Ps"][-1]))
            if gated:
                g = e.get_gate()
                for k in g:
                    assert g[k].tobytes() == tw["gate"][k].tobytes(), k
        check_untouched(a, n, Tn, Tn // every, f"n={n} T={Tn}")
        tr.check_against_twin(a, tw, ws["valid"], gated, every, f"n={n} T={Tn} every={every} gated={gated}")


# ----------------------------------------------------------------------------- 8. refusals
@GATED
def test_errors_change_nothing(w, gated):
    import torch
    kw = kw_of(w, "rec", None)
    st_ = torch.cuda.Stream()
    with tr.engine(w, gated) as e, torch.cuda.stream(st_):
        e.set_stream(st_)   # a capture needs a stream
        s0 = snapshot(e, gate=gated)
        ti, keep = e._inputs(kw, T, N)
        nis, stt, app = np.zeros((T, N), np.float32), np.zeros((T, N), np.uint8), np.zeros((T, N), np.uint8)
        xr = np.zeros((T, 6, N), np.float32)

        def out(**f):
            return raw_out(dict(nis=nis, status=stt, applied=app), **f)

        assert raw_call(e, ti, T, N, None) == EINVAL
        assert raw_call(e, ti, T, N, out(nis=None, status=None, applied=None)) == EINVAL
        assert raw_call(e, ti, T, N, out(reserved=1)) == EINVAL
        assert raw_call(e, ti, T, N, out(reserved2=1)) == EINVAL
        assert raw_call(e, ti, T, N, out(mem=7)) == EINVAL
        assert raw_call(e, ti, T, N, out(pitch=N - 1)) == EINVAL
        assert raw_call(e, ti, 0, N, out()) == EINVAL
        for every in (0, T + 1):
            assert raw_call(e, ti, T, N, out(x=xr.ctypes.data, every=every)) == EINVAL
            assert raw_call(e, ti, T, N, out(P=xr.ctypes.data, every=every)) == EINVAL
        dev = torch.zeros(T * N + 1, dtype=torch.float32, device="cuda")
        for k in ("nis", "x", "P"):   # a misaligned device float plane
            assert raw_call(e, ti, T, N, raw_out({}, mem=_lib.MEM_DEVICE, every=T, **{k: dev.data_ptr() + 2})) == EINVAL
        # everything fmskf_tick_many refuses
        assert raw_call(e, None, T, N, out()) == EINVAL
        assert raw_call(e, ti, T, N - 1, out()) == EINVAL
        for bad in (dict(kw, yaw_deg=np.ascontiguousarray(w["yaw"][:T])),       # records and a plane
                    dict(yaw_deg=np.ascontiguousarray(w["yaw"][:T]))):          # planes missing
            with pytest.raises(fmskf.FmskfError) as ei:
                e.tick_many_trace(T, **bad)
            assert ei.value.code == EINVAL
        # the host staging cannot be allocated: before any launch
        assert raw_call(e, ti, T, N, out(pitch=1 << 44)) == ENOMEM
        assert raw_call(e, ti, T, N, out(pitch=1 << 62)) == ENOMEM
        same(s0, snapshot(e, gate=gated), "refused calls")
        assert not nis.any() and not stt.any() and not app.any() and not xr.any()
        # inside a graph capture
        dti, dkeep = e._inputs(to_device(kw), T, N)
        darr = dict(status=torch.zeros((T, N), dtype=torch.uint8, device="cuda"))
        e.graph_begin()
        assert raw_call(e, dti, T, N, raw_out(darr)) == EINVAL
        e.predict()          # captured, never replayed
        e.graph_end()
        same(s0, snapshot(e, gate=gated), "refused in a capture")
        assert not darr["status"].any().item()
        r = e.tick_many_trace(T, **kw)   # and the handle still works
        e.sync()
        s1 = snapshot(e, gate=gated)
    with tr.engine(w, gated) as c:
        r2 = c.tick_many_trace(T, **kw)
        for k in PLANES:
            assert r[k].tobytes() == r2[k].tobytes(), k
        same(s1, snapshot(c, gate=gated), "after the refused calls")


@pytest.mark.parametrize("model,flags", [("rs", 0), ("ekf9", 0), ("kf12d", 0), ("kf6", fmskf.CFG_COMP_POS)])
def test_unsupported_handles(w, model, flags):
    n = 300
    kw = dict(kf6_rec=np.ascontiguousarray(w["rec"][:3, :n])) if model == "kf6" else \
        dict(yaw_deg=np.ascontiguousarray(w["yaw"][:3, :n]), rpm=np.ascontiguousarray(w["rpm"][:3, :n]))

    def snap(e):
        x, P = e.get_state()
        return [x] + ([P] if P is not None else []) + [np.array(e.get_counters(), np.uint64)]

    with Engine(model, n, flags=flags) as e:
        if model == "kf6":
            e.tick(kf6_rec=kw["kf6_rec"][0])
        s0 = snap(e)
        ti, keep = e._inputs(kw, 3, n)
        st = np.zeros((3, n), np.uint8)
        assert raw_call(e, ti, 3, n, raw_out(dict(status=st))) == ENOTSUP
        same(s0, snap(e), model)
        assert not st.any()
        if model == "kf6":
            e.tick(kf6_rec=kw["kf6_rec"][1])   # the handle still works
