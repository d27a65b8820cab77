"""fmskf_tick_many_smooth on the GPU: the forward pass is fmskf_tick_many, the window's last tick is
the filtered state, every tick against the float64 Rauch-Tung-Striebel reference within the bound
of tests/smooth_ref.py, every call form bit for bit, lane isolation, a history past 4 GiB, the
workspace, the error cases.

Shapes (smooth_ref): N = 4113 robots (no multiple of 256, three 2048-wide tiles), windows of
T = 37 ticks (odd: the loops unrolled by two end on their tail) behind 50 plain ticks."""
import ctypes as C
import json

import numpy as np
import pytest

import fmskf
from fmskf import Engine
from fmskf import _lib

import smooth_ref as sr

pytestmark = pytest.mark.gpu

N, T, WARM = sr.N, sr.T, sr.WARM
EINVAL, ENOMEM, ENOTSUP = _lib.EINVAL, _lib.ENOMEM, _lib.ENOTSUP
DIAG = [sr.pk(i, i) for i in range(6)]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def w(orc):
    return sr.window(orc)


def kw_of(w, form, valid, lo=None, hi=None):
    """the keyword inputs of ticks lo .. hi-1 (default: the window behind the warm-up)"""
    lo = w["warm"] if lo is None else lo
    hi = w["warm"] + w["T"] if hi is None else hi
    if form == "rec":
        kw = dict(kf6_rec=np.ascontiguousarray(w["rec"][lo:hi]))
    else:
        kw = dict(yaw_deg=np.ascontiguousarray(w["yaw"][lo:hi]), gyro_z_dps=np.ascontiguousarray(w["gz"][lo:hi]),
                  rpm=np.ascontiguousarray(w["rpm"][lo:hi]))
    if valid is not None:
        kw["valid"] = np.ascontiguousarray(valid)
    return kw


def to_device(kw):
    import torch
    out = {}
    for k, v in kw.items():
        if k == "kf6_rec":
            v = v.view(np.int32).reshape(v.shape + (4,))
        out[k] = torch.from_numpy(np.array(v)).cuda()   # a copy: the shared inputs are read-only
    return out


def warmed(w, warm=True, n=N):
    e = Engine("kf6", n)
    if warm:
        e.tick_many(w["warm"], **kw_of(w, "rec", None, 0, w["warm"]))
    return e


def snapshot(e, gate=False):
    x, P = e.get_state()
    s = [x, P, np.array(e.get_counters(), np.uint64)]
    if gate:
        s += list(e.get_gate().values())
    return s


def same(a, b, what):
    for k, (u, v) in enumerate(zip(a, b)):
        u, v = np.ascontiguousarray(u), np.ascontiguousarray(v)
        assert u.tobytes() == v.tobytes(), f"{what}: element {k} of the snapshot changed"


# ----------------------------------------------------------------------------- 1. forward identity
@pytest.mark.parametrize("masked", [False, True], ids=["all", "valid"])
@pytest.mark.parametrize("form", ["rec", "planes"])
def test_forward_is_tick_many(w, form, masked):
    kw = kw_of(w, form, w["valid"] if masked else None)
    with warmed(w) as e, warmed(w) as c:
        e.tick_many_smooth(T, **kw)
        c.tick_many(T, **kw)
        same(snapshot(e), snapshot(c), f"{form} masked={masked}")


# ----------------------------------------------------------------------------- 2. end of window
@pytest.mark.parametrize("Tn", [T, 1, 2])
def test_last_tick_is_the_filtered_state(w, Tn):
    valid = w["valid"][T - Tn:]          # ends on the window's last row: invalid for i % 7 == 2
    lo, hi = w["warm"], w["warm"] + Tn
    with warmed(w) as e, warmed(w) as c:
        xs, Ps = e.tick_many_smooth(Tn, want_P=True, **kw_of(w, "rec", valid, lo, hi))
        if Tn > 1:
            c.tick_many(Tn - 1, **kw_of(w, "rec", valid[:-1], lo, hi - 1))
        c.correct(**kw_of(w, "rec", valid[-1], hi - 1, hi))
        x, P = c.get_state()
    assert (valid[-1] == 0).any() and (valid[-1] == 1).any()
    rows = [0, 1, 3, 4, 5]
    assert np.array_equal(xs[-1][rows], x[rows])
    assert np.array_equal(xs[-1][2], sr.wrap_pi_f32(x[2]))
    assert np.array_equal(Ps[-1], P)


# ----------------------------------------------------------------------------- 3. against float64
@pytest.mark.parametrize("start", ["warm", "reset"])
def test_against_float64(w, start):
    """`warm`: behind 50 plain ticks; `reset`: straight from reset(), the diffuse prior P0, where a
    form that cancels shows (tick 0 is invalid for one robot in five)"""
    valid = w["valid"]
    z = w["z"][w["warm"]:]
    th = w["tr"].th[w["warm"]:]
    assert sr.crossings(th).size >= 1, "no robot's heading crosses +-pi inside the window"
    assert (valid[0] == 0).sum() > N // 6 and (valid[-1] == 0).sum() > N // 8
    with warmed(w, warm=start == "warm") as e:
        x0, P0 = e.get_state()
        xs, Ps = e.tick_many_smooth(T, want_P=True, **kw_of(w, "rec", valid))
    ref = sr.rts_f64(x0, P0, z, valid)
    x32, P32, _, _ = sr.smooth_f32(x0, P0, z, valid)
    dev32 = sr.deviations(x32, P32, ref)
    dev = sr.deviations(xs, Ps, ref)
    bx, bP = sr.bounds(dev32, ref)
    print("SMOOTH_DEV " + json.dumps(dict(start=start, n=N, T=T, x=dev[0].tolist(), P=dev[1].tolist(),
                                          x_f32=dev32[0].tolist(), P_f32=dev32[1].tolist(),
                                          x_bound=bx.tolist(), P_bound=bP.tolist())))
    assert np.isfinite(xs).all() and np.isfinite(Ps).all()
    assert (dev[0] <= bx).all(), (dev[0], bx)
    assert (dev[1] <= bP).all(), (dev[1], bP)
    assert (Ps[:, DIAG] > 0).all(), "a smoothed variance is not positive"


# ----------------------------------------------------------------------------- 4. forms agree
def test_forms_agree_bit_for_bit(w):
    import torch
    valid = w["valid"]
    kw = kw_of(w, "rec", valid)
    pitch = N + 59
    SENT = np.float32(-12345.5)

    def run(**opt):
        with warmed(w) as e:
            return e.tick_many_smooth(T, **opt)

    xs, Ps = run(want_P=True, **kw)
    assert xs.shape == (T, 6, N) and Ps.shape == (T, 21, N) and isinstance(xs, np.ndarray)
    # x alone (no covariance formed) is the x of the call with P
    assert np.array_equal(bits(run(**kw)), bits(xs)), "x without P"
    # a padded pitch, host and device: the same rows, the padding left alone
    hx, hP = np.full((T, 6, pitch), SENT, np.float32), np.full((T, 21, pitch), SENT, np.float32)
    run(out_x=hx, out_P=hP, pitch=pitch, **kw)
    dx = torch.full((T, 6, pitch), float(SENT), dtype=torch.float32, device="cuda")
    dP = torch.full((T, 21, pitch), float(SENT), dtype=torch.float32, device="cuda")
    run(out_x=dx, out_P=dP, pitch=pitch, **kw)
    torch.cuda.synchronize()
    for name, (ax, aP) in (("host", (hx, hP)), ("device", (dx.cpu().numpy(), dP.cpu().numpy()))):
        assert np.array_equal(bits(ax[:, :, :N]), bits(xs)) and np.array_equal(bits(aP[:, :, :N]), bits(Ps)), name
        assert (bits(ax[:, :, N:]) == bits(SENT)).all() and (bits(aP[:, :, N:]) == bits(SENT)).all(), name + " padding"
    # dense device outputs from host inputs
    ox = torch.empty((T, 6, N), dtype=torch.float32, device="cuda")
    oP = torch.empty((T, 21, N), dtype=torch.float32, device="cuda")
    run(out_x=ox, out_P=oP, **kw)
    torch.cuda.synchronize()
    assert np.array_equal(bits(ox.cpu().numpy()), bits(xs)) and np.array_equal(bits(oP.cpu().numpy()), bits(Ps))
    # device inputs (records, and planes against records), device results
    for form in ("rec", "planes"):
        tx, tP = run(want_P=True, **to_device(kw_of(w, form, valid)))
        assert tx.is_cuda and tP.is_cuda
        torch.cuda.synchronize()
        assert np.array_equal(bits(tx.cpu().numpy()), bits(xs)) and np.array_equal(bits(tP.cpu().numpy()), bits(Ps)), form


# ----------------------------------------------------------------------------- 5. lane isolation
def test_lane_isolation(w):
    """a NaN yaw for one robot at tick 20 (data, not a fault): every other robot's outputs are the
    clean run's bit for bit, the non-finite counter is tick_many's"""
    bad, tick = 2049, 20
    valid = w["valid"].copy()
    valid[tick, bad] = 1
    clean = kw_of(w, "planes", valid)
    dirty = dict(clean, yaw_deg=clean["yaw_deg"].copy())
    dirty["yaw_deg"][tick, bad] = np.nan
    with warmed(w) as e, warmed(w) as p, warmed(w) as c:
        xs, Ps = e.tick_many_smooth(T, want_P=True, **clean)
        xp, Pp = p.tick_many_smooth(T, want_P=True, **dirty)
        c.tick_many(T, **dirty)
        cnt_p, cnt_c, cnt_e = p.get_counters(), c.get_counters(), e.get_counters()
        same(snapshot(p), snapshot(c), "poisoned forward pass")
    others = np.setdiff1d(np.arange(N), [bad])
    assert np.array_equal(bits(xp[:, :, others]), bits(xs[:, :, others]))
    assert np.array_equal(bits(Pp[:, :, others]), bits(Ps[:, :, others]))
    assert np.isnan(xp[:, :, bad]).any()
    assert list(cnt_p) == list(cnt_c) and cnt_p[0] == 1 and cnt_e[0] == 0


# ----------------------------------------------------------------------------- 6. past 4 GiB
def test_history_past_4gib():
    """N = 4113, T = 6500, x only: 4.3 GB of history (the slice offset passes 2^32 bytes at tick
    6473) and 0.64 GB of outputs, all on the device.  The first and the last 64 robots equal two
    N = 64 engines fed their records: those histories stay below 4 GiB, and lanes are independent"""
    import torch
    Tn = 6500
    g = torch.Generator(device="cuda")
    g.manual_seed(6500)
    yaw = torch.rand((Tn, N), generator=g, device="cuda") * 360.0 - 180.0
    gz = torch.randn((Tn, N), generator=g, device="cuda") * 40.0
    rpm = torch.randint(-3000, 3000, (Tn, N, 4), generator=g, device="cuda", dtype=torch.int16)
    rec = fmskf.kf6_records(yaw, gz, rpm)
    del yaw, gz, rpm
    with Engine("kf6", N) as e:
        need = e.smooth_workspace_bytes(Tn)
        assert need >= 108 * N * Tn and need > 1 << 32
        assert e.smooth_workspace_bytes(6472) < 1 << 32 <= e.smooth_workspace_bytes(6473)
        xs = e.tick_many_smooth(Tn, kf6_rec=rec)
        torch.cuda.synchronize()
        for lo in (0, N - 64):
            with Engine("kf6", 64) as s:
                small = s.tick_many_smooth(Tn, kf6_rec=rec[:, lo:lo + 64].contiguous())
                torch.cuda.synchronize()
                assert torch.equal(small.view(torch.int32), xs[:, :, lo:lo + 64].contiguous().view(torch.int32)), lo
                xa, Pa = s.get_state()
            xb, Pb = e.get_state()
            assert np.array_equal(bits(xa), bits(xb[:, lo:lo + 64])) and np.array_equal(bits(Pa), bits(Pb[:, lo:lo + 64]))
        assert torch.isfinite(xs).all()


# ----------------------------------------------------------------------------- 7. workspace
def test_workspace(w):
    windows = [(w["warm"], w["warm"] + T), (0, 5), (10, 10 + T)]   # T = 37, 5, 37: different inputs
    with Engine("kf6", N) as e:
        sizes = [e.smooth_workspace_bytes(t) for t in (1, 2, 5, 36, 37, 38, 1000)]
        assert all(b >= 108 * N * t for b, t in zip(sizes, (1, 2, 5, 36, 37, 38, 1000)))
        assert sizes == sorted(sizes)
        e.smooth_reserve(T)
        got = []
        for k, (lo, hi) in enumerate(windows):
            e.reset()
            got.append(e.tick_many_smooth(hi - lo, want_P=True, **kw_of(w, "rec", None, lo, hi)))
            if k == 0:
                e.smooth_reserve(0)      # freed: the next call allocates again
        e.smooth_reserve(0)
        e.smooth_reserve(3)
        e.reset()
        again = e.tick_many_smooth(T, want_P=True, **kw_of(w, "rec", None, *windows[0]))   # grows from 3 ticks
    for (lo, hi), (xs, Ps) in zip(windows, got):
        with Engine("kf6", N) as f:
            fx, fP = f.tick_many_smooth(hi - lo, want_P=True, **kw_of(w, "rec", None, lo, hi))
        assert np.array_equal(bits(fx), bits(xs)) and np.array_equal(bits(fP), bits(Ps)), (lo, hi)
    assert np.array_equal(bits(again[0]), bits(got[0][0])) and np.array_equal(bits(again[1]), bits(got[0][1]))


# ----------------------------------------------------------------------------- 8. errors
def raw_call(e, ti, n_ticks, stride, so):
    return fmskf.load().fmskf_tick_many_smooth(e.h, C.byref(ti) if ti is not None else None, n_ticks, stride,
                                               C.byref(so) if so is not None else None)


def test_errors_change_nothing(w):
    import torch
    kw = kw_of(w, "rec", None)
    st_ = torch.cuda.Stream()
    with warmed(w) as e, torch.cuda.stream(st_):
        e.set_stream(st_)   # a capture needs a stream
        s0 = snapshot(e)
        ti, keep = e._inputs(kw, T, N)
        ox = np.zeros((T, 6, N), np.float32)

        def out(**f):
            so = _lib.SmoothOut()
            so.mem, so.pitch, so.x = _lib.MEM_HOST, 0, ox.ctypes.data
            for k, v in f.items():
                setattr(so, k, v)
            return so

        assert raw_call(e, ti, T, N, None) == EINVAL
        assert raw_call(e, ti, T, N, out(x=None)) == EINVAL
        assert raw_call(e, ti, T, N, out(reserved=1)) == EINVAL
        assert raw_call(e, ti, T, N, out(pitch=N - 1)) == EINVAL
        assert raw_call(e, ti, T, N, out(mem=7)) == EINVAL
        assert raw_call(e, ti, 0, N, out()) == EINVAL
        # everything fmskf_tick_many refuses
        assert raw_call(e, None, T, N, out()) == EINVAL
        assert raw_call(e, ti, T, N - 1, out()) == EINVAL
        for bad in (dict(kw, yaw_deg=np.ascontiguousarray(w["yaw"][:T])),       # records and a plane
                    dict(yaw_deg=np.ascontiguousarray(w["yaw"][:T]))):          # planes missing
            with pytest.raises(fmskf.FmskfError) as ei:
                e.tick_many_smooth(T, **bad)
            assert ei.value.code == EINVAL
        # the workspace cannot be allocated: before any launch
        with pytest.raises(fmskf.FmskfError) as ei:
            e.smooth_reserve(2 ** 31)    # 108 B x 4113 x 2^31: ~1e15 bytes
        assert ei.value.code == ENOMEM
        same(s0, snapshot(e), "refused calls")
        # inside a graph capture
        dev = to_device(kw)
        dxs = torch.empty((T, 6, N), dtype=torch.float32, device="cuda")
        e.graph_begin()
        with pytest.raises(fmskf.FmskfError) as ei:
            e.tick_many_smooth(T, out_x=dxs, **dev)
        assert ei.value.code == EINVAL
        with pytest.raises(fmskf.FmskfError) as ei:
            e.smooth_reserve(T)
        assert ei.value.code == EINVAL
        e.predict()          # captured, never replayed
        e.graph_end()
        same(s0, snapshot(e), "refused in a capture")
        xs = e.tick_many_smooth(T, **kw)   # and the handle still works
        e.sync()
    with warmed(w) as c:
        assert np.array_equal(bits(c.tick_many_smooth(T, **kw)), bits(xs))


@pytest.mark.parametrize("model,flags,gate", [("rs", 0, False), ("ekf9", 0, False), ("kf12d", 0, False),
                                              ("kf6", fmskf.CFG_COMP_POS, False), ("kf6", 0, True)])
def test_unsupported_handles(w, model, flags, gate):
    n = 300
    kw = dict(kf6_rec=np.ascontiguousarray(w["rec"][:3, :n])) if model == "kf6" else \
        dict(yaw_deg=np.ascontiguousarray(w["yaw"][:3, :n]), rpm=np.ascontiguousarray(w["rpm"][:3, :n]))
    with Engine(model, n, flags=flags) as e:
        if gate:
            e.set_gate(25.0, 3)
        if model == "kf6":
            e.tick(kf6_rec=kw["kf6_rec"][0])
        x, P = e.get_state()
        s0 = [x] + ([P] if P is not None else []) + [np.array(e.get_counters(), np.uint64)]
        if gate:
            s0 += list(e.get_gate().values())
        for call in (lambda: e.tick_many_smooth(3, **kw), lambda: e.smooth_workspace_bytes(3),
                     lambda: e.smooth_reserve(3)):
            with pytest.raises(fmskf.FmskfError) as ei:
                call()
            assert ei.value.code == ENOTSUP
        x, P = e.get_state()
        s1 = [x] + ([P] if P is not None else []) + [np.array(e.get_counters(), np.uint64)]
        if gate:
            s1 += list(e.get_gate().values())
        same(s0, s1, model)
