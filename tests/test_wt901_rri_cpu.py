"""WT901 register replies at read-register indices other than Q0 (CPU).

tests/golden/wt901_rri_ref.npz (tests/golden/make_golden_wt901_rri.py) holds what the reference's
own lib/wt901c/wit_c_sdk.c, compiled unmodified, answered at 30 indices over streams of the ten
poll kinds of tests/wt901_rri.py.  Here the oracle replays it, and the coverage conditions are
asserted on the fixture and on the sequences tests/test_gpu_wt901_rri.py runs on the device, so
that a reshuffle of the generator cannot silently empty those tests.
"""
import ctypes as C
import os

import numpy as np
import pytest

import wt901_rri as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "wt901_rri_ref.npz")


@pytest.fixture(scope="module")
def streams():
    return W.load_fixture(FIXTURE)


def test_fixture_shape(streams):
    assert os.path.getsize(FIXTURE) < 256 * 1024
    assert sorted({s["rri"] for s in streams}) == sorted(W.RRIS) and len(W.RRIS) == 30
    want = set(range(0x2B, 0x2F)) | set(range(0x31, 0x41)) | set(range(0x4E, 0x55)) | {0x00, 0x41, 0x8C}
    assert set(W.RRIS) == want
    for s in streams:
        assert len(s["polls"]) >= 10 and max(len(p) for p in s["polls"]) <= W.MAX_POLL
        assert [k for k, v in enumerate(s["latch"]) if v] == list(W.LATCH)
        assert all(r.shape == (0x90,) for r in s["regs"])
    assert {k for s in streams for k in s["kinds"]} == set(W.KINDS)


def test_oracle_replays_fixture(orc, streams):
    """registers, pending bytes and callbacks after every poll, through orc.Wt901.update (the
    latch included: it empties the parser window before the poll's bytes)"""
    for s in streams:
        w = orc.Wt901(s["rri"])
        for k, p in enumerate(s["polls"]):
            w.update(p, latch_qinit=s["latch"][k])
            msg = f"index {s['rri']:#x} poll {k} ({s['kinds'][k]})"
            np.testing.assert_array_equal(w.regs, s["regs"][k], err_msg=msg)
            assert len(w.parser) == s["pending"][k], msg
            assert w.take_cb() == s["cbs"][k], msg


def test_oracle_batch_replays_fixture(orc, streams):
    """the same through Wt901Batch and its regs / pending views (what the GPU tests compare with)"""
    for fl in W.fixture_fleets(streams):
        wb = orc.Wt901Batch(fl.n, fl.rri)
        for k in range(fl.npolls):
            wb.update(*fl.rows(k), latch_qinit=k in fl.latch)
            np.testing.assert_array_equal(wb.regs, np.stack([s["regs"][k] for s in fl.streams], axis=1))
            np.testing.assert_array_equal(wb.pending, [s["pending"][k] for s in fl.streams])
            cnt, reg, num = wb.take_cb()
            for i, s in enumerate(fl.streams):
                assert list(zip(reg[i, :cnt[i]].tolist(), num[i, :cnt[i]].tolist())) == s["cbs"][k]


def test_reference_sdk_reproduces_fixture_when_present(orc, streams, tmp_path):
    """where the reference's build exists: its SDK gives the fixture's registers and callbacks, and
    the generator writes the committed file again byte for byte"""
    if not os.path.exists(orc.REF_PATH):
        pytest.skip("oracle/_ref not built (the reference is not here)")
    for s in streams:
        ref = orc.RefWt901(s["rri"])
        for k, p in enumerate(s["polls"]):
            if s["latch"][k]:
                ref.latch()
            ref.feed(p)
            np.testing.assert_array_equal(ref.regs(), s["regs"][k])
            assert ref.take_cb() == s["cbs"][k]
    import importlib.util
    spec = importlib.util.spec_from_file_location(
        "make_golden_wt901_rri", os.path.join(ROOT, "tests", "golden", "make_golden_wt901_rri.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    out = tmp_path / "again.npz"
    gen.main(str(out))
    assert out.read_bytes() == open(FIXTURE, "rb").read()


def test_coverage_of_fixture(orc, streams):
    c = W.coverage(orc, W.fixture_fleets(streams))
    print("fixture", c)
    W.assert_coverage(c)


@pytest.mark.parametrize("stride", [48, 64])
def test_coverage_of_device_sequences(orc, stride):
    """the sequences of the GPU tests at the two strides the vector kernel takes (only it keeps
    registers in the snapshot row); at 48 the 55-byte S+R poll is clipped and loses its reply"""
    fls = [W.fleet(rri) for rri in W.RRIS]
    for fl in fls:
        assert fl.n == 293 and fl.npolls == 10 and fl.latch == (2, 6)
    c = W.coverage(orc, fls, stride)
    print("stride", stride, c)
    W.assert_coverage(c)


def test_create_checks_imu_read_reg():
    """a reply writes four words at imu_read_reg: 0x8C is the last index inside sReg[0x90]"""
    import fmskf
    lib = fmskf.load()
    cfg = fmskf.default_config("rs", 4)
    cfg.imu_read_reg = 0x8D
    h = C.c_void_p()
    assert lib.fmskf_create(C.byref(cfg), C.byref(h)) == fmskf._lib.EINVAL
    assert b"imu_read_reg" in lib.fmskf_last_error() and not h.value
    cfg.imu_read_reg = 0x8C
    rc = lib.fmskf_create(C.byref(cfg), C.byref(h))
    # accepted: the handle, or (no GPU here) the device error that comes after the argument checks
    assert rc in (fmskf._lib.OK, fmskf._lib.EDEVICE), (rc, lib.fmskf_last_error())
    if rc == fmskf._lib.OK:
        assert lib.fmskf_destroy(h) == fmskf._lib.OK
