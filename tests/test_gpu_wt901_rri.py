"""k_wt901 and register replies (0x5F frames) at read-register indices other than Q0 (GPU).

Since the standard poll keeps thirteen of its registers in the snapshot row and the imu_yg dword
only (F_ROWREGS), the one frame that can write an arbitrary register run is the reply, four
words at imu_read_reg.  Every test here runs one Engine per index of tests/wt901_rri.py (30 of
them) with n = 293 robots, one full block and a ragged 37, each robot on its own 10-poll
sequence of that module's ten poll kinds, polls 2 and 6 latching, and compares bit for bit with
the oracle (or the reference SDK's fixture) -- which tests/test_wt901_rri_cpu.py pins to the
reference, together with the counts of what these sequences contain.
"""
import os

import numpy as np
import pytest

import fmskf
from fmskf import Engine
import wt901_rri as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = W.N_ROBOTS


def bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    u = a.view(np.uint8), b.view(np.uint8)
    if not np.array_equal(*u):
        bad = np.argwhere(a.view(f"u{a.dtype.itemsize}") != b.view(f"u{a.dtype.itemsize}"))
        raise AssertionError(f"{what}: {len(bad)} words differ, first at {bad[0].tolist()}: "
                             f"{a[tuple(bad[0])]!r} != {b[tuple(bad[0])]!r}")


def check_all(e, wb, what):
    """registers, pending bytes, Data page and is_error against the oracle"""
    regs, pend = e.get_imu_regs()
    data, err = e.get_imu()
    bits(regs, wb.regs, what + " regs")
    bits(pend, wb.pending.astype(np.uint8), what + " pending")
    bits(data, wb.data, what + " data")
    bits(err, wb.is_error, what + " is_error")


def check_page(e, wb, what):
    data, err = e.get_imu()
    bits(data, wb.data, what + " data")
    bits(err, wb.is_error, what + " is_error")


# ---------------------------------------------------------------------------- fixture replay
@pytest.mark.parametrize("stride,readout", [(64, "every"), (64, "last"), (80, "every")])
def test_fixture_replay(stride, readout):
    """The reference SDK's streams (tests/golden/wt901_rri_ref.npz) on the device, robot i on
    stream i mod S: the register file and the pending count equal the fixture's after every poll.
    64: the vector kernel; 80: the byte kernel.  "last": read only after the last poll, so the
    replies meet row-resident registers (a readout after every poll clears the residency)."""
    fleets = W.fixture_fleets(W.load_fixture(os.path.join(ROOT, "tests", "golden", "wt901_rri_ref.npz")))
    assert [fl.rri for fl in fleets] == sorted(W.RRIS)
    for fl in fleets:
        pick = np.arange(N) % fl.n
        with Engine("rs", N, imu_read_reg=fl.rri) as e:
            for k in range(fl.npolls):
                buf, lens = fl.rows(k, stride)
                e.ingest_wt901(buf[pick], lens[pick], latch_qinit=k in fl.latch)
                if readout == "last" and k < fl.npolls - 1:
                    continue
                regs, pend = e.get_imu_regs()
                want = np.stack([s["regs"][k] for s in fl.streams], axis=1)[:, pick]
                bits(regs, np.ascontiguousarray(want), f"index {fl.rri:#x} poll {k} regs")
                bits(pend, np.array([s["pending"][k] for s in fl.streams], np.uint8)[pick],
                     f"index {fl.rri:#x} poll {k} pending")


# ---------------------------------------------------------------------------- row strides
@pytest.mark.parametrize("stride", [48, 64, 80, "48+4"])
def test_strides_read_every_poll(orc, stride):
    """Schedule (a): registers, Data page and is_error read after every poll, so residency is
    cleared each time.  48 and 64: the vector kernel (64 holds the 55-byte S+R poll whole); 80:
    the byte kernel; "48+4": device-resident rows of stride 48 whose base sits 4 bytes past a
    16-byte boundary, which launch_wt901 must hand to the byte kernel -- the oracle sees the same
    clipped polls as at 48, so the results are those of 48."""
    offset = stride == "48+4"
    st = 48 if offset else stride
    if offset:
        import torch
    for rri in W.RRIS:
        fl = W.fleet(rri)
        wb = orc.Wt901Batch(N, rri)
        with Engine("rs", N, imu_read_reg=rri) as e:
            if offset:
                e.set_stream(torch.cuda.current_stream())
            for k in range(fl.npolls):
                buf, lens = fl.rows(k, st)
                if offset:
                    raw = torch.zeros(N * st + 32, dtype=torch.uint8, device="cuda")
                    rows = raw[4:4 + N * st].view(N, st)
                    rows.copy_(torch.from_numpy(buf))
                    assert rows.data_ptr() % 16 == 4 and rows.is_contiguous()
                    dl = torch.from_numpy(lens.astype(np.int32)).cuda()
                    e.ingest_wt901(rows, dl, latch_qinit=k in fl.latch)
                else:
                    e.ingest_wt901(buf, lens, latch_qinit=k in fl.latch)
                wb.update(buf, lens, latch_qinit=k in fl.latch)
                check_all(e, wb, f"index {rri:#x} poll {k}")


# ---------------------------------------------------------------------------- readout schedules
@pytest.mark.parametrize("stride", [48, 64])
@pytest.mark.parametrize("schedule", ["b", "c"])
def test_residency_survives_polls(orc, tmp_path, schedule, stride):
    """Schedules (b) and (c) on the polls of (a): only fmskf_get_imu after every poll, the register
    file once at the end, so a reply meets registers that a standard poll left in the snapshot
    row; (c) also checkpoints after poll 4 (fmskf_save_state clears the residency) and goes on in
    a fresh handle of the same index."""
    for rri in W.RRIS:
        fl = W.fleet(rri)
        wb = orc.Wt901Batch(N, rri)
        e = Engine("rs", N, imu_read_reg=rri)
        try:
            for k in range(fl.npolls):
                buf, lens = fl.rows(k, stride)
                e.ingest_wt901(buf, lens, latch_qinit=k in fl.latch)
                wb.update(buf, lens, latch_qinit=k in fl.latch)
                check_page(e, wb, f"index {rri:#x} poll {k}")
                if schedule == "c" and k == 4:
                    path = tmp_path / f"ck_{rri:02x}.bin"
                    e.save_state(path)
                    e.close()
                    e = Engine("rs", N, imu_read_reg=rri)
                    e.load_state(path)
                    os.unlink(path)
                    check_page(e, wb, f"index {rri:#x} after the checkpoint")
            check_all(e, wb, f"index {rri:#x} at the end")
        finally:
            e.close()


# ---------------------------------------------------------------------------- consumers
@pytest.mark.parametrize("stride", [48, 64])
def test_consumers_follow_the_page(orc, stride):
    """What reads the snapshot without the register file.  After every poll an RS handle's
    correct() with a NULL yaw plane gives theta = deg2rad(Data.angle[2]) (VD_task_main.cpp:368),
    and a KF6 handle's tick with NULL yaw and gyro planes and the caller's rpm gives the x and P
    of orc.kf6_tick fed the oracle page's angle[2] and gyro[2]; at the end VehicleInfo's IMU
    fields are the page's."""
    deg2rad = np.float32(np.float32(3.14159265358979) / np.float32(180.0))  # util_mymath.hpp:14
    cfg = fmskf.default_config("kf6", N)
    prm = orc.kf6_params(cfg.dt, np.array(cfg.q[:21]), np.array(cfg.r[:10]), orc.TRIG_TABLE512)
    p0 = np.float32(np.array(cfg.p0[:21]))
    for rri in W.RRIS:
        fl = W.fleet(rri)
        wb = orc.Wt901Batch(N, rri)
        rng = np.random.default_rng([7, rri])
        x = np.zeros((6, N), np.float32)
        P = np.repeat(p0[:, None], N, 1).copy()
        with Engine("rs", N, imu_read_reg=rri) as rs, Engine("kf6", N, imu_read_reg=rri) as kf:
            for k in range(fl.npolls):
                buf, lens = fl.rows(k, stride)
                what = f"index {rri:#x} poll {k}"
                wb.update(buf, lens, latch_qinit=k in fl.latch)
                page = wb.data
                rs.ingest_wt901(buf, lens, latch_qinit=k in fl.latch)
                rs.correct()
                bits(rs.get_pose()[2], page[11] * deg2rad, what + " theta")
                rpm = rng.integers(-3000, 3000, (N, 4)).astype(np.int16)
                kf.ingest_wt901(buf, lens, latch_qinit=k in fl.latch)
                kf.tick(rpm=rpm)
                orc.kf6_tick(x, P, np.ascontiguousarray(page[11]), np.ascontiguousarray(page[5]), rpm, None,
                             prm, nthreads=0)
                xg, Pg = kf.get_state()
                bits(xg, x, what + " kf6 x")
                bits(Pg, P, what + " kf6 P")
            vi = kf.export_vehicle_info()
            page, err = wb.data, wb.is_error.astype(bool)
            what = f"index {rri:#x} VehicleInfo"
            assert np.all(vi["imu_fault"][err] == 0xFF) and not np.any(vi["imu_q"][err]), what
            good = ~err
            bits(vi["imu_q"][good], np.ascontiguousarray(page[12:16].T[good]), what + " q")
            bits(vi["imu_g"][good], np.ascontiguousarray(page[3:6].T[good]), what + " g")
            bits(vi["imu_a"][good], np.ascontiguousarray(page[0:3].T[good]), what + " a")
