"""Non-default dt, Q, R and P0 (tests/param_cases.py) on the CPU: the oracle -- the operation order
the kernels share -- against the independent dense fp64 filter (oracle/kf_ref.py) for every named
case, so that an algorithmic error the kernel and the oracle have in common (a wrong packed index,
a dropped Q or R term) shows where the defaults are zero; the AVX port against the oracle; and the
reference helpers' new optional-parameter paths against their old ones.

Recipe (as tests/test_oracle_kf_fp64.py, its grouping and its bounds): T = 300 ticks, n = 8 robots,
z from the fp32 frontend, of a trajectory sampled at the case's own dt.  (A 2.5 ms filter fed 1 ms
data has a biased innovation; the fp32 rounding of the small position-heading covariances that a
dense P0 leaves then adds up in the unobserved positions instead of averaging out, 3e-5 .. 3e-4 on
KF6: an fp32 conditioning effect of the mismatch, not of the parameters.)

Bounds.  KF6 and EKF9: the project's 1e-5; the parameter seeds (param_cases.SEEDS) are chosen so that
this reference pair stays inside it.  KF12D: 1e-12 where Q, R, P0 keep the default structure; the
dense cases 1e-10 (measured 1e-12 .. 1.2e-11 over 16 draws: the dense filter and the packed
sequential one differ in operation order only, an indexing error shows at 1e-3 or more), the bound
test_kf12d_oracle_vs_dense already grants its ill-conditioned R.  The trajectory seeds (TRAJ_SEED)
are test_oracle_kf_fp64.py's; the measured figures of every case are printed.  Measured (x86-64):
KF6 3.7e-7 .. 2.4e-6 (state) and 3.3e-7 .. 7.8e-6 (P, the largest at dt 10 ms); EKF9 5.9e-7 .. 3.6e-6
and 5.9e-8 .. 4.4e-6; KF12D default structure 5.0e-14 .. 2.5e-13, dense 3.5e-13 .. 1.7e-11."""
import numpy as np
import pytest

import fmskf
from fmskf.synth import Trajectory
from oracle import kf_ref

import gate_ref
import param_cases as pc
import seq_ref
from test_oracle_kf_fp64 import GROUPS, _check  # the project's 1e-5 (TOL) is _check's

T, N = 300, 8
TRAJ_SEED = {"kf6": 11, "ekf9": 12, "kf12d": 13}  # test_oracle_kf_fp64.py's


def _figures(x32, P32, x64, P64):
    """the two figures _check bounds: the largest grouped state error and covariance error"""
    ex = 0.0
    for grp in GROUPS[x64.shape[0]]:
        scale = max(np.abs(x64[list(grp)]).max(), 1e-30)
        ex = max(ex, max(np.abs(x32[k] - x64[k]).max() / scale for k in grp))
    return ex, (np.abs(P32 - P64).max(axis=0) / np.abs(P64).max(axis=0)).max()


@pytest.mark.parametrize("name", pc.CASES["kf6"])
def test_kf6_oracle_vs_dense(orc, name):
    prm = pc.case("kf6", name)
    yaw, gz, rpm = Trajectory(N, T, seed=TRAJ_SEED["kf6"], dt=prm.dt).kf6_inputs()
    op = pc.orc_params(orc, prm)
    x, P = pc.fresh(prm, N)
    valid = (np.arange(T) % 7 != 3).astype(np.uint8)  # some ticks without measurement
    zs = []
    for t in range(T):
        zs.append(orc.kf6_measure(yaw[t], gz[t], rpm[t], orc.TRIG_TABLE512))
        orc.kf6_tick(x, P, yaw[t], gz[t], rpm[t], np.full(N, valid[t], np.uint8), op)
    zs = np.stack(zs)
    q, r, p0 = (a.astype(np.float64) for a in (prm.q, prm.r, prm.p0))
    res = [kf_ref.kf6_run(np.zeros(6), p0, zs[:, :, i].astype(np.float64), q, r, float(np.float32(prm.dt)),
                          valid=valid)[-1] for i in range(N)]
    x64, P64 = np.stack([a for a, _ in res], 1), np.stack([b for _, b in res], 1)
    print(f"kf6 {name}: state {_figures(x, P, x64, P64)[0]:.2e}, P {_figures(x, P, x64, P64)[1]:.2e}")
    _check(x, P, x64, P64)


@pytest.mark.parametrize("name", pc.CASES["ekf9"])
def test_ekf9_oracle_vs_dense(orc, name):
    prm = pc.case("ekf9", name)
    raw = Trajectory(N, T, seed=TRAJ_SEED["ekf9"], dt=prm.dt).ekf9_raw()
    op = pc.orc_params(orc, prm, orc.TRIG_LIBM)
    x, P = pc.fresh(prm, N)
    zs = []
    for t in range(T):
        zs.append(orc.ekf9_measure(raw[t]))
        orc.ekf9_tick(x, P, raw[t], None, op)
    zs = np.stack(zs)
    q, r, p0 = (a.astype(np.float64) for a in (prm.q, prm.r, prm.p0))
    res = [kf_ref.ekf9_run(np.zeros(9), p0, zs[:, :, i].astype(np.float64), q, r, float(np.float32(prm.dt)))[-1]
           for i in range(N)]
    x64, P64 = np.stack([a for a, _ in res], 1), np.stack([b for _, b in res], 1)
    print(f"ekf9 {name}: state {_figures(x[:9], P, x64, P64)[0]:.2e}, P {_figures(x[:9], P, x64, P64)[1]:.2e}")
    _check(x[:9], P, x64, P64)


KF12D_DENSE = ("q_dense", "r_dense", "p0_dense", "all_dense", "all_dense_dt", "q_dense_r_indefinite",
               "q_dense_r_semidefinite")


@pytest.mark.parametrize("name", pc.CASES["kf12d"])
def test_kf12d_oracle_vs_dense(orc, name):
    tol = 1e-10 if name in KF12D_DENSE else 1e-12
    prm = pc.case("kf12d", name)
    assert pc.kf12d_path(orc, prm) == pc.PATHS[name]
    z = Trajectory(N, T, seed=TRAJ_SEED["kf12d"], dt=prm.dt).kf12d_z()
    op = pc.orc_params(orc, prm)
    x, P = pc.fresh(prm, N)
    for t in range(T):
        orc.kf12d_tick(x, P, np.ascontiguousarray(z[t]), None, op)
    worst_x = worst_p = 0.0
    for i in range(N):
        x64, P64 = kf_ref.kf12d_run(np.zeros(12), prm.p0, z[:, :, i], prm.q, prm.r, prm.dt)[-1]
        worst_x = max(worst_x, max(np.abs(x[k, i] - x64[k]) / max(np.abs(x64[k]), 1e-3) for k in range(12)))
        worst_p = max(worst_p, np.abs(P[:, i] - P64).max() / np.abs(P64).max())
    print(f"kf12d {name} [{pc.PATHS[name]}]: state {worst_x:.2e}, P {worst_p:.2e}, bound {tol:g}")
    assert worst_x <= tol and worst_p <= tol, (worst_x, worst_p)


def test_kf12d_paths(orc):
    """every KF12D case reaches the instantiation it names, all five are reached, and the R terms
    restated in param_cases are test_gpu_parity's"""
    import test_gpu_parity as tp
    assert pc.KF12D_R_INDEFINITE == tp.KF12D_R_CASES["cross_R_indefinite_joint"]
    assert pc.KF12D_R_SEMIDEFINITE == tp.KF12D_R_CASES["blockdiag_R_semidefinite_groups"]
    assert set(pc.PATHS) == set(pc.CASES["kf12d"])
    for name in pc.CASES["kf12d"]:
        prm = pc.case("kf12d", name)
        assert pc.kf12d_path(orc, prm) == pc.PATHS[name], name
        pd = bool(orc.kf12d_cinv(prm.r)[0])
        assert pd == (not pc.PATHS[name].startswith("k_kf12d")), name
    assert set(pc.PATHS.values()) == {"SP", "BLK && !SP", "!BLK", "k_kf12d SEQ", "k_kf12d joint"}
    assert pc.kf12d_path(orc, pc.default_params("kf12d")) == "SP"
    # the two block cases are what they say: block-diagonal, positive definite, not default-sparse
    for name in ("blk_r", "blk_q"):
        prm = pc.case("kf12d", name)
        ok, cinv = orc.kf12d_cinv(prm.r)
        assert ok and pc.kf12d_sequential(prm.r) and not pc.kf12d_sparse(cinv, prm.q)


@pytest.mark.parametrize("model", list(pc.DIMS))
def test_dense_cases_are_dense_and_positive_definite(model):
    nx, m, dtype = pc.DIMS[model]
    base = pc.default_params(model)
    prm = pc.case(model, "all_dense_dt")
    assert prm.dt == 2.5e-3
    for a, b, n in ((prm.q, base.q, nx), (prm.r, base.r, m), (prm.p0, base.p0, nx)):
        assert a.dtype == dtype and np.all(a != 0)
        M = pc.unpack(a.astype(np.float64), n)
        assert np.linalg.eigvalsh(M).min() > 0
        np.testing.assert_allclose(np.diag(M), np.diag(pc.unpack(b.astype(np.float64), n)), rtol=1e-6)
        assert len(set(np.abs(a).tolist())) > len(a) - n  # the entries differ from one another
    for name, (dt, dq, dr, dp) in pc._COMMON.items():
        c = pc.case(model, name)
        assert c.dt == dt
        for got, dflt, is_dense in ((c.q, base.q, dq), (c.r, base.r, dr), (c.p0, base.p0, dp)):
            assert np.array_equal(got, dflt) != is_dense, (name, is_dense)


def test_port_kf6_all_dense_dt_bit_exact(orc):
    """oracle/cpu_port.c (the tuned AVX KF6 tick) against orc.kf6_tick with dt, Q, R and P0 all
    non-default: bit for bit"""
    n, Tp = 1037, 40
    prm = pc.case("kf6", "all_dense_dt")
    yaw, gz, rpm = Trajectory(n, Tp, seed=5).kf6_inputs()
    op = pc.orc_params(orc, prm)
    xa, Pa = pc.fresh(prm, n)
    xb, Pb = pc.fresh(prm, n)
    for t in range(Tp):
        orc.kf6_tick(xa, Pa, yaw[t], gz[t], rpm[t], None, op)
        orc.port_kf6_tick(xb, Pb, yaw[t], gz[t], rpm[t], op)
    assert np.array_equal(xa.view(np.uint32), xb.view(np.uint32))
    assert np.array_equal(Pa.view(np.uint32), Pb.view(np.uint32))
    assert np.all(Pa != 0)


# ----------------------------------------------------------------------------- helper defaults
def _struct_bytes(s):
    import ctypes
    return bytes((ctypes.c_char * ctypes.sizeof(s)).from_buffer_copy(s))


def test_helper_defaults_unchanged(orc):
    """each helper's optional-parameter path, called with the default parameters, returns exactly
    what the path without them returns"""
    import test_gpu_parity as tp
    n = 5
    d = pc.default_params("kf6")
    for trig in (fmskf.TRIG_TABLE512, fmskf.TRIG_LIBM):
        assert _struct_bytes(gate_ref.params(orc, n, trig)) == _struct_bytes(gate_ref.params(orc, n, trig, prm=d))
    assert np.array_equal(gate_ref.r_packed(), gate_ref.r_packed(prm=d))
    for a, b in zip(gate_ref.fresh(n), gate_ref.fresh(n, prm=d)):
        assert a.dtype == b.dtype and np.array_equal(a, b)
    yaw, gz, rpm = Trajectory(n, 6, seed=3).kf6_inputs()
    x, P = gate_ref.fresh(n)
    prm = gate_ref.params(orc, n)
    for t in range(5):
        orc.kf6_tick(x, P, yaw[t], gz[t], rpm[t], None, prm)
    a = gate_ref.nis_f64(orc, x, P, yaw[5], gz[5], rpm[5])
    b = gate_ref.nis_f64(orc, x, P, yaw[5], gz[5], rpm[5], prm=d)
    assert np.array_equal(a, b) and np.all(a > 0)
    xa, Pa = tp._kf6_oracle(orc, n, yaw, gz, rpm, None, orc.TRIG_TABLE512, 6)
    xb, Pb = tp._kf6_oracle(orc, n, yaw, gz, rpm, None, orc.TRIG_TABLE512, 6, params=d)
    assert np.array_equal(xa.view(np.uint32), xb.view(np.uint32))
    assert np.array_equal(Pa.view(np.uint32), Pb.view(np.uint32))
    # a non-default set does change them (the argument is not ignored)
    nd = pc.case("kf6", "all_dense_dt")
    assert not np.array_equal(gate_ref.r_packed(), gate_ref.r_packed(prm=nd))
    assert not np.array_equal(gate_ref.fresh(n)[1], gate_ref.fresh(n, prm=nd)[1])
    xc, _ = tp._kf6_oracle(orc, n, yaw, gz, rpm, None, orc.TRIG_TABLE512, 6, params=nd)
    assert not np.array_equal(xa, xc)


@pytest.mark.parametrize("model", ["kf6", "ekf9", "rs"])
def test_fleet_defaults_unchanged(orc, model):
    """seq_ref.Fleet with the default parameter set is the Fleet without one, op by op"""
    n = 7
    ops = ["fused", "split", "three", "set_target", "fused", "predict_only", "correct_only", "control_rpm", "reset",
           "fused", "fused"]
    inp = seq_ref.Inputs(model, n, seq_ref.ticks_needed(ops), 3)
    d = pc.default_params(model)
    a, b = seq_ref.Fleet(orc, model, n, inp), seq_ref.Fleet(orc, model, n, inp, prm=d)
    for f in (a, b):
        f.start()
    for op in ops:
        fa, fb = a.apply(op), b.apply(op)
        assert (fa is None) == (fb is None)
        if fa is not None:
            assert np.array_equal(fa, fb), op
        for u, v in zip(a.state(), b.state()):
            assert (u is None and v is None) or np.array_equal(u.view(np.uint32), v.view(np.uint32)), op
    for k, v in a.motors().items():
        assert np.array_equal(v, b.motors()[k]), k
    for k, v in a.ctrl().items():
        assert np.array_equal(v, b.ctrl()[k]), k
    # and the directions are not ignored
    c, e = seq_ref.Fleet(orc, model, n, inp, prm=d._replace(motor_dir=(1, -1, 1, -1))), seq_ref.Fleet(orc, model, n, inp)
    for f in (c, e):
        f.start()
        for op in ops[:3]:
            f.apply(op)
    assert not np.array_equal(c.motors()["rpm"], e.motors()["rpm"])


# ----------------------------------------------------------------------------- the gate runs
@pytest.mark.parametrize("case", list(pc.GATE_SEED))
def test_gate_runs_meet_the_band_cap_on_the_cpu(orc, case):
    """the gated fleets of test_gpu_params.test_gate_with_dense_r through the oracle, NIS and
    decision in float64 (gate_ref.nis_f64 / decide): the 1e-3 band around nis_max holds at most
    0.1 % of the robot-ticks, and accepted, rejected, forced and skipped measurements all occur"""
    n, T, maxc = pc.GATE_N, pc.GATE_T, pc.GATE_MAXC
    prm = pc.case("kf6", case)
    yaw, gz, rpm, _ = gate_ref.gate_inputs(n, T, seed=pc.GATE_SEED[case], start=pc.GATE_START)
    valid = pc.gate_valid()
    op = gate_ref.params(orc, n, prm=prm)
    x, P = gate_ref.fresh(n, prm=prm)
    run = np.zeros(n, np.uint8)
    in_band, seen = 0, set()
    for t in range(T):
        nis = gate_ref.nis_f64(orc, x, P, yaw[t], gz[t], rpm[t], prm=prm)
        has = valid[t] != 0
        status, run_new, rejected = gate_ref.decide(nis, run, gate_ref.NIS_MAX, maxc)
        forced = run >= maxc
        in_band += int(np.count_nonzero(has & ~forced & (np.abs(nis - gate_ref.NIS_MAX) <= gate_ref.BAND * gate_ref.NIS_MAX)))
        seen.update(np.unique(np.where(has, status, fmskf.GATE_NONE)).tolist())
        run = np.where(has, run_new, run)
        orc.kf6_tick(x, P, yaw[t], gz[t], np.ascontiguousarray(rpm[t]), (has & ~rejected).astype(np.uint8), op)
    print(f"gate {case}: {in_band} of {n * T} robot-ticks in the band")
    assert in_band <= 1e-3 * n * T
    assert seen == {fmskf.GATE_NONE, fmskf.GATE_ACCEPTED, fmskf.GATE_REJECTED, fmskf.GATE_FORCED}
