"""The non-finite guard (fmskf_get_counters [0]) and lane isolation of every tick kernel.

Every test runs a handle `e` that is fed poison (a NaN / +Inf / -Inf planted in one element of x or P
through set_state, or a NaN / Inf input) next to a twin `c` with the same calls and no poison, and
after every launch checks
 1. counters[0] rose by exactly the number of robots whose stored state is not finite
    (nonfinite_ref.bad_robots of get_state(): what the launch stored is what it must have counted),
    once per launch whatever its tick count, and the twin's stayed 0;
 2. that set is the planted one, and every robot outside it equals the twin bit for bit in x, P and
    the hidden low parts.  Inside the set the data flow of the linear models (KF6, KF12D) keeps P
    apart from x: the update forms U, D^-1 and P -= U^T D^-1 U from P and R alone (kf_update_factor
    / kf_update_apply, kf_update_seq, kf12d_decor_update), the predict forms P from P and Q, and the
    innovation -- with it x and every input -- enters w and x only.  So after every ungated KF6 and
    KF12D launch a robot whose poison sits in x, or whose only fault is a bad input, must keep the
    twin's P bit for bit, with FMSKF_CFG_COMP_POS the low parts of P00, P10, P11 too (their slots
    are separate from those of px, py).  Only the gated handles (whether an update is applied
    depends on the NIS / d2, which x enters) and EKF9 (its Jacobian comes from x) mix the two: there
    the mask alone is asserted inside the set.
 3. for the plain KF6 and EKF9 handles, select(nonfinite=True) returns the same set.

Shapes (nonfinite_ref.SIZES): one lane; 257, where lane 0 of the two-per-lane KF6 / EKF9 kernels
serves robots 0 and 256 and every other lane's second robot is dead beside a bad last robot; ragged
rows of blocks and tiles.  Patterns (nonfinite_ref.plant_set): the wave and block edges with a whole
wave and a lane pair, the last robot alone (which every lane past N loads through its clamped
index), a seeded 30 %, and none.  The finite values stay below nonfinite_ref.FINITE_MAX, so the
guard's sum cannot overflow (see there)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import fmskf
from fmskf import Engine
from fmskf.synth import Trajectory

import nonfinite_ref as nf
import param_cases as pc

pytestmark = pytest.mark.gpu

COMP = fmskf.CFG_COMP_POS
ACC, REJ = fmskf.GATE_ACCEPTED, fmskf.GATE_REJECTED
WARM = 3   # clean ticks before the first plant: P and the low parts are no longer their start values
T_IN = 8   # ticks of inputs, cycled
CASES = [(m, n, p) for m in nf.DIMS for n in nf.SIZES[m] for p in nf.PATTERNS]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


_INPUTS = {}


def inputs(model, n):
    """T_IN ticks of one model's inputs, computed once per (model, n) and never written"""
    if (model, n) not in _INPUTS:
        tr = Trajectory(n, T_IN, seed=17)
        yaw, gz, rpm = tr.kf6_inputs()
        d = dict(tr=tr, rpm=rpm)
        if model == "kf6":
            d.update(yaw=yaw, gz=gz)
        elif model == "rs":
            d.update(yaw=yaw, sums=tr.rs_inputs()[1])
        elif model == "ekf9":
            d.update(raw=tr.ekf9_raw())
        else:
            d.update(z=np.ascontiguousarray(tr.kf12d_z()))
        for v in d.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _INPUTS[(model, n)] = d
    return _INPUTS[(model, n)]


def input_sets(n):
    """(J, J2): the robots whose inputs are poisoned, and those poisoned under valid == 0: fixed sets
    at the wave and block edges with the fleet's last robots.  Which of J2 are still clean depends on
    the pattern (all of them under `none` and, but for N - 1, under `last_only`): a clean one must
    stay the twin's, a bad one must not be counted twice."""
    J = np.array(sorted({k for k in (2, 65, 254, n - 2, n - 1) if 0 <= k < n}), np.int64)
    J2 = np.array(sorted({k for k in (0, 5, 66, 255, 256, n - 1) if 0 <= k < n}), np.int64)
    return J, J2


class Twin:
    """the poisoned handle e and its clean twin c, and the checks after every launch"""

    def __init__(self, model, n, flags=0, gate=None, **kw):
        self.model, self.n, self.flags, self.gate = model, n, flags, gate
        self.e, self.c = Engine(model, n, flags=flags, **kw), Engine(model, n, flags=flags, **kw)
        self.inp = inputs(model, n)
        self.t = 0
        self.cnt = 0
        self.planted = np.zeros(0, np.int64)
        self.tainted = np.zeros(0, np.int64)  # robots that had a bad input: they left the twin, bad or not
        # robots of the bad set whose P (and P low parts) must still be the twin's: the linear models
        # without a gate (module docstring, 2.)
        self.p_kept = np.zeros(0, np.int64)
        self.linear = model in ("kf6", "kf12d") and gate is None
        self.has_p = model != "rs"
        self.set_gates()
        for _ in range(WARM):
            self.launch("tick")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.e.close()
        self.c.close()

    def set_gates(self):
        """(gated handles) the gate off and on again: a zero gate state on both handles"""
        for h in (self.e, self.c):
            if self.gate is not None and self.model == "kf6":
                h.set_gate(None)
                h.set_gate(*self.gate)
            elif self.gate is not None:
                h.set_row_gate(None)
                h.set_row_gate(*self.gate)

    # ---------------------------------------------------------------- inputs
    def kw(self, t, form="planes", poison=None, valid=None, isr=False, can=False):
        """the keyword inputs of tick t; poison: robots whose float inputs are bad (a NaN yaw / z for
        the even ones, a +-Inf gyro / NaN z for the odd ones)"""
        m, d = self.model, self.inp
        t %= T_IN
        if m == "ekf9":
            out = dict(raw=d["raw"][t])
            if isr and not can:
                out["rpm"] = d["rpm"][t]
        elif m == "kf12d":
            z = d["z"][t]
            if poison is not None and len(poison):
                z = z.copy()
                for i in poison:
                    z[i % 8, i] = np.nan
            out = dict(z=z)
            if isr and not can:
                out["rpm"] = d["rpm"][t]
        else:
            yaw, g2 = d["yaw"][t], d.get("gz")
            gz = g2[t] if g2 is not None else None
            if poison is not None and len(poison):
                yaw = yaw.copy()
                gz = gz.copy() if gz is not None else None
                for i in poison:
                    if i % 2 == 0 or gz is None:
                        yaw[i] = np.nan
                    else:
                        gz[i] = np.inf if i % 4 == 1 else -np.inf
            if m == "rs":
                out = dict(yaw_deg=yaw) if can else dict(yaw_deg=yaw, angle_sum=d["sums"][t], rpm=d["rpm"][t])
            elif form == "rec":
                out = dict(kf6_rec=fmskf.kf6_records(yaw, gz, d["rpm"][t]))
            elif can:
                out = dict(yaw_deg=yaw, gyro_z_dps=gz)
            else:
                out = dict(yaw_deg=yaw, gyro_z_dps=gz, rpm=d["rpm"][t])
        if valid is not None:
            out["valid"] = valid
        return out

    def many_kw(self, t, T, form, poison, valid):
        """T ticks from t on as tick_many arrays; the poison in the middle tick"""
        ks = [self.kw(t + k, form, poison if k == T // 2 else None) for k in range(T)]
        out = {name: np.ascontiguousarray(np.stack([k[name] for k in ks])) for name in ks[0]}
        if valid is not None:
            out["valid"] = np.ascontiguousarray(np.stack([valid] * T))
        return out

    # ---------------------------------------------------------------- launches
    def launch(self, what, form="planes", poison=None, masked=None):
        """one launch form on both handles; `poison`: e's bad inputs, `masked`: bad inputs of e under
        valid == 0 (both handles get the mask).  Returns what the form hands back for e."""
        n, t = self.n, self.t
        valid = None
        if masked is not None:
            valid = np.ones(n, np.uint8)
            valid[masked] = 0
            poison = masked
        ret = None
        for h, bad in ((self.e, poison), (self.c, None)):
            if what == "tick":
                h.tick(**self.kw(t, form, bad, valid))
            elif what == "correct":
                h.correct(**self.kw(t, form, bad, valid))
            elif what == "predict":
                h.predict(**({} if self.model != "rs" else self.kw(t)))
            elif what == "many":
                h.tick_many(3, **self.many_kw(t, 3, form, bad, valid))
            elif what == "ens":
                r = h.tick_ensemble(**self.kw(t, form, bad, valid))
                assert r[0] == n, f"{what}: the record counts {r[0]} robots of {n}"
            elif what == "ens_async":
                h.tick_ensemble_begin(**self.kw(t, form, bad, valid))
                r = h.ensemble_end_count()
                assert r[2] == n and r[3] >= 1, f"{what}: the record counts {r[2]} robots of {n}"
            elif what == "isr":
                r = h.isr_tick(**self.kw(t, form, bad, valid, isr=True))
                assert r.shape == (n, 8)
            elif what == "isr_can":
                f, s = self.inp["tr"].can_frames(t % T_IN)
                r = h.isr_tick_can(f, s, **self.kw(t, form, bad, valid, isr=True, can=True))
                assert r.shape == (n, 8)
            else:
                raise ValueError(what)
            ret = r if h is self.e and what.startswith("ens") else ret
        self.t += 3 if what == "many" else 1
        return ret

    def replant(self, robots):
        """both handles take the twin's state through set_state, e's copy with the poison; set_state
        itself counts nothing.  set_state keeps the gate state, and e's robots that had bad inputs
        have another rejection history than the twin's: a gated pair restarts its gate state too."""
        self.set_gates()
        x, P = self.c.get_state()
        self.c.set_state(x, P)
        self.e.set_state(*nf.plant(self.model, x, P, robots))
        self.planted = np.asarray(robots, np.int64)
        self.tainted = np.zeros(0, np.int64)
        self.p_kept = nf.x_only(self.model, self.planted)
        assert self.e.get_counters()[0] == self.cnt, "set_state changed the counter"

    # ---------------------------------------------------------------- checks
    def state(self, h):
        x, P = h.get_state()
        return x, P, h.get_state_lo()

    def check(self, what, extra=(), strict=True, launches=1):
        """after `launches` launches: the counter against the stored state, the bad set against the
        planted one (plus `extra`, the robots with bad inputs; strict: exactly those), every other
        robot against the twin; returns the bad set"""
        what = f"{self.model} n={self.n} {what}"
        xe, Pe, le = self.state(self.e)
        xc, Pc, lc = self.state(self.c)
        nf.assert_small(xc, Pc, what + " (twin)")
        nf.assert_small(xe, Pe, what)
        assert nf.bad_robots(xc, Pc).size == 0 and self.c.get_counters()[0] == 0, f"{what}: the twin went bad"
        bad = nf.bad_robots(xe, Pe)
        cnt = self.e.get_counters()[0]
        want = self.cnt + (launches * bad.size if self.has_p else 0)
        assert cnt == want, f"{what}: counter {self.cnt} -> {cnt}, {bad.size} robots stored non-finite x {launches}"
        self.cnt = cnt
        self.tainted = np.union1d(self.tainted, np.asarray(extra, np.int64))
        self.p_kept = np.union1d(self.p_kept, np.setdiff1d(np.asarray(extra, np.int64), self.planted))
        may = np.union1d(self.planted, self.tainted)
        assert np.isin(self.planted, bad).all(), f"{what}: a planted robot is finite again"
        assert np.isin(bad, may).all(), f"{what}: robots {np.setdiff1d(bad, may)[:8]} went bad by themselves"
        if strict:
            assert np.array_equal(bad, may), f"{what}: bad set {bad[:8]}.. want {may[:8]}.."
        good = np.setdiff1d(np.arange(self.n), may)
        for name, u, v in (("x", xe, xc), ("P", Pe, Pc), ("lo", le, lc)):
            if u is not None:
                diff = np.nonzero((bits(u)[:, good] != bits(v)[:, good]).any(axis=0))[0]
                assert diff.size == 0, f"{what}: {name} of clean robots {good[diff][:8]} differs from the twin"
        if self.linear:
            k = self.p_kept
            diff = np.nonzero((bits(Pe)[:, k] != bits(Pc)[:, k]).any(axis=0))[0]
            assert diff.size == 0, f"{what}: P of robots {k[diff][:8]}, bad in x or in their inputs only, left the twin's"
            if le is not None:  # KF6 with FMSKF_CFG_COMP_POS: px, py, then P00, P10, P11
                diff = np.nonzero((bits(le)[2:, k] != bits(lc)[2:, k]).any(axis=0))[0]
                assert diff.size == 0, f"{what}: P low parts of robots {k[diff][:8]} left the twin's"
        if self.model in ("kf6", "ekf9") and not self.flags and self.gate is None:
            robots, reason, count = self.e.select(nonfinite=True)
            assert count == bad.size and np.array_equal(robots, bad), f"{what}: select(nonfinite)"
            assert np.all(reason == fmskf._lib.SEL_NONFINITE)
        return bad


def run_forms(model, n, pattern, flags=0, gate=None, forms=None, **kw):
    """every launch form of a handle: planted state, then bad inputs under valid == 0, then bad
    inputs (the models with float inputs)"""
    S = nf.plant_set(pattern, model, n)
    J, J2 = input_sets(n)
    floats = model in ("kf6", "kf12d")
    strict = gate is None  # a gate rejects a NaN NIS: a robot with a bad input may stay finite
    if forms is None:
        forms = [("tick", "planes"), ("correct", "planes"), ("predict", "planes"), ("many", "planes")]
        if model == "kf6":
            forms += [("tick", "rec"), ("correct", "rec"), ("many", "rec")]
        # the record: fused for the plain handles (KF12D: the default kernel only), the gated tick
        # and the stand-alone record for the gated ones
        if model != "kf12d" or not kw:
            forms += [("ens", "planes"), ("ens_async", "rec" if model == "kf6" else "planes")]
    with Twin(model, n, flags, gate, **kw) as tw:
        for what, form in forms:
            name = f"{pattern} {what}/{form}"
            tw.replant(S)
            reads = what != "predict"

            def step(label, strict=True, extra=(), **lkw):
                tw.launch(what, form, **lkw)
                tw.check(f"{name} {label}", extra=extra, strict=strict)
                if what == "correct":
                    # a predict between two updates, as a filter runs them: with the semidefinite
                    # R two updates in a row leave S = H P H^T + R exactly singular, twin included
                    tw.launch("predict")
                    tw.check(f"{name} {label}, then predict", strict=strict)

            # a gated handle four times: rejected, rejected, ..., then forced by max_consecutive
            for k in range(1 if gate is None else 4):
                step(f"planted #{k}")
            if floats and reads:
                step("bad inputs under valid == 0", masked=J2)
                step("bad inputs", extra=J, strict=strict, poison=J)
                step("left bad", strict=strict)  # counted again by the next launch


# ----------------------------------------------------------------------------- the tick kernels
@pytest.mark.parametrize("model,n,pattern", CASES)
def test_tick_forms(model, n, pattern):
    """tick, correct, predict, tick_many(3), tick_ensemble and tick_ensemble_begin / ensemble_end of
    the plain handles (KF6 with planes and with records; KF12D: the default R, k_kf12s)"""
    run_forms(model, n, pattern)


@pytest.mark.parametrize("model,n,pattern", [c for c in CASES if c[0] != "kf12d" and c[2] != "none"])
def test_comp_pos(model, n, pattern):
    """FMSKF_CFG_COMP_POS: the compensated instantiations, their low parts compared too"""
    run_forms(model, n, pattern, flags=COMP)


@pytest.mark.parametrize("gate", [(float("inf"), 0), (25.0, 3)], ids=["monitor", "threshold"])
@pytest.mark.parametrize("model,n,pattern", [c for c in CASES if c[0] != "kf12d" and c[2] in ("edges", "dense")])
def test_gated(model, n, pattern, gate):
    """set_gate (KF6) / set_row_gate (EKF9), monitor-only and with a threshold and max_consecutive: a
    NaN NIS / d2 is rejected, the state stays bad and is counted by every launch, forced updates
    included"""
    run_forms(model, n, pattern, gate=gate)


@pytest.mark.parametrize("case", ["indefinite_joint", "semidefinite_groups"])
@pytest.mark.parametrize("n,pattern", [(n, p) for n in nf.SIZES["kf12d"] for p in ("edges", "dense")])
def test_kf12d_fallback_r(case, n, pattern):
    """the two R cases that are not positive definite: k_kf12d, joint and group-sequential, whose
    lanes past N leave before the guard"""
    r = np.array(fmskf.default_config("kf12d", n).r[:36])
    for (i, j), v in (pc.KF12D_R_INDEFINITE if case == "indefinite_joint" else pc.KF12D_R_SEMIDEFINITE).items():
        r[i * (i + 1) // 2 + j] = v
    run_forms("kf12d", n, pattern, r=r)


# ----------------------------------------------------------------------------- the firmware ISR
def run_isr(model, n, pattern, fused=True):
    """isr_tick and isr_tick_can; fused: the one-kernel forms really ran (counters [1], [2])"""
    S = nf.plant_set(pattern, model, n)
    J, J2 = input_sets(n)
    with Twin(model, n) as tw:
        k = 0
        for what in ("isr", "isr_can"):
            tw.replant(S)
            tw.launch(what)
            tw.check(f"{pattern} {what} planted")
            k += 1
            if model in ("kf6", "kf12d"):
                tw.launch(what, masked=J2)
                tw.check(f"{pattern} {what} bad inputs under valid == 0")
                tw.launch(what, poison=J)
                tw.check(f"{pattern} {what} bad inputs", extra=J)
                k += 2
        c = tw.e.get_counters()
        if model == "kf12d" or not fused:
            assert c[2] == k, c[:3]  # every ISR ran as three kernels
        else:
            assert c[1] == 0 and c[2] == 0, c[:3]


@pytest.mark.parametrize("model,n,pattern", [c for c in CASES if c[2] != "last_only"])
def test_isr(model, n, pattern):
    """k_isr_kf6 and k_isr_ekf9, plain and with the CAN RX in front; KF12D's three-kernel ISR"""
    run_isr(model, n, pattern)


# ----------------------------------------------------------------------------- forced instantiations
def variant_run(what, models):
    """(child process) the tick forms, or the ISR as three kernels, of `models`"""
    for model in models:
        for n in nf.SIZES[model]:
            for pattern in ("edges", "dense"):
                if what == "isr":
                    run_isr(model, n, pattern, fused=False)
                else:
                    run_forms(model, n, pattern)
                    if model != "kf12d":
                        run_forms(model, n, pattern, flags=COMP,
                                  forms=[("tick", "planes"), ("many", "planes"), ("ens", "planes")])
    print("nonfinite variants ok")


@pytest.mark.parametrize("force,what,models", [({"FMSKF_KF6_VARIANT": "12"}, "ticks", "kf6"),
                                               ({"FMSKF_KF6_VARIANT": "15"}, "ticks", "kf6"),
                                               ({"FMSKF_EKF9_VARIANT": "2"}, "ticks", "ekf9"),
                                               ({"FMSKF_EKF9_VARIANT": "4"}, "ticks", "ekf9"),
                                               ({"FMSKF_STATE_NT": "1"}, "ticks", "kf6"),
                                               ({"FMSKF_STATE_NT": "1"}, "ticks", "ekf9"),
                                               ({"FMSKF_STATE_NT": "1"}, "ticks", "kf12d"),
                                               ({"FMSKF_ISR_FUSED": "0"}, "isr", "kf6,ekf9")])
def test_forced_instantiations(force, what, models):
    """the kernel forms the launcher takes at other sizes (two robots per lane / one at any N, the
    non-temporal state) and the ISR as three kernels, forced in a fresh child process as
    test_gpu_params.test_forced_kernel_variants does"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    script = ("import sys\nsys.path[:0] = sys.argv[1:4]\nimport test_gpu_nonfinite as m\n"
              "m.variant_run(sys.argv[4], sys.argv[5].split(','))\n")
    out = subprocess.run([sys.executable, "-c", script, root, os.path.join(root, "roboken-fmskf-robot-controller_amd"),
                          os.path.join(root, "tests"), what, models],
                         capture_output=True, text=True, timeout=240, env=dict(os.environ, **force))
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-3000:])
    assert "nonfinite variants ok" in out.stdout


# ----------------------------------------------------------------------------- correct_pose
@pytest.mark.parametrize("ticked", [False, True], ids=["planted", "ticked"])
@pytest.mark.parametrize("n", [257, 700])
@pytest.mark.parametrize("key", ["kf6", "kf6comp", "ekf9"])
def test_correct_pose(key, n, ticked):
    """fmskf_correct_pose counts applied fixes only: a listed robot with an Inf fix and nis_max = inf
    is applied, goes non-finite and is counted; a listed robot whose state is already NaN has a NaN
    NIS, is REJECTED, stays bit for bit and is not counted; bad robots that are not listed are not
    counted.  Every other robot, listed (a finite fix, the twin's) or not, equals the twin.
    The NIS of a position fix is formed from x[0], x[1], P00, P10, P11 (and their low parts) alone,
    so "already NaN" means a NaN in one of those.  A listed robot whose bad elements lie elsewhere
    has a finite NIS, is applied, stored and counted like any other robot stored non-finite; both
    classes are read off the state before the call.  `planted`: the fixes meet the planted state
    itself, one bad element per robot, so both classes are there by construction.  `ticked`: one
    tick first, whose update spreads a robot's poison over its whole state (x += U^T D^-1 w has no
    structural zeros), so that every bad robot has a bad position block.  One with an Inf and no NaN there (a P00 of +Inf gives 1 / S = 0) may have a
    finite, an infinite or a NaN NIS: for those the call's own status decides, and the rule is
    held either way -- ACCEPTED is stored and counted, REJECTED has a NaN NIS and is untouched."""
    model, flags = ("kf6", COMP) if key == "kf6comp" else (key, 0)
    S = nf.plant_set("edges", model, n)
    with Twin(model, n, flags) as tw:
        tw.replant(S)
        if ticked:
            tw.launch("tick")
            bad0 = tw.check("tick before the fixes")
        else:
            bad0 = nf.bad_robots(*tw.e.get_state())
            assert np.array_equal(bad0, S)
        clean = np.setdiff1d(np.arange(n), bad0)
        listed_bad = np.setdiff1d(bad0, bad0[2::5])  # four in five of the bad robots are listed
        inf_fix = clean[[0, clean.size // 2, -1]]   # an Inf fix: applied, goes bad
        fin_fix = np.setdiff1d(clean[3:-3:7], inf_fix)  # a finite fix: as the twin's
        robot = np.sort(np.concatenate([listed_bad, inf_fix, fin_fix])).astype(np.uint32)
        tr = tw.inp["tr"]
        px = tr.px[WARM, robot].astype(np.float32)
        py = tr.py[WARM, robot].astype(np.float32)
        pxe = px.copy()
        pxe[np.isin(robot, inf_fix)] = [np.inf, -np.inf, np.inf]
        pre = tw.state(tw.e)
        nis, status = tw.e.correct_pose(robot, pxe, py, r=1e-2, out=True)
        nc, sc = tw.c.correct_pose(robot, px, py, r=1e-2, out=True)
        post = tw.state(tw.e)
        assert np.all(sc == ACC) and np.isfinite(nc).all()
        pos = [pre[0][:2], pre[1][:3]] + ([pre[2]] if flags else [])  # what the NIS is formed from
        pos_ok = np.all([np.isfinite(a).all(axis=0) for a in pos], axis=0)
        pos_nan = np.any([np.isnan(a).any(axis=0) for a in pos], axis=0)
        st_of = dict(zip(robot.tolist(), status.tolist()))
        nis_of = dict(zip(robot.tolist(), nis.tolist()))
        must_rej, must_acc = listed_bad[pos_nan[listed_bad]], listed_bad[pos_ok[listed_bad]]
        assert must_rej.size >= 2, "too few listed robots with a NaN in their position block"
        if not ticked:
            assert must_acc.size >= 10, "too few listed robots that are bad outside their position block only"
        assert all(st_of[i] == REJ for i in must_rej) and all(st_of[i] == ACC and np.isfinite(nis_of[i]) for i in must_acc)
        assert all(st_of[i] in (ACC, REJ) and (st_of[i] == ACC or np.isnan(nis_of[i])) for i in listed_bad)
        acc_bad = np.array([i for i in listed_bad if st_of[i] == ACC], np.int64)
        assert np.all(status[np.isin(robot, inf_fix)] == ACC), (status[np.isin(robot, inf_fix)], nis[np.isin(robot, inf_fix)])
        fin = np.isin(robot, fin_fix)
        assert np.all(status[fin] == ACC) and np.array_equal(bits(nis[fin]), bits(nc[fin]))
        same = np.setdiff1d(bad0, acc_bad)  # rejected, or bad and not listed: bit for bit as it was
        for u, v in zip(pre, post):
            if u is not None:
                assert np.array_equal(bits(u)[:, same], bits(v)[:, same])
        bad1 = nf.bad_robots(post[0], post[1])
        assert np.array_equal(bad1, np.union1d(bad0, inf_fix))
        cnt = tw.e.get_counters()[0]
        want = inf_fix.size + acc_bad.size
        assert cnt == tw.cnt + want, f"counter {tw.cnt} -> {cnt}: {want} applied fixes were stored non-finite"
        # the state against the twin: check() expects one launch's count of the whole bad set, so
        # step the reference count by hand and let it compare the states
        tw.cnt = cnt - bad1.size
        tw.planted = bad1
        # P against the twin's, whose fixes were all applied: an applied fix forms P from P and R
        # alone, whatever x and the fix hold; a rejected one left P as it was
        rejected = np.array([i for i in listed_bad if st_of[i] == REJ], np.int64)
        tw.p_kept = np.union1d(np.setdiff1d(tw.p_kept, rejected), inf_fix)
        tw.check("after the fixes")


# ----------------------------------------------------------------------------- RS
@pytest.mark.parametrize("n", [1, 257, 700])
def test_rs_is_not_counted(n):
    """RS has no guard (documented): a NaN yaw poisons its own robot only and counters[0] stays 0"""
    J, _ = input_sets(n)
    with Twin("rs", n) as tw:
        for what in ("tick", "isr", "isr_can"):
            tw.launch(what, poison=J)
            x, _ = tw.e.get_state()
            assert np.array_equal(nf.bad_robots(x, None), J), what
            tw.check(what, extra=J)
            assert tw.e.get_counters()[0] == 0


# ----------------------------------------------------------------------------- lifecycle
@pytest.mark.parametrize("model", list(nf.DIMS))
def test_counter_lifecycle(model, tmp_path):
    """a robot left bad is counted by each later launch; set_state and set_state_subset do not touch
    the counter, save_state / load_state restore its value, reset zeroes it; get_counters with fewer
    than 8 slots writes only those"""
    n = 257
    S = nf.plant_set("dense", model, n)
    k = S.size
    with Twin(model, n) as tw:
        tw.replant(S)
        for j in range(3):
            tw.launch("tick")
            tw.check(f"tick {j}")
        assert tw.cnt == 3 * k
        path = str(tmp_path / "ck.bin")
        tw.e.save_state(path)
        tw.launch("tick")
        tw.check("tick after save")
        assert tw.cnt == 4 * k
        tw.e.load_state(path)
        assert tw.e.get_counters()[0] == 3 * k
        x, P = tw.e.get_state()
        tw.e.set_state(x, P)
        assert tw.e.get_counters()[0] == 3 * k
        if model != "kf12d":  # the listed-robot calls serve the fp32 models
            sub = S[:5].astype(np.uint32)
            xs, Ps, _ = tw.e.get_state_subset(sub)
            tw.e.set_state_subset(sub, xs, Ps)
            assert tw.e.get_counters()[0] == 3 * k
        L = fmskf._lib.load()
        for m in (1, 3, 7):
            out = (C.c_uint64 * 8)(*([0xDEAD] * 8))
            assert L.fmskf_get_counters(tw.e.h, out, m) == 0
            assert list(out)[:1] == [3 * k] and list(out)[m:] == [0xDEAD] * (8 - m), (m, list(out))
        tw.e.reset()
        tw.c.reset()
        assert tw.e.get_counters()[0] == 0
        x, P = tw.e.get_state()
        assert nf.bad_robots(x, P).size == 0
