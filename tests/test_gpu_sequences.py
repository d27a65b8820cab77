"""Call ORDERS over the C ABI against the oracle (tests/seq_ref.py): the handle's deferred state --
where the RS odometry's previous sums live (rs_prev_synced / rs_prev_stale), the control outputs
formed on demand (ctrl_derived_stale), the motor history order of a captured sequence (m_par,
graph_par0 / graph_par_end) -- must be consistent for every entry point that can follow, including
calls that are replayed from a graph after direct calls made since its capture.  Directed op
lists for the known orderings, and seeded random sequences (seq_ref.generate; the seeds and what
they cover: test_seq_cpu.py).  Bar: every comparison exact, floats as bit patterns."""
import numpy as np
import pytest

import seq_ref
from fmskf import Engine
from seq_ref import name
from test_seq_cpu import LENGTH, SEEDS

pytestmark = pytest.mark.gpu

N = 1001  # a multiple of neither the wave nor the tile width, more than one block


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def eq(got, want, what):
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=what)


class Runner:
    """One handle driven op by op next to its seq_ref.Fleet; the state is compared after every op."""

    def __init__(self, orc, model, n, ops, seed, tmp_path):
        import torch
        self.torch = torch
        self.model, self.n, self.ops, self.seed = model, n, list(ops), seed
        self.inp = seq_ref.Inputs(model, n, seq_ref.ticks_needed(ops), seed)
        self.fleet = seq_ref.Fleet(orc, model, n, self.inp)
        self.ck = str(tmp_path / f"{model}_{seed}.ck")
        self.stream = torch.cuda.Stream()  # graph capture needs a real stream
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device="cuda")  # noqa: E731
        # the fixed device buffers of the device-pointer ops and the captured calls (two sets: the
        # fused_dev2 kind reads two ticks per launch)
        self.buf = [dict(f=z((n, 4, 8), torch.uint8), s=z((n, 4), torch.int16), yaw=z((n,), torch.float32),
                         gz=z((n,), torch.float32), raw=z((n, 8), torch.int16)) for _ in range(2)]
        self.rpm_d, self.sum_d = z((n, 4), torch.int16), z((4, n), torch.int64)
        self.mask_d, self.out_d = z((n,), torch.uint8), z((n, 8), torch.uint8)
        self.e = None

    # ---- inputs
    def kw_host(self, t):
        i = self.inp
        if self.model == "ekf9":
            return dict(raw=i.raw[t])
        return dict(yaw_deg=i.yaw[t]) if self.model == "rs" else dict(yaw_deg=i.yaw[t], gyro_z_dps=i.gz[t])

    def kw_dev(self, k=0):
        b = self.buf[k]
        if self.model == "ekf9":
            return dict(raw=b["raw"])
        return dict(yaw_deg=b["yaw"]) if self.model == "rs" else dict(yaw_deg=b["yaw"], gyro_z_dps=b["gz"])

    def refresh(self, t, k=0):
        """tick t's inputs into device buffer set k (and the single rpm / sums / mask buffers)"""
        i, b, up = self.inp, self.buf[k], lambda a: self.torch.from_numpy(np.ascontiguousarray(a))
        f, s = i.can(t)
        b["f"].copy_(up(f))
        b["s"].copy_(up(s))
        b["yaw"].copy_(up(i.yaw[t]))
        b["gz"].copy_(up(i.gz[t]))
        if i.raw is not None:
            b["raw"].copy_(up(i.raw[t]))
        if k == 0:
            self.rpm_d.copy_(up(i.rpm[t]))
            self.mask_d.copy_(up(i.power(t)))
            if i.csum is not None:
                self.sum_d.copy_(up(i.csum[t]))

    # ---- the engine side of the ops
    def open(self):
        self.e = Engine(self.model, self.n)
        self.e.set_stream(self.stream)

    def start(self):
        self.open()
        if self.fleet.wb is not None:
            self.e.ingest_wt901(*self.inp.poll(), latch_qinit=True)
        self.e.set_power(self.inp.power(-1))
        self.e.set_target_vel(*self.inp.target(-1))
        self.fleet.start()

    def captured(self, kind):
        """the calls of a capture kind, on the fixed device buffers"""
        e, b = self.e, self.buf[0]
        if kind == "fused_dev":
            e.isr_tick_can(b["f"], b["s"], out=self.out_d, **self.kw_dev())
        elif kind == "fused_dev2":
            for k in range(2):
                e.isr_tick_can(self.buf[k]["f"], self.buf[k]["s"], out=self.out_d, **self.kw_dev(k))
        elif kind == "split":
            e.ingest_can(b["f"], b["s"])
            e.isr_tick(out=self.out_d, **(self.kw_dev() if self.model == "ekf9" else {}))
        elif kind == "caller_sums":
            e.ingest_can(b["f"], b["s"])
            e.tick(yaw_deg=b["yaw"], angle_sum=self.sum_d, rpm=self.rpm_d)
        elif kind == "control_rpm":
            e.control(self.rpm_d)
        elif kind == "set_power":
            e.set_power(self.mask_d)
        elif kind == "ingest_only":
            e.ingest_can(b["f"], b["s"])
        else:
            raise ValueError(kind)

    def run(self, op):
        """the engine's calls of `op`; the fleet is advanced alongside.  Returns (frames the
        engine produced or None, frames the fleet expects or None)."""
        e, i, fl, o = self.e, self.inp, self.fleet, name(op)
        t, got = fl.t, None
        if o not in seq_ref.NO_INPUT and o not in ("replay", "launch"):
            f, s = i.can(t)
        if o == "fused":
            got = e.isr_tick_can(f, s, **self.kw_host(t))
        elif o == "fused_dev":
            self.refresh(t)
            got = e.isr_tick_can(self.buf[0]["f"], self.buf[0]["s"], out=self.out_d, **self.kw_dev()).cpu().numpy()
        elif o == "split":  # RS, KF6: NULL planes, the ingested yaw / gyro page and the motor state
            e.ingest_can(f, s)
            got = e.isr_tick(**(self.kw_host(t) if self.model == "ekf9" else {}))
        elif o == "three":
            e.ingest_can(f, s)
            e.tick(**self.kw_host(t))
            e.control()
            got = e.can_tx()
        elif o == "caller_sums":
            e.ingest_can(f, s)
            e.tick(yaw_deg=i.yaw[t], angle_sum=i.csum[t], rpm=i.rpm[t])
        elif o == "caller_rpm":  # KF6: planes and a caller rpm, or records, in turn
            if self.model == "kf6" and t % 2:
                got = e.isr_tick_can(f, s, kf6_rec=i.rec[t])
            else:
                got = e.isr_tick_can(f, s, rpm=i.rpm[t], **self.kw_host(t))
        elif o == "predict_only":
            e.ingest_can(f, s)
            e.predict()
        elif o == "correct_only":
            e.correct(**self.kw_host(t))
        elif o == "ingest_only":
            e.ingest_can(f, s)
        elif o == "control_rpm":
            e.control(i.rpm[t])
        elif o == "set_power":
            e.set_power(i.power(t))
        elif o == "set_target":
            e.set_target_vel(*i.target(t))
        elif o == "set_params":
            e.set_ctrl_params(**seq_ref.PARAMS[i.params(t)])
        elif o == "reset":
            e.reset()
        elif o == "ckpt":
            e.save_state(self.ck)
            e.close()
            self.open()
            self.e.load_state(self.ck)
        elif o == "capture":
            e.graph_begin()
            self.captured(op[1])
            e.graph_end()
        elif o == "replay":
            kind = fl.graph[0]
            want = None
            for _ in range(op[1]):
                for k in range(seq_ref.KINDS[kind][0]):
                    self.refresh(fl.t + k, k)
                e.graph_launch(1)
                want = fl.replay_once()
                self.check_state(f"launch on tick {fl.t - 1}")
            if kind in seq_ref.KIND_FRAMES:
                got = self.out_d.cpu().numpy()
            return got, want
        elif o == "launch":  # one fmskf_graph_launch of k launches, all on the next tick's inputs
            kind = fl.graph[0]
            for k in range(seq_ref.KINDS[kind][0]):
                self.refresh(fl.t + k, k)
            e.graph_launch(op[1])
            if kind in seq_ref.KIND_FRAMES:
                got = self.out_d.cpu().numpy()
        elif o == "read_prev":
            eq(e.get_prev_sum(), fl.prev, "previous sums")
        elif o == "read_ctrl":
            self.check_ctrl()
        elif o == "read_motors":
            self.check_motors()
        else:
            raise ValueError(op)
        return got, fl.apply(op)

    # ---- comparisons
    def check_state(self, what=""):
        x, P = self.e.get_state()
        xo, Po = self.fleet.state()
        if self.model == "rs":
            eq(x[:3], xo[:3], f"pose {what}")
            eq(x[3:], xo[3:], f"velocity {what}")
        else:
            eq(x, xo, f"x {what}")
            eq(P, Po, f"P {what}")

    def check_ctrl(self):
        got, want = self.e.get_ctrl(), self.fleet.ctrl()
        for k in ("curr", "vel_tgt", "wheel_tgt", "wheel_ctrl"):
            eq(got[k], want[k], f"get_ctrl {k}")

    def check_motors(self):
        got = dict(self.e.get_motors(), **{"status_" + k: v for k, v in self.e.get_motor_status().items()})
        want = self.fleet.motors()
        assert set(got) == set(want)
        for k in got:
            eq(got[k], want[k], f"motor state {k}")

    def check_end(self):
        if self.model == "rs":
            eq(self.e.get_prev_sum(), self.fleet.prev, "previous sums")
        self.check_ctrl()
        self.check_motors()
        c = self.e.get_counters()
        assert c[0] == 0, c[:3]
        # which launch form ran: only the caller-rpm calls ran the CAN RX as its own kernel
        assert c[1] == self.fleet.can_split and c[2] == 0, (c[:3], self.fleet.can_split)

    def play(self):
        torch = self.torch
        prev_stream = torch.cuda.current_stream()
        torch.cuda.set_stream(self.stream)  # the buffer refreshes queue on the handle's stream
        idx = -1
        try:
            self.start()
            self.check_state("after the prologue")
            for idx, op in enumerate(self.ops):
                got, want = self.run(op)
                self.check_state("after the op")
                assert (got is None) == (want is None), "TX frames produced"
                if got is not None:
                    eq(got, want, "0x200 frames")
            idx = len(self.ops)
            self.check_end()
        except AssertionError as err:
            done = self.ops[:idx + 1]
            at = f"op {idx} {self.ops[idx]!r}" if 0 <= idx < len(self.ops) else "the end of the sequence" if idx >= 0 else "the prologue"
            raise AssertionError(f"{self.model} N={self.n} seed={self.seed}: mismatch at {at}\n{err}\n"
                                 f"ops so far: {done!r}") from err
        finally:
            if self.e is not None:
                self.e.close()
            torch.cuda.set_stream(prev_stream)


def play(orc, model, ops, tmp_path, seed=0, n=N):
    seq_ref.check_rules(model, ops)
    Runner(orc, model, n, ops, seed, tmp_path).play()


CAP = lambda kind: ("capture", kind)  # noqa: E731
REP = lambda k: ("replay", k)  # noqa: E731


# ---- directed regressions: one op list each, the state asserted after every op
def test_directed_rs_replay_after_two_direct_fused(orc, tmp_path):
    """A captured fused RS ISR reads and writes the prev planes (no PS form in a capture).  Two
    direct fused ticks after graph_end leave them one frame behind (the second runs PS); the
    replay must start from the current previous sums, not integrate that frame's motion again."""
    play(orc, "rs", [CAP("fused_dev"), "fused", "fused", REP(2), "read_prev", "fused", "read_prev"], tmp_path, 1)


def test_directed_rs_caller_sums_graph_then_materialize(orc, tmp_path):
    """A graph that ticks on caller sums leaves THOSE as the previous sums: a stale flag from
    the PS tick before it must not outlive the replay and overwrite them with the motor sums."""
    play(orc, "rs", [CAP("caller_sums"), "fused", "fused", REP(1), "read_prev"], tmp_path, 2)


@pytest.mark.parametrize("model", ["kf6", "rs"])
@pytest.mark.parametrize("case", ["listed", "capture_first", "set_params", "fused_step", "fused_step_set_params"])
def test_directed_power_only_graph_after_direct_step(orc, tmp_path, model, case):
    """fmskf_get_ctrl returns the last step's outputs under the power flags that step ran with,
    also when the flags change by a REPLAYED fmskf_set_power (a graph with no control step).
    The replayed mask differs from the current one on half the fleet.  `listed`: the step before
    the capture (graph_begin forms its outputs); the others: the step between the capture and
    the replay, so only the replay can form them in time."""
    ops = {"listed": ["control_rpm", CAP("set_power"), REP(1), "read_ctrl"],
           "capture_first": [CAP("set_power"), "control_rpm", REP(1), "read_ctrl"],
           "set_params": [CAP("set_power"), "control_rpm", "set_params", REP(1), "read_ctrl"],
           "fused_step": [CAP("set_power"), "fused", REP(1), "read_ctrl"],
           "fused_step_set_params": [CAP("set_power"), "fused", "set_params", REP(1), "read_ctrl"]}[case]
    # a few steps first, so the loops have run and the outputs of on and off robots differ
    play(orc, model, ["control_rpm"] * 3 + ops, tmp_path, 3)


@pytest.mark.parametrize("model", ["rs", "kf6", "ekf9"])
def test_directed_ingest_only_replays_between_direct_can_rx(orc, tmp_path, model):
    """An odd number of captured CAN RX calls toggles the motor history order per replay; direct
    CAN RX calls in between toggle it too.  Every Status field, s16_microsec_id and
    flt_dltOutAngle_rad among them, depends on that order."""
    play(orc, model, [CAP("ingest_only"), REP(1), "ingest_only", REP(2), "fused", REP(1), "read_motors"],
         tmp_path, 4)


@pytest.mark.parametrize("model", ["rs", "kf6", "ekf9"])
def test_directed_several_launches_in_one_call(orc, tmp_path, model):
    """fmskf_graph_launch(h, k > 1): with an odd number of captured CAN RX calls the history
    order is put back between the launches of ONE call as well, also after direct CAN RX; a
    fused ISR launched three times after two direct ticks starts from current previous sums."""
    ops = [CAP("ingest_only"), ("launch", 3), "read_motors", "fused", ("launch", 2), "read_motors",
           CAP("fused_dev"), "fused", "fused", ("launch", 3)]
    play(orc, model, ops + (["read_prev"] if model == "rs" else []) + ["read_ctrl", "read_motors"], tmp_path, 7)


@pytest.mark.parametrize("model", ["rs", "kf6"])
def test_directed_replay_after_reset(orc, tmp_path, model):
    ops = ["fused", "fused", CAP("fused_dev"), "reset", REP(2)]
    play(orc, model, ops + (["read_prev"] if model == "rs" else []) + ["read_ctrl", "read_motors"], tmp_path, 5)


@pytest.mark.parametrize("model", ["rs", "kf6", "ekf9"])
def test_directed_checkpoint_after_replay(orc, tmp_path, model):
    ops = [CAP("split"), "fused", "fused", REP(1), "ckpt", "fused"]
    play(orc, model, ops + (["read_prev"] if model == "rs" else []) + ["read_ctrl"], tmp_path, 6)


# ---- random sequences
@pytest.mark.parametrize("model,seed", [(m, s) for m in seq_ref.MODELS for s in SEEDS[m]])
def test_random_sequence(orc, tmp_path, model, seed):
    play(orc, model, seq_ref.generate(model, seed, LENGTH), tmp_path, seed)


@pytest.mark.parametrize("model", seq_ref.MODELS)
def test_random_sequence_one_robot(orc, tmp_path, model):
    seed = SEEDS[model][0]
    play(orc, model, seq_ref.generate(model, seed, LENGTH), tmp_path, seed, n=1)
