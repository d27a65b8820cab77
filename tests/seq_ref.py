"""Call sequences over the C ABI and their reference fleet (test_seq_cpu.py, test_gpu_sequences.py).

The handle keeps host-side flags that decide which form of a kernel runs and whether the planes it
reads are current (fmskf_ctx: rs_prev_synced / rs_prev_stale, ctrl_derived_stale, m_par and the
graph's graph_par0 / graph_par_end).  What goes wrong there is an ORDER of calls, so the tests run
op lists: `generate` draws one, `Fleet` is what the oracle says the fleet is after each op.  Fleet
holds no arithmetic of its own: orc.MotorBatch (the C610 rx_callback), orc.CtrlBatch (the control
half of VEHICLE_CTRL::update), orc.Wt901Batch (the ingested yaw / gyro page where an op reads it)
and orc.rs_tick / kf6_tick / ekf9_tick, applied one op at a time exactly as
test_isr_tick_can_firmware_60000_ticks and test_rs_prev_in_motor_sums apply them inline.

An op is a name, or ("capture", kind) / ("replay", k); the directed lists also use ("launch", k),
one fmskf_graph_launch of k launches on the same inputs.  Every op that takes per-tick inputs takes
those of the fleet's next tick (Inputs) and moves the tick counter on by one; a replay moves it by
the captured kind's ticks per launch.  A captured call does not run, so a capture leaves the fleet
where it is; a replay applies the captured call list once per launch with the inputs of that
launch, and with the control parameters of the capture (the captured kernels keep theirs).

No GPU is needed here: the engine side of the ops is in test_gpu_sequences.py."""
import numpy as np

import fmskf
from fmskf.synth import Trajectory

MODELS = ("rs", "kf6", "ekf9")

# op -> weight of a draw (generate); RS_ONLY ops are drawn for RS alone
WEIGHTS = (("fused", 6), ("fused_dev", 3), ("split", 3), ("three", 2), ("caller_sums", 2), ("caller_rpm", 2),
           ("predict_only", 2), ("correct_only", 1), ("ingest_only", 2), ("control_rpm", 2), ("set_power", 2),
           ("set_target", 2), ("set_params", 2), ("read_prev", 2), ("read_ctrl", 3), ("read_motors", 2),
           ("ckpt", 1), ("reset", 2), ("capture", 6))
RS_ONLY = ("caller_sums", "read_prev")
READS = ("read_prev", "read_ctrl", "read_motors")
# ops that take no per-tick inputs (the tick counter stays)
NO_INPUT = READS + ("ckpt", "reset", "capture")

# capture kind -> (ticks of inputs one launch reads, RS only)
KINDS = {"fused_dev": (1, False), "split": (1, False), "caller_sums": (1, True), "control_rpm": (1, False),
         "set_power": (1, False), "ingest_only": (1, False), "fused_dev2": (2, False)}
# kinds whose last captured call writes the 0x200 frames into the device `out`
KIND_FRAMES = ("fused_dev", "split", "fused_dev2")

# the two control parameter sets set_params switches between (test_gpu_ctrl.py)
PARAMS = (dict(),
          dict(ctrl_freq_hz=1000.0, ff_gain=0.01, p_gain=0.05, i_gain=0.2, d_gain=0.004, i_limit=0.8,
               lpf_freq_hz=25.0, ff_limit=0.7, interp_ts=np.float32(0.001), curr_limit_raw=2500))
_ORC_PARAMS = (dict(),
               dict(c_freq=1000.0, ff=0.01, pg=0.05, ig=0.2, dg=0.004, ilim=0.8, lpf=25.0, fflim=0.7,
                    ts=np.float32(0.001), clim=2500))


def name(op):
    return op if isinstance(op, str) else op[0]


def vocabulary(model):
    return [(o, w) for o, w in WEIGHTS if model == "rs" or o not in RS_ONLY]


def kinds(model):
    return [k for k, (_, rs) in KINDS.items() if model == "rs" or not rs]


def generate(model, seed, length):
    """The op list of (model, seed, length): a pure function.  What the ABI requires holds by
    construction: a replay only while a graph exists (a `ckpt` makes a new handle and so drops
    it, a `reset` keeps it); a capture is one op, so nothing reads or checkpoints inside it, and
    the sequences run on a stream of their own with timing off; RS-only ops for RS alone.  Half
    of the draws made while a graph exists are a replay of 1..3 launches, so direct ops land
    between a capture and its replay and between two replays."""
    if model not in MODELS:
        raise ValueError(model)
    rng = np.random.default_rng([0x5E9, MODELS.index(model), int(seed)])
    voc = vocabulary(model)
    names = [o for o, _ in voc]
    p = np.array([w for _, w in voc], np.float64)
    p /= p.sum()
    ks = kinds(model)
    ops, graph = [], False
    while len(ops) < length:
        if graph and rng.random() < 0.5:
            ops.append(("replay", int(rng.integers(1, 4))))
            continue
        o = names[int(rng.choice(len(names), p=p))]
        if o == "capture":
            ops.append(("capture", ks[int(rng.integers(len(ks)))]))
            graph = True
        else:
            ops.append(o)
            if o == "ckpt":
                graph = False
    return ops


def check_rules(model, ops):
    """raise AssertionError where `ops` breaks a rule of the ABI (see generate)"""
    graph = None
    for i, op in enumerate(ops):
        o = name(op)
        assert o in [v for v, _ in WEIGHTS] + ["replay", "launch"], (i, op)
        assert model == "rs" or o not in RS_ONLY, (i, op)
        if o == "capture":
            assert op[1] in kinds(model), (i, op)
            graph = op[1]
        elif o in ("replay", "launch"):
            assert graph is not None, (i, op, "replay without a graph")
            assert 1 <= op[1] <= 3, (i, op)
        elif o == "ckpt":
            graph = None


def ticks_needed(ops):
    """an upper bound of the input ticks `ops` read"""
    return sum(0 if name(o) in NO_INPUT else 2 * o[1] if name(o) in ("replay", "launch") else 1 for o in ops) + 1


def replayed_kinds(ops):
    """the capture kinds `ops` replay at least once"""
    out, graph = set(), None
    for op in ops:
        if name(op) == "capture":
            graph = op[1]
        elif name(op) == "ckpt":
            graph = None
        elif name(op) == "replay":
            out.add(graph)
    return out


def pairs(ops):
    """the ordered pairs of neighbouring op names"""
    n = [name(o) for o in ops]
    return set(zip(n, n[1:]))


def triples(ops):
    n = [name(o) for o in ops]
    return set(zip(n, n[1:], n[2:]))


class Inputs:
    """The per-tick inputs of one sequence: a Trajectory's CAN frames, yaw / gyro, raw records,
    caller rpm and caller sums (unrelated to the motor state's), and seeded power masks, targets
    and parameter choices."""

    def __init__(self, model, n, ticks, seed):
        self.model, self.n, self.ticks, self.seed = model, n, ticks, int(seed)
        self.tr = tr = Trajectory(n, ticks, seed=1000 + self.seed)
        self.yaw, self.gz, self.rpm = tr.kf6_inputs()
        self.csum = tr.rs_inputs()[1] if model == "rs" else None  # [T][4][N]
        self.raw = tr.ekf9_raw() if model == "ekf9" else None
        self.rec = fmskf.kf6_records(self.yaw, self.gz, self.rpm) if model == "kf6" else None
        self._can = {}

    def can(self, t):
        if t not in self._can:
            f, s = self.tr.can_frames(t)
            self._can[t] = (np.ascontiguousarray(f), np.ascontiguousarray(s))
        return self._can[t]

    def poll(self):
        """the WT901 poll of tick 0 (rows, lens): the page the NULL-yaw calls read"""
        return self.tr.wt901_poll_rows(0)

    def _rng(self, t, salt):
        return np.random.default_rng([self.seed, int(t) + 1, salt])

    def power(self, t):
        """[N] uint8, each robot on with probability 1/2: two masks differ on half the fleet"""
        return (self._rng(t, 1).random(self.n) < 0.5).astype(np.uint8)

    def target(self, t):
        """(vel, acl, jrk [3][N], mask [N]) as _schedule of test_gpu_ctrl.py draws them"""
        rng, n = self._rng(t, 2), self.n
        vel = np.stack([rng.uniform(-400, 400, n), rng.uniform(-400, 400, n),
                        rng.uniform(-6 * np.pi, 6 * np.pi, n)]).astype(np.float32)
        big = rng.random() < 0.5  # C_ACCEL/JERK_MAX_MOVE vs _STOP (VD_task_main.cpp:29-48)
        acl = np.array([[2000.0 if big else 1000.0], [2000.0 if big else 1000.0],
                        [70.0 if big else 30.0]], np.float32).repeat(n, 1)
        jrk = np.array([[30000.0 if big else 10000.0], [30000.0 if big else 10000.0],
                        [1000.0 if big else 300.0]], np.float32).repeat(n, 1)
        return vel, acl, jrk, (rng.random(n) < 0.7).astype(np.uint8)

    def params(self, t):
        """index into PARAMS"""
        return int(self._rng(t, 3).integers(2))


class Fleet:
    """The reference fleet of one model: what every readout of the handle must return after the
    ops applied so far.  `start()` is the sequences' common prologue (a WT901 poll for the models
    that read the ingested page, half the fleet powered, one target); `apply(op)` advances by one
    op and returns the 0x200 frames the op produced (None where it produced none)."""

    def __init__(self, orc, model, n, inp, prm=None):
        """prm (optional): a param_cases.Params -- dt, Q, R, P0 of the estimator and the motor
        directions; omitted: fmskf.default_config"""
        self.orc, self.model, self.n, self.inp = orc, model, n, inp
        self.cprm = [orc.ctrl_params(**kw) for kw in _ORC_PARAMS]
        self.pidx = 0
        self.dirs = (1, 1, -1, -1) if prm is None else tuple(prm.motor_dir)
        cfg = fmskf.default_config(model, n)
        if prm is not None and model in ("kf6", "ekf9"):
            assert prm.model == model
            mk = orc.kf6_params if model == "kf6" else orc.ekf9_params
            self.prm = mk(prm.dt, prm.q, prm.r, orc.TRIG_TABLE512)
            self.p0 = np.float32(prm.p0)
        elif model == "kf6":
            self.prm = orc.kf6_params(cfg.dt, np.array(cfg.q[:21]), np.array(cfg.r[:10]), orc.TRIG_TABLE512)
            self.p0 = np.float32(np.array(cfg.p0[:21]))
        elif model == "ekf9":
            self.prm = orc.ekf9_params(cfg.dt, np.array(cfg.q[:45]), np.array(cfg.r[:21]), orc.TRIG_TABLE512)
            self.p0 = np.float32(np.array(cfg.p0[:45]))
        self.t = 0
        self.graph = None       # (kind, index of the control parameters at the capture)
        self.can_split = 0      # fmskf_get_counters [1]: fmskf_isr_tick_can calls that ran as two
        self._zero()

    def _zero(self):
        orc, n = self.orc, self.n
        self.mb = orc.MotorBatch(n, self.dirs)
        self.ref = orc.CtrlBatch(n, self.cprm[self.pidx], motor_dir=self.dirs)
        self.wb = orc.Wt901Batch(n) if self.model != "ekf9" else None
        if self.model == "rs":
            self.pos, self.vel = np.zeros((3, n), np.float32), np.zeros((3, n), np.float32)
            self.prev = np.zeros((4, n), np.int64)
        else:  # EKF9: row 9 is the heading's low part (orc.ekf9_tick)
            self.x = np.zeros((10 if self.model == "ekf9" else 6, n), np.float32)
            self.P = np.repeat(self.p0[:, None], n, 1).copy()
        self.can_split = 0

    def start(self):
        if self.wb is not None:
            self.wb.update(*self.inp.poll(), latch_qinit=True)
        self.ref.set_power(self.inp.power(-1))
        self.ref.set_target_vel(*self.inp.target(-1))

    # ---- readouts
    def state(self):
        """(x rows as fmskf_get_state returns them, P or None)"""
        if self.model == "rs":
            return np.concatenate([self.pos, self.vel]), None
        return self.x[:9 if self.model == "ekf9" else 6], self.P

    def ctrl(self):
        r = self.ref
        return dict(vel_tgt=r.vel_tgt(), curr=r.curr(), wheel_tgt=r.wheel("tgt"), wheel_ctrl=r.wheel("ctrl"))

    def motors(self):
        """get_motors' fields, and get_motor_status' under status_*"""
        f = self.mb.field
        return dict(angle=f("angle"), rpm=f("rpm"), curr=f("curr"), angle_sum=f("angle_sum").T,
                    speed_radps=f("speed_radps").T, status_microsec_id=f("micro"), status_angle=f("angle"),
                    status_rpm=f("rpm"), status_curr=f("curr"), status_dlt_out_angle_rad=f("dlt_out_angle_rad"),
                    status_speed_radps=f("speed_radps"))

    def frames(self):
        return self.orc.can_tx(self.ref.curr())

    # ---- the primitive calls
    def _rx(self, t):
        self.mb.rx(*self.inp.can(t))

    def _est(self, t, yaw="host", rpm="motor", sums="motor", correct=True, predict=True):
        """one estimator call; returns the rpm record it read (the control half reads the same)"""
        orc, inp = self.orc, self.inp
        r = self.mb.field("rpm") if rpm == "motor" else inp.rpm[t]
        if yaw == "imu" and self.wb is not None:  # the ingested page: Data.angle[2], Data.gyro[2]
            d = self.wb.data
            y, g = np.ascontiguousarray(d[11]), np.ascontiguousarray(d[5])
        else:
            y, g = inp.yaw[t], inp.gz[t]
        if self.model == "rs":
            s = np.ascontiguousarray(self.mb.field("angle_sum").T if sums == "motor" else inp.csum[t])
            orc.rs_tick(self.pos, self.vel, self.prev, y, s, r, do_correct=correct, do_predict=predict)
        elif self.model == "kf6":
            orc.kf6_tick(self.x, self.P, y, g, r, None, self.prm, do_update=correct, do_predict=predict, nthreads=0)
        else:
            orc.ekf9_tick(self.x, self.P, inp.raw[t], None, self.prm, do_update=correct, do_predict=predict,
                          nthreads=0)
        return r

    def _step(self, rpm, pidx=None):
        """the control step; pidx: a captured step runs with the capture's parameters"""
        self.ref.p = self.cprm[self.pidx if pidx is None else pidx]
        self.ref.step(rpm)
        self.ref.p = self.cprm[self.pidx]

    def _isr(self, t, pidx=None, **kw):
        self._rx(t)
        self._step(self._est(t, **kw), pidx)
        return self.frames()

    # ---- ops
    def apply(self, op):
        o, t, out = name(op), self.t, None
        if o in ("fused", "fused_dev", "three"):
            out = self._isr(t)
        elif o == "split":
            out = self._isr(t, yaw="imu")
        elif o == "caller_rpm":
            out = self._isr(t, rpm="caller")
            self.can_split += 1
        elif o == "caller_sums":
            self._rx(t)
            self._est(t, rpm="caller", sums="caller")
        elif o == "predict_only":
            self._rx(t)
            self._est(t, correct=False)
        elif o == "correct_only":
            self._est(t, predict=False)
        elif o == "ingest_only":
            self._rx(t)
        elif o == "control_rpm":
            self._step(self.inp.rpm[t])
        elif o == "set_power":
            self.ref.set_power(self.inp.power(t))
        elif o == "set_target":
            self.ref.set_target_vel(*self.inp.target(t))
        elif o == "set_params":
            self.pidx = self.inp.params(t)
            self.ref.p = self.cprm[self.pidx]
        elif o == "reset":  # the parameters and the graph stay
            self._zero()
        elif o == "ckpt":  # a new handle: no graph, its host-side launch-form counters at zero
            self.graph = None
            self.can_split = 0
        elif o == "capture":
            self.graph = (op[1], self.pidx)
        elif o == "replay":
            for _ in range(op[1]):
                out = self.replay_once()
        elif o == "launch":  # k launches on the same inputs
            for _ in range(op[1]):
                out = self.replay_once(advance=False)
            self.t += KINDS[self.graph[0]][0]
        elif o not in READS:
            raise ValueError(op)
        if o not in NO_INPUT and o not in ("replay", "launch"):
            self.t += 1
        return out

    def replay_once(self, advance=True):
        """one launch of the captured graph on the inputs of the next tick(s)"""
        kind, pidx = self.graph
        t, out = self.t, None
        if kind == "fused_dev":
            out = self._isr(t, pidx)
        elif kind == "fused_dev2":
            self._isr(t, pidx)
            out = self._isr(t + 1, pidx)
        elif kind == "split":
            out = self._isr(t, pidx, yaw="imu")
        elif kind == "caller_sums":
            self._rx(t)
            self._est(t, rpm="caller", sums="caller")
        elif kind == "control_rpm":
            self._step(self.inp.rpm[t], pidx)
        elif kind == "set_power":
            self.ref.set_power(self.inp.power(t))
        elif kind == "ingest_only":
            self._rx(t)
        else:
            raise ValueError(kind)
        if advance:
            self.t += KINDS[kind][0]
        return out
