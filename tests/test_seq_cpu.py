"""tests/seq_ref.py without a GPU: the sequence generator keeps the ABI's rules and is
deterministic, the committed seeds cover the orderings the GPU sequences exist for
(test_gpu_sequences.py), and the reference fleet is the oracle applied one op at a time."""
import numpy as np
import pytest

import seq_ref
from seq_ref import name

LENGTH = 48  # ops per random sequence

# The seeds test_gpu_sequences.py runs, per model.  What they must cover is stated below
# (required_pairs / required_triples / the capture kinds); a seed list that misses a condition is
# replaced by another, the conditions stay.
SEEDS = {"rs": (0, 4, 14, 35, 37, 187), "kf6": (0, 1, 2, 62, 118, 142), "ekf9": (0, 1, 2, 3, 8, 272)}

BEFORE_REPLAY = ("fused", "split", "caller_rpm", "control_rpm", "set_power", "set_params", "ingest_only", "reset",
                 "read_ctrl")
AFTER_REPLAY = ("fused", "ckpt", "set_power", "control_rpm", "read_ctrl", "read_motors")


def required_pairs(model):
    """ordered pairs of neighbouring ops the model's sequences must contain between them"""
    req = [(a, "replay") for a in BEFORE_REPLAY] + [("replay", b) for b in AFTER_REPLAY]
    if model == "rs":
        req += [("caller_sums", "replay"), ("predict_only", "replay"), ("replay", "read_prev")]
    return req


def required_triples(model):
    # the second fused tick is the PS one (it skips the prev planes)
    return [("fused", "fused", "replay")] if model == "rs" else []


def sequences(model):
    return {s: seq_ref.generate(model, s, LENGTH) for s in SEEDS[model]}


def coverage(model):
    """{condition: the seeds whose sequence meets it}"""
    seqs = sequences(model)
    cov = {}
    for p in required_pairs(model):
        cov[p] = [s for s, ops in seqs.items() if p in seq_ref.pairs(ops)]
    for t in required_triples(model):
        cov[t] = [s for s, ops in seqs.items() if t in seq_ref.triples(ops)]
    for k in seq_ref.kinds(model):
        cov[("replayed", k)] = [s for s, ops in seqs.items() if k in seq_ref.replayed_kinds(ops)]
    return cov


@pytest.mark.parametrize("model", seq_ref.MODELS)
def test_generate_is_deterministic_and_keeps_the_rules(model):
    for seed in list(SEEDS[model]) + [97, 12345]:
        ops = seq_ref.generate(model, seed, LENGTH)
        assert len(ops) == LENGTH
        assert ops == seq_ref.generate(model, seed, LENGTH)
        assert ops[:20] == seq_ref.generate(model, seed, 20)  # a prefix of the longer draw
        seq_ref.check_rules(model, ops)
        # a replay follows its capture in the same handle: no ckpt in between
        graph = False
        for op in ops:
            if name(op) == "capture":
                graph = True
            elif name(op) == "ckpt":
                graph = False
            assert name(op) != "replay" or graph
        if model != "rs":
            assert not [o for o in ops if name(o) in seq_ref.RS_ONLY or o == ("capture", "caller_sums")]
    assert seq_ref.generate(model, 0, LENGTH) != seq_ref.generate(model, 1, LENGTH)
    # every op of the vocabulary and every capture kind is drawn
    seen = {name(o) for s in range(40) for o in seq_ref.generate(model, s, LENGTH)}
    assert seen == {o for o, _ in seq_ref.vocabulary(model)} | {"replay"}
    kinds = {o[1] for s in range(40) for o in seq_ref.generate(model, s, LENGTH) if name(o) == "capture"}
    assert kinds == set(seq_ref.kinds(model))


def test_check_rules_refuses_what_the_abi_refuses():
    with pytest.raises(AssertionError):
        seq_ref.check_rules("rs", [("replay", 1)])
    with pytest.raises(AssertionError):
        seq_ref.check_rules("rs", [("capture", "fused_dev"), "ckpt", ("replay", 1)])
    with pytest.raises(AssertionError):
        seq_ref.check_rules("kf6", ["read_prev"])
    with pytest.raises(AssertionError):
        seq_ref.check_rules("kf6", [("capture", "caller_sums")])
    seq_ref.check_rules("rs", [("capture", "caller_sums"), "reset", ("replay", 3), "read_prev"])


def test_half_of_the_draws_with_a_graph_are_replays():
    n_graph = n_replay = 0
    for model in seq_ref.MODELS:
        for s in range(60):
            graph = False
            for op in seq_ref.generate(model, s, LENGTH):
                n_graph += graph
                n_replay += name(op) == "replay"
                if name(op) == "capture":
                    graph = True
                elif name(op) == "ckpt":
                    graph = False
    assert 0.45 < n_replay / n_graph < 0.55, (n_replay, n_graph)


@pytest.mark.parametrize("model", seq_ref.MODELS)
def test_seeds_cover_the_orderings(model):
    assert len(SEEDS[model]) >= 6 and len(set(SEEDS[model])) == len(SEEDS[model])
    cov = coverage(model)
    missing = [c for c, seeds in cov.items() if len(seeds) < (2 if c[0] == "replayed" else 1)]
    assert not missing, f"{model}: seeds {SEEDS[model]} miss {missing}"


@pytest.mark.parametrize("model", seq_ref.MODELS)
def test_fleet_is_the_oracle_inline(orc, model):
    """20 `fused` ops through seq_ref.Fleet against the inline loop of
    test_isr_tick_can_firmware_60000_ticks on the same inputs, bit for bit."""
    import fmskf
    n, T = 257, 20
    inp = seq_ref.Inputs(model, n, T + 1, 11)
    fl = seq_ref.Fleet(orc, model, n, inp)
    fl.start()
    mb, ref = orc.MotorBatch(n), orc.CtrlBatch(n)
    ref.set_power(inp.power(-1))
    ref.set_target_vel(*inp.target(-1))
    cfg = fmskf.default_config(model, n)
    if model == "rs":
        pos, vel, prev = np.zeros((3, n), np.float32), np.zeros((3, n), np.float32), np.zeros((4, n), np.int64)
    elif model == "kf6":
        prm = orc.kf6_params(cfg.dt, np.array(cfg.q[:21]), np.array(cfg.r[:10]), orc.TRIG_TABLE512)
        xo = np.zeros((6, n), np.float32)
        Po = np.repeat(np.float32(np.array(cfg.p0[:21]))[:, None], n, 1).copy()
    else:
        prm = orc.ekf9_params(cfg.dt, np.array(cfg.q[:45]), np.array(cfg.r[:21]), orc.TRIG_TABLE512)
        xo = np.zeros((10, n), np.float32)
        Po = np.repeat(np.float32(np.array(cfg.p0[:45]))[:, None], n, 1).copy()
    for t in range(T):
        frames = fl.apply("fused")
        assert fl.t == t + 1
        mb.rx(*inp.can(t))
        rpm = mb.field("rpm")
        if model == "rs":
            orc.rs_tick(pos, vel, prev, inp.yaw[t], np.ascontiguousarray(mb.field("angle_sum").T), rpm)
        elif model == "kf6":
            orc.kf6_tick(xo, Po, inp.yaw[t], inp.gz[t], rpm, None, prm, nthreads=0)
        else:
            orc.ekf9_tick(xo, Po, inp.raw[t], None, prm, nthreads=0)
        ref.step(rpm)
        np.testing.assert_array_equal(frames, orc.can_tx(ref.curr()))
    x, P = fl.state()
    if model == "rs":
        np.testing.assert_array_equal(x.view(np.uint32), np.concatenate([pos, vel]).view(np.uint32))
        np.testing.assert_array_equal(fl.prev, prev)
        assert prev.any() and pos.any()
    else:
        np.testing.assert_array_equal(x.view(np.uint32), xo[:x.shape[0]].view(np.uint32))
        np.testing.assert_array_equal(P.view(np.uint32), Po.view(np.uint32))
    got = fl.ctrl()
    np.testing.assert_array_equal(got["curr"], ref.curr())
    for k, want in (("vel_tgt", ref.vel_tgt()), ("wheel_tgt", ref.wheel("tgt")), ("wheel_ctrl", ref.wheel("ctrl"))):
        np.testing.assert_array_equal(got[k].view(np.uint32), want.view(np.uint32))
    np.testing.assert_array_equal(fl.motors()["angle_sum"], mb.field("angle_sum").T)
    assert np.abs(ref.curr()).max() > 0  # the loops drove the wheels


@pytest.mark.parametrize("model", seq_ref.MODELS)
def test_fleet_applies_every_committed_sequence(orc, model):
    """every op of the committed sequences has its reference, within the inputs drawn for it"""
    n = 33
    for seed, ops in sequences(model).items():
        inp = seq_ref.Inputs(model, n, seq_ref.ticks_needed(ops), seed)
        fl = seq_ref.Fleet(orc, model, n, inp)
        fl.start()
        for op in ops:
            out = fl.apply(op)
            produced = name(op) in ("fused", "fused_dev", "split", "three", "caller_rpm") or \
                (name(op) == "replay" and fl.graph[0] in seq_ref.KIND_FRAMES)
            assert (out is not None) == produced, (seed, op)
        assert fl.t < inp.ticks
        x, P = fl.state()
        assert np.isfinite(x).all() and (P is None or np.isfinite(P).all())


def test_fleet_replay_is_the_captured_calls_with_the_captures_parameters(orc):
    """a capture leaves the fleet where it is; a replayed control step runs with the parameters
    of the capture, a direct one after it with the current ones"""
    n = 33
    ops = ["control_rpm", ("capture", "control_rpm"), "set_params", ("replay", 2), "control_rpm"]
    inp = seq_ref.Inputs("kf6", n, seq_ref.ticks_needed(ops), 3)
    inp.params = lambda t: 1  # the other parameter set
    fl = seq_ref.Fleet(orc, "kf6", n, inp)
    fl.start()
    ref = orc.CtrlBatch(n)
    ref.set_power(inp.power(-1))
    ref.set_target_vel(*inp.target(-1))
    fl.apply(ops[0])
    ref.step(inp.rpm[0])
    before = fl.ctrl()
    fl.apply(ops[1])
    assert fl.t == 1 and all(np.array_equal(before[k], v) for k, v in fl.ctrl().items())
    fl.apply(ops[2])
    fl.apply(ops[3])
    ref.step(inp.rpm[2])  # tick 1 went to set_params
    ref.step(inp.rpm[3])
    fl.apply(ops[4])
    ref.p = orc.ctrl_params(**seq_ref._ORC_PARAMS[1])
    ref.step(inp.rpm[4])
    assert fl.t == 5
    # ("launch", k): k launches on the same inputs, one tick of them consumed
    seq_ref.check_rules("kf6", [("capture", "ingest_only"), ("launch", 3)])
    fl.apply(("capture", "ingest_only"))
    fl.apply(("launch", 3))
    mb = orc.MotorBatch(n)
    for _ in range(3):
        mb.rx(*inp.can(5))
    assert fl.t == 6
    np.testing.assert_array_equal(fl.motors()["status_dlt_out_angle_rad"].view(np.uint32),
                                  mb.field("dlt_out_angle_rad").view(np.uint32))
    np.testing.assert_array_equal(fl.ctrl()["curr"], ref.curr())
    np.testing.assert_array_equal(fl.ctrl()["wheel_ctrl"].view(np.uint32), ref.wheel("ctrl").view(np.uint32))
