"""WT901 register replies (0x5F frames at imu_read_reg indices other than Q0) meeting registers
that live in the snapshot row: the poll sequences of tests/test_gpu_wt901_rri.py, the streams of
tests/golden/wt901_rri_ref.npz (make_golden_wt901_rri.py) and the coverage counts that
tests/test_wt901_rri_cpu.py asserts on both.

A poll is one of ten kinds, drawn by a seeded generator:

  S    the standard four frames 0x51 0x52 0x53 0x59
  R    0x5F alone
  RQ   0x5F 0x59 (the quaternion frame lands on reply-written words)
  QR   0x59 0x5F (the reply lands after the quaternion)
  S+R  five whole frames, 55 bytes: whole frames, but not the standard poll
  M    0x54 0x51: fails and writes HX-HZ
  MQ   0x54 0x59 0x52
  D    a standard poll with one damaged byte
  T    a standard poll cut at a random byte; its tail opens the next poll
  E    empty

No poll is longer than 64 bytes (the widest row the vector kernel takes): the kind after a T is
drawn again until tail and content fit.  A narrower row clips the poll (`Fleet.rows`), and the
oracle is fed the clipped bytes.
"""
from __future__ import annotations

import functools

import numpy as np

# every index whose window [rri, rri + 4) touches VERSION (0x2E), AX..TEMP (0x34..0x40) or Q0-Q3
# (0x51..0x54), and the plain cases 0x00, 0x41, 0x8C
RRIS = [0x00] + list(range(0x2B, 0x2F)) + list(range(0x31, 0x42)) + list(range(0x4E, 0x55)) + [0x8C]
KINDS = ("S", "R", "RQ", "QR", "S+R", "M", "MQ", "D", "T", "E")
_WEIGHTS = np.array([0.28, 0.12, 0.08, 0.08, 0.08, 0.12, 0.06, 0.06, 0.06, 0.06])
_CUM = np.cumsum(_WEIGHTS / _WEIGHTS.sum())
_STD = (0x51, 0x52, 0x53, 0x59)
_TYPES = {"S": _STD, "R": (0x5F,), "RQ": (0x5F, 0x59), "QR": (0x59, 0x5F), "S+R": _STD + (0x5F,),
          "M": (0x54, 0x51), "MQ": (0x54, 0x59, 0x52), "D": _STD, "T": _STD, "E": ()}
MAX_POLL = 64
N_POLLS = 10
LATCH = (2, 6)      # polls (from 0) that latch q_init
N_ROBOTS = 293      # one full block and a ragged 37
FLEET_SEED = 0x5F52

# registers by name (lib/wt901c/REG.h)
ROW_REGS = {"AX": 0x34, "AY": 0x35, "AZ": 0x36, "GX": 0x37, "GY": 0x38, "GZ": 0x39, "HX": 0x3A, "HY": 0x3B,
            "HZ": 0x3C, "Roll": 0x3D, "Pitch": 0x3E, "Yaw": 0x3F, "Q0": 0x51, "Q1": 0x52, "Q2": 0x53,
            "Q3": 0x54}


def _frames(rng, types) -> bytes:
    """whole frames of the given types with random data words"""
    k = len(types)
    if k == 0:
        return b""
    f = np.empty((k, 11), np.uint8)
    f[:, 0] = 0x55
    f[:, 1] = types
    f[:, 2:10] = rng.integers(0, 256, (k, 8), dtype=np.uint8)
    f[:, 10] = f[:, :10].sum(axis=1, dtype=np.uint32) & 0xFF
    return f.tobytes()


def draw_sequence(rng, npolls=N_POLLS):
    """one robot's polls: [(kind, bytes)]"""
    out, tail = [], b""
    for _ in range(npolls):
        while True:
            kind = KINDS[int(np.searchsorted(_CUM, rng.random(), side="right").clip(0, len(KINDS) - 1))]
            if len(tail) + 11 * len(_TYPES[kind]) <= MAX_POLL:
                break
        body, carry = _frames(rng, _TYPES[kind]), b""
        if kind == "D":
            b = bytearray(body)
            k = int(rng.integers(0, len(b)))
            b[k] = (b[k] + int(rng.integers(1, 256))) & 0xFF
            body = bytes(b)
        elif kind == "T":
            c = int(rng.integers(1, len(body)))
            body, carry = body[:c], body[c:]
        out.append((kind, tail + body))
        tail = carry
    return out


class Fleet:
    """n robots' sequences at one register index as rows: bufs [P][n][64] uint8, lens [P][n]
    uint32, kinds [n][P] (indices into KINDS)"""

    def __init__(self, rri, seqs, latch=LATCH):
        self.rri, self.n, self.latch = int(rri), len(seqs), tuple(latch)
        self.npolls = len(seqs[0])
        assert all(len(s) == self.npolls for s in seqs)
        self.bufs = np.zeros((self.npolls, self.n, MAX_POLL), np.uint8)
        self.lens = np.zeros((self.npolls, self.n), np.uint32)
        self.kinds = np.zeros((self.n, self.npolls), np.uint8)
        for i, s in enumerate(seqs):
            for k, (kind, b) in enumerate(s):
                assert len(b) <= MAX_POLL
                self.bufs[k, i, :len(b)] = np.frombuffer(b, np.uint8)
                self.lens[k, i] = len(b)
                self.kinds[i, k] = KINDS.index(kind)

    def rows(self, k, stride=MAX_POLL):
        """poll k as ([n][stride] rows, [n] lens): clipped to a narrower row, padded to a wider"""
        buf = np.zeros((self.n, stride), np.uint8)
        w = min(stride, MAX_POLL)
        lens = np.minimum(self.lens[k], stride).astype(np.uint32)
        buf[:, :w] = self.bufs[k][:, :w]
        buf[np.arange(stride)[None, :] >= lens[:, None]] = 0
        return buf, lens


@functools.lru_cache(maxsize=None)
def fleet(rri, n=N_ROBOTS) -> Fleet:
    """the GPU tests' sequences at index rri: every robot its own"""
    rng = np.random.default_rng([FLEET_SEED, int(rri)])
    return Fleet(rri, [draw_sequence(rng) for _ in range(n)])


def _covers(cnt, reg, num, r):
    """[n] bool: a callback of the poll wrote register r"""
    live = np.arange(reg.shape[1])[None, :] < cnt[:, None]
    return (live & (reg <= r) & (r < reg.astype(np.int64) + num)).any(axis=1)


def coverage(orc, fleets, stride=MAX_POLL):
    """The coverage counts of `fleets` (Fleet objects) at a row stride, from the oracle alone.

    A second oracle with read_reg_index 0 sees the same bytes: the parser does not depend on the
    index, and nothing but a reply writes register 0, so its callback (0, 4) marks the polls in
    which a reply was dispatched, and a poll that completes at the real index but not at index 0
    completes only because a reply covered Q3.

    reply[name]   robot-polls in which a reply writes that register and the robot's previous poll
                  was a standard poll taken with an empty window (its thirteen registers are
                  row-resident when the reply lands, if no readout of the register file intervenes)
    reply_only_q  polls that succeed only because a reply covered Q3
    mag_fail      failed polls that write HX-HZ after an earlier success; mag_fail_then_std /
                  mag_fail_then_mag: those directly followed by a standard poll (empty window) /
                  by another failed poll that writes HX-HZ
    at_latch / after_latch   the kinds seen at a latching poll / directly after one
    """
    c = {"reply": {k: 0 for k in ROW_REGS}, "reply_only_q": 0, "mag_fail": 0, "mag_fail_then_std": 0,
         "mag_fail_then_mag": 0, "at_latch": set(), "after_latch": set()}
    for fl in fleets:
        real, shadow = orc.Wt901Batch(fl.n, fl.rri), orc.Wt901Batch(fl.n, 0x00)
        had_ok = np.zeros(fl.n, bool)
        prev_std = np.zeros(fl.n, bool)
        prev_magfail = np.zeros(fl.n, bool)
        for k in range(fl.npolls):
            buf, lens = fl.rows(k, stride)
            latch = k in fl.latch
            empty = (real.pending == 0) | latch
            real.update(buf, lens, latch_qinit=latch)
            shadow.update(buf, lens, latch_qinit=latch)
            cb, scb = real.take_cb(), shadow.take_cb()
            reply = _covers(*scb, 0x00)
            ok = _covers(*cb, 0x54)
            ok0 = _covers(*scb, 0x54)
            std = (fl.kinds[:, k] == KINDS.index("S")) & empty & (lens == 44)
            assert not np.any(std & ~ok)
            for name, r in ROW_REGS.items():
                if fl.rri <= r < fl.rri + 4:
                    c["reply"][name] += int((reply & prev_std).sum())
            c["reply_only_q"] += int((ok & ~ok0).sum())
            mag = _covers(*cb, 0x3A) | _covers(*cb, 0x3B) | _covers(*cb, 0x3C)
            magfail = mag & ~ok
            c["mag_fail_then_std"] += int((prev_magfail & std).sum())
            c["mag_fail_then_mag"] += int((prev_magfail & magfail).sum())
            prev_magfail = magfail & had_ok
            c["mag_fail"] += int(prev_magfail.sum())
            had_ok |= ok
            prev_std = std
            if latch:
                c["at_latch"] |= {KINDS[j] for j in np.unique(fl.kinds[:, k])}
            if k - 1 in fl.latch:
                c["after_latch"] |= {KINDS[j] for j in np.unique(fl.kinds[:, k])}
    return c


def assert_coverage(c):
    """the conditions that keep a reshuffle of the generator from emptying the tests"""
    for name, cnt in c["reply"].items():
        assert cnt >= 20, (name, cnt)
    assert c["reply_only_q"] >= 50, c["reply_only_q"]
    assert c["mag_fail"] >= 50, c["mag_fail"]
    assert c["mag_fail_then_std"] >= 10, c["mag_fail_then_std"]
    assert c["mag_fail_then_mag"] >= 10, c["mag_fail_then_mag"]
    assert c["at_latch"] == set(KINDS), set(KINDS) - c["at_latch"]
    assert c["after_latch"] == set(KINDS), set(KINDS) - c["after_latch"]


# ---------------------------------------------------------------------------- the fixture
def load_fixture(path):
    """tests/golden/wt901_rri_ref.npz as a list of streams: dicts with rri, polls [bytes], kinds
    [names], latch [bool], regs [P][0x90], pending [P], cbs [P][(reg, num)]"""
    with np.load(path) as z:
        g = {k: z[k] for k in z.files}
    names = [str(s) for s in g["kind_names"]]
    streams, ob, op, oc = [], 0, 0, 0
    for s, np_ in enumerate(g["n_polls"]):
        st = dict(rri=int(g["read_reg_index"][s]), polls=[], kinds=[], latch=[], regs=[], pending=[], cbs=[])
        for _ in range(int(np_)):
            L = int(g["poll_len"][op])
            st["polls"].append(bytes(g["bytes"][ob:ob + L]))
            ob += L
            st["kinds"].append(names[int(g["kind"][op])])
            st["latch"].append(bool(g["latch"][op]))
            st["regs"].append(g["regs"][op])
            st["pending"].append(int(g["pending"][op]))
            n = int(g["cb_count"][op])
            st["cbs"].append(list(zip(g["cb_reg"][oc:oc + n].tolist(), g["cb_num"][oc:oc + n].tolist())))
            oc += n
            op += 1
        streams.append(st)
    assert ob == g["bytes"].size and op == g["poll_len"].size and oc == g["cb_reg"].size
    return streams


def fixture_fleets(streams):
    """the fixture's streams grouped by index, as Fleet objects (their common latch polls)"""
    out = []
    for rri in sorted({s["rri"] for s in streams}):
        grp = [s for s in streams if s["rri"] == rri]
        latch = tuple(k for k, v in enumerate(grp[0]["latch"]) if v)
        assert all(tuple(k for k, v in enumerate(s["latch"]) if v) == latch for s in grp)
        fl = Fleet(rri, [list(zip(s["kinds"], s["polls"])) for s in grp], latch)
        fl.streams = grp
        out.append(fl)
    return out
