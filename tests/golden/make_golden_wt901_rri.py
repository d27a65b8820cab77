"""Generate tests/golden/wt901_rri_ref.npz from the REFERENCE's own WT901 SDK.

Register replies (0x5F frames) at read-register indices other than Q0: lib/wt901c/wit_c_sdk.c
(compiled unmodified by oracle/Makefile into oracle/_ref/libwit_ref.so) is run at each of the 30
indices of tests/wt901_rri.py over seeded streams of that module's ten poll kinds, ten polls a
stream, polls 2 and 6 latching (WitInit before their bytes, as IMU_IF_WT901C::init does).  After
every poll the file records sReg[0x90] and the register-update callbacks (reg, num) the SDK fired.

The SDK keeps its byte count (s_uiWitDataCnt) private, so `pending` is the oracle's count,
recorded only after the oracle's register file and callbacks were found equal to the SDK's at
every poll of the stream (asserted here); a wrong count would move the registers of the polls
that follow.

Streams per index: 14 at 0x51-0x54 (only there can a reply complete a poll), 8 elsewhere; the
seed is one at which the coverage conditions of tests/wt901_rri.py hold (asserted below).

Run only where the reference exists:  python tests/golden/make_golden_wt901_rri.py
The output is data (inputs and expected outputs), committed; nothing of the reference travels
with it.
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "roboken-fmskf-robot-controller_amd"), os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

from oracle import oracle  # noqa: E402
import wt901_rri as W  # noqa: E402

OUT = os.path.join(HERE, "wt901_rri_ref.npz")
SEED = 0x5F0002


def n_streams(rri):
    return 14 if 0x51 <= rri <= 0x54 else 8


def save_npz(path, **arrays):
    """np.savez_compressed with fixed member timestamps: the same arrays give the same file"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(a), version=(1, 0), allow_pickle=False)
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            z.writestr(zi, buf.getvalue(), compresslevel=9)


def main(out=OUT):
    oracle.build()
    rri_l, npolls, plen, allb, latch, kind, regs, pend, cb_cnt, cb_reg, cb_num = ([] for _ in range(11))
    for rri in W.RRIS:
        rng = np.random.default_rng([SEED, rri])
        for _ in range(n_streams(rri)):
            seq = W.draw_sequence(rng)
            ref, orc = oracle.RefWt901(rri), oracle.Wt901(rri)
            rri_l.append(rri)
            npolls.append(len(seq))
            for k, (kd, p) in enumerate(seq):
                lt = k in W.LATCH
                if lt:
                    ref.latch()
                    orc.s.cnt = 0
                ref.feed(p)
                orc.feed(p)
                r, cbs = ref.regs(), ref.take_cb()
                assert np.array_equal(orc.regs, r) and orc.take_cb() == cbs, (hex(rri), k, kd)
                plen.append(len(p))
                allb.append(np.frombuffer(p, np.uint8))
                latch.append(lt)
                kind.append(W.KINDS.index(kd))
                regs.append(r)
                pend.append(len(orc.parser))
                cb_cnt.append(len(cbs))
                cb_reg += [c[0] for c in cbs]
                cb_num += [c[1] for c in cbs]
    save_npz(
        out,
        read_reg_index=np.array(rri_l, np.uint32),
        n_polls=np.array(npolls, np.uint32),
        poll_len=np.array(plen, np.uint32),
        bytes=np.concatenate(allb).astype(np.uint8),
        latch=np.array(latch, np.uint8),
        kind=np.array(kind, np.uint8),
        kind_names=np.array(W.KINDS),
        regs=np.stack(regs).astype(np.int16),
        pending=np.array(pend, np.uint8),
        cb_count=np.array(cb_cnt, np.uint32),
        cb_reg=np.array(cb_reg, np.uint16),
        cb_num=np.array(cb_num, np.uint16),
    )
    c = W.coverage(oracle, W.fixture_fleets(W.load_fixture(out)))
    W.assert_coverage(c)
    print(f"wrote {out}: {len(npolls)} streams, {len(plen)} polls, {sum(plen)} bytes, "
          f"{len(cb_reg)} callbacks, {os.path.getsize(out)} bytes on disk")
    print(c)


if __name__ == "__main__":
    main()
