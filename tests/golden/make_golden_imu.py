"""Generate tests/golden/imu_ref.npz from the REFERENCE's own IMU_IF_WT901C.

Runs IMT::IMU_IF_WT901C (src/Imu/imu_if_wt901c.cpp with src/Utility/util_mymath.hpp, on the
reference's WT901 SDK; compiled unmodified from /root/reference by oracle/Makefile into
oracle/_ref/libimu_ref.so) over seeded UART streams.  A stream is a sequence of polls; a poll
either answers init() (the q_init latch: WitInit, the register read, getDataImmediately) or is
the bytes update() finds in the serial queue.  After every poll the file records isError() and
getDataLatest() (the 16 floats of the Data page), and it stores every poll's bytes.

The reference file needs Arduino.h, CMSIS-DSP and the RTOS, which do not exist here;
oracle/ref_standin/ holds stand-ins: fixed-width integers, PI, and FreeRTOS_TEENSY4.h with a
HardwareSerial backed by a byte queue, Serial6, vTaskDelay and a general-purpose timer that
stands still.  The trig stand-ins are not used on this path.

Streams cover the standard four-frame poll, failed polls (no quaternion frame: the page
stays), a magnetometer frame inside a failed poll, damaged quaternion frames, two latches in
one stream (the second one after a failed poll; after a poll that left the head of a frame in
the parser window, with the latching poll beginning at a frame boundary, where the SDK's
resync hides whether WitInit dropped the window; and with the latching poll beginning with the
REST of the split frame, an accelerometer and a quaternion frame, where it does not: the
firmware drops the head, so the frame is lost), and normalize_deg_0to360(roll) - 180 on rolls
of both signs and at the ends of the range.  Every poll fits the 44 bytes of the standard one.

Left out, because an x86 build does not behave there as the firmware does: a latch on a poll
without a quaternion frame (init() spins for ever; asserted before the reference is called, and
the stand-in's serial port ends such a call with an error).

The SDK and the interface keep file-static state, so every stream runs in a process of its own
(this script with --stream K, answering on its standard output).

Run only where /root/reference exists:  python tests/golden/make_golden_imu.py
The output is data (inputs and expected outputs), committed; nothing of the reference travels
with it.
"""
from __future__ import annotations

import io
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

from oracle import oracle  # noqa: E402

OUT = os.path.join(HERE, "imu_ref.npz")
ACC, GYRO, ANGLE, MAG, QUAT = 0x51, 0x52, 0x53, 0x54, 0x59


def wt901_frame(ftype, w):
    """one 11-byte NORMAL-protocol frame: 0x55, type, four little-endian words, the byte sum"""
    body = bytes([0x55, ftype & 0xFF] + [b for x in w for b in (int(x) & 0xFF, (int(x) >> 8) & 0xFF)])
    return body + bytes([sum(body) & 0xFF])


def words(rng):
    return rng.integers(0, 65536, 4)


def std_poll(rng, roll=None):
    ang = words(rng)
    if roll is not None:
        ang[0] = int(roll) & 0xFFFF
    return (wt901_frame(ACC, words(rng)) + wt901_frame(GYRO, words(rng)) + wt901_frame(ANGLE, ang) +
            wt901_frame(QUAT, words(rng)))


def no_quat(rng, *types):
    return b"".join(wt901_frame(t, words(rng)) for t in types)


def damaged(fr: bytes) -> bytes:
    b = bytearray(fr)
    b[10] ^= 0x5A
    return bytes(b)


def streams(rng):
    """list of (name, [(bytes, latch)])"""
    S = []
    S.append(("standard", [(std_poll(rng), 1)] + [(std_poll(rng), 0) for _ in range(20)]))
    p = [(std_poll(rng), 1)]
    for k in range(20):
        p.append((std_poll(rng), 0) if k % 3 == 0 else (no_quat(rng, ACC, GYRO, ANGLE), 0))
    S.append(("failed_polls", p))
    p = [(std_poll(rng), 1), (std_poll(rng), 0)]
    for k in range(6):
        p += [(no_quat(rng, ACC, MAG, ANGLE), 0), (no_quat(rng, MAG), 0), (std_poll(rng), 0),
              (no_quat(rng, GYRO, MAG, ANGLE, ACC), 0), (wt901_frame(QUAT, words(rng)), 0)]
    S.append(("mag_in_failed_poll", p))
    p = [(wt901_frame(QUAT, words(rng)), 1)]
    for k in range(12):
        q = wt901_frame(QUAT, words(rng))
        p.append((no_quat(rng, ACC, GYRO, ANGLE) + (damaged(q) if k % 2 else q), 0))
    S.append(("damaged_quaternion", p))
    p = [(std_poll(rng), 1)] + [(std_poll(rng), 0) for _ in range(6)] + [(std_poll(rng), 1)] + \
        [(std_poll(rng), 0) for _ in range(6)]
    S.append(("two_latches", p))
    p = [(std_poll(rng), 1), (std_poll(rng), 0), (no_quat(rng, ACC, GYRO), 0), (std_poll(rng), 1),
         (std_poll(rng), 0), (no_quat(rng, ANGLE), 0), (std_poll(rng), 0)]
    S.append(("latch_after_failed_poll", p))
    tail = wt901_frame(ACC, words(rng))[:6]
    p = [(std_poll(rng), 1), (std_poll(rng), 0), (no_quat(rng, ACC, GYRO, ANGLE) + tail, 0), (std_poll(rng), 1),
         (std_poll(rng), 0), (std_poll(rng)[:40], 0), (std_poll(rng), 1), (std_poll(rng), 0)]
    S.append(("latch_at_frame_boundary_after_partial", p))
    rolls = [0, 1, -1, 16384, -16384, 32767, -32768, 8192, -8192, 100, -100, 32766, -32767]
    p = [(std_poll(rng, 0), 1)] + [(std_poll(rng, r), 0) for r in rolls] + \
        [(std_poll(rng, int(r)), 0) for r in rng.integers(-32768, 32768, 12)]
    S.append(("rolls_both_signs", p))
    # WitInit (s_uiWitDataCnt = 0) at the head of init(): the head of a frame split across the
    # poll before is dropped, the rest arriving with the latching poll is resynced away
    acc, q = wt901_frame(ACC, words(rng)), wt901_frame(QUAT, words(rng))
    p = [(std_poll(rng), 1), (std_poll(rng), 0), (no_quat(rng, GYRO, ANGLE) + acc[:6], 0),
         (acc[6:] + no_quat(rng, GYRO, ANGLE, QUAT), 1), (std_poll(rng), 0),
         (no_quat(rng, ACC, GYRO) + q[:7], 0), (q[7:] + no_quat(rng, ANGLE, MAG, QUAT), 1), (std_poll(rng), 0),
         (no_quat(rng, ANGLE) + acc[:10], 0), (acc[10:] + std_poll(rng)[:33], 0), (std_poll(rng), 0)]
    S.append(("latch_drops_split_frame", p))
    return S


def has_quat(orc_imu, data):
    """would this poll complete (a quaternion frame parsed)?  asked of a copy of the oracle's parser"""
    c = oracle.Wt901()
    c.s = type(orc_imu.s).from_buffer_copy(orc_imu.s)
    c.s.cnt = 0  # asked only of latching polls: init() begins with WitInit
    return c.feed(data)


def run_stream(k):
    """in a process of its own: (data [P][16], is_error [P]) of stream k from the reference"""
    rng = np.random.default_rng(0x494D5539)
    name, polls = streams(rng)[k]
    imu = oracle.RefImu()
    shadow = oracle.Wt901()  # the oracle's parser, only to assert the exclusion below
    data, err = [], []
    for b, latch in polls:
        assert len(b) <= 44, (name, len(b))
        if latch:
            assert has_quat(shadow, b), (name, "a latch on a poll without a quaternion frame")
            imu.init(b)
        else:
            imu.poll(b)
        shadow.update(b, latch_qinit=bool(latch))
        d, e = imu.read()
        data.append(d)
        err.append(e)
    return np.stack(data), np.array(err, np.uint8)


def generate():
    """the fixture as a dict of arrays"""
    oracle.build()
    rng = np.random.default_rng(0x494D5539)
    S = streams(rng)
    data, err = [], []
    for k in range(len(S)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--stream", str(k)], check=True,
                           stdout=subprocess.PIPE)
        z = np.load(io.BytesIO(r.stdout))
        data.append(z["data"])
        err.append(z["is_error"])
    polls = [p for _, ps in S for p in ps]
    return dict(name=np.array([n for n, _ in S]), n_polls=np.array([len(ps) for _, ps in S], np.uint32),
                poll_len=np.array([len(b) for b, _ in polls], np.uint32),
                latch=np.array([l for _, l in polls], np.uint8),
                bytes=np.frombuffer(b"".join(b for b, _ in polls), np.uint8).copy(),
                data=np.concatenate(data), is_error=np.concatenate(err))


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--stream":
        d, e = run_stream(int(sys.argv[2]))
        buf = io.BytesIO()
        np.savez(buf, data=d, is_error=e)
        sys.stdout.buffer.write(buf.getvalue())
        return
    d = generate()
    np.savez_compressed(OUT, **d)
    print(f"wrote {OUT}: {len(d['name'])} streams, {len(d['latch'])} polls, {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
