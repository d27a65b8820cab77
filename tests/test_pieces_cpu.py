"""The output pieces of fmskf_tick_many_loglik and fmskf_tick_many_em (csrc/window_pieces.hpp) on the
CPU: the stand-alone host program tests/native/piece_table.cpp, built here with g++ from that header
alone, prints the plan of the device mirror -- its size, and per piece the offset, the bytes of a
row, the bytes between rows and the rows.  The expected values are literals (nothing is imported
from the header under test): a piece's bytes are rows x step x elem rounded up to 256, a plain [N]
plane and the total are one row of N (4 or 34 for the total) elements, a multi-row plane has the
caller's pitch between its rows and N elements in each.

pitch = 2^62 overflows the arithmetic: the plan itself fails (FMSKF_ENOMEM).  pitch = 2^44 does
not: the plan asks for 1.9e15 / 4.3e15 bytes, which the allocation behind it refuses with the same
code (tests/test_gpu_loglik.py, tests/test_gpu_em.py test_errors_change_nothing).  No GPU."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (call, N, pitch) -> answer line
PLANS = {
    ("loglik", 1, 0): "1536 | 0 4 4 1 | 256 8 8 1 | 512 8 8 1 | 768 8 8 4 | 1024 8 8 10 | 1280 32 32 1",
    ("loglik", 257, 0): "35328 | 0 1028 1028 1 | 1280 2056 2056 1 | 3584 2056 2056 1 | 5888 2056 2056 4 | "
                        "14336 2056 2056 10 | 35072 32 32 1",
    ("loglik", 257, 300): "39936 | 0 1028 1028 1 | 1280 2056 2056 1 | 3584 2056 2056 1 | 5888 2056 2400 4 | "
                          "15616 2056 2400 10 | 39680 32 32 1",
    ("em", 1, 0): "1280 | 0 4 4 1 | 256 8 8 21 | 512 8 8 10 | 768 272 272 1",
    ("em", 257, 0): "65792 | 0 1028 1028 1 | 1280 2056 2056 21 | 44544 2056 2056 10 | 65280 272 272 1",
    ("em", 257, 300): "76288 | 0 1028 1028 1 | 1280 2056 2400 21 | 51712 2056 2400 10 | 75776 272 272 1",
}
# N = 257, pitch = 300: the padded bytes of every piece, and the rest of its answer
PADDED = {"loglik": [1280, 2304, 2304, 9728, 24064, 256], "em": [1280, 50432, 24064, 512]}
SHAPE = {"loglik": ["1028 1028 1", "2056 2056 1", "2056 2056 1", "2056 2400 4", "2056 2400 10", "32 32 1"],
         "em": ["1028 1028 1", "2056 2400 21", "2056 2400 10", "272 272 1"]}


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("pieces") / "piece_table")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", os.path.join(ROOT, "tests", "native", "piece_table.cpp"),
                    "-o", exe], check=True)

    def run(lines):
        out = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True,
                             check=True).stdout.splitlines()
        assert len(out) == len(lines)
        return out
    return run


def test_plans(table):
    keys = list(PLANS)
    got = table([f"{c} {n} {p} 0" for c, n, p in keys])
    assert got == [PLANS[k] for k in keys]


@pytest.mark.parametrize("call", ["loglik", "em"])
def test_one_null_pointer(table, call):
    """a null piece takes no room: the pieces behind it move up by its padded bytes"""
    pad, shape = PADDED[call], SHAPE[call]
    assert PLANS[call, 257, 300].startswith(f"{sum(pad)} | 0 ")
    got = table([f"{call} 257 300 {1 << k}" for k in range(len(pad))])
    for null, line in enumerate(got):
        off, want = 0, []
        for k, b in enumerate(pad):
            want.append("-" if k == null else f"{off} {shape[k]}")
            off += 0 if k == null else b
        assert line == " | ".join([str(sum(pad) - pad[null])] + want), (null, line)


def test_overflow(table):
    got = table([f"loglik 4113 {1 << 62} 0", f"em 4113 {1 << 62} 0", f"loglik 4113 {1 << 62} 55",
                 f"loglik 4113 {1 << 44} 0", f"em 4113 {1 << 44} 0"])
    assert got[:2] == ["ENOMEM", "ENOMEM"]
    # only the innovation sums asked for, as tests/test_gpu_loglik.py does: 4 x 2^62 x 8 bytes
    assert got[2] == "ENOMEM"
    # 2^44: n_meas 16640, nis_sum and logdet_sum 33024 each, the total 256 / 512, and 14 / 31 rows of
    # 2^44 doubles -- beyond any device, within 64 bits
    assert got[3].split(" | ")[0] == str(16640 + 2 * 33024 + 256 + 14 * 8 * (1 << 44)) == "1970324837057536"
    assert got[4].split(" | ")[0] == str(16640 + 512 + 31 * 8 * (1 << 44)) == "4362862139032320"
