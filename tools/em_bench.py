"""Time fmskf_tick_many_em: its forward and backward pass (the fold of the total included), with
the fleet total alone and with the per-robot sums as well, by kernel time (fmskf_set_timing),
against the yardstick fmskf_tick_many_smooth with P_s to device outputs of the package given with
--yardstick-pkg (the parent commit's roboken-fmskf-robot-controller_amd, built: its fmskf/ and
lib/libfmskf.so) on the same records -- the only way to these operands without this call, before
any host reduction.  The same yardstick of this build is timed too: the spread between the two
builds is the margin.

  python tools/em_bench.py --yardstick-pkg /path/to/parent/roboken-fmskf-robot-controller_amd --out em_bench.json

2^20 robots, T = 64, device records, the workspace reserved (the yardstick's outputs allocated
beforehand, the EM call's few megabytes from torch's caching allocator); --passes alternating passes of --reps calls each, the minimum and the median of every row
reported.  The passes are told apart by FMSKF_SMOOTH_TIME (csrc/api_smooth.cpp), which lets the
timing events bracket one pass alone.  Algorithmic bytes per robot-tick: forward 16 in + 108
history (the state, 216 B per robot, once per launch); backward 124 read, and 4 + 31 * 8 B per
robot and launch written with the per-robot sums (the smoother's: 124 read + 108 written).

The yardsticks run in a child process each (one library per process; the child imports the
package FMSKF_BENCH_PKG names), before this process opens the GPU; prints one JSON line and, with
--out, writes it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.environ.get("FMSKF_BENCH_PKG") or os.path.join(ROOT, "roboken-fmskf-robot-controller_amd")]

SEED = 64
PASSES = ("both", "fwd", "bwd")
VARIANTS = {"total": dict(per_robot=False, total=True), "per_robot_total": dict(per_robot=True, total=True)}


def ring(n, T):
    import fmskf
    from fmskf.synth import kf6_ring_torch
    return fmskf.kf6_records(*kf6_ring_torch(n, T, seed=SEED))


def row(ms, T, bytes_per_tick):
    best = min(ms)
    return dict(ms_per_tick=best / T, ms_per_tick_median=statistics.median(ms) / T,
                algo_TBps=bytes_per_tick / (best / T * 1e-3) / 1e12, samples=len(ms))


def timed(args, call):
    """{pass: [ms]} of call(), --passes alternating passes of --reps calls"""
    ms = {p: [] for p in PASSES}
    for _ in range(args.passes):
        for p in PASSES:
            os.environ["FMSKF_SMOOTH_TIME"] = p
            for _ in range(args.reps):
                ms[p].append(call())
    os.environ.pop("FMSKF_SMOOTH_TIME")
    return ms


def rows(ms, T, n, bwd_bytes):
    fwd_b = (16 + 108 + 216 / T) * n
    return dict(both=row(ms["both"], T, fwd_b + bwd_bytes), forward=row(ms["fwd"], T, fwd_b),
                backward=row(ms["bwd"], T, bwd_bytes))


def yardstick(args):
    """(child) fmskf_tick_many_smooth with P_s, device outputs, of the package this process imported"""
    import torch
    import fmskf
    n, T = args.n, args.ticks
    rec = ring(n, T)
    ox = torch.empty((T, 6, n), dtype=torch.float32, device="cuda")
    oP = torch.empty((T, 21, n), dtype=torch.float32, device="cuda")
    with fmskf.Engine("kf6", n) as e:
        e.set_stream(torch.cuda.current_stream())
        e.smooth_reserve(T)
        e.tick_many_smooth(T, out_x=ox, out_P=oP, kf6_rec=rec)
        e.set_timing(True)

        def call():
            e.tick_many_smooth(T, out_x=ox, out_P=oP, kf6_rec=rec)
            return e.last_kernel_ms()

        ms = timed(args, call)
        e.set_timing(False)
    print("YARDSTICK " + json.dumps(dict(smooth_xP=rows(ms, T, n, (124 + 108) * n))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--ticks", type=int, default=64)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--yardstick-pkg", default=None, help="the parent commit's package directory, built")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return yardstick(args)
    n, T = args.n, args.ticks

    def child(pkg):
        env = dict(os.environ)
        env.pop("FMSKF_LIB", None)
        if pkg:
            env["FMSKF_BENCH_PKG"] = os.path.abspath(pkg)
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--n", str(n), "--ticks", str(T),
                              "--passes", str(args.passes), "--reps", str(args.reps)], env=env, capture_output=True,
                             text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-3000:]
        return json.loads(next(ln for ln in out.stdout.splitlines() if ln.startswith("YARDSTICK "))[10:])

    res = dict(n=n, T=T, passes=args.passes, reps=args.reps)
    if args.yardstick_pkg:   # the children first: this process has not opened the GPU yet
        res["parent"] = child(args.yardstick_pkg)
    res["this"] = child(None)
    import torch
    import fmskf
    assert torch.cuda.is_available(), "em_bench needs a GPU"
    res["device"] = torch.cuda.get_device_name(0)
    rec = ring(n, T)
    with fmskf.Engine("kf6", n) as e:
        e.set_stream(torch.cuda.current_stream())
        e.smooth_reserve(T)
        res["workspace_bytes"] = e.smooth_workspace_bytes(T)
        for opt in VARIANTS.values():   # warm every kernel the timed window uses
            e.tick_many_em(T, kf6_rec=rec, **opt)
        e.set_timing(True)
        for v, opt in VARIANTS.items():
            def call():
                e.tick_many_em(T, kf6_rec=rec, **opt)   # outputs from torch's caching allocator
                return e.last_kernel_ms()
            res[v] = rows(timed(args, call), T, n, (124 + (252 / T if opt["per_robot"] else 0)) * n)
        e.set_timing(False)
        tot = e.tick_many_em(T, kf6_rec=rec)["total"]
        torch.cuda.synchronize()
        tot = tot.cpu().numpy()
    res["left_out"] = float(tot[2])
    res["r_diag_fit"] = [float(tot[24 + k] / tot[1]) for k in (0, 2, 5, 9)]
    yard = res.get("parent", res["this"])
    res["yardstick"] = "parent" if "parent" in res else "this"
    y = yard["smooth_xP"]
    res["ratio_to_smooth_xP"] = {v: {p: res[v][p]["ms_per_tick"] / y[p]["ms_per_tick"] for p in ("both", "forward", "backward")}
                                 for v in VARIANTS}
    if "parent" in res:
        res["yardstick_build_spread"] = {p: abs(res["this"]["smooth_xP"][p]["ms_per_tick"] / y[p]["ms_per_tick"] - 1.0)
                                         for p in ("both", "forward", "backward")}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
