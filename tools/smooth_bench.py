"""Time fmskf_tick_many_smooth: its forward and backward pass, x only and with P_s, by kernel
time (fmskf_set_timing), against the yardsticks fmskf_tick_many(T) and T x fmskf_tick of the
package given with --yardstick-pkg (the parent commit's roboken-fmskf-robot-controller_amd, built:
its fmskf/ and lib/libfmskf.so) on the same inputs.

  python tools/smooth_bench.py --yardstick-pkg /path/to/parent/roboken-fmskf-robot-controller_amd --out smooth_bench.json

2^20 robots, T = 64, device records, the workspace and the outputs allocated beforehand; --passes
alternating passes of --reps calls each, the minimum and the median of every row reported.  The
passes are told apart by FMSKF_SMOOTH_TIME (csrc/api_smooth.cpp), which lets the timing events
bracket one pass alone.  Algorithmic bytes per robot-tick: forward 16 in + 108 history (the state,
216 B per robot, once per launch); backward 124 read + 24 written, + 84 written with P_s.

The yardsticks run in a child process each (one library per process; the child imports the
package FMSKF_BENCH_PKG names); prints one JSON line and, with --out, writes it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.environ.get("FMSKF_BENCH_PKG") or os.path.join(ROOT, "roboken-fmskf-robot-controller_amd")]

SEED = 64


def ring(n, T):
    import fmskf
    from fmskf.synth import kf6_ring_torch
    return fmskf.kf6_records(*kf6_ring_torch(n, T, seed=SEED))


def row(ms, T, bytes_per_tick):
    best = min(ms)
    return dict(ms_per_tick=best / T, ms_per_tick_median=statistics.median(ms) / T,
                algo_TBps=bytes_per_tick / (best / T * 1e-3) / 1e12, samples=len(ms))


def yardstick(args):
    """(child) fmskf_tick_many(T) and T x fmskf_tick of the package this process imported"""
    import torch
    import fmskf
    n, T = args.n, args.ticks
    rec = ring(n, T)
    many, single = [], []
    with fmskf.Engine("kf6", n) as e:
        e.set_stream(torch.cuda.current_stream())
        prep = [e.prepare(kf6_rec=rec[t]) for t in range(T)]
        e.tick_many(T, kf6_rec=rec)
        for p in prep:
            e.tick_prepared(p)
        for _ in range(args.passes):
            for _ in range(args.reps):
                e.set_timing(True)
                e.tick_many(T, kf6_rec=rec)
                many.append(e.last_kernel_ms())
            for _ in range(args.reps):
                e.set_timing(True)
                for p in prep:
                    e.tick_prepared(p)
                tot, cnt = e.kernel_time_total()
                assert cnt == T
                single.append(tot)
        e.set_timing(False)
    b = 232.0 * n
    print("YARDSTICK " + json.dumps(dict(tick_many=row(many, T, (16 + 216 / T) * n), tick=row(single, T, b))))


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
    assert torch.cuda.is_available(), "smooth_bench needs a GPU"
    res["device"] = torch.cuda.get_device_name(0)
    rec = ring(n, T)
    ox = torch.empty((T, 6, n), dtype=torch.float32, device="cuda")
    oP = torch.empty((T, 21, n), dtype=torch.float32, device="cuda")
    ms = {(v, p): [] for v in ("x", "xP") for p in ("both", "fwd", "bwd")}
    with fmskf.Engine("kf6", n) as e:
        e.set_stream(torch.cuda.current_stream())
        e.smooth_reserve(T)
        res["workspace_bytes"] = e.smooth_workspace_bytes(T)
        for v in ("x", "xP"):   # warm every kernel the timed window uses
            e.tick_many_smooth(T, out_x=ox, out_P=oP if v == "xP" else None, kf6_rec=rec)
        e.set_timing(True)
        for _ in range(args.passes):
            for v in ("x", "xP"):
                for p in ("both", "fwd", "bwd"):
                    os.environ["FMSKF_SMOOTH_TIME"] = p
                    for _ in range(args.reps):
                        e.tick_many_smooth(T, out_x=ox, out_P=oP if v == "xP" else None, kf6_rec=rec)
                        ms[(v, p)].append(e.last_kernel_ms())
        os.environ.pop("FMSKF_SMOOTH_TIME")
        e.set_timing(False)
    fwd_b = (16 + 108 + 216 / T) * n
    bwd_b = {"x": (124 + 24) * n, "xP": (124 + 24 + 84) * n}
    for v in ("x", "xP"):
        res[v] = dict(both=row(ms[(v, "both")], T, fwd_b + bwd_b[v]), forward=row(ms[(v, "fwd")], T, fwd_b),
                      backward=row(ms[(v, "bwd")], T, bwd_b[v]))
    yard = res.get("parent", res["this"])
    res["yardstick"] = "parent" if "parent" in res else "this"
    res["ratio_to_tick_many"] = {v: res[v]["both"]["ms_per_tick"] / yard["tick_many"]["ms_per_tick"] for v in ("x", "xP")}
    res["ratio_to_ticks"] = {v: res[v]["both"]["ms_per_tick"] / yard["tick"]["ms_per_tick"] for v in ("x", "xP")}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
