"""Time fmskf_tick_many_loglik: the likelihood-only launch, the innovation-sum launch and the
launch with the fleet total (its fold included), by kernel time (fmskf_set_timing), against the
yardstick fmskf_tick_many(T) of the package given with --yardstick-pkg (the parent commit's
roboken-fmskf-robot-controller_amd, built: its fmskf/ and lib/libfmskf.so) on the same inputs.

  python tools/loglik_bench.py --yardstick-pkg /path/to/parent/roboken-fmskf-robot-controller_amd --out loglik_bench.json

2^20 robots, T = 64, device records, device outputs; --passes alternating
passes of --reps calls each over the variants, the minimum and the median of every row reported.
Algorithmic bytes per robot and launch: 108 + 16 T read and 108 + 20 written, + 112 with the
innovation sums (tick_many: 216 + 16 T).

The yardstick runs in a child process per package (one library per process; the child imports
the package FMSKF_BENCH_PKG names), before this process opens the GPU; prints one JSON line and,
with --out, writes it."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.environ.get("FMSKF_BENCH_PKG") or os.path.join(ROOT, "roboken-fmskf-robot-controller_amd")]

SEED = 64
VARIANTS = {"likelihood": dict(moments=False, total=False), "likelihood_total": dict(moments=False, total=True),
            "innovation_sums": dict(moments=True, total=False)}


def ring(n, T):
    import fmskf
    from fmskf.synth import kf6_ring_torch
    return fmskf.kf6_records(*kf6_ring_torch(n, T, seed=SEED))


def row(ms, T, bytes_per_launch):
    best = min(ms)
    return dict(ms_per_tick=best / T, ms_per_tick_median=statistics.median(ms) / T, ms_per_launch=best,
                algo_TBps=bytes_per_launch / (best * 1e-3) / 1e12, samples=len(ms))


def yardstick(args):
    """(child) fmskf_tick_many(T) of the package this process imported"""
    import torch
    import fmskf
    n, T = args.n, args.ticks
    rec = ring(n, T)
    many = []
    with fmskf.Engine("kf6", n) as e:
        e.set_stream(torch.cuda.current_stream())
        e.tick_many(T, kf6_rec=rec)
        e.set_timing(True)
        for _ in range(args.passes * args.reps):
            e.tick_many(T, kf6_rec=rec)
            many.append(e.last_kernel_ms())
        e.set_timing(False)
    print("YARDSTICK " + json.dumps(dict(tick_many=row(many, T, (216 + 16 * T) * n))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1 << 20)
    ap.add_argument("--ticks", type=int, default=64)
    ap.add_argument("--passes", type=int, default=3)
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
    assert torch.cuda.is_available(), "loglik_bench needs a GPU"
    res["device"] = torch.cuda.get_device_name(0)
    rec = ring(n, T)
    ms = {v: [] for v in VARIANTS}
    with fmskf.Engine("kf6", n) as e:
        e.set_stream(torch.cuda.current_stream())
        for opt in VARIANTS.values():   # warm every kernel the timed window uses
            e.tick_many_loglik(T, kf6_rec=rec, **opt)
        e.set_timing(True)
        for _ in range(args.passes):
            for v, opt in VARIANTS.items():
                for _ in range(args.reps):
                    r = e.tick_many_loglik(T, kf6_rec=rec, **opt)   # outputs from torch's caching allocator
                    ms[v].append(e.last_kernel_ms())
                    if opt["total"]:
                        last = r["total"]
        e.set_timing(False)
        torch.cuda.synchronize()
        tot = last.cpu().numpy()
    res["mean_nis"] = float(tot[1] / tot[0])
    io = {"likelihood": 108 + 16 * T + 108 + 20, "likelihood_total": 108 + 16 * T + 108 + 20,
          "innovation_sums": 108 + 16 * T + 108 + 132}
    for v in VARIANTS:
        res[v] = row(ms[v], T, io[v] * n)
    yard = res.get("parent", res["this"])
    res["yardstick"] = "parent" if "parent" in res else "this"
    res["ratio_to_tick_many"] = {v: res[v]["ms_per_tick"] / yard["tick_many"]["ms_per_tick"] for v in VARIANTS}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
