"""Factorised compact grad / div / interp (pb_compact_{grad,div,interp}_fast) against the
reference-order calls, per cubic grid: one process, the compared paths interleaved rep by rep
(fast, reference-order, fast Laplacian, ...), each rep timed on its own between two stream syncs.
One JSON line per grid and operator: the fast call's and the reference-order call's median / min /
max ms, the same process's pb_compact_lapl_fast time and copy probe, the algorithmic B/DoF, the
achieved rate as a fraction of the probe and of the Laplacian's achieved rate (its 80 B/DoF).

usage: python scripts/bench_compact_ops.py [n ...] [--reps R] [--out DIR]
writes DIR/bench_<n>.jsonl (default DIR: profiles/compact_ops) and prints the same lines."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import poissbox_amd as pb  # noqa: E402

BYTES = {"grad": 112, "div": 112, "interp": 48, "lapl": 80}


def stats(ms):
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4),
            "max_ms": round(max(ms), 4), "spread": round(max(ms) / min(ms), 4)}


def bench(ctx, n, reps):
    n3 = (n, n, n)
    h = (2 * np.pi / n,) * 3
    da = pb.DA(ctx, n3, (2 * np.pi,) * 3)
    v = [pb.Vec(da) for _ in range(5)]
    for i in range(4):
        v[i].set_random(7 + i)
    f, a, b, c, out = v
    calls = {
        "grad": (lambda: pb.compact_grad_fast(da, h, f, [a, b, c]),
                 lambda: pb.compact_grad(da, h, f, [a, b, c])),
        "div": (lambda: pb.compact_div_fast(da, h, [a, b, c], out),
                lambda: pb.compact_div(da, h, [a, b, c], out)),
        "interp": (lambda: pb.compact_interp_fast(da, -1, f, out),
                   lambda: pb.compact_interp(da, -1, f, out)),
    }
    lapl = lambda: pb.compact_lapl_fast(da, h, f, out)

    def timed(fn):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        return (time.perf_counter() - t0) * 1e3

    rows = []
    N = float(n) ** 3
    for op, (fast, ref) in calls.items():
        for fn in (fast, ref, lapl):  # warm-up: scratch, factor caches, occupancy queries
            fn()
            fn()
        t = {"fast": [], "ref": [], "lapl": []}
        for _ in range(reps):
            t["fast"].append(timed(fast))
            t["ref"].append(timed(ref))
            t["lapl"].append(timed(lapl))
        if op == "grad":  # div's inputs: random again, not the gradient just written
            for i in (1, 2, 3):
                v[i].set_random(7 + i)
        probe_best, probe_med = f.copy_probe(out, 10)
        s = {k: stats(x) for k, x in t.items()}
        rate = BYTES[op] * N / s["fast"]["median_ms"] / 1e6           # GB/s
        lapl_rate = BYTES["lapl"] * N / s["lapl"]["median_ms"] / 1e6
        rows.append({"n": n, "op": op, "reps": reps, "B_per_DoF": BYTES[op], "fast": s["fast"],
                     "ref_order": s["ref"], "lapl_fast": s["lapl"],
                     "speedup_median": round(s["ref"]["median_ms"] / s["fast"]["median_ms"], 3),
                     "copy_probe_GBps": {"best": round(probe_best, 1), "median": round(probe_med, 1)},
                     "fast_GBps": round(rate, 1), "lapl_GBps": round(lapl_rate, 1),
                     "frac_of_probe": round(rate / probe_med, 4),
                     "frac_of_lapl_rate": round(rate / lapl_rate, 4)})
    for x in v:
        x.destroy()
    da.destroy()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("sizes", nargs="*", type=int, default=[256, 512])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "compact_ops"))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    ctx = pb.Context(0)
    for n in args.sizes:
        with open(os.path.join(args.out, f"bench_{n}.jsonl"), "w") as fh:
            for row in bench(ctx, n, args.reps):
                line = json.dumps(row)
                print(line, flush=True)
                fh.write(line + "\n")
    ctx.destroy()


if __name__ == "__main__":
    main()
