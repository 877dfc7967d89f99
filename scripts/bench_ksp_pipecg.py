"""-ksp_type pipecg on one GPU, one process, the compared paths interleaved rep by rep (same
buffers, same clocks). One JSON line per part:

  f  the engine pass of an iteration on the 7-point operator with Jacobi (timer pipecg_pass,
     128 B/DoF) against the unfused sequence of the same process (tuning pipecg_fused = 0: timers
     pipecg_pc + stencil + pipecg_update, 16 + 16 + 144 = 176 B/DoF) and against the copy probe,
     8 iterations per solve, the two interleaved rep by rep; the finalize launch beside them;
  b  -ksp_type pipecg -pc_type jacobi against -ksp_type cg, both to rtol 1e-8;
  c  -ksp_type pipecg -pc_type mg against cg + mg, both to rtol 1e-10.
  b and c report iterations, reason, wall ms and the true residual ||b - A x|| / ||b||.

usage: python scripts/bench_ksp_pipecg.py [--n 512] [--reps 5] [--parts f,b,c]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ksp_fgmres import compare, med, stats, system  # noqa: E402
import poissbox_amd as pb  # noqa: E402

ITERS = 8


def part_f(ctx, n, reps):
    N = n ** 3
    da, P, A, x, b, xt = system(ctx, n)
    k = pb.KSP(A, P, pb.ksp_options(["-ksp_type", "pipecg", "-pc_type", "jacobi"],
                                    rtol=0.0, atol=0.0, dtol=1e300, max_it=ITERS))
    names = ["pipecg_pass", "pipecg_pc", "stencil", "pipecg_update", "pipecg_finalize"]
    wall = {1: [], 0: []}
    for rep in range(reps + 2):  # two warm-up rounds: allocations, first touch
        if rep == 2:
            ctx.set_timing(True, only=names)
            ctx.reset_timing()
        for fused in (1, 0):
            pb.tune_set("pipecg_fused", fused)
            ctx.sync()
            t0 = time.perf_counter()
            k.solve(b, x)
            ctx.sync()
            if rep >= 2:
                wall[fused].append((time.perf_counter() - t0) * 1e3)
    pb.tune_reset()
    ctx.sync()
    # the setup's launches of pipecg_pc and stencil (one or two per solve) are full passes too and
    # stay in; launches that exited at entry would be microseconds: keep those that ran
    t = {}
    for nm in names:
        v = [float(u) for u in ctx.timing_samples(nm)]
        t[nm] = [u for u in v if u >= 0.5 * max(v)] if nm != "pipecg_finalize" else v
    ctx.set_timing(False)
    probe_best, probe_med = ctx.copy_probe(N, 10)
    fused_ms = med(t["pipecg_pass"])
    seq = ["pipecg_pc", "stencil", "pipecg_update"]
    unfused_ms = sum(med(t[nm]) for nm in seq)
    spread = sum(max(t[nm]) - min(t[nm]) for nm in seq)
    gbps = lambda bytes_per_dof, ms: bytes_per_dof * N / (ms * 1e-3) / 1e9
    out = {"part": "f", "n": n, "iterations_per_solve": ITERS}
    out.update({nm: stats(t[nm]) for nm in names})
    out.update({"unfused_sequence_median_ms": unfused_ms, "unfused_spread_ms": spread,
                "unfused_over_fused": unfused_ms / fused_ms,
                "fused_beats_unfused_by_more_than_spread": unfused_ms - fused_ms > spread,
                "copy_probe_gbps": {"best": probe_best, "median": probe_med},
                "fused_gbps_at_128B": gbps(128.0, fused_ms),
                "fused_frac_of_probe": gbps(128.0, fused_ms) / probe_med,
                "unfused_frac_of_probe": gbps(176.0, unfused_ms) / probe_med,
                "solve_wall_fused": stats(wall[1]), "solve_wall_unfused": stats(wall[0])})
    print(json.dumps(out), flush=True)
    for o in (k, x, b, xt, A, P, da):
        o.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="f,b,c")
    args = ap.parse_args()
    parts = args.parts.split(",")
    ctx = pb.Context(0)
    pc, cg = ["-ksp_type", "pipecg"], ["-ksp_type", "cg"]
    if "f" in parts:
        part_f(ctx, args.n, args.reps)
    if "b" in parts:
        compare(ctx, args.n, args.reps, "b", ["-pc_type", "jacobi", "-ksp_rtol", "1e-8"],
                [("pipecg", pc), ("cg", cg)])
    if "c" in parts:
        compare(ctx, args.n, args.reps, "c", ["-pc_type", "mg", "-ksp_rtol", "1e-10"],
                [("pipecg", pc), ("cg", cg)])
    ctx.destroy()


if __name__ == "__main__":
    main()
