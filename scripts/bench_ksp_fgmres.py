"""-ksp_type fgmres on one GPU, one process, the compared solvers interleaved rep by rep (same
buffers, same clocks). One JSON line per part:

  a  the cost of one Arnoldi step by cycle position (-pc_type jacobi, restart 30, no stopping
     test): pb_ksp_begin, then pb_ksp_iterate(1) + a wait per step, wall ms; the position-0 step
     after the cycle's last carries the restart (solution build, residual, norm). Beside it the
     copy probe of the same process and the bytes a step moves (16 B/DoF per stored vector from
     the multi-dot and multi-axpy, on top of the step's fixed passes);
  f  the engine pass that starts a step on the 7-point operator with Jacobi (timer fgmres_fused,
     32 B/DoF) against the unfused sequence of the same process (tuning fgmres_fused = 0: timers
     fgmres_scale + fgmres_pc + stencil, 48 B/DoF) and against the copy probe, 8 steps per solve,
     the two interleaved rep by rep;
  b  -ksp_type fgmres -pc_type jacobi against -ksp_type cg, both to rtol 1e-8 (fgmres with
     --max-it as its limit: restarted GMRES without a real preconditioner may stall);
  c  -ksp_type fgmres -pc_type mg against cg + mg, both to rtol 1e-10.
  b and c report iterations, reason, wall ms and the true residual ||b - A x|| / ||b||.

usage: python scripts/bench_ksp_fgmres.py [--n 512] [--reps 5] [--parts f,a,b,c] [--max-it 3000]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import poissbox_amd as pb  # noqa: E402

SEED = 20231015


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def stats(v):
    return {"median_ms": float(med(v)), "min_ms": float(min(v)), "max_ms": float(max(v)),
            "n": len(v)}


def system(ctx, n):
    da = pb.DA(ctx, (n,) * 3)
    P, A, x, b = pb.initialise_linear_system(da, (1.0 / n,) * 3)
    xt = pb.Vec(da)
    xt.set_random(SEED)
    A.mult(xt, b)
    return da, P, A, x, b, xt


def rel_residual(A, b, x, w):
    A.mult(x, w)
    w.axpy(-1.0, b)
    return w.norm() / b.norm()


def part_a(ctx, n, reps, restart):
    N = n ** 3
    da, P, A, x, b, xt = system(ctx, n)
    steps = restart + 2  # one full cycle, the restart, one more step
    k = pb.KSP(A, P, pb.ksp_options(["-ksp_type", "fgmres", "-pc_type", "jacobi",
                                     "-ksp_gmres_restart", str(restart)],
                                    rtol=0.0, atol=0.0, dtol=1e300, max_it=steps + 1,
                                    check_every=1))
    per = [[] for _ in range(steps)]
    for rep in range(reps + 1):  # the first round allocates the basis
        k.begin(b, x)
        for i in range(steps):
            ctx.sync()
            t0 = time.perf_counter()
            k.iterate(1)
            ctx.sync()
            if rep >= 1:
                per[i].append((time.perf_counter() - t0) * 1e3)
        k.end()
    probe_best, probe_med = ctx.copy_probe(N, 10)
    out = {"part": "a", "n": n, "restart": restart, "pc": "jacobi",
           "step_ms_by_position": [stats(p) for p in per[:restart]],
           "step_after_restart_ms": stats(per[restart]),
           "last_step_of_cycle_includes_restart": True,
           "copy_probe_gbps": {"best": probe_best, "median": probe_med},
           # the multi-dot reads w and k + 1 vectors, the multi-axpy the same and writes w
           "bytes_per_dof_per_stored_vector": 16}
    m = [s["median_ms"] for s in out["step_ms_by_position"]]
    if restart >= 12:
        # the slope over positions 1 .. restart - 2 (the last carries the restart)
        slope = (m[restart - 2] - m[1]) / (restart - 3)
        out["ms_per_stored_vector"] = slope
        out["stored_vector_gbps_at_16B"] = 16.0 * N / (slope * 1e-3) / 1e9
    print(json.dumps(out), flush=True)
    for o in (k, x, b, xt, A, P, da):
        o.destroy()


def part_f(ctx, n, reps):
    N = n ** 3
    da, P, A, x, b, xt = system(ctx, n)
    k = pb.KSP(A, P, pb.ksp_options(["-ksp_type", "fgmres", "-pc_type", "jacobi",
                                     "-ksp_gmres_restart", "8"],
                                    rtol=0.0, atol=0.0, dtol=1e300, max_it=8))
    names = ["fgmres_fused", "fgmres_scale", "fgmres_pc", "stencil"]
    wall = {1: [], 0: []}
    for rep in range(reps + 2):  # two warm-up rounds: allocations, first touch
        if rep == 2:
            ctx.set_timing(True, only=names)
            ctx.reset_timing()
        for fused in (1, 0):
            pb.tune_set("fgmres_fused", fused)
            ctx.sync()
            t0 = time.perf_counter()
            k.solve(b, x)
            ctx.sync()
            if rep >= 2:
                wall[fused].append((time.perf_counter() - t0) * 1e3)
    pb.tune_reset()
    ctx.sync()
    # launches enqueued behind the one that ended the solve exit at entry in microseconds: keep
    # the ones that ran (at least half the longest)
    t = {}
    for nm in names:
        v = [float(u) for u in ctx.timing_samples(nm)]
        t[nm] = [u for u in v if u >= 0.5 * max(v)]
    ctx.set_timing(False)
    probe_best, probe_med = ctx.copy_probe(N, 10)
    fused_ms = med(t["fgmres_fused"])
    parts = [med(t["fgmres_scale"]), med(t["fgmres_pc"]), med(t["stencil"])]
    unfused_ms = sum(parts)
    # the unfused reps' own spread: the sum of the three kernels' (max - min) over the kept launches
    spread = sum(max(t[nm]) - min(t[nm]) for nm in names[1:])
    gbps = lambda bytes_per_dof, ms: bytes_per_dof * N / (ms * 1e-3) / 1e9
    out = {"part": "f", "n": n, "steps_per_solve": 8,
           "fgmres_fused": stats(t["fgmres_fused"]), "fgmres_scale": stats(t["fgmres_scale"]),
           "fgmres_pc": stats(t["fgmres_pc"]), "stencil": stats(t["stencil"]),
           "unfused_sequence_median_ms": unfused_ms, "unfused_spread_ms": spread,
           "unfused_over_fused": unfused_ms / fused_ms,
           "fused_beats_unfused_by_more_than_spread": unfused_ms - fused_ms > spread,
           "copy_probe_gbps": {"best": probe_best, "median": probe_med},
           "fused_gbps_at_32B": gbps(32.0, fused_ms),
           "fused_frac_of_probe": gbps(32.0, fused_ms) / probe_med,
           "unfused_frac_of_probe": gbps(48.0, unfused_ms) / probe_med,
           "solve_wall_fused": stats(wall[1]), "solve_wall_unfused": stats(wall[0])}
    print(json.dumps(out), flush=True)
    for o in (k, x, b, xt, A, P, da):
        o.destroy()


def compare(ctx, n, reps, part, tol, solvers):
    da, P, A, x, b, xt = system(ctx, n)
    w = pb.Vec(da)
    ksps = [(key, pb.KSP(A, P, pb.ksp_options(argv + tol))) for key, argv in solvers]
    out = {"part": part, "n": n}
    acc = {key: [] for key, _ in ksps}
    for rep in range(reps + 1):
        for key, k in ksps:
            ctx.sync()
            t0 = time.perf_counter()
            reason, its, _ = k.solve(b, x)
            ctx.sync()
            ms = (time.perf_counter() - t0) * 1e3
            if rep >= 1:
                acc[key].append(ms)
            out.setdefault(key, {}).update(reason=int(reason), its=int(its))
            if rep == 1:
                out[key]["rel_residual"] = rel_residual(A, b, x, w)
    for key, k in ksps:
        out[key].update(stats(acc[key]))
        out[key]["ms_per_iteration"] = out[key]["median_ms"] / max(out[key]["its"], 1)
    print(json.dumps(out), flush=True)
    for o in [k for _, k in ksps] + [x, b, xt, w, A, P, da]:
        o.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--parts", default="f,a,b,c")
    ap.add_argument("--restart", type=int, default=30)
    ap.add_argument("--max-it", type=int, default=3000)
    args = ap.parse_args()
    parts = args.parts.split(",")
    ctx = pb.Context(0)
    fg = ["-ksp_type", "fgmres", "-ksp_gmres_restart", str(args.restart)]
    if "f" in parts:
        part_f(ctx, args.n, args.reps)
    if "a" in parts:
        part_a(ctx, args.n, args.reps, args.restart)
    if "b" in parts:
        compare(ctx, args.n, args.reps, "b", ["-pc_type", "jacobi", "-ksp_rtol", "1e-8"],
                [("fgmres", fg + ["-ksp_max_it", str(args.max_it)]), ("cg", ["-ksp_type", "cg"])])
    if "c" in parts:
        compare(ctx, args.n, args.reps, "c", ["-pc_type", "mg", "-ksp_rtol", "1e-10"],
                [("fgmres", fg), ("cg", ["-ksp_type", "cg"])])
    ctx.destroy()


if __name__ == "__main__":
    main()
