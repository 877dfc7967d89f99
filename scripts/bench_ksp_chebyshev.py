"""-ksp_type chebyshev on one GPU, one process, the compared paths interleaved rep by rep (same
buffers, same clocks). One JSON line per part:

  a  Chebyshev's fused update + residual pass (timer cheb_update, 48 B/DoF) against the unfused
     pair of the same process (tuning cheb_fused = 0: timers cheb_axpy + rich_resid, 56 B/DoF) and
     against the copy probe (16 B/DoF), Jacobi, 9 updates per solve (the first is Richardson's);
  b  -ksp_type chebyshev -pc_type jacobi with the analytic bounds (emin = the smallest non-zero
     value of the operator's symbol over the diagonal, emax = 2) against -ksp_type cg, both to rtol
     1e-8: iterations, wall ms and the true residual ||b - A x|| / ||b||;
  c  -ksp_type chebyshev -pc_type mg with estimated bounds against cg + mg and richardson + mg to
     rtol 1e-10 (the estimate runs in the warm-up solves, outside the timed ones).

usage: python scripts/bench_ksp_chebyshev.py [--n 512] [--reps 10] [--parts a,b,c]
"""
import argparse
import json
import math
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
    return {"median_ms": float(med(v)), "min_ms": float(min(v)), "n": len(v)}


def timed_solve(ctx, k, b, x):
    ctx.sync()
    t0 = time.perf_counter()
    reason, its, _ = k.solve(b, x)
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, int(reason), int(its)


def rel_residual(A, b, x, w):
    A.mult(x, w)
    w.axpy(-1.0, b)
    return w.norm() / b.norm()


def system(ctx, n):
    da = pb.DA(ctx, (n,) * 3)
    P, A, x, b = pb.initialise_linear_system(da, (1.0 / n,) * 3)
    xt = pb.Vec(da)
    xt.set_random(SEED)
    A.mult(xt, b)
    return da, P, A, x, b, xt


def part_a(ctx, n, reps):
    N = n ** 3
    da, P, A, x, b, xt = system(ctx, n)
    k = pb.KSP(A, P, pb.ksp_options(["-ksp_type", "chebyshev", "-pc_type", "jacobi",
                                     "-ksp_chebyshev_eigenvalues", "0.05,2.0"],
                                    rtol=0.0, atol=0.0, dtol=1e300, max_it=9))
    names = ["cheb_update", "cheb_axpy", "rich_resid"]
    wall = {1: [], 0: []}
    for rep in range(reps + 2):  # two warm-up rounds: allocations, first touch
        if rep == 2:
            ctx.set_timing(True, only=names)
            ctx.reset_timing()
        for fused in (1, 0):
            pb.tune_set("cheb_fused", fused)
            ms, reason, its = timed_solve(ctx, k, b, x)
            if rep >= 2:
                wall[fused].append(ms)
    pb.tune_reset()
    ctx.sync()
    # a solve enqueues updates ahead of its convergence poll; those past the last exit at entry in
    # microseconds: keep the launches that ran (at least half the longest)
    t = {}
    for nm in names:
        s = [float(v) for v in ctx.timing_samples(nm)]
        t[nm] = [v for v in s if v >= 0.5 * max(s)]
    ctx.set_timing(False)
    probe_best, probe_med = ctx.copy_probe(N, 10)
    fused_ms = med(t["cheb_update"])
    unfused_ms = med(t["cheb_axpy"]) + med(t["rich_resid"])
    gbps = lambda bytes_per_dof, ms: bytes_per_dof * N / (ms * 1e-3) / 1e9
    out = {"part": "a", "n": n, "updates_per_solve": 9,
           "cheb_update": stats(t["cheb_update"]), "cheb_axpy": stats(t["cheb_axpy"]),
           "rich_resid": stats(t["rich_resid"]), "unfused_pair_median_ms": unfused_ms,
           "unfused_over_fused": unfused_ms / fused_ms,
           "copy_probe_gbps": {"best": probe_best, "median": probe_med},
           "fused_gbps_at_48B": gbps(48.0, fused_ms),
           "fused_frac_of_probe": gbps(48.0, fused_ms) / probe_med,
           "unfused_frac_of_probe": gbps(56.0, unfused_ms) / probe_med,
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
    for rep in range(reps + 2):
        for key, k in ksps:
            ms, reason, its = timed_solve(ctx, k, b, x)
            if rep >= 2:
                acc[key].append(ms)
            out.setdefault(key, {}).update(reason=reason, its=its)
            if rep == 2:
                out[key]["rel_residual"] = rel_residual(A, b, x, w)
    for key, k in ksps:
        out[key].update(stats(acc[key]))
        out[key]["ms_per_iteration"] = out[key]["median_ms"] / max(out[key]["its"], 1)
        if key == "chebyshev":
            emin, emax, est = k.chebyshev_eigenvalues()
            out[key].update(emin=emin, emax=emax, estimated=est)
    print(json.dumps(out), flush=True)
    for o in [k for _, k in ksps] + [x, b, xt, w, A, P, da]:
        o.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parts", default="a,b,c")
    args = ap.parse_args()
    parts = args.parts.split(",")
    n = args.n
    ctx = pb.Context(0)
    if "a" in parts:
        part_a(ctx, n, args.reps)
    if "b" in parts:
        # D^-1 A on the uniform cube: symbol (sum_d (1 - cos t_d)) / 3, smallest non-zero value at
        # one t_d = 2 pi / n, largest 2 (n even)
        emin = (1.0 - math.cos(2.0 * math.pi / n)) / 3.0
        compare(ctx, n, args.reps, "b", ["-pc_type", "jacobi", "-ksp_rtol", "1e-8"],
                [("chebyshev", ["-ksp_type", "chebyshev", "-ksp_chebyshev_eigenvalues",
                                f"{emin!r},2.0"]),
                 ("cg", ["-ksp_type", "cg"])])
    if "c" in parts:
        compare(ctx, n, args.reps, "c", ["-pc_type", "mg", "-ksp_rtol", "1e-10"],
                [("chebyshev", ["-ksp_type", "chebyshev"]), ("cg", ["-ksp_type", "cg"]),
                 ("richardson", ["-ksp_type", "richardson"])])
    ctx.destroy()


if __name__ == "__main__":
    main()
