"""-ksp_type preonly and richardson on one GPU, one process, the compared paths interleaved rep by
rep (same buffers, same clocks). One JSON line per part:

  a  the direct solve: -ksp_type preonly -pc_type fft against -ksp_type cg -pc_type fft to rtol
     1e-10 on the same b, for the 7-point operator ("star7") and config 5 (compact A = P on the
     2 pi box, "config5"): wall ms of pb_ksp_solve and the true residual ||b - A x|| / ||b|| of both;
  b  Richardson's fused update + residual pass (timer rich_update, 40 B/DoF) against the unfused
     pair of the same process (tuning rich_fused = 0: timers rich_axpy + rich_resid, 48 B/DoF) and
     against the copy probe (16 B/DoF), Jacobi, 8 updates per solve;
  c  -ksp_type richardson -pc_type mg against -ksp_type cg -pc_type mg to rtol 1e-10: iterations
     and wall ms (information: stand-alone multigrid against multigrid-preconditioned CG).

usage: python scripts/bench_ksp_types.py [--n 512] [--reps 10] [--parts a,b,c]
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


def part_a(ctx, n, reps, name):
    n3 = (n,) * 3
    L3 = (2 * math.pi,) * 3 if name == "config5" else (1.0, 1.0, 1.0)
    h = tuple(l / n for l in L3)
    da = pb.DA(ctx, n3, L3)
    A = pb.Mat(da, pb.COMPACT if name == "config5" else pb.STAR7, h)
    x, b, xt, w = pb.Vec(da), pb.Vec(da), pb.Vec(da), pb.Vec(da)
    xt.set_random(SEED)
    A.mult(xt, b)
    kp = pb.KSP(A, A, pb.ksp_options(["-ksp_type", "preonly", "-pc_type", "fft"]))
    kc = pb.KSP(A, A, pb.ksp_options(["-ksp_type", "cg", "-pc_type", "fft", "-ksp_rtol", "1e-10"]))
    out = {"part": "a", "op": name, "n": n}
    tp, tc = [], []
    for rep in range(reps + 2):  # two warm-up rounds: allocations, first touch
        ms, reason, its = timed_solve(ctx, kp, b, x)
        if rep >= 2:
            tp.append(ms)
        out.setdefault("preonly", {}).update(reason=reason, its=its)
        if rep == 2:
            out["preonly"]["rel_residual"] = rel_residual(A, b, x, w)
        ms, reason, its = timed_solve(ctx, kc, b, x)
        if rep >= 2:
            tc.append(ms)
        out.setdefault("cg", {}).update(reason=reason, its=its)
        if rep == 2:
            out["cg"]["rel_residual"] = rel_residual(A, b, x, w)
    out["preonly"].update(stats(tp))
    out["cg"].update(stats(tc))
    out["cg_over_preonly"] = out["cg"]["median_ms"] / out["preonly"]["median_ms"]
    print(json.dumps(out), flush=True)
    for o in (kp, kc, x, b, xt, w, A, da):
        o.destroy()


def part_b(ctx, n, reps):
    n3 = (n,) * 3
    N = n ** 3
    h = (1.0 / n,) * 3
    da = pb.DA(ctx, n3)
    P, A, x, b = pb.initialise_linear_system(da, h)
    xt = pb.Vec(da)
    xt.set_random(SEED)
    A.mult(xt, b)
    k = pb.KSP(A, P, pb.ksp_options(["-ksp_type", "richardson", "-pc_type", "jacobi",
                                     "-ksp_richardson_scale", "0.667"],
                                    rtol=0.0, atol=0.0, dtol=1e300, max_it=8))
    names = ["rich_update", "rich_axpy", "rich_resid"]
    wall = {1: [], 0: []}
    for rep in range(reps + 2):
        if rep == 2:
            ctx.set_timing(True, only=names)
            ctx.reset_timing()
        for fused in (1, 0):
            pb.tune_set("rich_fused", fused)
            ms, reason, its = timed_solve(ctx, k, b, x)
            if rep >= 2:
                wall[fused].append(ms)
    pb.tune_reset()
    ctx.sync()
    # a solve enqueues updates ahead of its convergence poll; those past the 8th exit at entry in
    # microseconds: keep the launches that ran (at least half the longest)
    t = {}
    for nm in names:
        s = [float(v) for v in ctx.timing_samples(nm)]
        t[nm] = [v for v in s if v >= 0.5 * max(s)]
    ctx.set_timing(False)
    probe_best, probe_med = ctx.copy_probe(N, 10)
    fused_ms = med(t["rich_update"])
    unfused_ms = med(t["rich_axpy"]) + med(t["rich_resid"])
    out = {"part": "b", "n": n, "updates_per_solve": 8,
           "rich_update": stats(t["rich_update"]), "rich_axpy": stats(t["rich_axpy"]),
           "rich_resid": stats(t["rich_resid"]), "unfused_pair_median_ms": unfused_ms,
           "unfused_over_fused": unfused_ms / fused_ms,
           "copy_probe_gbps": {"best": probe_best, "median": probe_med},
           "fused_gbps_at_40B": 40.0 * N / (fused_ms * 1e-3) / 1e9,
           "fused_frac_of_probe": 40.0 * N / (fused_ms * 1e-3) / 1e9 / probe_med,
           "unfused_frac_of_probe": 48.0 * N / (unfused_ms * 1e-3) / 1e9 / probe_med,
           "solve_wall_fused": stats(wall[1]), "solve_wall_unfused": stats(wall[0])}
    print(json.dumps(out), flush=True)
    for o in (k, x, b, xt, A, P, da):
        o.destroy()


def part_c(ctx, n, reps):
    n3 = (n,) * 3
    h = (1.0 / n,) * 3
    da = pb.DA(ctx, n3)
    P, A, x, b = pb.initialise_linear_system(da, h)
    xt, w = pb.Vec(da), pb.Vec(da)
    xt.set_random(SEED)
    A.mult(xt, b)
    tol = ["-pc_type", "mg", "-ksp_rtol", "1e-10"]
    kr = pb.KSP(A, P, pb.ksp_options(["-ksp_type", "richardson"] + tol))
    kc = pb.KSP(A, P, pb.ksp_options(["-ksp_type", "cg"] + tol))
    out = {"part": "c", "n": n}
    tr, tc = [], []
    for rep in range(reps + 2):
        for key, k, acc in (("richardson", kr, tr), ("cg", kc, tc)):
            ms, reason, its = timed_solve(ctx, k, b, x)
            if rep >= 2:
                acc.append(ms)
            out.setdefault(key, {}).update(reason=reason, its=its)
            if rep == 2:
                out[key]["rel_residual"] = rel_residual(A, b, x, w)
    out["richardson"].update(stats(tr))
    out["cg"].update(stats(tc))
    print(json.dumps(out), flush=True)
    for o in (kr, kc, x, b, xt, w, A, P, da):
        o.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parts", default="a,b,c")
    args = ap.parse_args()
    parts = args.parts.split(",")
    ctx = pb.Context(0)
    if "a" in parts:
        part_a(ctx, args.n, args.reps, "star7")
        part_a(ctx, args.n, args.reps, "config5")
    if "b" in parts:
        part_b(ctx, args.n, args.reps)
    if "c" in parts:
        part_c(ctx, args.n, args.reps)
    ctx.destroy()


if __name__ == "__main__":
    main()
