"""PB_OP_VARCOEF (div(beta grad)) on one GPU, one process, the compared paths
interleaved rep by rep (same buffers, same clocks). One JSON line per part:

  a  the apply y = A x, both means (timer varcoef, 24 B/DoF: x and beta read, y written), against
     the PB_OP_STAR7 matvec of the same process (timer stencil, 16 B/DoF) and the copy probe:
     ms per launch (median, min) and achieved bytes/s; the three launches alternate;
  d  the CG iteration's p . Ap taken by the operator's own pass (tuning varcoef_dot_fused = 1:
     timer varcoef alone) against the separate dot kernel (0: varcoef + cg_gen_dot, 16 B/DoF
     more), 8 iterations per solve, variable Jacobi, harmonic mean, the two interleaved;
  s  full solves to rtol 1e-8 on the sphere jump (beta = 1 outside, 1 / contrast inside the
     sphere of radius 0.3; harmonic mean), contrast 10 and 1000: cg + the variable Jacobi, cg + mg
     and cg + fft from a constant-coefficient PB_OP_STAR7 P; iterations, reason, wall ms and the
     true residual ||b - A x|| / ||b||.

usage: python scripts/bench_varcoef.py [--n 512] [--reps 10] [--parts a,d,s] [--max-it 20000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ksp_fgmres import med, rel_residual, stats  # noqa: E402
import poissbox_amd as pb  # noqa: E402

SEED = 20231015
ITERS = 8


def sphere(n, inside, radius=0.3):
    """beta of the sphere jump on the n^3 unit box (cell centres), flat, x fastest"""
    c = ((np.arange(n) + 0.5) / n - 0.5) ** 2
    r2 = c[:, None, None] + c[None, :, None] + c[None, None, :]
    return np.where(r2 < radius * radius, inside, 1.0).reshape(-1)


def varcoef(da, n, contrast, mean):
    A = pb.Mat(da, pb.VARCOEF, (1.0 / n,) * 3)
    bv = pb.Vec(da)
    bv.set_values(sphere(n, 1.0 / contrast))
    A.set_coefficient(bv, mean)
    bv.destroy()
    return A


def ran(samples):
    """launches enqueued behind the one that ended a solve exit at entry in microseconds: keep
    the ones that ran (at least half the longest)"""
    v = [float(u) for u in samples]
    return [u for u in v if u >= 0.5 * max(v)] if v else v


def gbps(bytes_per_dof, N, ms):
    return bytes_per_dof * N / (ms * 1e-3) / 1e9


def part_a(ctx, n, reps):
    N = n ** 3
    da = pb.DA(ctx, (n,) * 3)
    ops = {"arithmetic": varcoef(da, n, 1000.0, pb.COEF_ARITHMETIC),
           "harmonic": varcoef(da, n, 1000.0, pb.COEF_HARMONIC)}
    S = pb.Mat(da, pb.STAR7, (1.0 / n,) * 3)
    x, y = pb.Vec(da), pb.Vec(da)
    x.set_random(SEED)
    t = {"arithmetic": [], "harmonic": [], "stencil": []}
    for rep in range(reps + 2):  # two warm-up rounds
        for name, A in list(ops.items()) + [("stencil", S)]:
            ctx.reset_timing()
            ctx.set_timing(True, only=["varcoef", "stencil"])
            A.mult(x, y)
            ctx.sync()
            v = ctx.timing_samples("stencil" if name == "stencil" else "varcoef")
            ctx.set_timing(False)
            if rep >= 2:
                t[name].append(float(v[0]))
    probe_best, probe_med = ctx.copy_probe(N, 10)
    out = {"part": "a", "n": n, "copy_probe_gbps": {"best": probe_best, "median": probe_med}}
    for name, bpd in (("arithmetic", 24.0), ("harmonic", 24.0), ("stencil", 16.0)):
        m = med(t[name])
        out[name] = dict(stats(t[name]), bytes_per_dof=bpd, gbps=gbps(bpd, N, m),
                         frac_of_probe=gbps(bpd, N, m) / probe_med)
    out["pro_rata_of_matvec_ms"] = med(t["stencil"]) * 1.5
    print(json.dumps(out), flush=True)
    for o in list(ops.values()) + [S, x, y, da]:
        o.destroy()


def part_d(ctx, n, reps):
    N = n ** 3
    da = pb.DA(ctx, (n,) * 3)
    A = varcoef(da, n, 1000.0, pb.COEF_HARMONIC)
    x, b, xt = pb.Vec(da), pb.Vec(da), pb.Vec(da)
    xt.set_random(SEED)
    A.mult(xt, b)
    k = pb.KSP(A, A, pb.ksp_options(["-ksp_type", "cg", "-pc_type", "jacobi"], rtol=0.0, atol=0.0,
                                    dtol=1e300, max_it=ITERS))
    names = ["varcoef", "cg_gen_dot"]
    t = {0: {nm: [] for nm in names}, 1: {nm: [] for nm in names}}
    wall = {0: [], 1: []}
    for rep in range(reps + 2):
        for fused in (1, 0):
            pb.tune_set("varcoef_dot_fused", fused)
            ctx.reset_timing()
            ctx.set_timing(True, only=names)
            ctx.sync()
            t0 = time.perf_counter()
            k.solve(b, x)
            ctx.sync()
            w = (time.perf_counter() - t0) * 1e3
            got = {nm: ran(ctx.timing_samples(nm)) for nm in names}
            ctx.set_timing(False)
            if rep >= 2:
                wall[fused].append(w)
                for nm in names:
                    t[fused][nm] += got[nm]
    pb.tune_reset()
    probe_best, probe_med = ctx.copy_probe(N, 10)
    fused_ms = med(t[1]["varcoef"])
    unfused_ms = med(t[0]["varcoef"]) + med(t[0]["cg_gen_dot"])
    spread = sum(max(t[0][nm]) - min(t[0][nm]) for nm in names)
    out = {"part": "d", "n": n, "iterations_per_solve": ITERS,
           "fused_varcoef": stats(t[1]["varcoef"]), "unfused_varcoef": stats(t[0]["varcoef"]),
           "unfused_cg_gen_dot": stats(t[0]["cg_gen_dot"]),
           "fused_cg_gen_dot_launches": len(t[1]["cg_gen_dot"]),
           "unfused_pair_median_ms": unfused_ms, "unfused_spread_ms": spread,
           "fused_median_ms": fused_ms, "saved_ms": unfused_ms - fused_ms,
           "fused_beats_unfused_by_more_than_spread": unfused_ms - fused_ms > spread,
           "copy_probe_gbps": {"best": probe_best, "median": probe_med},
           "solve_wall_fused": stats(wall[1]), "solve_wall_unfused": stats(wall[0])}
    print(json.dumps(out), flush=True)
    for o in (k, x, b, xt, A, da):
        o.destroy()


def part_s(ctx, n, reps, max_it):
    da = pb.DA(ctx, (n,) * 3)
    P = pb.Mat(da, pb.STAR7, (1.0 / n,) * 3)
    x, b, xt, w = pb.Vec(da), pb.Vec(da), pb.Vec(da), pb.Vec(da)
    xt.set_random(SEED)
    for contrast in (10.0, 1000.0):
        A = varcoef(da, n, contrast, pb.COEF_HARMONIC)
        A.mult(xt, b)
        rows = []
        for name, Pm, pc in (("cg + variable jacobi", A, "jacobi"), ("cg + mg (constant P)", P, "mg"),
                             ("cg + fft (constant P)", P, "fft")):
            k = pb.KSP(A, Pm, pb.ksp_options(["-ksp_type", "cg", "-pc_type", pc, "-ksp_rtol",
                                              "1e-8", "-ksp_max_it", str(max_it)]))
            ms = []
            for rep in range(reps):
                x.set(0.0)
                ctx.sync()
                t0 = time.perf_counter()
                reason, its, hist = k.solve(b, x)
                ctx.sync()
                ms.append((time.perf_counter() - t0) * 1e3)
            rows.append({"solver": name, "reason": pb.REASONS.get(reason, reason), "its": int(its),
                         "wall": stats(ms), "true_residual": rel_residual(A, b, x, w)})
            k.destroy()
        print(json.dumps({"part": "s", "n": n, "contrast": contrast, "mean": "harmonic",
                          "rtol": 1e-8, "solves": rows}), flush=True)
        A.destroy()
    for o in (x, b, xt, w, P, da):
        o.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parts", default="a,d,s")
    ap.add_argument("--max-it", type=int, default=20000)
    args = ap.parse_args()
    parts = args.parts.split(",")
    ctx = pb.Context(0)
    if "a" in parts:
        part_a(ctx, args.n, args.reps)
    if "d" in parts:
        part_d(ctx, args.n, args.reps)
    if "s" in parts:
        part_s(ctx, args.n, max(1, args.reps // 5), args.max_it)
    ctx.destroy()


if __name__ == "__main__":
    main()
