"""-ksp_norm_type on one GPU, one process, the norm types interleaved rep by rep (same buffers, same
clocks; the protocol of scripts/bench_ksp_types.py). One JSON line per part:

  iter   per-iteration wall ms (split form: begin, then `iters` iterations timed as one batch, end)
         under preconditioned / unpreconditioned / natural / none for cg + jacobi,
         cg + jacobi -ksp_cg_single_reduction, cg + mg, cg + fft (compact A = P, config 5) and
         richardson + mg (no natural): median and minimum over the reps, and each type's ratio to
         the preconditioned median beside the spread (max / min) of the preconditioned reps;
  solve  full solves to rtol 1e-10 under each testing type: iterations, wall ms and the true
         residual ||b - A x|| / ||b|| each ends at;
  setup  the nonzero-guess setup (pb_ksp_begin, x0 = a perturbed solution) of cg + mg under
         preconditioned and unpreconditioned: wall ms (one V-cycle fewer).

usage: python scripts/bench_ksp_norm_type.py [--n 512] [--reps 7] [--out profiles/ksp_norm_type/bench_512.jsonl]
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
TYPES = ("preconditioned", "unpreconditioned", "natural", "none")
FIXED = ["-ksp_rtol", "0", "-ksp_atol", "0", "-ksp_divtol", "1e300"]
PATHS = {
    "cg+jacobi": (["-ksp_type", "cg", "-pc_type", "jacobi"], "star7", 40),
    "cg+jacobi sr": (["-ksp_type", "cg", "-pc_type", "jacobi", "-ksp_cg_single_reduction"],
                     "star7", 40),
    "cg+mg": (["-ksp_type", "cg", "-pc_type", "mg"], "star7", 8),
    "cg+fft config5": (["-ksp_type", "cg", "-pc_type", "fft"], "config5", 1),
    "richardson+mg": (["-ksp_type", "richardson", "-pc_type", "mg"], "star7", 8),
}


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def system(ctx, n, kind):
    n3 = (n,) * 3
    L3 = (2 * math.pi,) * 3 if kind == "config5" else (1.0, 1.0, 1.0)
    h = tuple(l / n for l in L3)
    da = pb.DA(ctx, n3, L3)
    if kind == "config5":
        A = pb.Mat(da, pb.COMPACT, h)
        P = A
    else:
        A, P = pb.Mat(da, pb.STAR7, h), pb.Mat(da, pb.ASSEMBLED27, h)
    x, b, xt, w = pb.Vec(da), pb.Vec(da), pb.Vec(da), pb.Vec(da)
    xt.set_random(SEED)
    A.mult(xt, b)
    return da, A, P, x, b, xt, w


def types_of(name):
    return [t for t in TYPES if not (t == "natural" and name.startswith("richardson"))]


def part_iter(ctx, n, reps, emit):
    for name, (argv, kind, iters) in PATHS.items():
        da, A, P, x, b, xt, w = system(ctx, n, kind)
        ks = {t: pb.KSP(A, P, pb.ksp_options(argv + FIXED + ["-ksp_max_it", "100000",
                                                             "-ksp_norm_type", t]))
              for t in types_of(name)}
        ms = {t: [] for t in ks}
        for rep in range(reps + 1):  # (rep 0 warms up)
            for t, k in ks.items():
                k.begin(b, x)
                ctx.sync()
                t0 = time.perf_counter()
                k.iterate(iters)
                ctx.sync()
                dt = (time.perf_counter() - t0) * 1e3 / iters
                k.end()
                if rep:
                    ms[t].append(dt)
        ref = med(ms["preconditioned"])
        emit({"part": "iter", "path": name, "n": n, "iters": iters, "reps": reps,
              "preconditioned_spread": max(ms["preconditioned"]) / min(ms["preconditioned"]),
              "types": {t: {"median_ms": med(v), "min_ms": min(v), "ratio": med(v) / ref}
                        for t, v in ms.items()}})
        for k in ks.values():
            k.destroy()
        for o in {A, P, x, b, xt, w}:
            o.destroy()
        da.destroy()


def part_solve(ctx, n, reps, emit):
    for name, (argv, kind, _) in PATHS.items():
        da, A, P, x, b, xt, w = system(ctx, n, kind)
        out = {}
        for t in types_of(name):
            if t == "none":
                continue
            k = pb.KSP(A, P, pb.ksp_options(argv + ["-ksp_rtol", "1e-10", "-ksp_norm_type", t]))
            ms = []
            for rep in range(min(reps, 3) + 1):
                ctx.sync()
                t0 = time.perf_counter()
                reason, its, hist = k.solve(b, x)
                ctx.sync()
                if rep:
                    ms.append((time.perf_counter() - t0) * 1e3)
            A.mult(x, w)
            w.axpy(-1.0, b)
            out[t] = {"reason": int(reason), "its": int(its), "median_ms": med(ms),
                      "true_residual": w.norm() / b.norm(), "rnorm_over_rnorm0":
                      float(hist[-1] / hist[0]) if len(hist) and hist[0] else None}
            k.destroy()
        emit({"part": "solve", "path": name, "n": n, "rtol": 1e-10, "types": out})
        for o in {A, P, x, b, xt, w}:
            o.destroy()
        da.destroy()


def part_setup(ctx, n, reps, emit):
    da, A, P, x, b, xt, w = system(ctx, n, "star7")
    argv = ["-ksp_type", "cg", "-pc_type", "mg", "-ksp_initial_guess_nonzero"]
    ks = {t: pb.KSP(A, P, pb.ksp_options(argv + ["-ksp_norm_type", t]))
          for t in ("preconditioned", "unpreconditioned")}
    ms = {t: [] for t in ks}
    for rep in range(reps + 1):
        for t, k in ks.items():
            x.set(0.0)
            x.axpy(1.0 + 1e-6, xt)  # x0 = the solution, perturbed
            ctx.sync()
            t0 = time.perf_counter()
            k.begin(b, x)
            ctx.sync()
            dt = (time.perf_counter() - t0) * 1e3
            k.end()
            if rep:
                ms[t].append(dt)
    emit({"part": "setup", "path": "cg+mg nonzero guess", "n": n,
          "types": {t: {"median_ms": med(v), "min_ms": min(v)} for t, v in ms.items()}})
    for k in ks.values():
        k.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--parts", default="iter,solve,setup")
    ap.add_argument("--out", default=os.path.join("profiles", "ksp_norm_type", "bench_512.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    ctx = pb.Context(0)
    with open(args.out, "w") as f:
        def emit(d):
            line = json.dumps(d)
            print(line, flush=True)
            f.write(line + "\n")
            f.flush()
        for part in args.parts.split(","):
            {"iter": part_iter, "solve": part_solve, "setup": part_setup}[part](ctx, args.n,
                                                                                 args.reps, emit)
    ctx.destroy()


if __name__ == "__main__":
    main()
