"""The -mg_levels_* level smoothers of -pc_type mg on one GPU, one process, the compared paths
interleaved rep by rep (same buffers, same clocks), CG to rtol 1e-10. One JSON line per part:

  solve   per path (SOR V(1,1) = the default, SOR nu = 2, Chebyshev/Jacobi nu = 1, 2, 3,
          Richardson/Jacobi scale 6/7 nu = 2): wall ms of pb_ksp_solve, iterations, the true
          residual ||b - A x|| / ||b||, wall ms of one V-cycle (pb_ksp_pc_apply);
  fused   Chebyshev/Jacobi nu = 2 with tuning mg_poly_fused = 0 (vector kernel + residual pass)
          against 1, solve and V-cycle;
  pass    the engine pass (timer mg_poly) per launch on the fine level, by form -- from b alone
          (24 B/DoF), from y and r (40 B/DoF), from y, y_prev and r (48 B/DoF) -- against the same
          process's copy probe (16 B/DoF) at those algorithmic bytes.

usage: python scripts/bench_mg_smoothers.py [--n 512] [--reps 10] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import poissbox_amd as pb  # noqa: E402

SEED = 20231015
CHEB = ["-mg_levels_ksp_type", "chebyshev", "-mg_levels_pc_type", "jacobi"]
PATHS = [
    ("sor_v11_default", []),
    ("sor_nu2", ["-mg_levels_ksp_max_it", "2"]),
    ("cheb_jacobi_nu1", CHEB + ["-mg_levels_ksp_max_it", "1"]),
    ("cheb_jacobi_nu2", CHEB + ["-mg_levels_ksp_max_it", "2"]),
    ("cheb_jacobi_nu3", CHEB + ["-mg_levels_ksp_max_it", "3"]),
    ("rich_jacobi_6_7_nu2", ["-mg_levels_pc_type", "jacobi", "-mg_levels_ksp_richardson_scale",
                             repr(6.0 / 7.0), "-mg_levels_ksp_max_it", "2"]),
]


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def stats(v):
    return {"median_ms": float(med(v)), "min_ms": float(min(v)), "max_ms": float(max(v)),
            "n": len(v)}


def timed(ctx, fn):
    ctx.sync()
    t0 = time.perf_counter()
    r = fn()
    ctx.sync()
    return (time.perf_counter() - t0) * 1e3, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    n, N = args.n, args.n ** 3
    lines = []

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        lines.append(s)

    ctx = pb.Context(0)
    h = (1.0 / n,) * 3
    da = pb.DA(ctx, (n,) * 3)
    P, A, x, b = pb.initialise_linear_system(da, h)
    xt, w = pb.Vec(da), pb.Vec(da)
    xt.set_random(SEED)
    A.mult(xt, b)
    base = ["-ksp_type", "cg", "-pc_type", "mg", "-ksp_rtol", "1e-10"]
    ksps = {name: pb.KSP(A, P, pb.ksp_options(base + extra)) for name, extra in PATHS}

    def residual():
        A.mult(x, w)
        w.axpy(-1.0, b)
        return w.norm() / b.norm()

    # ---- solve: every path, interleaved ----
    out = {name: {"solve": [], "vcycle": []} for name, _ in PATHS}
    for rep in range(args.reps + 2):  # two warm-up rounds: allocations, first touch
        for name, _ in PATHS:
            k = ksps[name]
            ms, (reason, its, _) = timed(ctx, lambda: k.solve(b, x))
            if rep >= 2:
                out[name]["solve"].append(ms)
            out[name].update(reason=int(reason), its=int(its))
            if rep == 2:
                out[name]["rel_residual"] = residual()
            ms, _ = timed(ctx, lambda: k.pc_apply(b, w))
            if rep >= 2:
                out[name]["vcycle"].append(ms)
    for name, _ in PATHS:
        o = out[name]
        emit({"part": "solve", "path": name, "n": n, "reason": o["reason"], "its": o["its"],
              "rel_residual": o["rel_residual"], "solve": stats(o["solve"]),
              "vcycle": stats(o["vcycle"]),
              "ms_per_iteration": med(o["solve"]) / max(o["its"], 1)})

    # ---- fused against unfused (bit-identical), Chebyshev/Jacobi nu = 2 ----
    k = ksps["cheb_jacobi_nu2"]
    fu = {1: {"solve": [], "vcycle": []}, 0: {"solve": [], "vcycle": []}}
    for rep in range(args.reps + 1):
        for fused in (1, 0):
            pb.tune_set("mg_poly_fused", fused)
            ms, (reason, its, _) = timed(ctx, lambda: k.solve(b, x))
            ms2, _ = timed(ctx, lambda: k.pc_apply(b, w))
            if rep >= 1:
                fu[fused]["solve"].append(ms)
                fu[fused]["vcycle"].append(ms2)
            fu[fused]["its"] = int(its)
    pb.tune_reset()
    emit({"part": "fused", "path": "cheb_jacobi_nu2", "n": n,
          "mg_poly_fused_1": {"its": fu[1]["its"], "solve": stats(fu[1]["solve"]),
                              "vcycle": stats(fu[1]["vcycle"])},
          "mg_poly_fused_0": {"its": fu[0]["its"], "solve": stats(fu[0]["solve"]),
                              "vcycle": stats(fu[0]["vcycle"])},
          "unfused_over_fused_vcycle": med(fu[0]["vcycle"]) / med(fu[1]["vcycle"])})

    # ---- the engine pass per launch, by form (Chebyshev/Jacobi nu = 3: every form runs) ----
    # launches of one V-cycle in order: fine level pre-smoothing (b; y, r; y, y_prev, r), the
    # same on every coarser engine level, then the post-smoothing steps that store a residual
    # (y, r; y, y_prev, r) from the coarsest engine level up to the fine one
    k = ksps["cheb_jacobi_nu3"]
    k.pc_apply(b, w)
    ctx.set_timing(True, only=["mg_poly"])
    ctx.reset_timing()
    for _ in range(args.reps):
        k.pc_apply(b, w)
    ctx.sync()
    s = [float(v) for v in ctx.timing_samples("mg_poly")]
    ctx.set_timing(False)
    per = len(s) // args.reps
    probe_best, probe_med = ctx.copy_probe(N, 10)
    forms = {"from_b_24B": ([0], 24.0), "from_y_r_40B": ([1, per - 2], 40.0),
             "from_y_yprev_r_48B": ([2, per - 1], 48.0)}
    rec = {"part": "pass", "n": n, "launches_per_vcycle": per,
           "copy_probe_gbps": {"best": probe_best, "median": probe_med}}
    if per >= 5 and per * args.reps == len(s):
        for name, (idx, bytes_) in forms.items():
            v = [s[r * per + i] for r in range(args.reps) for i in idx]
            gbps = bytes_ * N / (med(v) * 1e-3) / 1e9
            rec[name] = dict(stats(v), gbps=gbps, frac_of_probe=gbps / probe_med)
    else:
        rec["samples"] = s[:64]
    emit(rec)

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    for o in list(ksps.values()) + [x, b, xt, w, A, P, da]:
        o.destroy()
    ctx.destroy()


if __name__ == "__main__":
    main()
