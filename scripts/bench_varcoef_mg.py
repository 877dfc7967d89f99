"""The variable-coefficient -pc_type sor | mg (pb_ksp_pc_set_coefficient_from) on
one GPU, one process, the compared paths interleaved rep by rep. One JSON line per part:

  k  the level-0 passes of one apply, per launch, under the four settings of mg_varcoef_pre_fused x
     mg_varcoef_dinv_stored (interleaved): the zero-start pre-smoothing as one pass (timer vmg_pre)
     against its two launches (vmg_pre_red + vmg_pre_black), the in-place half-sweep (vmg_half),
     the residual (vmg_residual, the largest launch of a V-cycle = level 0), each as ms and as
     bytes/s at its nominal traffic against the same process's copy probe; and the V-cycle
     (mg_apply) of the variable levels against the constant-coefficient one of the same KSP.
     Nominal B/DoF (whole lines of every array touched): pre 32 (b, dinv, beta read, x written),
     half-sweep 40 with the stored dinv (x, beta, b, dinv read, x written) and 32 forming it,
     residual 32 (x, beta, b read, res written).
  s  CG to rtol 1e-8: the sphere jump (harmonic mean) at contrast 10 and 1000 and the random
     field of contrast 1e3 (arithmetic mean), with the variable mg, mg and fft from a constant P
     and the variable Jacobi: iterations, reason, wall ms, true residual ||b - A x|| / ||b||.

usage: python scripts/bench_varcoef_mg.py [--n 512] [--reps 10] [--parts k,s] [--max-it 20000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ksp_fgmres import med, rel_residual, stats  # noqa: E402
from bench_varcoef import gbps, sphere  # noqa: E402
import poissbox_amd as pb  # noqa: E402

SEED = 20231015
TIMERS = ["vmg_pre", "vmg_pre_red", "vmg_pre_black", "vmg_half", "vmg_residual", "mg_apply"]
BYTES = {"vmg_pre": 32.0, "vmg_half_stored": 40.0, "vmg_half_formed": 32.0, "vmg_residual": 32.0}
# (the two launches: red from zero reads b [and dinv | beta] and writes x, then a half-sweep)
PAIR_BYTES = {1: 24.0 + 40.0, 0: 24.0 + 32.0}


def random_field(n, contrast=1e3, seed=20240607):
    """log-uniform in [1 / contrast, 1] (tests/varcoef_restatement.beta_random)"""
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(-np.log(contrast), 0.0, n ** 3))


def operator(da, n, beta, mean):
    A = pb.Mat(da, pb.VARCOEF, (1.0 / n,) * 3)
    bv = pb.Vec(da)
    bv.set_values(beta)
    A.set_coefficient(bv, mean)
    bv.destroy()
    return A


def part_k(ctx, n, reps):
    N = n ** 3
    da = pb.DA(ctx, (n,) * 3)
    P = pb.Mat(da, pb.STAR7, (1.0 / n,) * 3)
    r, z = pb.Vec(da), pb.Vec(da)
    r.set_random(SEED)
    out = {"part": "k", "n": n}
    for mean_name, mean in (("arithmetic", pb.COEF_ARITHMETIC), ("harmonic", pb.COEF_HARMONIC)):
        A = operator(da, n, sphere(n, 1e-3), mean)
        k = pb.KSP(A, P, pb.ksp_options(["-pc_type", "mg"]))
        kc = pb.KSP(A, P, pb.ksp_options(["-pc_type", "mg"]))  # the constant-coefficient levels
        k.pc_set_coefficient_from(A)
        k.pc_apply(r, z)  # (builds the levels outside the timed applies)
        settings = [(f, d) for f in (1, 0) for d in (1, 0)]
        t = {s: {nm: [] for nm in TIMERS} for s in settings}
        const = []
        for rep in range(reps + 2):  # two warm-up rounds
            for s in settings + ["const"]:
                pb.tune_reset()
                if s != "const":
                    pb.tune_set("mg_varcoef_pre_fused", s[0])
                    pb.tune_set("mg_varcoef_dinv_stored", s[1])
                ctx.reset_timing()
                ctx.set_timing(True, only=TIMERS)
                (kc if s == "const" else k).pc_apply(r, z)
                ctx.sync()
                got = {nm: [float(v) for v in ctx.timing_samples(nm)] for nm in TIMERS}
                ctx.set_timing(False)
                if rep < 2:
                    continue
                if s == "const":
                    const.append(got["mg_apply"][0])
                    continue
                for nm in TIMERS:  # level 0 = the longest launch of a phase
                    if got[nm]:
                        t[s][nm].append(max(got[nm]))
        pb.tune_reset()
        probe_best, probe_med = ctx.copy_probe(N, 10)

        def rate(name, ms):
            g = gbps(BYTES[name], N, ms)
            return {"median_ms": ms, "gbps": g, "frac_of_probe": g / probe_med}

        res = {"copy_probe_gbps": {"best": probe_best, "median": probe_med},
               "vcycle_constant": stats(const)}
        for s in settings:
            row = {"vcycle": stats(t[s]["mg_apply"]), "half": stats(t[s]["vmg_half"]),
                   "half_rate": rate("vmg_half_stored" if s[1] else "vmg_half_formed",
                                     med(t[s]["vmg_half"])),
                   "residual": stats(t[s]["vmg_residual"]),
                   "residual_rate": rate("vmg_residual", med(t[s]["vmg_residual"]))}
            if s[0]:
                row["pre"] = stats(t[s]["vmg_pre"])
                row["pre_rate"] = rate("vmg_pre", med(t[s]["vmg_pre"]))
            else:
                pair = [a + c for a, c in zip(t[s]["vmg_pre_red"], t[s]["vmg_pre_black"])]
                row["pre_red"] = stats(t[s]["vmg_pre_red"])
                row["pre_black"] = stats(t[s]["vmg_pre_black"])
                row["pre_pair"] = stats(pair)
                BYTES["pair"] = PAIR_BYTES[s[1]]
                row["pre_pair_rate"] = rate("pair", med(pair))
            res[f"pre_fused_{s[0]}_dinv_stored_{s[1]}"] = row
        for d in (1, 0):  # the fused pre-pass against the two launches and their own spread
            fu = res[f"pre_fused_1_dinv_stored_{d}"]["pre"]
            un = res[f"pre_fused_0_dinv_stored_{d}"]["pre_pair"]
            res[f"pre_fused_ahead_by_more_than_spread_dinv_{d}"] = (
                un["median_ms"] - fu["median_ms"] > un["max_ms"] - un["min_ms"])
        h1 = res["pre_fused_1_dinv_stored_1"]["half"]
        h0 = res["pre_fused_1_dinv_stored_0"]["half"]
        res["dinv_stored_ahead_by_more_than_spread"] = (
            h0["median_ms"] - h1["median_ms"] > h0["max_ms"] - h0["min_ms"])
        out[mean_name] = res
        k.destroy()
        kc.destroy()
        A.destroy()
    print(json.dumps(out), flush=True)
    for o in (r, z, P, da):
        o.destroy()


def part_s(ctx, n, reps, max_it):
    da = pb.DA(ctx, (n,) * 3)
    P = pb.Mat(da, pb.STAR7, (1.0 / n,) * 3)
    x, b, xt, w = pb.Vec(da), pb.Vec(da), pb.Vec(da), pb.Vec(da)
    xt.set_random(SEED)
    cases = [("sphere", 10.0, "harmonic", pb.COEF_HARMONIC), ("sphere", 1000.0, "harmonic", pb.COEF_HARMONIC),
             ("random", 1000.0, "arithmetic", pb.COEF_ARITHMETIC)]
    for field, contrast, mean_name, mean in cases:
        beta = sphere(n, 1.0 / contrast) if field == "sphere" else random_field(n, contrast)
        A = operator(da, n, beta, mean)
        A.mult(xt, b)
        rows = []
        for name, Pm, pc, var in (("cg + variable mg", P, "mg", True), ("cg + mg (constant P)", P, "mg", False),
                                  ("cg + fft (constant P)", P, "fft", False),
                                  ("cg + variable jacobi", A, "jacobi", False)):
            k = pb.KSP(A, Pm, pb.ksp_options(["-ksp_type", "cg", "-pc_type", pc, "-ksp_rtol",
                                              "1e-8", "-ksp_max_it", str(max_it)]))
            if var:
                k.pc_set_coefficient_from(A)
            ms = []
            for rep in range(1 if pc == "jacobi" else reps):
                x.set(0.0)
                ctx.sync()
                t0 = time.perf_counter()
                reason, its, hist = k.solve(b, x)
                ctx.sync()
                ms.append((time.perf_counter() - t0) * 1e3)
            rows.append({"solver": name, "reason": pb.REASONS.get(reason, reason), "its": int(its),
                         "wall": stats(ms), "true_residual": rel_residual(A, b, x, w)})
            k.destroy()
        print(json.dumps({"part": "s", "n": n, "field": field, "contrast": contrast,
                          "mean": mean_name, "rtol": 1e-8, "solves": rows}), flush=True)
        A.destroy()
    for o in (x, b, xt, w, P, da):
        o.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parts", default="k,s")
    ap.add_argument("--max-it", type=int, default=20000)
    args = ap.parse_args()
    parts = args.parts.split(",")
    ctx = pb.Context(0)
    if "k" in parts:
        part_k(ctx, args.n, args.reps)
    if "s" in parts:
        part_s(ctx, args.n, max(3, args.reps // 3), args.max_it)
    ctx.destroy()


if __name__ == "__main__":
    main()
