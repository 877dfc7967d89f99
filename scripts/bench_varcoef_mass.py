"""The mass term of PB_OP_VARCOEF (pb_op_set_mass) on one GPU, one process, the
compared launches interleaved rep by rep. One JSON line per part:

  a  the apply with the mass off (the kernel without the term), a scalar mass and a field mass,
     both means, on one operator whose mass is switched between the launches: ms median
     (min - max), GB/s at the nominal 24 / 24 / 32 B/DoF (x, beta [, m] read, y written) and the
     fraction of the same process's copy probe; whether the scalar form sits inside the mass-off
     launches' own spread and the field form's time as a multiple of the mass-off median
     (32 / 24 = 1.33 by the bytes).
  v  the variable V-cycle (pb_ksp_pc_apply of -pc_type mg with its levels from the operator)
     without and with a field mass, interleaved, one KSP each.
  s  CG to rtol 1e-8 with the variable mg, the variable sor and the variable Jacobi, the random
     field of contrast 1e3 (arithmetic mean), m uniform in [0.5, 1.5], s in {1, 100}, h = 1 / n,
     nullspace 0: iterations, reason, wall ms (best of 3), true residual ||b - A x|| / ||b||.

usage: python scripts/bench_varcoef_mass.py [--n 512] [--reps 10] [--parts a,v,s] [--max-it 20000]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from bench_ksp_fgmres import med, rel_residual, stats  # noqa: E402
from bench_varcoef import gbps  # noqa: E402
from bench_varcoef_mg import operator, random_field  # noqa: E402
import poissbox_amd as pb  # noqa: E402

SEED = 20231015
FORMS = [("off", 24.0), ("scalar", 24.0), ("field", 32.0)]


def mass_field(da, n, seed=20240911):
    """uniform in [0.5, 1.5] (tests/varcoef_mass_restatement.mass_uniform)"""
    mv = pb.Vec(da)
    mv.set_values(np.random.default_rng(seed).uniform(0.5, 1.5, n ** 3))
    return mv


def set_form(A, form, mv, s=100.0):
    if form == "off":
        A.set_mass(None, 0.0)
    elif form == "scalar":
        A.set_mass(None, s)
    else:
        A.set_mass(mv, s)


def part_a(ctx, n, reps):
    N = n ** 3
    da = pb.DA(ctx, (n,) * 3)
    beta = random_field(n)
    mv = mass_field(da, n)
    x, y = pb.Vec(da), pb.Vec(da)
    x.set_random(SEED)
    out = {"part": "a", "n": n}
    for mean_name, mean in (("arithmetic", pb.COEF_ARITHMETIC), ("harmonic", pb.COEF_HARMONIC)):
        # one operator per form: the launches alone are interleaved, not the copies of m
        ops = {}
        for form, _ in FORMS:
            ops[form] = operator(da, n, beta, mean)
            set_form(ops[form], form, mv)
        t = {form: [] for form, _ in FORMS}
        for rep in range(reps + 2):  # two warm-up rounds
            for form, _ in FORMS:
                ctx.reset_timing()
                ctx.set_timing(True, only=["varcoef"])
                ops[form].mult(x, y)
                ctx.sync()
                v = ctx.timing_samples("varcoef")
                ctx.set_timing(False)
                if rep >= 2:
                    t[form].append(float(v[0]))
        probe_best, probe_med = ctx.copy_probe(N, 10)
        res = {"copy_probe_gbps": {"best": probe_best, "median": probe_med}}
        for form, bpd in FORMS:
            m = med(t[form])
            res[form] = dict(stats(t[form]), bytes_per_dof=bpd, gbps=gbps(bpd, N, m),
                             frac_of_probe=gbps(bpd, N, m) / probe_med)
        off = res["off"]
        spread = off["max_ms"] - off["min_ms"]
        res["off_spread_ms"] = spread
        res["scalar_minus_off_ms"] = res["scalar"]["median_ms"] - off["median_ms"]
        res["scalar_inside_off_spread"] = abs(res["scalar_minus_off_ms"]) <= spread
        res["field_over_off"] = res["field"]["median_ms"] / off["median_ms"]
        res["field_minus_pro_rata_ms"] = res["field"]["median_ms"] - off["median_ms"] * 32.0 / 24.0
        res["field_inside_off_spread_of_pro_rata"] = abs(res["field_minus_pro_rata_ms"]) <= spread
        out[mean_name] = res
        for A in ops.values():
            A.destroy()
    print(json.dumps(out), flush=True)
    for o in (x, y, mv, da):
        o.destroy()


def part_v(ctx, n, reps):
    da = pb.DA(ctx, (n,) * 3)
    P = pb.Mat(da, pb.STAR7, (1.0 / n,) * 3)
    mv = mass_field(da, n)
    r, z = pb.Vec(da), pb.Vec(da)
    r.set_random(SEED)
    out = {"part": "v", "n": n}
    for mean_name, mean in (("arithmetic", pb.COEF_ARITHMETIC), ("harmonic", pb.COEF_HARMONIC)):
        ks = {}
        for form in ("off", "field"):
            A = operator(da, n, random_field(n), mean)
            set_form(A, form, mv)
            k = pb.KSP(A, P, pb.ksp_options(["-pc_type", "mg"], nullspace=0))
            k.pc_set_coefficient_from(A)
            k.pc_apply(r, z)  # (builds the levels outside the timed applies)
            ks[form] = (A, k)
        t = {form: [] for form in ks}
        for rep in range(reps + 2):
            for form, (A, k) in ks.items():
                ctx.reset_timing()
                ctx.set_timing(True, only=["mg_apply"])
                k.pc_apply(r, z)
                ctx.sync()
                v = ctx.timing_samples("mg_apply")
                ctx.set_timing(False)
                if rep >= 2:
                    t[form].append(float(v[0]))
        res = {form: stats(t[form]) for form in ks}
        res["field_over_off"] = res["field"]["median_ms"] / res["off"]["median_ms"]
        out[mean_name] = res
        for A, k in ks.values():
            k.destroy()
            A.destroy()
    print(json.dumps(out), flush=True)
    for o in (r, z, mv, P, da):
        o.destroy()


def part_s(ctx, n, max_it):
    da = pb.DA(ctx, (n,) * 3)
    P = pb.Mat(da, pb.STAR7, (1.0 / n,) * 3)
    mv = mass_field(da, n)
    x, b, xt, w = pb.Vec(da), pb.Vec(da), pb.Vec(da), pb.Vec(da)
    xt.set_random(SEED)
    A = operator(da, n, random_field(n), pb.COEF_ARITHMETIC)
    for s in (1.0, 100.0):
        A.set_mass(mv, s)
        A.mult(xt, b)
        rows = []
        for name, Pm, pc, var in (("cg + variable mg", P, "mg", True),
                                  ("cg + variable sor", P, "sor", True),
                                  ("cg + variable jacobi", A, "jacobi", False)):
            k = pb.KSP(A, Pm, pb.ksp_options(["-ksp_type", "cg", "-pc_type", pc, "-ksp_rtol",
                                              "1e-8", "-ksp_max_it", str(max_it)], nullspace=0))
            if var:
                k.pc_set_coefficient_from(A)
            ms = []
            for rep in range(3):
                x.set(0.0)
                ctx.sync()
                t0 = time.perf_counter()
                reason, its, hist = k.solve(b, x)
                ctx.sync()
                ms.append((time.perf_counter() - t0) * 1e3)
            rows.append({"solver": name, "reason": pb.REASONS.get(reason, reason), "its": int(its),
                         "best_ms": float(min(ms)), "wall": stats(ms),
                         "true_residual": rel_residual(A, b, x, w)})
            k.destroy()
        print(json.dumps({"part": "s", "n": n, "field": "random", "contrast": 1000.0,
                          "mean": "arithmetic", "s": s, "h": 1.0 / n, "rtol": 1e-8,
                          "solves": rows}), flush=True)
    A.destroy()
    for o in (x, b, xt, w, mv, P, da):
        o.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parts", default="a,v,s")
    ap.add_argument("--max-it", type=int, default=20000)
    args = ap.parse_args()
    parts = args.parts.split(",")
    ctx = pb.Context(0)
    if "a" in parts:
        part_a(ctx, args.n, args.reps)
    if "v" in parts:
        part_v(ctx, args.n, args.reps)
    if "s" in parts:
        part_s(ctx, args.n, args.max_it)
    ctx.destroy()


if __name__ == "__main__":
    main()
