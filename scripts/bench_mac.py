"""The MAC-grid gradient, projection and divergence of the 7-point operators (pb_op_mac_*,
DESIGN.md §3.5 "Projection") on one GPU, one process, the compared paths interleaved rep by rep
(same buffers, same clocks). One JSON line per part:

  a  per launch, by the library's timers mac_grad / mac_project / mac_div: ms (median, min, max),
     achieved bytes/s at the algorithmic bytes (grad 16 + 24 B/DoF, project 64, div 24 + 8; on
     PB_OP_STAR7, with no beta to read, 8 + 24 and 56) and the fraction of the same process's copy
     probe, for PB_OP_VARCOEF under both means and PB_OP_STAR7; the nine launches alternate;
  u  mac_project (64 B/DoF) against the sequence it replaces, mac_grad and three pb_vec_axpy (40 +
     3 x 24 = 112 B/DoF), arithmetic mean: wall ms per sequence between two syncs, `seq` sequences
     per timed section, the two interleaved, each one's own spread beside the difference;
  p  one whole projection step on the random field (contrast 1000, arithmetic mean): mac_div, cg +
     the variable mg to rtol 1e-8, mac_project, wall ms each, and the share the two new passes
     take of the step.

usage: python scripts/bench_mac.py [--n 512] [--reps 10] [--parts a,u,p]
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
SEQ = 4
BYTES = {"mac_grad": (40.0, 32.0), "mac_project": (64.0, 56.0), "mac_div": (32.0, 32.0)}


def beta_random(N, contrast=1e3, seed=20240607):
    """log-uniform in [1 / contrast, 1]"""
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(-np.log(contrast), 0.0, N))


def operators(da, n, beta):
    h = (1.0 / n,) * 3
    bv = pb.Vec(da)
    bv.set_values(beta)
    ops = {}
    for name, mean in (("arithmetic", pb.COEF_ARITHMETIC), ("harmonic", pb.COEF_HARMONIC)):
        ops[name] = pb.Mat(da, pb.VARCOEF, h)
        ops[name].set_coefficient(bv, mean)
    ops["star7"] = pb.Mat(da, pb.STAR7, h)
    bv.destroy()
    return ops


def face_field(da, seed0):
    u3 = [pb.Vec(da) for _ in range(3)]
    for d, u in enumerate(u3):
        u.set_random(seed0 + d)
    return u3


def gbps(bytes_per_dof, N, ms):
    return bytes_per_dof * N / (ms * 1e-3) / 1e9


def part_a(ctx, n, reps, ops, p, u3, out):
    N = n ** 3
    calls = {"mac_grad": lambda A: A.mac_grad(p, u3),
             "mac_project": lambda A: A.mac_project(p, 1e-3, u3),
             "mac_div": lambda A: A.mac_div(u3, out)}
    t = {(op, c): [] for op in ops for c in calls}
    for rep in range(reps + 2):  # two warm-up rounds
        for c, call in calls.items():
            for op, A in ops.items():
                ctx.reset_timing()
                ctx.set_timing(True, only=list(calls))
                call(A)
                ctx.sync()
                v = ctx.timing_samples(c)
                ctx.set_timing(False)
                if rep >= 2:
                    t[op, c].append(float(v[0]))
    probe_best, probe_med = ctx.copy_probe(N, 10)
    row = {"part": "a", "n": n, "copy_probe_gbps": {"best": probe_best, "median": probe_med}}
    for op in ops:
        row[op] = {}
        for c in calls:
            bpd = BYTES[c][1 if op == "star7" else 0]
            m = med(t[op, c])
            row[op][c] = dict(stats(t[op, c]), bytes_per_dof=bpd, gbps=gbps(bpd, N, m),
                              frac_of_probe=gbps(bpd, N, m) / probe_med)
    print(json.dumps(row), flush=True)


def part_u(ctx, n, reps, A, p, u3, g3):
    s = 1e-3

    def fused():
        A.mac_project(p, s, u3)

    def unfused():
        A.mac_grad(p, g3)
        for u, g in zip(u3, g3):
            u.axpy(-s, g)

    t = {"fused": [], "unfused": []}
    for rep in range(reps + 2):
        for name, f in (("fused", fused), ("unfused", unfused)):
            ctx.sync()
            t0 = time.perf_counter()
            for _ in range(SEQ):
                f()
            ctx.sync()
            if rep >= 2:
                t[name].append((time.perf_counter() - t0) * 1e3 / SEQ)
    fm, um = med(t["fused"]), med(t["unfused"])
    spread = max(max(v) - min(v) for v in t.values())
    print(json.dumps({"part": "u", "n": n, "mean": "arithmetic", "sequences_per_section": SEQ,
                      "mac_project": dict(stats(t["fused"]), bytes_per_dof=64.0),
                      "mac_grad_plus_3_axpy": dict(stats(t["unfused"]), bytes_per_dof=112.0),
                      "saved_ms": um - fm, "ratio": um / fm, "larger_spread_ms": spread,
                      "fused_ahead_by_more_than_spread": um - fm > spread}), flush=True)


def part_p(ctx, n, reps, A, P, p, u3, b, w):
    k = pb.KSP(A, P, pb.ksp_options(["-ksp_type", "cg", "-pc_type", "mg", "-ksp_rtol", "1e-8"]))
    k.pc_set_coefficient_from(A)
    dt = 1e-3
    t = {"mac_div": [], "solve": [], "mac_project": []}
    its_all = []
    for rep in range(reps + 1):  # one warm-up step (the first solve builds the levels)
        for d, u in enumerate(u3):
            u.set_random(SEED + 10 * rep + d)
        p.set(0.0)
        step = {}
        for name, f in (("mac_div", lambda: A.mac_div(u3, b, 1.0 / dt)),
                        ("solve", lambda: k.solve(b, p)),
                        ("mac_project", lambda: A.mac_project(p, dt, u3))):
            ctx.sync()
            t0 = time.perf_counter()
            r = f()
            ctx.sync()
            step[name] = (time.perf_counter() - t0) * 1e3
            if name == "solve":
                reason, its = r[0], r[1]
        if rep >= 1:
            for name in t:
                t[name].append(step[name])
            its_all.append(int(its))
    true_res = rel_residual(A, b, p, w)
    A.mac_div(u3, w, 1.0 / dt)
    total = sum(med(v) for v in t.values())
    print(json.dumps({"part": "p", "n": n, "field": "random, contrast 1000", "mean": "arithmetic",
                      "solver": "cg + variable mg", "rtol": 1e-8,
                      "reason": pb.REASONS.get(reason, reason), "its": its_all,
                      "true_residual": true_res, "div_after_over_rhs": w.norm() / b.norm(),
                      "mac_div": stats(t["mac_div"]), "solve": stats(t["solve"]),
                      "mac_project": stats(t["mac_project"]), "step_median_ms": total,
                      "share_of_new_passes": (med(t["mac_div"]) + med(t["mac_project"])) / total}),
          flush=True)
    k.destroy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--parts", default="a,u,p")
    args = ap.parse_args()
    parts = args.parts.split(",")
    n, N = args.n, args.n ** 3
    ctx = pb.Context(0)
    da = pb.DA(ctx, (n,) * 3)
    ops = operators(da, n, beta_random(N))
    p, out, w = pb.Vec(da), pb.Vec(da), pb.Vec(da)
    p.set_random(SEED)
    u3, g3 = face_field(da, SEED + 1), face_field(da, SEED + 4)
    if "a" in parts:
        part_a(ctx, n, args.reps, ops, p, u3, out)
    if "u" in parts:
        part_u(ctx, n, args.reps, ops["arithmetic"], p, u3, g3)
    if "p" in parts:
        part_p(ctx, n, max(2, args.reps // 3), ops["arithmetic"], ops["star7"], p, u3, out, w)
    for o in list(ops.values()) + [p, out, w] + u3 + g3 + [da]:
        o.destroy()
    ctx.destroy()


if __name__ == "__main__":
    main()
