"""The projected initial guess (-ksp_guess_type fischer) on one GPU, 7-point operator. One JSON line
per part, printed and appended to profiles/guess_fischer/bench_<n>.jsonl:

  probe  pb_ctx_copy_probe of this process (the rates below are put beside its median);
  vec    pb_vec_mdot / pb_vec_maxpy with nv vectors: the kernels' timers (`guess_mdot`,
         `guess_maxpy`) as GB/s at their algorithmic 8 (nv + 1) and 8 (nv + 2) B/DoF, and the wall
         time of the calls against the same projection composed from nv pb_vec_dot and nv
         pb_vec_axpy calls (what a caller had before), with the byte ratios 2 nv / (nv + 1) and
         3 nv / (nv + 2) they predict;
  loop   a time loop b_t = r0 + sin(0.3 t) r1 + 0.5 cos(0.2 t) r2 + drift * d_t (r_i, d_t = A applied
         to random fields) solved cold, warm-started (-ksp_initial_guess_nonzero) and with the
         projected guess, with jacobi and mg: iterations and wall ms per step, and for the
         projected guess the `guess_*` phase times per step.

usage: python scripts/bench_guess_fischer.py [--n 512] [--steps 12] [--nv 10] [--maxl 10]
       [--parts probe,vec,loop] [--pcs jacobi,mg]          (--n 256 for a quick run)
"""
import argparse
import json
import math
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import poissbox_amd as pb  # noqa: E402

PHASES = ["guess_mdot", "guess_maxpy", "guess_matvec", "guess_scale"]


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def wall(ctx, fn, reps):
    out = []
    for _ in range(reps):
        ctx.sync()
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--nv", type=int, default=10)
    ap.add_argument("--maxl", type=int, default=10)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rtol", type=float, default=1e-8)
    ap.add_argument("--drift", type=float, default=1e-6)
    ap.add_argument("--parts", default="probe,vec,loop")
    ap.add_argument("--pcs", default="jacobi,mg")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    parts = args.parts.split(",")
    n3, N = (args.n,) * 3, args.n ** 3
    path = args.out or os.path.join(REPO, "profiles", "guess_fischer", f"bench_{args.n}.jsonl")
    os.makedirs(os.path.dirname(path), exist_ok=True)

    def emit(rec):
        rec = dict(rec, n=args.n)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(path, "a") as f:
            f.write(line + "\n")

    ctx = pb.Context(0)
    da = pb.DA(ctx, n3)
    copy_med = None
    if "probe" in parts or "vec" in parts:
        best, copy_med = ctx.copy_probe(N, args.reps)
        emit({"part": "probe", "copy_best_gbs": best, "copy_median_gbs": copy_med})

    if "vec" in parts:
        nv = args.nv
        x, y = pb.Vec(da), pb.Vec(da)
        vs = [pb.Vec(da) for _ in range(nv)]
        x.set_random(1)
        for i, v in enumerate(vs):
            v.set_random(10 + i)
        alphas = [(-1.0) ** i * 1e-3 * (i + 1) for i in range(nv)]
        for _ in range(2):  # warm-up
            x.mdot(vs)
            y.maxpy(alphas, vs)
        ctx.set_timing(True, only=["guess_mdot", "guess_maxpy"])
        ctx.reset_timing()
        w_mdot = wall(ctx, lambda: x.mdot(vs), args.reps)
        w_maxpy = wall(ctx, lambda: y.maxpy(alphas, vs), args.reps)
        k_mdot = float(med(list(ctx.timing_samples("guess_mdot"))))
        k_maxpy = float(med(list(ctx.timing_samples("guess_maxpy"))))
        ctx.set_timing(False)

        def dots():
            for v in vs:
                x.dot(v)

        def axpys():
            for a, v in zip(alphas, vs):
                y.axpy(a, v)

        dots()
        axpys()
        w_dots, w_axpys = wall(ctx, dots, args.reps), wall(ctx, axpys, args.reps)
        gbs_mdot = 8 * (nv + 1) * N / (k_mdot * 1e-3) / 1e9
        gbs_maxpy = 8 * (nv + 2) * N / (k_maxpy * 1e-3) / 1e9
        emit({"part": "vec", "nv": nv,
              "mdot_kernel_ms": k_mdot, "mdot_gbs": gbs_mdot, "mdot_of_copy": gbs_mdot / copy_med,
              "maxpy_kernel_ms": k_maxpy, "maxpy_gbs": gbs_maxpy,
              "maxpy_of_copy": gbs_maxpy / copy_med,
              "mdot_wall_ms": med(w_mdot), "composed_dots_wall_ms": med(w_dots),
              "dots_speedup": med(w_dots) / med(w_mdot), "dots_byte_ratio": 2 * nv / (nv + 1),
              "maxpy_wall_ms": med(w_maxpy), "composed_axpys_wall_ms": med(w_axpys),
              "axpys_speedup": med(w_axpys) / med(w_maxpy), "axpys_byte_ratio": 3 * nv / (nv + 2)})
        for v in [x, y] + vs:
            v.destroy()

    if "loop" in parts:
        h = (1.0 / args.n,) * 3
        P, A, x, b = pb.initialise_linear_system(da, h)
        tmp, dn = pb.Vec(da), pb.Vec(da)
        r = [pb.Vec(da) for _ in range(3)]
        for i, v in enumerate(r):
            tmp.set_random(41 + i)
            A.mult(tmp, v)

        def rhs(t):
            tmp.set_random(1000 + t)
            A.mult(tmp, dn)
            r[0].copy_to(b)
            b.maxpy([math.sin(0.3 * t), 0.5 * math.cos(0.2 * t), args.drift], [r[1], r[2], dn])

        modes = {"cold": [], "warm": ["-ksp_initial_guess_nonzero"],
                 "fischer": ["-ksp_guess_type", "fischer", "-ksp_guess_fischer_model",
                             f"1,{args.maxl}"]}
        for pc in args.pcs.split(","):
            for mode, extra in modes.items():
                argv = ["-ksp_type", "cg", "-pc_type", pc, "-ksp_rtol", repr(args.rtol)] + extra
                k = pb.KSP(A, P, pb.ksp_options(argv))
                x.set(0.0)
                ctx.set_timing(mode == "fischer", only=PHASES)
                its, ms, phases = [], [], []
                for t in range(args.steps):
                    rhs(t)
                    ctx.reset_timing()
                    ctx.sync()
                    t0 = time.perf_counter()
                    _, it, _ = k.solve(b, x)
                    ctx.sync()
                    ms.append((time.perf_counter() - t0) * 1e3)
                    its.append(int(it))
                    if mode == "fischer":
                        phases.append({p: ctx.timing(p)[0] for p in PHASES})
                ctx.set_timing(False)
                rec = {"part": "loop", "pc": pc, "mode": mode, "rtol": args.rtol,
                       "drift": args.drift, "its": its, "ms": ms,
                       "ms_median_from_step_3": med(ms[3:]) if len(ms) > 3 else None}
                if mode == "fischer":
                    rec.update(maxl=args.maxl, phases_ms=phases,
                               guess_ms_median_from_step_3=med(
                                   [sum(p.values()) for p in phases[3:]])
                               if len(phases) > 3 else None)
                emit(rec)
                k.destroy()
    ctx.destroy()


if __name__ == "__main__":
    main()
