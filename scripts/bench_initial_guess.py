"""Setup and solve from a nonzero initial guess (-ksp_initial_guess_nonzero) on one GPU, 7-point
operator, Jacobi. One JSON line per part:

  a  the fused setup pass (reads x0, b; writes r, p: 32 B/DoF) -- its timer `cg_init_guess`, its
     fraction of the 8 TB/s peak beside the matvec's (16 B/DoF, timer `stencil`) from this
     process, and the wall time of a whole pb_ksp_begin;
  b  the same setup emulated through the public vector calls, as a caller had to before the
     option existed: pb_op_apply (w = A x0), pb_vec_aypx (w = b - w), zero-guess pb_ksp_begin on w
     -- wall time of the three calls, and the timers of the two that have one. Runs on any build
     of the library (PB_LIB=variants/<parent>.so times the parent commit);
  c  a full solve to rtol 1e-10 from x0 = x* + 1e-6 random (x* = the cold solve's x, whose
     entries are O(1)) against the cold solve.

usage: python scripts/bench_initial_guess.py [--n 512] [--reps 20] [--parts a,b,c]
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import poissbox_amd as pb  # noqa: E402

SEED = 20231015
PEAK_GBS = 8000.0
JACOBI = ["-ksp_type", "cg", "-pc_type", "jacobi"]


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def timer_ms(ctx, name):
    s = ctx.timing_samples(name)
    return {"median_ms": float(med(list(s))), "min_ms": float(s.min()), "launches": int(len(s))} \
        if len(s) else None


def frac(ms, bytes_per_dof, N):
    return bytes_per_dof * N / (ms * 1e-3) / 1e9 / PEAK_GBS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parts", default="a,b,c")
    args = ap.parse_args()
    parts = args.parts.split(",")
    n3 = (args.n,) * 3
    N = args.n ** 3
    h = (1.0 / args.n,) * 3
    ctx = pb.Context(0)
    da = pb.DA(ctx, n3)
    P, A, x, b = pb.initialise_linear_system(da, h)
    xt, w, d = pb.Vec(da), pb.Vec(da), pb.Vec(da)
    xt.set_random(SEED)
    A.mult(xt, b)
    x.set_random(7)
    lib = os.environ.get("PB_LIB", "in-tree")
    still = dict(rtol=0.0, atol=0.0, dtol=1e300, max_it=8)

    if "a" in parts:
        k = pb.KSP(A, P, pb.ksp_options(JACOBI + ["-ksp_initial_guess_nonzero"], **still))
        for _ in range(2):  # warm-up: allocations, first touch
            k.begin(b, x)
            k.end()
            A.mult(x, w)
        ctx.set_timing(True, only=["cg_init_guess", "stencil"])
        ctx.reset_timing()
        wall = []
        for _ in range(args.reps):
            ctx.sync()
            t0 = time.perf_counter()
            k.begin(b, x)
            wall.append((time.perf_counter() - t0) * 1e3)
            k.end()
            A.mult(x, w)
        ctx.sync()
        ti, tm = timer_ms(ctx, "cg_init_guess"), timer_ms(ctx, "stencil")
        ctx.set_timing(False)
        k.destroy()
        print(json.dumps({"part": "a", "lib": lib, "n": args.n, "setup_pass": ti, "matvec": tm,
                          "setup_pass_frac_of_peak": frac(ti["median_ms"], 32, N),
                          "matvec_frac_of_peak": frac(tm["median_ms"], 16, N),
                          "begin_wall_ms_median": med(wall), "begin_wall_ms_min": min(wall)}),
              flush=True)

    if "b" in parts:
        k = pb.KSP(A, P, pb.ksp_options(JACOBI, **still))

        def emulate():
            A.mult(x, w)      # w = A x0
            w.aypx(-1.0, b)   # w = b - w
            k.begin(w, d)     # zero-guess setup of the correction's solve

        for _ in range(2):
            emulate()
            k.end()
        ctx.set_timing(True, only=["cg_init", "stencil"])
        ctx.reset_timing()
        wall = []
        for _ in range(args.reps):
            ctx.sync()
            t0 = time.perf_counter()
            emulate()
            wall.append((time.perf_counter() - t0) * 1e3)
            k.end()
        ctx.sync()
        ti, tm = timer_ms(ctx, "cg_init"), timer_ms(ctx, "stencil")
        ctx.set_timing(False)
        # the aypx pass has no timer of its own: timed alone, between synchronisations
        ay = []
        for _ in range(args.reps):
            ctx.sync()
            t0 = time.perf_counter()
            w.aypx(-1.0, b)
            ctx.sync()
            ay.append((time.perf_counter() - t0) * 1e3)
        k.destroy()
        print(json.dumps({"part": "b", "lib": lib, "n": args.n, "cg_init": ti, "matvec": tm,
                          "aypx_wall_ms_median": med(ay),
                          "kernels_ms_median": ti["median_ms"] + tm["median_ms"] + med(ay),
                          "emulation_wall_ms_median": med(wall),
                          "emulation_wall_ms_min": min(wall)}), flush=True)

    if "c" in parts:
        opts = JACOBI + ["-ksp_rtol", "1e-10"]
        kc = pb.KSP(A, P, pb.ksp_options(opts))
        kw = pb.KSP(A, P, pb.ksp_options(opts + ["-ksp_initial_guess_nonzero"]))
        kc.solve(b, x)  # warm-up; x = x*
        out = {"part": "c", "lib": lib, "n": args.n}
        ctx.sync()
        t0 = time.perf_counter()
        reason, its, hist = kc.solve(b, x)
        ctx.sync()
        out["cold"] = {"reason": int(reason), "its": int(its),
                       "solve_ms": (time.perf_counter() - t0) * 1e3}
        xt.set_random(11)
        x.copy_to(d)  # d = x*
        for rep in range(2):  # (the first warm solve also allocates nothing new: same buffers)
            d.copy_to(x)
            x.axpy(1e-6, xt)
            ctx.sync()
            t0 = time.perf_counter()
            reason, its, hist = kw.solve(b, x)
            ctx.sync()
            out["warm"] = {"reason": int(reason), "its": int(its),
                           "solve_ms": (time.perf_counter() - t0) * 1e3,
                           "z0_over_rnorm0": float(hist[0] / kw.result.rnorm0)}
        A.mult(x, w)
        w.axpy(-1.0, b)
        out["warm"]["rel_residual"] = w.norm() / b.norm()
        print(json.dumps(out), flush=True)
        kc.destroy()
        kw.destroy()
    ctx.destroy()


if __name__ == "__main__":
    main()
