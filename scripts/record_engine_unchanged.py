"""Record what every user of the 7-point engine (star7_kernel / tiled_epi_kernel, pb_star7.hpp)
computes, bit for bit, so that a later change to the engine or to its launch path can be checked
against the commit this ran on (tests/test_gpu_engine_unchanged.py compares a fresh run with the
file by np.array_equal).

The kernels' partial sums depend on the tile shape, the z-chunks and the march direction the host
launch path chooses, so every user runs once per tile shape the dispatch (for_tile_shape) can take:

  64x64x64     V = 2, TY = 4
  63x30x17     V = 1, TY = 2
  66x33x16     V = 2, TY = 1
  512x512x8    the TALL promotion to 8-row tiles (plane >= 512^2, ny a multiple of 8)
  1024x1024x4  the WIDE8 promotion (more 4-row columns than WGCU x CUs on a 256-CU part)

(the chunk skew is reached only at 512^3: tests/test_gpu_fullsize.py covers it.)

Users: the operator apply (two applies, one per march direction; digests only), and short solves
of 10 iterations (rtol 0, so none stops early) from a random right-hand side:
  cg            -ksp_type cg -pc_type jacobi as it runs by default: the stages folded into the
                passes' prologues, p stored by pass B (the PSTORE_B form), x deferred over four
  cg_unfolded   tuning cg_fold = 0: the separate finalize launches
  cg_defer2, cg_defer0   tuning cg_defer_x = 2 / 0: pass B's other x-update variants
  cg_sr         -ksp_cg_single_reduction (passes P and S)
  cg_guess      -ksp_initial_guess_nonzero from a random x0 (GuessInit)
  richardson, chebyshev, fgmres, pipecg      their fused passes
  pipecg_unfused   tuning pipecg_fused = 0: PcgEpi from stored fields (launch_tiled)
  mg_sor, mg_rich, mg_cheb   cg with -pc_type mg and the SOR / damped-Jacobi / Chebyshev level
                smoothers, tuning mg_engine_min_plane = 0 so that every level runs the engine passes
                (SorHalf, Red0Load, ResidEpi, PolyLoad / PolyEpi); with a stored-z PC pass A stores
                p and pass B takes the plain p (PassA, PassB without PST)
Of each solve the file keeps the residual history as raw float64, the (reason, its) pair, a blake2b
digest of the solution and every 257th value of it -- on the two large shapes every 4th / 8th of
those (at most 2048 values per solution), which keeps the file below 1 MiB; the digest covers
every bit either way, the samples only show where to look after a mismatch.
At 64^3 the multigrid solves reach rounding level before 10 iterations: mg_rich and mg_cheb end
after 9 and 7 with DIVERGED_INDEFINITE_PC, reproducibly; reason and count are part of the pin.

Pairs left out: multigrid needs even extents, so mg_sor, mg_rich and mg_cheb do not run on 63x30x17
and 66x33x16. A (user, shape) pair the library refuses is recorded as its error code under
"<shape>__<user>__error" -- the test then fails if that ever changes; at the commit recorded these
are exactly the six multigrid pairs above.

usage (on the commit to record, with a GPU): python scripts/record_engine_unchanged.py [OUT.npz]
default OUT: tests/golden/engine_unchanged.npz"""
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import poissbox_amd as pb  # noqa: E402
from oracle import oracle as O  # noqa: E402

SHAPES = [(64, 64, 64), (63, 30, 17), (66, 33, 16), (512, 512, 8), (1024, 1024, 4)]
SEED = 20231015
STRIDE = 257
MAX_SAMPLES = 2048
ITS = 10
FIXED = ["-ksp_rtol", "0", "-ksp_atol", "0", "-ksp_divtol", "1e300", "-ksp_max_it", str(ITS)]
JACOBI = ["-pc_type", "jacobi"]
MG = ["-ksp_type", "cg", "-pc_type", "mg"]
ENGINE = {"mg_engine_min_plane": 0}


def levels(ksp, pc, nu, scale=None):
    a = ["-mg_levels_ksp_type", ksp, "-mg_levels_pc_type", pc, "-mg_levels_ksp_max_it", str(nu)]
    return a + (["-mg_levels_ksp_richardson_scale", repr(scale)] if scale else [])


# user -> (argv, tuning, nonzero initial guess)
USERS = {
    "cg": (["-ksp_type", "cg"] + JACOBI, {}, False),
    "cg_unfolded": (["-ksp_type", "cg"] + JACOBI, {"cg_fold": 0}, False),
    "cg_defer2": (["-ksp_type", "cg"] + JACOBI, {"cg_defer_x": 2}, False),
    "cg_defer0": (["-ksp_type", "cg"] + JACOBI, {"cg_defer_x": 0}, False),
    "cg_sr": (["-ksp_type", "cg", "-ksp_cg_single_reduction"] + JACOBI, {}, False),
    "cg_guess": (["-ksp_type", "cg", "-ksp_initial_guess_nonzero"] + JACOBI, {}, True),
    "richardson": (["-ksp_type", "richardson", "-ksp_richardson_scale", repr(2.0 / 3.0)] + JACOBI,
                   {}, False),
    "chebyshev": (["-ksp_type", "chebyshev"] + JACOBI, {}, False),
    "fgmres": (["-ksp_type", "fgmres"] + JACOBI, {}, False),
    "pipecg": (["-ksp_type", "pipecg"] + JACOBI, {}, False),
    "pipecg_unfused": (["-ksp_type", "pipecg"] + JACOBI, {"pipecg_fused": 0}, False),
    "mg_sor": (MG, ENGINE, False),
    "mg_rich": (MG + levels("richardson", "jacobi", 2, 6.0 / 7.0), ENGINE, False),
    "mg_cheb": (MG + levels("chebyshev", "jacobi", 3), ENGINE, False),
}


def digest(a):
    return np.frombuffer(hashlib.blake2b(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def sample(x):
    """every STRIDE-th value; of a long solution every (STRIDE * m)-th, at most MAX_SAMPLES"""
    m = -(-x.size // (STRIDE * MAX_SAMPLES))
    return x[::STRIDE * m].copy()


def shape_tag(n3):
    return "x".join(str(m) for m in n3)


def record_shape(ctx, n3, users=None):
    """name -> array, for one shape (users: a subset of USERS and "apply", default all)"""
    N = int(np.prod(n3))
    h = tuple(1.0 / m for m in n3)
    tag = shape_tag(n3)
    b = O.fill_random(N, SEED + N)
    x0 = O.fill_random(N, SEED + N + 1)
    rec = {}
    da = pb.DA(ctx, n3)
    P, A = pb.Mat(da, pb.ASSEMBLED27, h), pb.Mat(da, pb.STAR7, h)
    xv, bv = pb.Vec(da), pb.Vec(da)
    try:
        if users is None or "apply" in users:
            bv.set_values(b)
            for d in (0, 1):  # consecutive applies march in alternating directions
                A.mult(bv, xv)
                rec[f"{tag}__apply{d}__digest"] = digest(xv.get_values())
        for user, (argv, tuning, guess) in USERS.items():
            if users is not None and user not in users:
                continue
            pb.tune_reset()
            for name, v in tuning.items():
                pb.tune_set(name, v)
            bv.set_values(b)
            xv.set_values(x0 if guess else np.full(N, 7.25))  # (a zero-guess solve overwrites x)
            k = None
            try:
                k = pb.KSP(A, P, pb.ksp_options(argv + FIXED))
                reason, its, hist = k.solve(bv, xv)
            except pb.PbError as e:
                rec[f"{tag}__{user}__error"] = np.array([e.code], dtype=np.int64)
                continue
            finally:
                if k is not None:
                    k.destroy()
                pb.tune_reset()
            x = xv.get_values()
            rec[f"{tag}__{user}__history"] = np.asarray(hist, dtype=np.float64).copy()
            rec[f"{tag}__{user}__status"] = np.array([reason, its], dtype=np.int64)
            rec[f"{tag}__{user}__digest"] = digest(x)
            rec[f"{tag}__{user}__sample"] = sample(x)
    finally:
        for o in (A, P, xv, bv):
            o.destroy()
        da.destroy()
    return rec


def record(ctx):
    rec = {}
    for n3 in SHAPES:
        rec.update(record_shape(ctx, n3))
    return rec


if __name__ == "__main__":
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden",
                                                             "engine_unchanged.npz")
    ctx = pb.Context(0)
    rec = record(ctx)
    ctx.destroy()
    np.savez_compressed(dst, **rec)
    errors = sorted(k for k in rec if k.endswith("__error"))
    print("wrote", dst, len(rec), "arrays; refused:", errors)
