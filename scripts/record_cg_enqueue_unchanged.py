"""Record what the CG host enqueue paths compute, bit for bit, on every topology that takes another
branch of them, so that a change to the host code of the default solver (which launches run, in what
order, with which partial offsets and state slots) can be checked against the commit this ran on
(tests/test_gpu_cg_enqueue_unchanged.py compares a fresh run with the file by np.array_equal).

tests/golden/engine_unchanged.npz pins one rank and pb_ksp_solve only. Here every solve runs as
begin, iterate(3), iterate(7), end -- the batch tails and the state slots across calls are part of
the pin -- with record_engine_unchanged.py's options (10 iterations, rtol 0, divtol 1e300), its
digest and its samples.

Topologies (TOPOLOGIES) and their cases:
  one       one rank, 32x24x16:
              cg, cg_c1          -pc_type jacobi with check_every 8 (the stages folded into the
                                 passes' prologues) and 1 (the separate finalize launches)
              cg_sr, cg_sr_c1    -ksp_cg_single_reduction, the same two
              guess, guess_sr, guess_mg   -ksp_initial_guess_nonzero from a random x0 with jacobi,
                                 with the single reduction, with -pc_type mg
              mg_unp             -pc_type mg -ksp_norm_type unpreconditioned (the RrParts path)
              assembled          A = P = the assembled matrix with jacobi (the generic iteration)
  one64     one rank, 64x64x64, period 2 pi, A = the compact operator:
              compact_fft        P = A, -pc_type fft (CgFuse and the spectral r update)
              compact_fft_star   P = the 7-point star, -pc_type fft (the same passes over a history
                                 that does not end at rounding level after one iteration)
              compact_jacobi     P = the assembled matrix, jacobi (the generic path)
  host2     2 ranks on the in-process host transport, 32x16x4: two planes per rank, the nzl < 3
            branch of the halo overlap
  host3     3 ranks, 32x16x12: four planes per rank, the overlapped branch
              both: apply (two operator applies), cg, cg_c1, cg_sr, cg_sr_c1, guess, mg
  comm      one rank with a one-rank RCCL communicator (tuning force_comm = 1), 32x24x16: the
            comm-stream boundary launches: apply, cg, cg_c1, cg_sr, guess

Of each solve the file keeps the residual history as raw float64, the (reason, its) pair, a blake2b
digest of the rank's part of the solution and every 257th value of it; of each apply the digest.
Keys are "<topology>__<case>__r<rank>__<what>". A case the library refuses is recorded as its error
code under "...__error"; the test then fails if that ever changes.

usage (on the commit to record, with a GPU): python scripts/record_cg_enqueue_unchanged.py [OUT.npz]
default OUT: tests/golden/cg_enqueue_unchanged.npz"""
import importlib.util
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import poissbox_amd as pb  # noqa: E402
from oracle import oracle as O  # noqa: E402

_spec = importlib.util.spec_from_file_location(
    "record_engine_unchanged", os.path.join(REPO, "scripts", "record_engine_unchanged.py"))
E = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(E)

SPLIT = (3, E.ITS - 3)  # iterate(3), iterate(rest)
JACOBI = ["-ksp_type", "cg", "-pc_type", "jacobi"]
SR = JACOBI + ["-ksp_cg_single_reduction"]
GUESS = ["-ksp_initial_guess_nonzero"]
MG = ["-ksp_type", "cg", "-pc_type", "mg"]

# case -> (argv, check_every, nonzero initial guess)
STAR_CASES = {
    "cg": (JACOBI, 8, False),
    "cg_c1": (JACOBI, 1, False),
    "cg_sr": (SR, 8, False),
    "cg_sr_c1": (SR, 1, False),
    "guess": (JACOBI + GUESS, 8, True),
    "guess_sr": (SR + GUESS, 8, True),
    "guess_mg": (MG + GUESS, 8, True),
    "mg": (MG, 8, False),
    "mg_unp": (MG + ["-ksp_norm_type", "unpreconditioned"], 8, False),
}
FFT = ["-ksp_type", "cg", "-pc_type", "fft"]

# topology -> (ranks, grid, force_comm, cases); "apply" and the names of STAR_CASES run on
# A = the 7-point star, P = the assembled matrix; the others are set up by operators()
TOPOLOGIES = {
    "one": (1, (32, 24, 16), 0, ["cg", "cg_c1", "cg_sr", "cg_sr_c1", "guess", "guess_sr",
                                 "guess_mg", "mg_unp", "assembled"]),
    "one64": (1, (64, 64, 64), 0, ["compact_fft", "compact_fft_star", "compact_jacobi"]),
    "host2": (2, (32, 16, 4), 0, ["apply", "cg", "cg_c1", "cg_sr", "cg_sr_c1", "guess", "mg"]),
    "host3": (3, (32, 16, 12), 0, ["apply", "cg", "cg_c1", "cg_sr", "cg_sr_c1", "guess", "mg"]),
    "comm": (1, (32, 24, 16), 1, ["apply", "cg", "cg_c1", "cg_sr", "guess"]),
}


def operators(da, case, h):
    """(A, P, argv, check_every, guess, what to destroy) of one case"""
    if case == "assembled":
        P = pb.Mat(da, pb.ASSEMBLED27, h)
        return P, P, JACOBI, 8, False, [P]
    if case.startswith("compact"):
        A = pb.Mat(da, pb.COMPACT, h)
        if case == "compact_fft":
            return A, A, FFT, 8, False, [A]
        P = pb.Mat(da, pb.STAR7 if case == "compact_fft_star" else pb.ASSEMBLED27, h)
        return A, P, FFT if case == "compact_fft_star" else JACOBI, 8, False, [A, P]
    A, P = pb.Mat(da, pb.STAR7, h), pb.Mat(da, pb.ASSEMBLED27, h)
    return (A, P) + STAR_CASES[case] + ([A, P],)


def record_rank(ctx, rank, topo, cases=None):
    """name -> array: what this rank computes on one topology (cases: a subset, default all)"""
    _, n3, _, all_cases = TOPOLOGIES[topo]
    N = int(np.prod(n3))
    compact = topo == "one64"
    L = (2 * np.pi,) * 3 if compact else (1.0,) * 3
    h = tuple(l / m for l, m in zip(L, n3))
    b = O.fill_random(N, E.SEED + N).reshape(n3[2], -1)
    x0 = O.fill_random(N, E.SEED + N + 1).reshape(n3[2], -1)
    rec = {}
    da = pb.DA(ctx, n3, L)
    (_, _, k0), (_, _, nk) = da.get_corners()
    b, x0 = b[k0:k0 + nk].reshape(-1), x0[k0:k0 + nk].reshape(-1)
    xv, bv = pb.Vec(da), pb.Vec(da)
    try:
        for case in all_cases:
            if cases is not None and case not in cases:
                continue
            pre = f"{topo}__{case}__r{rank}"
            if case == "apply":
                A = pb.Mat(da, pb.STAR7, h)
                bv.set_values(b)
                for d in (0, 1):  # consecutive applies march in alternating directions
                    A.mult(bv, xv)
                    rec[f"{pre}__digest{d}"] = E.digest(xv.get_values())
                A.destroy()
                continue
            A, P, argv, check, guess, mats = operators(da, case, h)
            bv.set_values(b)
            xv.set_values(x0 if guess else np.full(b.size, 7.25))  # (a zero guess overwrites x)
            k = None
            try:
                k = pb.KSP(A, P, pb.ksp_options(argv + E.FIXED, check_every=check))
                k.begin(bv, xv)
                for its in SPLIT:
                    k.iterate(its)
                reason, its, hist = k.end()
            except pb.PbError as e:
                rec[f"{pre}__error"] = np.array([e.code], dtype=np.int64)
                continue
            finally:
                if k is not None:
                    k.destroy()
                for m in mats:
                    m.destroy()
            x = xv.get_values()
            rec[f"{pre}__history"] = np.asarray(hist, dtype=np.float64).copy()
            rec[f"{pre}__status"] = np.array([reason, its], dtype=np.int64)
            rec[f"{pre}__digest"] = E.digest(x)
            rec[f"{pre}__sample"] = E.sample(x)
    finally:
        for o in (xv, bv):
            o.destroy()
        da.destroy()
    return rec


def record_topology(topo, cases=None, ctx=None):
    """every rank's arrays of one topology. ctx: the caller's one-rank context for "one" / "one64";
    the other topologies make their own contexts (host transport threads, force_comm)"""
    nranks, _, force_comm, _ = TOPOLOGIES[topo]
    rec = {}
    if nranks > 1:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        from test_gpu_parity import run_ranks
        for part in run_ranks(nranks, lambda c, rank: record_rank(c, rank, topo, cases)):
            rec.update(part)
        return rec
    own = ctx is None or force_comm
    if own:
        pb.tune_reset()
        pb.tune_set("force_comm", force_comm)
        ctx = pb.Context(0)
        pb.tune_set("force_comm", 0)
    try:
        return record_rank(ctx, 0, topo, cases)
    finally:
        if own:
            ctx.destroy()


def record():
    rec = {}
    for topo in TOPOLOGIES:
        rec.update(record_topology(topo))
    return rec


if __name__ == "__main__":
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden",
                                                             "cg_enqueue_unchanged.npz")
    rec = record()
    np.savez_compressed(dst, **rec)
    errors = sorted(k for k in rec if k.endswith("__error"))
    print("wrote", dst, len(rec), "arrays; refused:", errors)
