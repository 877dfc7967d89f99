"""Record what the multigrid host path computes and launches, bit for bit, on the smallest shapes
at which each of its dispatch branches is taken, so that a change to the V-cycle's host code (which
passes a level takes, in what order, with which ghost planes) can be checked against the commit
this ran on (tests/test_gpu_mg_vcycle_unchanged.py compares a fresh run with the file by
np.array_equal).

Every case runs one pc_apply of a random vector and one CG solve as begin, iterate(3), iterate(7),
end, with record_engine_unchanged.py's options (10 iterations, rtol 0, divtol 1e300), its digest
and its samples. Timing is on and reset before the case, and the launch count of every multigrid
phase (PHASES) over the case is kept: a pass that moved to another kernel, or ran once more, shows
there even where the bits agree.

Topologies (TOPOLOGIES) and their cases (<what>_<selector>; the selectors are the entries of
MG_KERNELS in tests/test_gpu_parity.py):
  one128    one rank, 128x40x16: level 0 takes the fused restriction and post-sweep under
            "engine", level 1 is too narrow for them
  one32     one rank, 32x24x16: the pair kernels and the LDS tail
              both: mg_default, mg_engine, mg_legacy, mg_unfused, mg_bigtail (the tail in global
                    memory), sor_default, sor_engine (one level: the sums taken in the coarse
                    solve), l2c3_engine (-pc_mg_levels 2 -pc_mg_coarse_its 3)
              one128 also: the level smoothers rich (richardson + jacobi, 2 sweeps, scale 6/7),
                    cheb (chebyshev + jacobi, 3 sweeps) and rsor (richardson + sor, 2 sweeps), each
                    as <smoother>_e<0|1>_f<0|1>: mg_engine_min_plane 10^9 | 0, mg_poly_fused 0 | 1
  host2     2 ranks on the in-process host transport, 128x16x32: 16 planes per rank
  host3     3 ranks, 128x8x12: 4 planes per rank
              both: mg_default, mg_splitfused, mg_noagg, mg_nosplitfused (the only path to the
                    fused pre-smoothing + residual pass and the prolongation into the residual
                    scratch followed by the two-colour sweep), cheb2_default (chebyshev + jacobi,
                    2 sweeps)
  comm      one rank with a one-rank RCCL communicator (tuning force_comm = 1), 128x16x32:
            mg_default, mg_splitfused

Keys are "<topology>__<case>__r<rank>__<what>", <what> one of apply_digest, history, status, digest,
sample, launches (in the order of PHASES; the level-smoother cases leave out the driver's four
phase timers, which that path may or may not record). A case the library refuses is recorded as
its error code under "...__error"; the test then fails if that ever changes.

usage (on the commit to record, with a GPU): python scripts/record_mg_vcycle_unchanged.py [OUT.npz]
default OUT: tests/golden/mg_vcycle_unchanged.npz"""
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
DRIVER_PHASES = ["mg_fine_smooth_first", "mg_fine_resid_restrict", "mg_fine_prolong_post",
                 "mg_coarse_levels"]
PHASES = ["mg_apply", "mg_sor", "mg_residual", "mg_poly", "mg_sor_sweep2", "mg_post_sweep",
          "mg_presmooth_restrict", "mg_presmooth_residual"] + DRIVER_PHASES
CG = ["-ksp_type", "cg"]
PCS = {"mg": CG + ["-pc_type", "mg"], "sor": CG + ["-pc_type", "sor"],
       "l2c3": CG + ["-pc_type", "mg", "-pc_mg_levels", "2", "-pc_mg_coarse_its", "3"]}
SMOOTHERS = {"rich": E.levels("richardson", "jacobi", 2, 6.0 / 7.0),
             "cheb": E.levels("chebyshev", "jacobi", 3),
             "rsor": E.levels("richardson", "sor", 2),
             "cheb2": E.levels("chebyshev", "jacobi", 2)}


def parity():
    """tests/test_gpu_parity.py: MG_KERNELS and run_ranks"""
    tests = os.path.join(REPO, "tests")
    if tests not in sys.path:
        sys.path.insert(0, tests)
    import test_gpu_parity
    return test_gpu_parity


def selector(sel):
    """MG_KERNELS[sel] with the tunings' own names"""
    return {k[3:].lower(): int(v) for k, v in parity().MG_KERNELS[sel].items()}


def case_of(name):
    """(argv, tuning, level smoother?) of a case name"""
    what, rest = name.split("_", 1)
    if what in PCS:
        return PCS[what], selector(rest), False
    tuning = selector(rest) if rest in parity().MG_KERNELS else {
        "mg_engine_min_plane": 0 if "e1" in rest else 10 ** 9,
        "mg_poly_fused": int("f1" in rest)}
    return PCS["mg"] + SMOOTHERS[what], tuning, True


DEFAULT_CASES = [f"mg_{s}" for s in ("default", "engine", "legacy", "unfused", "bigtail")] + [
    "sor_default", "sor_engine", "l2c3_engine"]
SMOOTHER_CASES = [f"{s}_e{e}_f{f}" for s in ("rich", "cheb", "rsor") for e in (1, 0)
                  for f in (1, 0)]
SPLIT_CASES = [f"mg_{s}" for s in ("default", "splitfused", "noagg", "nosplitfused")] + [
    "cheb2_default"]

# topology -> (ranks, grid, force_comm, cases)
TOPOLOGIES = {
    "one128": (1, (128, 40, 16), 0, DEFAULT_CASES + SMOOTHER_CASES),
    "one32": (1, (32, 24, 16), 0, DEFAULT_CASES),
    "host2": (2, (128, 16, 32), 0, SPLIT_CASES),
    "host3": (3, (128, 8, 12), 0, SPLIT_CASES),
    "comm": (1, (128, 16, 32), 1, ["mg_default", "mg_splitfused"]),
}


# the arrays a case that ran leaves per rank
WHAT = ["apply_digest", "digest", "history", "launches", "sample", "status"]


def record_case(ctx, rank, topo, case):
    """name -> array: what this rank computes in one case (the tunings are the caller's)"""
    _, n3, _, _ = TOPOLOGIES[topo]
    argv, _, custom = case_of(case)
    N = int(np.prod(n3))
    h = tuple(1.0 / m for m in n3)
    b = O.fill_random(N, E.SEED + N).reshape(n3[2], -1)
    r = O.fill_random(N, E.SEED + N + 1).reshape(n3[2], -1)
    pre = f"{topo}__{case}__r{rank}"
    rec = {}
    da = pb.DA(ctx, n3)
    (_, _, k0), (_, _, nk) = da.get_corners()
    b, r = b[k0:k0 + nk].reshape(-1), r[k0:k0 + nk].reshape(-1)
    A, P = pb.Mat(da, pb.STAR7, h), pb.Mat(da, pb.ASSEMBLED27, h)
    xv, bv = pb.Vec(da), pb.Vec(da)
    k = None
    ctx.sync()
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        k = pb.KSP(A, P, pb.ksp_options(argv + E.FIXED))
        bv.set_values(r)
        k.pc_apply(bv, xv)
        rec[f"{pre}__apply_digest"] = E.digest(xv.get_values())
        bv.set_values(b)
        xv.set_values(np.full(b.size, 7.25))  # (a zero guess overwrites x)
        k.begin(bv, xv)
        for its in SPLIT:
            k.iterate(its)
        reason, its, hist = k.end()
        ctx.sync()
        x = xv.get_values()
        rec[f"{pre}__history"] = np.asarray(hist, dtype=np.float64).copy()
        rec[f"{pre}__status"] = np.array([reason, its], dtype=np.int64)
        rec[f"{pre}__digest"] = E.digest(x)
        rec[f"{pre}__sample"] = E.sample(x)
        phases = PHASES[:-len(DRIVER_PHASES)] if custom else PHASES
        rec[f"{pre}__launches"] = np.array([ctx.timing(p)[1] for p in phases], dtype=np.int64)
    except pb.PbError as e:
        rec = {f"{pre}__error": np.array([e.code], dtype=np.int64)}
    finally:
        ctx.set_timing(False)
        for o in (k, A, P, xv, bv):
            if o is not None:
                o.destroy()
        da.destroy()
    return rec


def record_topology(topo, cases=None, ctx=None):
    """every rank's arrays of one topology (cases: a subset, default all). ctx: the caller's
    one-rank context for "one128" / "one32"; the other topologies make their own contexts (host
    transport threads, force_comm). The tunings are process-wide, so on several ranks every case
    is a run_ranks of its own, set up before the threads start"""
    nranks, _, force_comm, all_cases = TOPOLOGIES[topo]
    rec = {}
    own = nranks == 1 and (ctx is None or force_comm)
    if own:
        pb.tune_reset()
        pb.tune_set("force_comm", force_comm)
        ctx = pb.Context(0)
    try:
        for case in all_cases:
            if cases is not None and case not in cases:
                continue
            pb.tune_reset()
            for name, v in case_of(case)[1].items():
                pb.tune_set(name, v)
            if nranks > 1:
                def body(c, rank, case=case):
                    return record_case(c, rank, topo, case)
                for part in parity().run_ranks(nranks, body):
                    rec.update(part)
            else:
                rec.update(record_case(ctx, 0, topo, case))
    finally:
        pb.tune_reset()
        if own:
            ctx.destroy()
    return rec


def record():
    rec = {}
    for topo in TOPOLOGIES:
        rec.update(record_topology(topo))
    return rec


if __name__ == "__main__":
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden",
                                                             "mg_vcycle_unchanged.npz")
    rec = record()
    np.savez_compressed(dst, **rec)
    errors = sorted(k for k in rec if k.endswith("__error"))
    print("wrote", dst, len(rec), "arrays; refused:", errors)
