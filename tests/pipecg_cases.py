"""The pipelined-CG cases the GPU tier runs (tests/test_gpu_pipecg.py), named, with the
restatement's arguments -- shared with scripts/pipecg_sensitivity.py, which runs the restatement of
every case under its three summation variants and records how far they differ
(profiles/ksp_pipecg/sensitivity.json): the source of each case's bars. The method, the paths and
the shapes are tests/fgmres_cases.py's.

A case: (Problem arguments, pipecg keyword arguments, extras). extras: "nranks" (operator pieces),
"x0" (a nonzero guess: fill_random of this seed scaled by 0.01), "zero_rhs".
"""
import functools
import json
import os

import numpy as np

from oracle import oracle as O
from fgmres_cases import FIXED_KW, PATHS, SHAPES, hist_diff, shape_id, true_residual, x_diff  # noqa: F401
from ksp_types_restatement import Problem
from parity_bars import HIST_RTOL, HIST_RTOL_PC, X_RTOL
from pipecg_restatement import pipecg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENSITIVITY = os.path.join(REPO, "profiles", "ksp_pipecg", "sensitivity.json")
NORMS = ("unpreconditioned", "natural", "none")


def _cases():
    c = {}
    for name, pk in PATHS.items():
        for m in range(1, 7):
            c[f"fixed-{name}-{m}"] = (pk, dict(max_it=m, **FIXED_KW), {})
    for n3, deltas in SHAPES:
        c[shape_id(n3, deltas)] = (dict(n3=n3, deltas=deltas), dict(max_it=7, **FIXED_KW), {})
        c[shape_id(n3, deltas) + "-none"] = (dict(n3=n3, deltas=deltas, pc="none"),
                                             dict(max_it=7, **FIXED_KW), {})
    c["tol-jacobi"] = (dict(n3=(32, 32, 32)), dict(rtol=1e-8), {})
    c["tol-mg"] = (dict(n3=(32, 32, 32), pc="mg"), dict(rtol=1e-10), {})
    c["tol-fft"] = (dict(n3=(32, 40, 48), pc="fft"), dict(rtol=1e-8), {})
    for nt in NORMS:
        for pc in ("jacobi", "mg"):
            c[f"norm-{nt}-{pc}"] = (dict(n3=(16, 16, 12), pc=pc),
                                    dict(max_it=6, norm=nt, **FIXED_KW), {})
    c["norm-unpreconditioned-tol"] = (dict(n3=(16, 16, 12)),
                                      dict(rtol=1e-6, norm="unpreconditioned"), {})
    c["guess-jacobi"] = (dict(n3=(16, 16, 12)), dict(rtol=1e-6), {"x0": 77})
    c["guess-jacobi-initial"] = (dict(n3=(16, 16, 12)), dict(rtol=1e-6, mode="initial"),
                                 {"x0": 77})
    c["zero-rhs"] = (dict(n3=(16, 16, 12)), dict(), {"zero_rhs": True})
    c["ranks2-jacobi"] = (dict(n3=(16, 16, 12)), dict(max_it=7, **FIXED_KW), {"nranks": 2})
    c["ranks2-mg"] = (dict(n3=(16, 16, 12), pc="mg"), dict(max_it=7, **FIXED_KW), {"nranks": 2})
    return c


CASES = _cases()


@functools.lru_cache(maxsize=None)
def setup(cid):
    """(problem, b, x0 or None) of a case: computed once."""
    pk, _, ex = CASES[cid]
    prob = Problem(**pk)
    nranks = ex.get("nranks", 1)
    b = np.zeros(prob.N) if ex.get("zero_rhs") else prob.rhs(nranks=nranks)
    x0 = 0.01 * O.fill_random(prob.N, ex["x0"]) if "x0" in ex else None
    return prob, b, x0


@functools.lru_cache(maxsize=None)
def restated(cid, sums="pairwise"):
    """(x, reason, its, history, rnorm0) of the restatement: computed once, left unchanged."""
    prob, b, x0 = setup(cid)
    _, kw, ex = CASES[cid]
    return pipecg(prob, b, x0=x0, nranks=ex.get("nranks", 1), sums=sums, **kw)


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(SENSITIVITY) as f:
        return json.load(f)["cases"]


def bars(cid):
    """(history bar, x bar) of a case: 100 x the recorded spread between the restatement's
    summation variants (the two orders of margin parity_bars.py states), never below the CG bars
    (with the spectral PC: 1e-10 of the first entry, test_gpu_ksp_types.check's bar)."""
    rec = _recorded()[cid]
    prob = setup(cid)[0]
    floor = HIST_RTOL_PC if prob.pc in ("sor", "mg") else HIST_RTOL
    if prob.pc == "fft":
        floor = 1e-10
    return max(100.0 * rec["d_hist"], floor), max(100.0 * rec["d_x"], X_RTOL)


def stop_margin_ok(cid):
    """Where the stopping iteration is asserted: the restatement's last two norms lie further
    from ttol (relative) than the case's own history bar, so sums within the bar cannot move it."""
    _, kw, _ = CASES[cid]
    _, _, _, hist, rn0 = restated(cid)
    ttol = max(kw.get("rtol", 1e-5) * rn0, kw.get("atol", 1e-50))
    hbar = bars(cid)[0]
    fft = setup(cid)[0].pc == "fft"  # (entries held relative to the first: hist_diff)
    return all(abs(v - ttol) > hbar * (hist[0] if fft else max(v, ttol)) for v in hist[-2:])
