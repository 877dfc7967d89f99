"""The FGMRES cases the GPU tier runs (tests/test_gpu_fgmres.py), named, with the restatement's
arguments -- shared with scripts/fgmres_sensitivity.py, which runs the restatement of every case
under its three summation variants and records how far they differ
(profiles/ksp_fgmres/sensitivity.json): the source of each case's bars.

A case: (Problem arguments, fgmres keyword arguments, extras). extras: "nranks" (operator pieces),
"x0" (a nonzero guess: fill_random of this seed scaled by 0.01), "rhs_shift" / "zero_rhs".
"""
import functools
import json
import os

import numpy as np

from oracle import oracle as O
from fgmres_restatement import fgmres
from ksp_types_restatement import Problem
from parity_bars import HIST_RTOL, HIST_RTOL_PC, X_RTOL

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SENSITIVITY = os.path.join(REPO, "profiles", "ksp_fgmres", "sensitivity.json")
FIXED_KW = dict(rtol=0.0, atol=0.0, dtol=1e300)

PATHS = {
    "jacobi": dict(n3=(16, 16, 12)),
    "none": dict(n3=(16, 16, 12), pc="none"),
    "jacobi_deltas": dict(n3=(32, 40, 48), deltas=(0.05, 0.03, 0.07)),
    "sor": dict(n3=(16, 16, 12), pc="sor"),
    "mg": dict(n3=(16, 16, 12), pc="mg"),
    "fft": dict(n3=(32, 40, 48), pc="fft"),
    "compact_fft": dict(n3=(32, 32, 32), pc="fft", op="compact"),
    "assembled_jacobi": dict(n3=(16, 16, 12), op="assembled"),
}
SHAPES = [((24, 20, 12), None), ((17, 18, 9), None), ((130, 6, 33), None), ((16, 16, 16), None),
          ((1024, 1024, 4), None), ((24, 20, 12), (0.05, 0.03, 0.07))]


def shape_id(n3, deltas):
    return "shape-" + "x".join(map(str, n3)) + ("-deltas" if deltas else "")


def _cases():
    c = {}
    for name, pk in PATHS.items():
        for m in range(1, 8):
            c[f"fixed-{name}-{m}"] = (pk, dict(restart=3, max_it=m, **FIXED_KW), {})
    for n3, deltas in SHAPES:
        c[shape_id(n3, deltas)] = (dict(n3=n3, deltas=deltas),
                                   dict(restart=4, max_it=7, **FIXED_KW), {})
        c[shape_id(n3, deltas) + "-none"] = (dict(n3=n3, deltas=deltas, pc="none"),
                                             dict(restart=4, max_it=7, **FIXED_KW), {})
    c["tol-jacobi-r30"] = (dict(n3=(32, 32, 32)), dict(restart=30, rtol=1e-8), {})
    c["tol-jacobi-r5"] = (dict(n3=(32, 32, 32)), dict(restart=5, rtol=1e-8), {})
    c["tol-mg"] = (dict(n3=(32, 32, 32), pc="mg"), dict(restart=30, rtol=1e-10), {})
    c["tol-fft"] = (dict(n3=(32, 40, 48), pc="fft"), dict(restart=30, rtol=1e-8), {})
    c["refine-jacobi"] = (dict(n3=(32, 32, 32)), dict(restart=30, rtol=1e-8, refine=True), {})
    c["guess-jacobi"] = (dict(n3=(16, 16, 12)), dict(restart=5, rtol=1e-6), {"x0": 77})
    c["guess-jacobi-initial"] = (dict(n3=(16, 16, 12)),
                                 dict(restart=5, rtol=1e-6, mode="initial"), {"x0": 77})
    c["zero-rhs"] = (dict(n3=(16, 16, 12)), dict(restart=5), {"zero_rhs": True})
    c["none-jacobi"] = (dict(n3=(16, 16, 12)),
                        dict(restart=3, max_it=7, norm_none=True, **FIXED_KW), {})
    c["ahead-mg"] = (dict(n3=(32, 32, 32), pc="mg"), dict(restart=30, rtol=1e-12), {})
    c["ranks2-jacobi"] = (dict(n3=(16, 16, 12)), dict(restart=3, max_it=7, **FIXED_KW),
                          {"nranks": 2})
    c["ranks2-mg"] = (dict(n3=(16, 16, 12), pc="mg"), dict(restart=3, max_it=7, **FIXED_KW),
                      {"nranks": 2})
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
    return fgmres(prob, b, x0=x0, nranks=ex.get("nranks", 1), sums=sums, **kw)


def hist_diff(prob, h, ho):
    """The largest history difference, relative entry by entry -- with the spectral PC one step
    takes the estimate from ||r_0|| to its rounding noise (1e-15 ||r_0||), where a relative
    comparison measures nothing: there the later entries are held relative to ||r_0||, as
    test_gpu_ksp_types.check holds them."""
    h, ho = np.asarray(h, dtype=float), np.asarray(ho, dtype=float)
    assert h.shape == ho.shape, (h.shape, ho.shape)
    if not ho.size or ho[0] == 0.0:
        return float(np.max(np.abs(h - ho), initial=0.0))
    den = np.full_like(ho, ho[0]) if prob.pc == "fft" else np.where(ho > 0, ho, ho[0])
    den[0] = ho[0]
    return float(np.max(np.abs(h - ho) / den))


def x_diff(x, xo):
    s = float(np.max(np.abs(xo)))
    return float(np.max(np.abs(x - xo))) / (s if s > 0 else 1.0)


def true_residual(prob, b, x, nranks=1):
    nb = float(np.linalg.norm(b))
    return float(np.linalg.norm(b - prob.apply(x, nranks))) / (nb if nb > 0 else 1.0)


@functools.lru_cache(maxsize=None)
def _recorded():
    with open(SENSITIVITY) as f:
        return json.load(f)["cases"]


def bars(cid):
    """(history bar, x bar, residual factor) of a case: 100 x the recorded spread between the
    restatement's summation variants (the two orders of margin parity_bars.py states), never
    below the CG bars; the factor by which the restatement's own true residual exceeds its last
    estimate (at least 1), times 10."""
    rec = _recorded()[cid]
    prob = setup(cid)[0]
    floor = HIST_RTOL_PC if prob.pc in ("sor", "mg") else HIST_RTOL
    if prob.pc == "fft":
        floor = 1e-10  # (of ||r_0||: test_gpu_ksp_types.check's bar for the spectral PC)
    return (max(100.0 * rec["d_hist"], floor), max(100.0 * rec["d_x"], X_RTOL),
            10.0 * max(rec["resid_factor"], 1.0))
