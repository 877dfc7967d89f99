"""CPU tier of -ksp_norm_type: the option's parser (pure host code of the
library), the enum, and the properties of the numpy restatement the GPU tests compare against
(tests/norm_type_restatement.py), tied to the pinned oracle through the preconditioned norm.

The parser tests fail without the feature (pb_ksp_norm_type_parse does not exist)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import poissbox_amd as pb
from poissbox_amd import _lib as L
from oracle import oracle as O
import chebyshev_restatement as CR
import ksp_types_restatement as KR
import norm_type_restatement as NR
from norm_type_restatement import Problem

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNSUPPORTED = 5
FIXED = dict(rtol=0.0, atol=0.0, dtol=1e300)


def parse(argv, start=-1):
    t = C.c_int(start)
    arr = (C.c_char_p * max(len(argv), 1))(*[a.encode() for a in argv])
    L.call("pb_ksp_norm_type_parse", C.byref(t), len(argv), arr)
    return t.value


# ---------------------------------------------------------------------------------------------
# the parser and the enum
# ---------------------------------------------------------------------------------------------
def test_enum_values_are_petscs():
    assert (pb.KSP_NORM_DEFAULT, pb.KSP_NORM_NONE, pb.KSP_NORM_PRECONDITIONED,
            pb.KSP_NORM_UNPRECONDITIONED, pb.KSP_NORM_NATURAL) == (-1, 0, 1, 2, 3)
    header = open(os.path.join(REPO, "include", "poissbox_gpu.h")).read()
    body = re.search(r"enum pb_ksp_norm_type \{(.*?)\};", header, re.S).group(1)
    got = {k: int(v) for k, v in re.findall(r"(PB_KSP_NORM_\w+) = (-?\d+)", body)}
    assert got == {"PB_KSP_NORM_DEFAULT": -1, "PB_KSP_NORM_NONE": 0,
                   "PB_KSP_NORM_PRECONDITIONED": 1, "PB_KSP_NORM_UNPRECONDITIONED": 2,
                   "PB_KSP_NORM_NATURAL": 3}
    assert NR.NORM_CODES == {k[len("PB_KSP_NORM_"):].lower(): v for k, v in got.items()}


@pytest.mark.parametrize("word,value", sorted(NR.NORM_CODES.items()))
def test_parse_every_word(word, value):
    assert parse(["-ksp_type", "cg", "-ksp_norm_type", word, "-pc_type", "mg"], start=7) == value


def test_parse_last_occurrence_wins():
    assert parse(["-ksp_norm_type", "none", "-ksp_rtol", "1e-8", "-ksp_norm_type", "natural"]) == 3
    assert parse(["-ksp_norm_type", "natural", "-ksp_norm_type", "default"], start=2) == -1


def test_parse_absent_or_trailing_option_leaves_the_value():
    assert parse([], start=2) == 2
    assert parse(["-ksp_type", "cg"], start=3) == 3
    assert parse(["-ksp_norm_type"], start=1) == 1
    assert parse(["-ksp_norm_type", "unpreconditioned", "-ksp_norm_type"], start=1) == 2


@pytest.mark.parametrize("argv", [["-ksp_norm_type", "frobenius"],
                                  ["-ksp_norm_type", "natural", "-ksp_norm_type", "2"],
                                  ["-ksp_norm_type", "-ksp_rtol", "1e-8"]])
def test_parse_unknown_word(argv):
    t = C.c_int(2)
    arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
    with pytest.raises(pb.PbError) as e:
        L.call("pb_ksp_norm_type_parse", C.byref(t), len(argv), arr)
    assert e.value.code == UNSUPPORTED and "norm_type" in str(e.value)
    assert t.value == 2  # untouched, also when an earlier occurrence was valid


def test_ksp_opts_parse_still_skips_the_option():
    """The option struct and its parser are as they were: the option is unknown to them."""
    base = pb.ksp_options(["-ksp_rtol", "1e-7", "-pc_type", "mg"])
    for word in ("unpreconditioned", "frobenius"):
        o = L.KspOpts()
        L.call("pb_ksp_opts_default", C.byref(o))
        argv = ["-ksp_norm_type", word, "-ksp_rtol", "1e-7", "-pc_type", "mg"]
        arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
        L.call("pb_ksp_opts_parse", C.byref(o), len(argv), arr)
        assert bytes(o) == bytes(base)[:C.sizeof(L.KspOpts)]
    assert L.KspOpts._fields_[-1][0] == "richardson_scale"


def test_ksp_options_carries_the_type():
    assert pb.ksp_options().norm_type == pb.KSP_NORM_DEFAULT
    assert pb.ksp_options(["-ksp_norm_type", "natural"]).norm_type == pb.KSP_NORM_NATURAL
    assert pb.ksp_options(norm_type=pb.KSP_NORM_NONE).norm_type == pb.KSP_NORM_NONE
    with pytest.raises(pb.PbError):
        pb.ksp_options(["-ksp_norm_type", "frobenius"])


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(pc="jacobi", n3=(16, 16, 12)):
    prob = Problem(n3, pc=pc)
    return prob, prob.rhs()


def test_preconditioned_cg_is_the_oracles():
    """16 x 16 x 12, Jacobi: the oracle's own history to 1e-14 relative, x to the bit of its
    iteration count -- the tie to what is already pinned."""
    prob, b = case()
    xo, ro, itso, ho = O.cg_solve(b, prob.n3, prob.h, rtol=1e-8)
    x, reason, its, hist, rn0 = NR.cg(prob, b, rtol=1e-8)
    assert (reason, its, len(hist)) == (ro, itso, len(ho))
    rel = float(np.max(np.abs(hist - ho) / ho))
    print(f"restated against oracle history: {rel:.3e}")
    assert rel <= 1e-14 and rn0 == hist[0]
    assert np.max(np.abs(x - xo)) <= 1e-13 * np.max(np.abs(xo))


def test_preconditioned_single_reduction_cg_is_the_oracles():
    prob, b = case()
    xo, ro, itso, ho = O.cg_solve(b, prob.n3, prob.h, rtol=1e-8, single_reduction=2)
    x, reason, its, hist, _ = NR.cg(prob, b, rtol=1e-8, single_reduction=True)
    assert (reason, its, len(hist)) == (ro, itso, len(ho))
    assert float(np.max(np.abs(hist - ho) / ho)) <= 1e-14


def test_wrapped_stationary_solvers_delegate():
    prob, b = case()
    a = NR.richardson(prob, b, scale=2.0 / 3.0, max_it=5, **FIXED)
    w = KR.richardson(prob, b, scale=2.0 / 3.0, max_it=5, **FIXED)
    assert a[1:3] == w[1:3] and np.array_equal(a[3], w[3]) and np.array_equal(a[0], w[0])
    lo, hi = CR.jacobi_spectrum(prob)
    a = NR.chebyshev(prob, b, lo, hi, max_it=5, **FIXED)
    w = CR.chebyshev(prob, b, lo, hi, max_it=5, **FIXED)
    assert a[1:3] == w[1:3] and np.array_equal(a[3], w[3]) and np.array_equal(a[0], w[0])
    # and the frame the other types run in is that restatement's: same iterates under `none`
    n = NR.chebyshev(prob, b, lo, hi, norm_type="none", max_it=5, **FIXED)
    assert np.array_equal(n[0], w[0]) and n[1:3] == (4, 5)


@pytest.mark.parametrize("pc,sr", [("jacobi", False), ("jacobi", True), ("mg", False)])
def test_same_iterates_under_every_type(pc, sr):
    """alpha, beta, p, x, r do not depend on the norm type: while no test fires, x after the same
    number of iterations is identical. (Single reduction runs with Jacobi / no PC.)"""
    prob, b = case(pc)
    runs = {t: NR.cg(prob, b, norm_type=t, single_reduction=sr, max_it=5, **FIXED)
            for t in NR.NORM_TYPES}
    for t, (x, reason, its, hist, rn0) in runs.items():
        assert np.array_equal(x, runs["preconditioned"][0]), t
        assert (reason, its, len(hist)) == ((4 if t == "none" else -3), 5, 6), t


@pytest.mark.parametrize("pc", ["jacobi", "mg", "fft"])
def test_unpreconditioned_history_is_the_true_residual(pc):
    prob, b = case(pc, (16, 16, 12) if pc != "fft" else (16, 20, 12))
    for k in (1, 2, 3):
        x, _, its, hist, rn0 = NR.cg(prob, b, norm_type="unpreconditioned", max_it=k, **FIXED)
        true = float(np.linalg.norm(b - prob.apply(x)))
        # (r is updated by recurrence: equal to rounding, far inside 1e-10 after k <= 3 steps)
        assert abs(hist[its] - true) <= 1e-10 * hist[0], (pc, k, hist[its], true)
        assert rn0 == hist[0] and abs(hist[0] - np.linalg.norm(b)) <= 1e-14 * hist[0]
    # richardson recomputes r: the logged norm is ||b - A x_i|| of the iterate itself
    xs = NR.richardson(prob, b, scale=0.5, norm_type="unpreconditioned", max_it=3, **FIXED)
    assert abs(xs[3][-1] - np.linalg.norm(b - prob.apply(xs[0]))) <= 1e-13 * xs[3][0]


def test_natural_history_squared_is_r_dot_z():
    prob, b = case("mg")
    x, _, its, hist, _ = NR.cg(prob, b, norm_type="natural", max_it=4, **FIXED)
    r = b - prob.apply(x)
    z = prob.remove(prob.pc_apply(r))
    assert abs(hist[-1] ** 2 - abs(float(np.sum(r * z)))) <= 1e-9 * hist[0] ** 2
    # an SPD pair: the energy norm of the error sits between the other two norms' scales
    assert np.all(np.diff(hist) < 0)  # CG minimises it: monotone


@pytest.mark.parametrize("solver", ["cg", "sr", "richardson", "chebyshev"])
@pytest.mark.parametrize("max_it", [0, 1, 4])
def test_none_runs_max_it_and_logs_zeros(solver, max_it):
    prob, b = case()
    lo, hi = CR.jacobi_spectrum(prob)
    run = {"cg": lambda: NR.cg(prob, b, norm_type="none", max_it=max_it),
           "sr": lambda: NR.cg(prob, b, norm_type="none", single_reduction=True, max_it=max_it),
           "richardson": lambda: NR.richardson(prob, b, scale=0.5, norm_type="none", max_it=max_it),
           "chebyshev": lambda: NR.chebyshev(prob, b, lo, hi, norm_type="none", max_it=max_it)}
    x, reason, its, hist, rn0 = run[solver]()
    assert (reason, its, rn0) == (4, max_it, 0.0)
    assert len(hist) == max_it + 1 and np.all(hist == 0.0)
    if max_it == 0:
        assert np.all(x == 0.0)


def test_none_keeps_the_nan_check_of_cgs_dots():
    prob, b = case()
    b = b.copy()
    b[37] = np.nan
    assert NR.cg(prob, b, norm_type="none", max_it=5)[1:3] == (-9, 0)


@pytest.mark.parametrize("norm_type", ["preconditioned", "unpreconditioned", "natural"])
@pytest.mark.parametrize("mode", ["default", "initial", "min"])
def test_nonzero_guess_reference(norm_type, mode):
    prob, b = case("mg")
    x0 = 1e-3 * O.fill_random(prob.N, 7)
    _, _, _, hist, rn0 = NR.cg(prob, b, x0=x0, norm_type=norm_type, mode=mode, max_it=2, **FIXED)
    zb = prob.remove(prob.pc_apply(b))
    nb = {"preconditioned": np.linalg.norm(zb), "unpreconditioned": np.linalg.norm(b),
          "natural": np.sqrt(abs(np.sum(b * zb)))}[norm_type]
    want = {"default": nb, "initial": hist[0], "min": min(nb, hist[0])}[mode]
    assert abs(rn0 - want) <= 1e-13 * want


def test_unpreconditioned_tolerance_is_independent_of_the_pc():
    """What the option is for: rtol on ||r|| / ||b|| ends every PC's solve at a true residual
    below rtol ||b||, which the preconditioned norm does not promise."""
    for pc in ("jacobi", "mg"):
        prob, b = case(pc, (16, 16, 16))
        x, reason, its, hist, rn0 = NR.cg(prob, b, norm_type="unpreconditioned", rtol=1e-8)
        assert reason == 2 and abs(rn0 - np.linalg.norm(b)) <= 1e-14 * rn0
        assert np.linalg.norm(b - prob.apply(x)) <= 1e-8 * np.linalg.norm(b) * (1 + 1e-6)
