"""CPU tier of -ksp_type fgmres: the option parser and setter rules that need no GPU
(pb_ksp_fgmres_opts_parse, the name table), and the numpy restatement itself
(tests/fgmres_restatement.py) against a dense least-squares solve of the projected system."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import poissbox_amd as pb
from poissbox_amd import _lib as L
import fgmres_cases as F
from fgmres_restatement import fgmres
from ksp_types_restatement import Problem

ARG, UNSUPPORTED = 1, 5


def parse(argv, start=None):
    o = L.KspFgmresOpts()
    L.call("pb_ksp_fgmres_opts_default", C.byref(o))
    if start:
        o.restart, o.haptol, o.cgs_refinement = start
    arr = (C.c_char_p * max(len(argv), 1))(*[a.encode() for a in argv])
    L.call("pb_ksp_fgmres_opts_parse", C.byref(o), len(argv), arr)
    return o.restart, o.haptol, o.cgs_refinement


def test_defaults_and_type_name():
    assert parse([]) == (30, 1e-30, pb.FGMRES_REFINE_NEVER)
    o = pb.ksp_options(["-ksp_type", "fgmres"])
    assert o.ksp_type == pb.KSP_FGMRES == 4
    assert (o.fgmres_restart, o.fgmres_haptol, o.fgmres_cgs_refinement) == (30, 1e-30, 0)
    # the new reasons are PETSc's values
    assert pb.REASONS[-5] == "DIVERGED_BREAKDOWN" and pb.REASONS[7] == "CONVERGED_HAPPY_BREAKDOWN"


def test_options_accepted():
    assert parse(["-ksp_gmres_restart", "5"])[0] == 5
    assert parse(["-ksp_gmres_restart", "1"])[0] == 1
    assert parse(["-ksp_gmres_restart", "64"])[0] == 64
    assert parse(["-ksp_gmres_haptol", "1e-20"])[1] == 1e-20
    assert parse(["-ksp_gmres_cgs_refinement_type", "refine_always"])[2] == pb.FGMRES_REFINE_ALWAYS
    assert parse(["-ksp_gmres_cgs_refinement_type", "refine_never"], (7, 1e-9, 2)) == (7, 1e-9, 0)
    # flags: no effect, with or without a value; the options after them are still read
    for flag in ("-ksp_gmres_classicalgramschmidt", "-ksp_gmres_preallocate"):
        assert parse([flag, "-ksp_gmres_restart", "9"])[0] == 9
        assert parse([flag, "true", "-ksp_gmres_restart", "9"])[0] == 9
        assert parse(["-ksp_gmres_restart", "9", flag])[0] == 9
    assert parse(["-ksp_gmres_modifiedgramschmidt", "false", "-ksp_gmres_restart", "4"])[0] == 4
    # through ksp_options, beside the options of the other structs
    o = pb.ksp_options(["-ksp_type", "fgmres", "-ksp_gmres_restart", "5", "-pc_type", "mg",
                        "-ksp_rtol", "1e-9", "-ksp_gmres_haptol", "1e-25"])
    assert (o.fgmres_restart, o.fgmres_haptol, o.pc_type, o.rtol) == (5, 1e-25, pb.PC_MG, 1e-9)
    # pb_ksp_opts_parse itself skips them (its struct and parser are pinned)
    k = L.KspOpts()
    L.call("pb_ksp_opts_default", C.byref(k))
    argv = ["-ksp_gmres_restart", "0", "-ksp_gmres_modifiedgramschmidt", "-ksp_max_it", "3"]
    L.call("pb_ksp_opts_parse", C.byref(k), len(argv), (C.c_char_p * 5)(*[a.encode() for a in argv]))
    assert k.max_it == 3


def test_unknown_and_valueless_options_are_skipped():
    assert parse(["-foo", "-ksp_gmres_nothing", "3", "-ksp_rtol", "1e-3"]) == (30, 1e-30, 0)
    for opt in ("-ksp_gmres_restart", "-ksp_gmres_haptol", "-ksp_gmres_cgs_refinement_type"):
        assert parse(["-ksp_gmres_restart", "8", opt]) == (8, 1e-30, 0)


@pytest.mark.parametrize("argv,code", [
    (["-ksp_gmres_restart", "0"], ARG),
    (["-ksp_gmres_restart", "65"], ARG),
    (["-ksp_gmres_restart", "-3"], ARG),
    (["-ksp_gmres_restart", "abc"], ARG),
    (["-ksp_gmres_haptol", "0"], ARG),
    (["-ksp_gmres_haptol", "-1e-30"], ARG),
    (["-ksp_gmres_haptol", "inf"], ARG),
    (["-ksp_gmres_haptol", "nan"], ARG),
    (["-ksp_gmres_haptol", "x"], ARG),
    (["-ksp_gmres_modifiedgramschmidt"], UNSUPPORTED),
    (["-ksp_gmres_modifiedgramschmidt", "true"], UNSUPPORTED),
    (["-ksp_gmres_cgs_refinement_type", "refine_ifneeded"], UNSUPPORTED),
    (["-ksp_gmres_cgs_refinement_type", "sometimes"], UNSUPPORTED),
])
def test_options_rejected_and_struct_untouched(argv, code):
    o = L.KspFgmresOpts(11, 1e-12, 2)
    full = ["-ksp_gmres_restart", "13"] + argv  # a valid option first: it must not be committed
    arr = (C.c_char_p * len(full))(*[a.encode() for a in full])
    with pytest.raises(pb.PbError) as e:
        L.call("pb_ksp_fgmres_opts_parse", C.byref(o), len(full), arr)
    assert e.value.code == code, argv
    assert (o.restart, o.haptol, o.cgs_refinement) == (11, 1e-12, 2)
    with pytest.raises(pb.PbError) as e:
        pb.ksp_options(["-ksp_type", "fgmres"] + argv)
    assert e.value.code == code


def test_gmres_stays_unsupported():
    with pytest.raises(pb.PbError) as e:
        pb.ksp_options(["-ksp_type", "gmres"])
    assert e.value.code == UNSUPPORTED and "fgmres" in str(e.value)


# ---------------------------------------------------------------------------------------------
# the restatement
# ---------------------------------------------------------------------------------------------
def test_restatement_solves_the_projected_least_squares_problem():
    """12^3, Jacobi, one cycle (restart >= the iteration count): x - x_0 = Z y with y the dense
    least-squares solution of min || ||r_0|| e_1 - H y || over the unrotated Hessenberg, which
    A Z = V H rebuilds from the stored bases; the estimate is that minimum."""
    # (the tolerances: the basis loses orthogonality to about 1e-7 here, see below)
    prob = Problem((12, 12, 12))
    b = prob.rhs()
    detail = {}
    x, reason, its, hist, rn0 = fgmres(prob, b, restart=60, rtol=1e-8, detail=detail)
    assert reason == 2 and 10 < its < 60 and len(hist) == its + 1
    V, Z = np.array(detail["V"]).T, np.array(detail["Z"]).T
    assert V.shape[1] == its + 1 and Z.shape[1] == its
    # the basis is orthonormal to what unrefined classical Gram-Schmidt keeps
    assert np.max(np.abs(V.T @ V - np.eye(its + 1))) < 1e-6
    AZ = np.stack([prob.apply(Z[:, j].copy()) for j in range(its)], axis=1)
    # (its + 1) x its, upper Hessenberg: A Z = V H holds to rounding whatever orthogonality the
    # basis lost, so H is recovered from it by least squares, not as V' A Z
    H = np.linalg.lstsq(V, AZ, rcond=None)[0]
    assert np.max(np.abs(np.tril(H, -2))) < 1e-9 * np.max(np.abs(H))
    e1 = np.zeros(its + 1)
    e1[0] = hist[0]
    y, *_ = np.linalg.lstsq(H, e1, rcond=None)
    x_ls = Z @ y
    assert np.max(np.abs(x - x_ls)) <= 1e-9 * np.max(np.abs(x_ls))
    assert abs(np.linalg.norm(e1 - H @ y) - hist[-1]) <= 1e-6 * hist[-1]
    # right preconditioning: the estimate is the true residual norm
    assert abs(np.linalg.norm(b - prob.apply(x)) - hist[-1]) <= 1e-6 * hist[-1]
    assert rn0 == hist[0] == float(np.sqrt(np.sum(b * b)))


def test_restatement_restart_and_limits():
    prob = Problem((12, 12, 12))
    b = prob.rhs()
    long = fgmres(prob, b, restart=4, max_it=11, **F.FIXED_KW)
    assert (long[1], long[2], len(long[3])) == (-3, 11, 12)
    # the history of a shorter run is a prefix; a restart shows as a slower decrease, not a jump
    short = fgmres(prob, b, restart=4, max_it=6, **F.FIXED_KW)
    assert np.array_equal(short[3], long[3][:7])
    assert np.all(np.diff(long[3]) <= 0)
    # max_it 0, the zero right-hand side, the norm type none, a NaN
    assert fgmres(prob, b, max_it=0)[1:3] == (-3, 0)
    z = fgmres(prob, np.zeros_like(b))
    assert z[1:3] == (3, 0) and not np.any(z[0])
    none = fgmres(prob, b, restart=4, max_it=6, norm_none=True)
    assert none[1:3] == (4, 6) and np.array_equal(none[0], short[0])
    bad = b.copy()
    bad[5] = np.nan
    assert fgmres(prob, bad)[1:3] == (-9, 0)
    # refine_always: the same solve to rounding, another history at rounding level
    ref = fgmres(prob, b, restart=4, max_it=6, refine=True, **F.FIXED_KW)
    assert np.allclose(ref[3], short[3], rtol=1e-10, atol=0)


def test_sensitivity_file_covers_every_case():
    """profiles/ksp_fgmres/sensitivity.json (scripts/fgmres_sensitivity.py) has the measured
    spread of every case the GPU tier takes its bars from, and a spot check reproduces it."""
    rec = json.load(open(F.SENSITIVITY))["cases"]
    assert set(rec) == set(F.CASES)
    assert all(v["same_outcome"] for v in rec.values())
    for cid in F.CASES:
        hbar, xbar, factor = F.bars(cid)
        assert hbar >= 1e-11 and xbar >= 1e-10 and factor >= 10.0
    cid = "fixed-jacobi-5"
    prob = F.setup(cid)[0]
    a, c = F.restated(cid), F.restated(cid, "sequential")
    assert F.hist_diff(prob, a[3], c[3]) <= rec[cid]["d_hist"]
    assert F.x_diff(a[0], c[0]) <= rec[cid]["d_x"]
    assert os.path.exists(os.path.join(F.REPO, "scripts", "fgmres_sensitivity.py"))
