"""CPU tier: -ksp_type cg|preonly|richardson and -ksp_richardson_scale through pb_ksp_opts_parse,
the appended pb_ksp_opts field, and the properties of the numpy restatement the GPU tests compare
against (tests/ksp_types_restatement.py).
"""
import ctypes as C

import numpy as np
import pytest

import poissbox_amd as pb
from oracle import oracle as O
from poissbox_amd import _lib as L
from ksp_types_restatement import Problem, preonly, richardson

UNSUPPORTED, ARG = 5, 1


def test_enum_values():
    assert (pb.KSP_CG, pb.KSP_PREONLY, pb.KSP_RICHARDSON) == (0, 1, 2)


def test_defaults():
    o = pb.ksp_options()
    assert o.ksp_type == pb.KSP_CG and o.richardson_scale == 1.0


@pytest.mark.parametrize("name,value", [("cg", 0), ("preonly", 1), ("richardson", 2)])
def test_ksp_type_parsed(name, value):
    o = pb.ksp_options(["-ksp_type", name, "-pc_type", "mg", "-ksp_max_it", "7"])
    assert o.ksp_type == value and o.pc_type == pb.PC_MG and o.max_it == 7
    assert o.richardson_scale == 1.0


@pytest.mark.parametrize("name", ["gmres", "bcgs", "Richardson", "pre_only", ""])
def test_other_ksp_types_unsupported(name):
    with pytest.raises(pb.PbError) as e:
        pb.ksp_options(["-ksp_type", name])
    assert e.value.code == UNSUPPORTED


def test_later_ksp_type_wins():
    assert pb.ksp_options(["-ksp_type", "preonly", "-ksp_type", "cg"]).ksp_type == pb.KSP_CG


def test_richardson_scale_parsed():
    o = pb.ksp_options(["-ksp_type", "richardson", "-ksp_richardson_scale", "0.667"])
    assert o.ksp_type == pb.KSP_RICHARDSON and o.richardson_scale == 0.667
    # the scale alone leaves the type, and negative / zero scales are the caller's business
    o = pb.ksp_options(["-ksp_richardson_scale", "-2.5e-1"])
    assert o.ksp_type == pb.KSP_CG and o.richardson_scale == -0.25
    assert pb.ksp_options(richardson_scale=0.5).richardson_scale == 0.5


@pytest.mark.parametrize("v", ["nan", "inf", "-inf"])
def test_richardson_scale_must_be_finite(v):
    with pytest.raises(pb.PbError) as e:
        pb.ksp_options(["-ksp_richardson_scale", v])
    assert e.value.code == ARG


def test_self_scale_unsupported():
    for argv in (["-ksp_richardson_self_scale"], ["-ksp_richardson_self_scale", "true"],
                 ["-ksp_type", "richardson", "-ksp_richardson_self_scale", "-ksp_rtol", "1e-3"]):
        with pytest.raises(pb.PbError) as e:
            pb.ksp_options(argv)
        assert e.value.code == UNSUPPORTED
    # switched off explicitly it is PETSc's default
    assert pb.ksp_options(["-ksp_richardson_self_scale", "false"]).richardson_scale == 1.0


def test_ctypes_field_appended():
    names = [f[0] for f in L.KspOpts._fields_]
    assert names[-1] == "richardson_scale" and names[-2] == "guess_fischer_maxl"
    assert names.index("ksp_type") == 4
    off = L.KspOpts.richardson_scale.offset
    assert off % 8 == 0 and off >= L.KspOpts.guess_fischer_maxl.offset + 4
    assert C.sizeof(L.KspOpts) == off + 8


def test_version_unchanged():
    major, minor = C.c_int(), C.c_int()
    L.call("pb_version", C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == (0, 2)


# ---------------------------------------------------------------------------------------------
# the restatement's own properties (oracle blocks on the CPU)
# ---------------------------------------------------------------------------------------------
def test_restatement_richardson_fft_is_one_iteration():
    """The spectral PC inverts the 7-point symbol: the first update solves the system, the second
    norm is rounding noise."""
    prob = Problem((16, 16, 12), pc="fft")
    b = prob.rhs()
    x, reason, its, hist, rn0 = richardson(prob, b)
    assert (reason, its, len(hist)) == (2, 1, 2)
    assert hist[1] < 1e-12 * hist[0] and rn0 == hist[0]
    bm = b - b.mean()
    assert np.linalg.norm(bm - prob.apply(x)) < 1e-12 * np.linalg.norm(b)


def test_restatement_overrelaxed_jacobi_diverges():
    """Jacobi's iteration matrix has eigenvalues in (-1, 1]: scale 2.5 amplifies the highest modes
    by up to 4 per step, and the default dtol = 1e5 stops it."""
    prob = Problem((17, 18, 9))
    x, reason, its, hist, rn0 = richardson(prob, prob.rhs(), scale=2.5)
    assert (reason, its, len(hist)) == (-4, 10, 11)
    assert hist[-1] >= 1e5 * rn0 > hist[-2]


def test_restatement_damped_jacobi_contracts():
    prob = Problem((16, 16, 12))
    _, reason, its, hist, _ = richardson(prob, prob.rhs(), scale=2.0 / 3.0, rtol=0.0, atol=0.0,
                                         max_it=6)
    assert (reason, its, len(hist)) == (-3, 6, 7)
    assert np.all(np.diff(hist) < 0)


def test_restatement_preonly():
    prob = Problem((16, 16, 12), pc="fft")
    b = prob.rhs()
    x, reason, its, hist, rn0 = preonly(prob, b)
    assert (reason, its, len(hist), rn0) == (4, 1, 0, 0.0)
    # no mean subtraction with the spectral PC: the mean is at rounding level by itself
    assert abs(x.mean()) < 1e-15 * np.max(np.abs(x))
    x1 = richardson(prob, b, rtol=0.0, atol=0.0, max_it=1)[0]
    assert np.max(np.abs(x1 - x)) <= 1e-14 * np.max(np.abs(x))
    # jacobi: D^-1 b with its mean removed
    pj = Problem((16, 16, 12))
    xj = preonly(pj, b + 1.0)[0]
    assert abs(xj.mean()) < 1e-12 * np.max(np.abs(xj))
    assert np.allclose(xj, (b - b.mean()) / O.diag(pj.h), rtol=1e-12, atol=1e-12 * np.max(np.abs(xj)))


def test_restatement_guess_reference_norm():
    """From a nonzero guess rnorm0 is ||N(M^-1 b)||, the norm the zero-guess solve logs first."""
    prob = Problem((16, 16, 12))
    b = prob.rhs()
    cold = richardson(prob, b, scale=2.0 / 3.0, rtol=0.0, atol=0.0, max_it=4)
    warm = richardson(prob, b, x0=cold[0], scale=2.0 / 3.0, rtol=0.0, atol=0.0, max_it=2)
    assert warm[4] == cold[3][0]
    # continuing from the fourth iterate repeats iterations 4, 5, 6 of the cold run
    cold6 = richardson(prob, b, scale=2.0 / 3.0, rtol=0.0, atol=0.0, max_it=6)
    assert np.allclose(warm[3], cold6[3][4:], rtol=1e-12)
