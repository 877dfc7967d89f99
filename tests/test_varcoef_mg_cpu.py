"""CPU tier of the variable-coefficient -pc_type sor | mg: properties of its definition,
tests/varcoef_mg_restatement.py (no GPU, no library call).

The bounds: 1e-12 relative where two orders of summation of the same quantity are compared (a
V-cycle at these sizes is a few hundred rounded operations per point, each within 2^-53); the
iteration counts against the constant-coefficient V-cycle of the same problem, as the numpy
experiment behind the feature measured them at 32^3 (variable / constant: random 1e3 arithmetic
18 / 130, contrast-10 harmonic sphere 12 / 32, 1e-3 harmonic sphere 37 / 66).
"""
import functools

import numpy as np
import pytest

import mg_smoothers_restatement as M
import varcoef_mg_restatement as VM
import varcoef_restatement as V

SEED = 20231015


def rel(a, b):
    return float(np.max(np.abs(a - b)) / np.max(np.abs(b)))


@pytest.mark.parametrize("n3,h", [((16, 16, 16), (1 / 16,) * 3), ((24, 20, 16), (0.05, 0.03, 0.07))])
@pytest.mark.parametrize("pc", ["mg", "sor"])
def test_beta_one_is_the_constant_coefficient_pc(n3, h, pc):
    """Level operators and M^-1 r against mg_smoothers_restatement.VCycle: not bit-equal (the flux
    form sums in another order), equal to 1e-12 relative."""
    rng = np.random.default_rng(SEED)
    levels = 0 if pc == "mg" else 1
    for sm, omega in ((M.Smoother(), 1.0), (M.Smoother(nu=2), 1.3)):
        var = VM.VarVCycle(n3, h, V.beta_one(n3), V.ARITHMETIC, sm, omega=omega, pc=pc)
        con = M.VCycle(n3, h, sm, levels=levels, coarse_its=8 if pc == "mg" else 1, omega=omega)
        assert var.L == con.L and (pc == "sor" or var.L >= 2)
        for lv, lc in zip(var.lv, con.lv):
            assert np.all(lv.beta == 1.0)
            x = rng.standard_normal(lv.shape)
            assert rel(lv.apply(x), lc.apply(x)) <= 1e-12
            assert rel(lv.diag, np.full(lv.shape, lc.cc)) <= 1e-12
        r = rng.standard_normal(int(np.prod(n3)))
        assert rel(var.apply(r), con.apply(r)) <= 1e-12


def test_coarsening_is_the_mean_of_the_eight_children():
    n3 = (8, 12, 4)
    beta = V.beta_random(n3).reshape(n3[2], n3[1], n3[0])
    c = VM.coarsen(beta)
    assert c.shape == (2, 6, 4)
    want = beta.reshape(2, 2, 6, 2, 4, 2).mean(axis=(1, 3, 5))
    assert rel(c, want) <= 4e-16
    assert np.all(VM.coarsen(np.full((4, 4, 4), 0.3)) == 0.3)


@pytest.mark.parametrize("mean", [V.ARITHMETIC, V.HARMONIC])
@pytest.mark.parametrize("pc", ["mg", "sor"])
def test_pc_is_symmetric(mean, pc):
    n3 = (16, 16, 16)
    vc = VM.VarVCycle(n3, (1 / 16,) * 3, V.beta_random(n3), mean, pc=pc)
    rng = np.random.default_rng(SEED)
    u, v = rng.standard_normal(16 ** 3), rng.standard_normal(16 ** 3)
    uMv, vMu = float(u @ vc.apply(v)), float(v @ vc.apply(u))
    assert abs(uMv - vMu) <= 1e-12 * abs(uMv)


@functools.lru_cache(maxsize=None)
def counts(field, inside_or_contrast, mean):
    """(variable-mg count, constant-P-mg count) of CG to rtol 1e-8 at 32^3."""
    n3 = (32, 32, 32)
    beta = (V.beta_sphere(n3, inside=inside_or_contrast) if field == "sphere"
            else V.beta_random(n3, contrast=inside_or_contrast))
    out = []
    for prob in (VM.VarMgProblem(n3, beta, mean, pc="vmg"), V.VarProblem(n3, beta, mean, pc="mg")):
        b = prob.rhs(SEED)
        x, reason, its, hist = M.cg(prob, b, rtol=1e-8)
        assert reason == 2
        out.append(its)
    return tuple(out)


def test_iteration_counts_against_the_constant_coefficient_pc():
    var, con = counts("random", 1e3, V.ARITHMETIC)
    print(f"random 1e3 arithmetic: variable {var} constant {con}")
    assert 2 * var <= con
    var, con = counts("sphere", 0.1, V.HARMONIC)
    print(f"sphere 0.1 harmonic: variable {var} constant {con}")
    assert 2 * var <= con
    var, con = counts("sphere", 1e-3, V.HARMONIC)
    print(f"sphere 1e-3 harmonic: variable {var} constant {con}")
    assert var < con
