"""CPU tier of the mass term of PB_OP_VARCOEF (pb_op_set_mass): properties of its definition,
tests/varcoef_mass_restatement.py (no GPU, no library call).

The bounds: bit equality where the definition promises it (symmetry, A 1 = -q, the mass off); 1e-12
relative for the V-cycle's symmetry, test_varcoef_mg_cpu.py's bound and for its reason (two orders
of summation of the same quantity; a V-cycle at 16^3 is a few hundred rounded operations per point,
each within 2^-53); the iteration counts of the variable V-cycle against the variable Jacobi as the
numpy experiment behind the feature measured them at 32^3, m uniform in [0.5, 1.5], nullspace 0
(variable mg / variable Jacobi: random 1e3 arithmetic 18 / 151 at s = 1 and 13 / 39 at s = 100,
sphere 1e-3 harmonic 28 / 156 and 10 / 71). The near-singular s = 1e-3 (the coarsest level only
sweeps and nothing removes the almost-constant mode) and the mass-dominated s = 1e4 are not
asserted.
"""
import numpy as np
import pytest

import mg_smoothers_restatement as M
import varcoef_mass_restatement as VMS
import varcoef_mg_restatement as VM
import varcoef_restatement as V

SEED = 20231015
MEANS = [V.ARITHMETIC, V.HARMONIC]


def dense(n3, h, beta, mean, m, s):
    N = int(np.prod(n3))
    A = np.empty((N, N))
    for c in range(N):
        e = np.zeros(N)
        e[c] = 1.0
        A[:, c] = VMS.apply(e, beta, n3, h, mean, m, s)
    return A


@pytest.mark.parametrize("mean", MEANS)
@pytest.mark.parametrize("mass", ["field", "scalar", "field-with-zeros"])
def test_dense_matrix(mean, mass):
    n3, h = (4, 3, 3), (0.25, 0.3, 0.35)
    N = int(np.prod(n3))
    beta = V.beta_random(n3)
    m, s = (None, 37.5) if mass == "scalar" else (VMS.mass_uniform(n3), 100.0)
    if mass == "field-with-zeros":
        m = m.copy()
        m[:N // 2] = 0.0
    q = VMS.q_of(m, s, n3)
    qf = np.full(N, q) if np.isscalar(q) else q.reshape(-1)
    A = dense(n3, h, beta, mean, m, s)
    assert np.array_equal(A, A.T)
    assert np.array_equal(VMS.apply(np.ones(N), beta, n3, h, mean, m, s), -qf)
    assert np.array_equal(np.diag(A), VMS.diag(beta, n3, h, mean, m, s))
    assert np.array_equal(VMS.diag(beta, n3, h, mean, m, s), V.diag(beta, n3, h, mean) - qf)
    ev = np.linalg.eigvalsh(A)
    print(f"{mass} mean {mean}: eigenvalues in [{ev[0]:.6e}, {ev[-1]:.6e}]")
    assert np.all(ev < 0.0)
    # the mass off: the parent's bits, whatever m is
    x = np.random.default_rng(SEED).standard_normal(N)
    assert np.array_equal(VMS.apply(x, beta, n3, h, mean, m, 0.0), V.apply(x, beta, n3, h, mean))
    assert np.array_equal(VMS.diag(beta, n3, h, mean, m, 0.0), V.diag(beta, n3, h, mean))
    # ... where the parent's matrix is singular
    assert np.all(V.apply(np.ones(N), beta, n3, h, mean) == 0.0)


def test_levels_of_the_mass():
    n3, h = (16, 12, 8), (1 / 16, 1 / 12, 1 / 8)
    beta, m = V.beta_random(n3), VMS.mass_uniform(n3)
    assert np.all(VM.coarsen(np.full((4, 4, 4), 37.5)) == 37.5)
    # a scalar mass stays s on every level; the mass off gives the parent's levels
    vc = VMS.MassVCycle(n3, h, beta, V.HARMONIC, None, 37.5)
    assert vc.L >= 2 and all(np.isscalar(lv.q) and lv.q == 37.5 for lv in vc.lv)
    off, par = VMS.MassVCycle(n3, h, beta, V.HARMONIC, m, 0.0), VM.VarVCycle(n3, h, beta, V.HARMONIC)
    r = np.random.default_rng(SEED).standard_normal(int(np.prod(n3)))
    assert np.array_equal(off.apply(r), par.apply(r))
    # a field: q_0 = s * m, then the 8-child mean; dinv = 1.0 / ((-G6) - q)
    vc = VMS.MassVCycle(n3, h, beta, V.ARITHMETIC, m, 100.0)
    q = 100.0 * m.reshape(n3[2], n3[1], n3[0])
    for l, lv in enumerate(vc.lv):
        if l > 0:
            q = VM.coarsen(q)
        assert np.array_equal(lv.q, q)
        d = V.diag(lv.beta, lv.n, lv.h, lv.mean).reshape(lv.shape) - q
        assert np.array_equal(lv.diag, d) and np.array_equal(lv.dinv, 1.0 / d)
        x = np.random.default_rng(SEED + l).standard_normal(lv.shape)
        assert np.array_equal(lv.apply(x), V.apply(x, lv.beta, lv.n, lv.h, lv.mean).reshape(lv.shape)
                              - q * x)


@pytest.mark.parametrize("mean", MEANS)
@pytest.mark.parametrize("pc", ["mg", "sor"])
def test_pc_with_a_mass_is_symmetric(mean, pc):
    n3 = (16, 16, 16)
    vc = VMS.MassVCycle(n3, (1 / 16,) * 3, V.beta_random(n3), mean, VMS.mass_uniform(n3), 100.0,
                        pc=pc)
    rng = np.random.default_rng(SEED)
    u, v = rng.standard_normal(16 ** 3), rng.standard_normal(16 ** 3)
    uMv, vMu = float(u @ vc.apply(v)), float(v @ vc.apply(u))
    print(f"{pc} mean {mean}: u.Mv {uMv:.15e} v.Mu {vMu:.15e}")
    assert abs(uMv - vMu) <= 1e-12 * abs(uMv)


COUNT_CASES = [("random", 1e3, V.ARITHMETIC), ("sphere", 1e-3, V.HARMONIC)]


@pytest.mark.parametrize("s", [1.0, 100.0])
@pytest.mark.parametrize("field,arg,mean", COUNT_CASES, ids=[c[0] for c in COUNT_CASES])
def test_iteration_counts_against_the_variable_jacobi(field, arg, mean, s):
    n3 = (32, 32, 32)
    beta = V.beta_sphere(n3, inside=arg) if field == "sphere" else V.beta_random(n3, contrast=arg)
    m = VMS.mass_uniform(n3)
    its = {}
    for name, prob in (("vmg", VMS.MassMgProblem(n3, beta, mean, m, s, pc="vmg")),
                       ("vjacobi", VMS.MassProblem(n3, beta, mean, m, s, pc="vjacobi"))):
        assert prob.nullspace == 0 and prob.h == (1 / 32,) * 3
        b = prob.rhs(SEED)
        x, reason, its[name], hist = M.cg(prob, b, rtol=1e-8)
        assert reason == 2, (name, reason)
    print(f"{field} s = {s}: variable mg {its['vmg']} variable Jacobi {its['vjacobi']}")
    assert 2 * its["vmg"] <= its["vjacobi"]
