"""CPU tier of PB_OP_VARCOEF: the numpy restatement (tests/varcoef_restatement.py) that defines the
operator, checked for what the definition promises, and `VarProblem` under the KSP restatements
the GPU tier compares against.

With beta = 1 the operator is the 7-point Laplacian in another summation (six flux terms instead of
seven products), so it agrees with the oracle's O.stencil to rounding, not to the bit. Measured
here, max |A_var x - A_star x| / max |A_star x| for x = fill_random(20231015), either mean:
    17 x 12 x 9  (h = 1 / n)             2.76e-16
    24 x 20 x 10 (h = 0.05, 0.03, 0.07)  2.95e-16
STENCIL_BAR is 100 x the larger of the two (parity_bars.py's two orders of margin).
"""
import numpy as np
import pytest

from oracle import oracle as O
import chebyshev_restatement as CR
import fgmres_restatement as FR
import ksp_types_restatement as KR
import norm_type_restatement as NR
import pipecg_restatement as PR
import varcoef_restatement as V

STENCIL_BAR = 100 * 2.95e-16
SEED = 20231015
MEAN_IDS = ["arithmetic", "harmonic"]


@pytest.mark.parametrize("mean", [V.ARITHMETIC, V.HARMONIC], ids=MEAN_IDS)
@pytest.mark.parametrize("n3,h", [((17, 12, 9), None), ((24, 20, 10), (0.05, 0.03, 0.07))])
def test_beta_one_is_the_stencil(n3, h, mean):
    h = h or tuple(1.0 / m for m in n3)
    x = O.fill_random(int(np.prod(n3)), SEED)
    ys = O.stencil(x, n3, h)
    yv = V.apply(x, V.beta_one(n3), n3, h, mean)
    rel = float(np.max(np.abs(ys - yv)) / np.max(np.abs(ys)))
    print(f"{n3} mean {mean}: max |A_var x - A_star x| / max |A_star x| = {rel:.3e}")
    assert rel <= STENCIL_BAR
    # the diagonal with beta = 1 is the star's centre coefficient to rounding
    d = V.diag(V.beta_one(n3), n3, h, mean)
    assert np.max(np.abs(d - O.diag(h))) <= STENCIL_BAR * abs(O.diag(h))


@pytest.mark.parametrize("mean", [V.ARITHMETIC, V.HARMONIC], ids=MEAN_IDS)
@pytest.mark.parametrize("field", list(V.FIELDS))
def test_constants_are_in_the_null_space_to_the_bit(field, mean):
    n3, h = (24, 20, 10), (0.05, 0.03, 0.07)
    beta = V.FIELDS[field](n3)
    for c in (1.0, -3.7, 1e-300):
        y = V.apply(np.full(int(np.prod(n3)), c), beta, n3, h, mean)
        assert np.all(y == 0.0) and not np.any(np.signbit(y))


@pytest.mark.parametrize("mean", [V.ARITHMETIC, V.HARMONIC], ids=MEAN_IDS)
def test_face_is_commutative_to_the_bit(mean):
    rng = np.random.default_rng(5)
    a = np.exp(rng.uniform(-7, 7, 20000))
    b = np.exp(rng.uniform(-7, 7, 20000))
    assert np.array_equal(V.face(a, b, mean), V.face(b, a, mean))
    if mean == V.ARITHMETIC:  # (the harmonic mean of a with itself rounds a * a first)
        assert np.all(V.face(a, a, mean) == a)


@pytest.mark.parametrize("mean", [V.ARITHMETIC, V.HARMONIC], ids=MEAN_IDS)
@pytest.mark.parametrize("field", ["random", "sphere"])
def test_dense_matrix_is_symmetric_to_the_bit(field, mean):
    n3, h = (4, 3, 3), (0.3, 0.2, 0.25)
    N = int(np.prod(n3))
    beta = V.FIELDS[field](n3)
    M = np.empty((N, N))
    for j in range(N):
        e = np.zeros(N)
        e[j] = 1.0
        M[:, j] = V.apply(e, beta, n3, h, mean)
    assert np.array_equal(M, M.T)
    assert np.array_equal(np.diag(M), V.diag(beta, n3, h, mean))
    assert np.all(np.diag(M) < 0.0)  # the Laplacian's sign: -A is positive semi-definite


def _true_residual(prob, b, x):
    return float(np.linalg.norm(b - prob.apply(x)) / np.linalg.norm(b))


N3 = (16, 16, 16)


def _problem(pc, mean=V.HARMONIC, contrast=10.0):
    prob = V.VarProblem(N3, V.beta_sphere(N3, inside=1.0 / contrast), mean, pc=pc)
    return prob, prob.rhs()


@pytest.mark.parametrize("pc", ["vjacobi", "none", "jacobi", "sor", "mg", "fft"])
def test_cg_restatement_on_varproblem(pc):
    """norm_type_restatement.cg with the variable operator and every PC the GPU tier runs: it
    converges, to a true residual of the order of rtol, and the variable Jacobi and the constant
    P's multigrid / spectral PC need fewer iterations than no PC (the issue's premise)."""
    prob, b = _problem(pc)
    x, reason, its, hist, rn0 = NR.cg(prob, b, rtol=1e-8)
    assert reason == 2 and len(hist) == its + 1
    assert _true_residual(prob, b, x) < 1e-7
    if pc != "none":
        its_none = NR.cg(_problem("none")[0], b, rtol=1e-8)[2]
        assert its <= its_none, (pc, its, its_none)


def test_variable_jacobi_is_the_reciprocal_diagonal():
    prob, b = _problem("vjacobi")
    d = V.diag(prob.beta, prob.n3, prob.h, prob.mean)
    assert np.array_equal(prob.pc_apply(b), (1.0 / d) * b)
    prob.set_beta(V.beta_random(N3), V.ARITHMETIC)
    d2 = V.diag(prob.beta, prob.n3, prob.h, V.ARITHMETIC)
    assert np.array_equal(prob.pc_apply(b), (1.0 / d2) * b) and not np.array_equal(d, d2)


def test_richardson_restatement_on_varproblem():
    prob, b = _problem("mg")
    x, reason, its, hist, rn0 = KR.richardson(prob, b, rtol=1e-6)
    assert reason == 2 and _true_residual(prob, b, x) < 1e-5
    prob, b = _problem("vjacobi")
    x, reason, its, hist, rn0 = KR.richardson(prob, b, scale=2.0 / 3.0, max_it=6, rtol=0.0,
                                              atol=0.0, dtol=1e300)
    assert (reason, its) == (-3, 6) and hist[-1] < hist[0]


def test_chebyshev_restatement_on_varproblem():
    prob, b = _problem("vjacobi")
    # D^-1 A of a flux-form operator has its spectrum in [0, 2] as the constant one's
    x, reason, its, hist, rn0 = CR.chebyshev(prob, b, 0.05, 2.0, max_it=40, rtol=0.0, atol=0.0,
                                             dtol=1e300)
    assert (reason, its) == (-3, 40) and hist[-1] < 1e-2 * hist[0]


def test_fgmres_restatement_on_varproblem():
    prob, b = _problem("fft")
    x, reason, its, hist, rn0 = FR.fgmres(prob, b, rtol=1e-8)
    assert reason == 2 and _true_residual(prob, b, x) <= 1e-8 * 1.001


def test_pipecg_restatement_on_varproblem():
    prob, b = _problem("vjacobi")
    x, reason, its, hist, rn0 = PR.pipecg(prob, b, rtol=1e-8)
    assert reason == 2 and _true_residual(prob, b, x) < 1e-7
    # CG in exact arithmetic: the same count as cg to within the pipelined recurrences' drift
    its_cg = NR.cg(prob, b, rtol=1e-8)[2]
    assert abs(its - its_cg) <= 2, (its, its_cg)
