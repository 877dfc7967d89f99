"""CPU tier of the MAC-grid gradient, projection and divergence: the numpy restatement
(tests/mac_restatement.py) that defines them, checked for the mathematics the GPU tier then
inherits bit for bit -- D G = A to rounding, so a field projected with the solved p is discretely
divergence-free.

The bounds, with u = 2^-53, g_n the operator's six face coefficients, EA_c = sum_n g_n (|p_n| +
|p_c|) and EU_c = sum_d r_d (m_d(c) + m_d(c - e_d)), m_d = |u*_d| + |s G_d| (mac_restatement.ea /
.eu):
    |D(G p) - A p|_c                     <= 32 u EA_c                 s = 1
    |D(u* - s G p) - (D u* - s A p)|_c   <= 32 u (s EA_c + EU_c)      s = 0.75
Why 32: a first-order count of the roundings on the two paths gives about 28 u (per term of
D(G p): the difference, the face mean, r_d * face, the product, D's difference, D's product by r_d
against A's c_d = 1 / h_d^2 with its own rounding, and the sums of six against three terms). The
largest ratios this file prints over the cases below (p and u* from fill_random, seeds 20231015 ..
20231018) are 5.51 u (24x20x10, random, arithmetic) and 2.94 u; the run behind the feature's
request, on its own inputs, gave 7.1 u and 3.1 u. Either way the restatement alone stays inside the
bound with a margin above 4x. Every test prints its ratio before it asserts.
"""
import numpy as np
import pytest

from oracle import oracle as O
import mac_restatement as M
import varcoef_restatement as V

U = 2.0 ** -53
SEED = 20231015
DELTAS = (0.05, 0.03, 0.07)
SHAPES = [((9, 7, 5), None), ((17, 12, 9), None), ((24, 20, 10), DELTAS), ((32, 32, 32), None)]
SHAPE_IDS = [f"{s[0]}" for s in SHAPES]
MEAN_IDS = ["arithmetic", "harmonic"]


def spacing(n3, deltas):
    return tuple(deltas) if deltas else tuple(1.0 / m for m in n3)


def fields(n3):
    N = int(np.prod(n3))
    return O.fill_random(N, SEED), tuple(O.fill_random(N, SEED + 1 + d) for d in range(3))


@pytest.mark.parametrize("mean", [V.ARITHMETIC, V.HARMONIC], ids=MEAN_IDS)
@pytest.mark.parametrize("field", list(V.FIELDS))
@pytest.mark.parametrize("n3,deltas", SHAPES, ids=SHAPE_IDS)
def test_div_of_grad_is_the_operator(n3, deltas, field, mean):
    h = spacing(n3, deltas)
    beta = V.FIELDS[field](n3)
    p, _ = fields(n3)
    dg = M.div(M.grad(p, beta, n3, h, mean), n3, h, 1.0)
    ap = V.apply(p, beta, n3, h, mean)
    ratio = float(np.max(np.abs(dg - ap) / M.ea(p, beta, n3, h, mean))) / U
    print(f"{n3} {field} mean {mean}: max |D G p - A p| / EA = {ratio:.2f} u")
    assert ratio <= 32.0


@pytest.mark.parametrize("mean", [V.ARITHMETIC, V.HARMONIC], ids=MEAN_IDS)
@pytest.mark.parametrize("field", list(V.FIELDS))
@pytest.mark.parametrize("n3,deltas", SHAPES, ids=SHAPE_IDS)
def test_divergence_of_the_projected_field(n3, deltas, field, mean):
    h = spacing(n3, deltas)
    s = 0.75
    beta = V.FIELDS[field](n3)
    p, us = fields(n3)
    got = M.div(M.project(us, p, s, beta, n3, h, mean), n3, h, 1.0)
    want = M.div(us, n3, h, 1.0) - s * V.apply(p, beta, n3, h, mean)
    bound = s * M.ea(p, beta, n3, h, mean) + M.eu(us, p, s, beta, n3, h, mean)
    ratio = float(np.max(np.abs(got - want) / bound)) / U
    print(f"{n3} {field} mean {mean}: max |D(u* - s G p) - (D u* - s A p)| / (s EA + EU) = "
          f"{ratio:.2f} u")
    assert ratio <= 32.0


@pytest.mark.parametrize("mean", [V.ARITHMETIC, V.HARMONIC], ids=MEAN_IDS)
@pytest.mark.parametrize("n3,deltas", SHAPES, ids=SHAPE_IDS)
def test_beta_one_is_the_star7_form_to_the_bit(n3, deltas, mean):
    h = spacing(n3, deltas)
    p, us = fields(n3)
    one = V.beta_one(n3)
    for a, b in zip(M.grad(p, one, n3, h, mean), M.grad(p, None, n3, h)):
        assert np.array_equal(a, b)
    for a, b in zip(M.project(us, p, 0.75, one, n3, h, mean), M.project(us, p, 0.75, None, n3, h)):
        assert np.array_equal(a, b)


def test_a_constant_has_no_gradient_and_a_constant_field_no_divergence():
    n3, h = (24, 20, 10), DELTAS
    N = int(np.prod(n3))
    for g in M.grad(np.full(N, -3.7), V.beta_random(n3), n3, h, V.HARMONIC):
        assert np.all(g == 0.0)
    assert np.all(M.div(tuple(np.full(N, c) for c in (1.5, -2.0, 1e-300)), n3, h, 8.0) == 0.0)
