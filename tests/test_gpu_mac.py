"""GPU tier of the MAC-grid gradient, projection and divergence of the 7-point operators
(pb_op_mac_grad / pb_op_mac_project / pb_op_mac_div) against their numpy restatement
(tests/mac_restatement.py, which defines them; DESIGN.md §3.5 "Projection").

Every result and every rank's slab must be bit-identical to the restatement: the same operations
in the same order, every one rounded (no FMA contraction, correctly rounded fp64 division). The
kernels pick their variants as the variable-coefficient apply does -- by nx's parity (two / one
point per lane) and ny's divisibility by 4 / 2 (rows per wave) -- and by the operator (no beta,
arithmetic, harmonic) and no others, so the shapes are that operator's six: 9x7x5 (odd x, 1 row),
17x12x9 (odd x, 4 rows), 24x20x10 (even x, 4 rows, unequal deltas), 130x6x4 (two x segments, 2
rows), 256x8x3 (full segments, the smallest z) and 64^3 (several tiles and z-chunks).

The projection end to end (test_projection_is_divergence_free): with u = 2^-53, EA and EU the
magnitudes of mac_restatement.ea / .eu (tests/test_mac_cpu.py pins |D(u* - s G p) - (D u* - s A p)|
<= 32 u (s EA + EU) per cell), the divergence left after the correction is the solve's own true
residual plus that rounding term: ||D u||_2 <= ||b - A p||_2 + ||32 u (EA + EU)||_2, and with the
solve at rtol 1e-10 it is below 1e-8 ||b||_2 (README's true residuals for cg + mg sit below the
rtol in every table; the factor 100 covers the gap between the recurrence residual and the true
one). sum b telescopes to zero but for D's roundings: |sum b| <= 32 u sum_d r_d sum |u*_d|.

Every test here fails without the feature: the symbols do not exist.
"""
import math

import numpy as np
import pytest

import poissbox_amd as pb
from oracle import oracle as O
import mac_restatement as M
import varcoef_restatement as V

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED = 1, 5
U = 2.0 ** -53
SEED = 20231015
SENTINEL = 7.25
MEANS = [V.ARITHMETIC, V.HARMONIC]
DELTAS = (0.05, 0.03, 0.07)
SHAPES = [((9, 7, 5), None), ((17, 12, 9), None), ((24, 20, 10), DELTAS), ((130, 6, 4), None),
          ((256, 8, 3), None), ((64, 64, 64), None)]
# (field, mean); field None: PB_OP_STAR7
CASES = [(None, V.ARITHMETIC)] + [(f, m) for f in V.FIELDS for m in MEANS]


def spacing(n3, deltas):
    return tuple(deltas) if deltas else tuple(1.0 / m for m in n3)


def cut(v, n3, rows):
    return v if rows is None else v.reshape(n3[2], -1)[rows[0]:rows[0] + rows[1]].reshape(-1)


def vec_of(da, values):
    v = pb.Vec(da)
    v.set_values(values)
    return v


def inputs(n3):
    N = int(np.prod(n3))
    return O.fill_random(N, SEED), tuple(O.fill_random(N, SEED + 1 + d) for d in range(3))


def beta_of(field, n3):
    return None if field is None else V.FIELDS[field](n3)


def operator(da, field, mean, n3, h, rows=None):
    """the Mat of a case on da; beta cut to the planes of rows"""
    if field is None:
        return pb.Mat(da, pb.STAR7, h)
    A = pb.Mat(da, pb.VARCOEF, h)
    bv = vec_of(da, cut(V.FIELDS[field](n3), n3, rows))
    A.set_coefficient(bv, mean)
    bv.destroy()
    return A


def run_case(A, da, p, us, n3, rows):
    """grad, project (s = 0.75, 1) and div (s = 1, 8) of the inputs' planes `rows` on A: a dict of
    host arrays. Outputs are prefilled with a sentinel."""
    pv = vec_of(da, cut(p, n3, rows))
    g3 = [pb.Vec(da) for _ in range(3)]
    out = {}
    for g in g3:
        g.set(SENTINEL)
    A.mac_grad(pv, g3)
    out["grad"] = [g.get_values() for g in g3]
    for s in (0.75, 1.0):
        for g, u in zip(g3, us):
            g.set_values(cut(u, n3, rows))
        A.mac_project(pv, s, g3)
        out["project", s] = [g.get_values() for g in g3]
    for g, u in zip(g3, us):
        g.set_values(cut(u, n3, rows))
    dv = pb.Vec(da)
    for s in (1.0, 8.0):
        dv.set(SENTINEL)
        A.mac_div(g3, dv, s)
        out["div", s] = dv.get_values()
    dv.set(SENTINEL)
    A.mac_div(g3, dv)  # s defaults to 1
    assert np.array_equal(dv.get_values(), out["div", 1.0])
    for v in g3 + [pv, dv]:
        v.destroy()
    return out


def expected(p, us, beta, n3, h, mean):
    want = {"grad": M.grad(p, beta, n3, h, mean)}
    for s in (0.75, 1.0):
        want["project", s] = M.project(us, p, s, beta, n3, h, mean)
    for s in (1.0, 8.0):
        want["div", s] = M.div(us, n3, h, s)
    return want


def assert_same(got, want, n3, rows, what):
    for key, w in want.items():
        g = got[key]
        if isinstance(w, tuple):
            for d, (gd, wd) in enumerate(zip(g, w)):
                assert np.array_equal(gd, cut(wd, n3, rows)), (what, key, d)
        else:
            assert np.array_equal(g, cut(w, n3, rows)), (what, key)


# ---------------------------------------------------------------------------------------------
# 1. grad, project and div bit-identical to the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n3,deltas", SHAPES, ids=[f"{s[0]}" for s in SHAPES])
def test_bit_identical(ctx, n3, deltas):
    h = spacing(n3, deltas)
    p, us = inputs(n3)
    da = pb.DA(ctx, n3)
    for field, mean in CASES:
        A = operator(da, field, mean, n3, h)
        got = run_case(A, da, p, us, n3, None)
        assert_same(got, expected(p, us, beta_of(field, n3), n3, h, mean), n3, None, (field, mean))
        A.destroy()
    da.destroy()


def test_set_deltas(ctx):
    n3 = (17, 12, 9)
    p, us = inputs(n3)
    da = pb.DA(ctx, n3)
    for field, mean in [(None, V.ARITHMETIC), ("random", V.HARMONIC)]:
        A = operator(da, field, mean, n3, spacing(n3, None))
        A.set_deltas(DELTAS)
        got = run_case(A, da, p, us, n3, None)
        assert_same(got, expected(p, us, beta_of(field, n3), n3, DELTAS, mean), n3, None, field)
        A.destroy()
    da.destroy()


# ---------------------------------------------------------------------------------------------
# 2. N ranks over the host transport: every slab bit-identical to the one-rank result.
# (4, 16x8x4): one plane per rank, both the z+ plane of p and the z- plane of uz are ghosts
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks,n3", [(2, (16, 16, 12)), (3, (20, 16, 7)), (2, (16, 16, 4)),
                                       (4, (16, 8, 4))])
def test_ranks_bit_identical(ctx, nranks, n3):
    from test_gpu_parity import run_ranks
    h = spacing(n3, None)
    p, us = inputs(n3)

    def one(c, rows):
        da = pb.DA(c, n3)
        out = []
        for field, mean in CASES:
            A = operator(da, field, mean, n3, h, rows)
            out.append(run_case(A, da, p, us, n3, rows))
            A.destroy()
        return out

    whole = one(ctx, None)
    for (field, mean), got in zip(CASES, whole):
        assert_same(got, expected(p, us, beta_of(field, n3), n3, h, mean), n3, None, (field, mean))

    def body(c, rank):
        rows = pb.slab_partition(n3[2], nranks, rank)
        return rows, one(c, rows)

    for rows, slabs in run_ranks(nranks, body):
        for case, got, w in zip(CASES, slabs, whole):
            want = {k: (tuple(v) if isinstance(v, list) else v) for k, v in w.items()}
            assert_same(got, want, n3, rows, (rows, case))


# ---------------------------------------------------------------------------------------------
# 3. errors leave every output untouched; the mass term is no part of G
# ---------------------------------------------------------------------------------------------
def test_errors_leave_outputs_untouched(ctx):
    n3 = (17, 12, 9)
    h = spacing(n3, None)
    p, us = inputs(n3)
    da, other = pb.DA(ctx, n3), pb.DA(ctx, (16, 12, 9))
    pv, dv = vec_of(da, p), pb.Vec(da)
    u3 = [vec_of(da, u) for u in us]
    po, uo = pb.Vec(other), pb.Vec(other)
    po.set(1.0)
    uo.set(1.0)
    dv.set(SENTINEL)

    def unchanged():
        assert all(np.array_equal(v.get_values(), u) for v, u in zip(u3, us))
        assert np.array_equal(pv.get_values(), p) and np.all(dv.get_values() == SENTINEL)

    def raises(code, call):
        with pytest.raises(pb.PbError) as e:
            call()
        assert e.value.code == code
        unchanged()

    for kind in (pb.COMPACT, pb.ASSEMBLED27):
        B = pb.Mat(da, kind, h)
        raises(UNSUPPORTED, lambda: B.mac_grad(pv, u3))
        raises(UNSUPPORTED, lambda: B.mac_project(pv, 0.75, u3))
        raises(UNSUPPORTED, lambda: B.mac_div(u3, dv))
        B.destroy()
    for field in (None, "random"):
        A = operator(da, field, V.HARMONIC, n3, h)
        # a vector of another grid
        raises(ARG, lambda: A.mac_grad(po, u3))
        raises(ARG, lambda: A.mac_grad(pv, [u3[0], uo, u3[2]]))
        raises(ARG, lambda: A.mac_project(po, 0.75, u3))
        raises(ARG, lambda: A.mac_project(pv, 0.75, [u3[0], u3[1], uo]))
        raises(ARG, lambda: A.mac_div([uo, u3[1], u3[2]], dv))
        raises(ARG, lambda: A.mac_div(u3, po))
        # three components that are not distinct
        for trio in ([u3[0], u3[0], u3[2]], [u3[0], u3[1], u3[0]], [u3[0], u3[1], u3[1]]):
            raises(ARG, lambda: A.mac_grad(pv, trio))
            raises(ARG, lambda: A.mac_project(pv, 0.75, trio))
            raises(ARG, lambda: A.mac_div(trio, dv))
        # p among g / u, out among u
        for d in range(3):
            trio = list(u3)
            trio[d] = pv
            raises(ARG, lambda: A.mac_grad(pv, trio))
            raises(ARG, lambda: A.mac_project(pv, 0.75, trio))
            raises(ARG, lambda: A.mac_div(u3, u3[d]))
        # a non-finite s
        for s in (np.nan, np.inf, -np.inf):
            raises(ARG, lambda: A.mac_project(pv, s, u3))
            raises(ARG, lambda: A.mac_div(u3, dv, s))
        A.destroy()
    # a field mass set on the operator changes nothing in G
    beta = V.beta_random(n3)
    A = operator(da, "random", V.ARITHMETIC, n3, h)
    mv = vec_of(da, V.beta_sphere(n3))
    A.set_mass(mv, 2.5)
    got = run_case(A, da, p, us, n3, None)
    assert_same(got, expected(p, us, beta, n3, h, V.ARITHMETIC), n3, None, "mass")
    for o in [A, mv, pv, dv, po, uo] + u3:
        o.destroy()
    other.destroy()
    da.destroy()


# ---------------------------------------------------------------------------------------------
# 4. the projection, end to end
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("field,mean", [("random", V.ARITHMETIC), ("sphere", V.HARMONIC),
                                        (None, V.ARITHMETIC)],
                         ids=["random-arithmetic", "sphere-harmonic", "star7"])
def test_projection_is_divergence_free(ctx, field, mean):
    n3 = (32, 32, 32)
    h = spacing(n3, None)
    _, us = inputs(n3)
    beta = beta_of(field, n3)
    da = pb.DA(ctx, n3)
    A = operator(da, field, mean, n3, h)
    P = A if field is None else pb.Mat(da, pb.STAR7, h)
    u3 = [vec_of(da, u) for u in us]
    bv, pv, wv = pb.Vec(da), pb.Vec(da), pb.Vec(da)
    # 1. b = D u*
    A.mac_div(u3, bv)
    b = bv.get_values()
    rsum = sum(r * math.fsum(np.abs(u)) for r, u in zip(M.recips(h), us))
    print(f"|sum b| = {abs(math.fsum(b)):.3e}, bound {32 * U * rsum:.3e}")
    assert abs(math.fsum(b)) <= 32 * U * rsum
    # 2. div(beta grad p) = b: cg with the multigrid of the operator's own coefficient
    k = pb.KSP(A, P, pb.ksp_options(["-ksp_type", "cg", "-pc_type", "mg", "-ksp_rtol", "1e-10"]))
    if field is not None:
        k.pc_set_coefficient_from(A)
    reason, its, _ = k.solve(bv, pv)
    assert reason > 0, (reason, its)
    # 3. u = u* - G p
    A.mac_project(pv, 1.0, u3)
    # the divergence left, against the solve's true residual by the library's own apply
    A.mac_div(u3, wv)
    d = wv.get_values()
    A.mult(pv, wv)
    p = pv.get_values()
    res = b - wv.get_values()
    rounding = 32 * U * (M.ea(p, beta, n3, h, mean) + M.eu(us, p, 1.0, beta, n3, h, mean))
    nd, nr, ne, nb = (float(np.linalg.norm(v)) for v in (d, res, rounding, b))
    print(f"{field} its {its}: ||D u|| = {nd:.3e}, ||b - A p|| = {nr:.3e}, rounding term {ne:.3e}, "
          f"||b|| = {nb:.3e}")
    assert nd <= nr + ne
    assert nd <= 1e-8 * nb
    k.destroy()
    for o in [bv, pv, wv] + u3 + ([A] if P is A else [A, P]):
        o.destroy()
    da.destroy()


def test_timers(ctx):
    """the three passes are timed under their own names (pb_ctx_get_timing)"""
    n3 = (24, 20, 10)
    p, us = inputs(n3)
    da = pb.DA(ctx, n3)
    A = operator(da, "random", V.ARITHMETIC, n3, spacing(n3, None))
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        run_case(A, da, p, us, n3, None)
        ctx.sync()
        counts = {name: ctx.timing(name)[1] for name in ("mac_grad", "mac_project", "mac_div")}
    finally:
        ctx.set_timing(False)
    assert counts == {"mac_grad": 1, "mac_project": 2, "mac_div": 3}
    A.destroy()
    da.destroy()
