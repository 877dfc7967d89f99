"""GPU tier of PB_OP_VARCOEF, the variable-coefficient 7-point operator y = div(beta grad x),
against its numpy restatement (tests/varcoef_restatement.py, which defines it) and, under a
KSP, against the KSP restatements run on `VarProblem`.

The apply, the diagonal and every rank's slab must be bit-identical to the restatement: same
operations in the same order, every one rounded (no FMA contraction, the compiler's correctly
rounded fp64 division). The kernel picks its variants by nx's parity (two / one point per lane) and
ny's divisibility by 4 / 2 (rows per wave) alone -- it has no variant by plane size or row length
(no 8-row tiles, no residency cap), so the shapes are the issue's six and no 512x512x4 or
1024x1024x4 is added: 9x7x5 (odd x, 1 row), 17x12x9 (odd x, 4 rows), 24x20x10 (even x, 4 rows,
unequal deltas), 130x6x4 (two x segments, 2 rows), 256x8x3 (full segments, the smallest z) and 64^3
(several tiles and z-chunks).

Bars under a KSP: tests/parity_bars.py as the other KSP tiers use them -- HIST_RTOL (HIST_RTOL_PC
with sor / mg / fft), X_RTOL, exact reason and counts (where the restatement's last norms are
further than 1e-6 from ttol: ttol_margin_ok, asserted). fgmres and pipecg are more sensitive to the
summation order than CG (test_gpu_fgmres.py, test_gpu_pipecg.py): their bar is 100 x the spread of
the restatement itself between pairwise, sequential and exactly rounded sums on the case, never
below the CG bar, as those files derive theirs.

Every test here fails without the feature: operator kind 3 is PB_ERR_ARG.
"""
import functools

import numpy as np
import pytest

import poissbox_amd as pb
from oracle import oracle as O
import chebyshev_restatement as CR
import fgmres_restatement as FR
import ksp_types_restatement as KR
import norm_type_restatement as NR
import pipecg_restatement as PR
import varcoef_restatement as V
from ksp_types_restatement import ttol_margin_ok
from parity_bars import HIST_RTOL, HIST_RTOL_PC, X_RTOL, check_history, check_x
from test_gpu_ksp_types import FIXED, FIXED_KW, check

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED, STATE = 1, 5, 6
SEED = 20231015
MEANS = [V.ARITHMETIC, V.HARMONIC]
DELTAS = (0.05, 0.03, 0.07)
SHAPES = [((9, 7, 5), None), ((17, 12, 9), None), ((24, 20, 10), DELTAS), ((130, 6, 4), None),
          ((256, 8, 3), None), ((64, 64, 64), None)]


def spacing(n3, deltas):
    return tuple(deltas) if deltas else tuple(1.0 / m for m in n3)


def cut(v, n3, rows):
    return v if rows is None else v.reshape(n3[2], -1)[rows[0]:rows[0] + rows[1]].reshape(-1)


def vec_of(da, values):
    v = pb.Vec(da)
    v.set_values(values)
    return v


# ---------------------------------------------------------------------------------------------
# 1. the apply, 3. the diagonal
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n3,deltas", SHAPES, ids=[f"{s[0]}" for s in SHAPES])
def test_apply_and_diagonal_bit_identical(ctx, n3, deltas):
    h = spacing(n3, deltas)
    N = int(np.prod(n3))
    x = O.fill_random(N, SEED)
    da = pb.DA(ctx, n3)
    A = pb.Mat(da, pb.VARCOEF, h)
    xv, yv, bv = vec_of(da, x), pb.Vec(da), pb.Vec(da)
    # a fresh operator: beta = 1, arithmetic
    assert A.coefficient(bv) == V.ARITHMETIC and np.all(bv.get_values() == 1.0)
    A.mult(xv, yv)
    assert np.array_equal(yv.get_values(), V.apply(x, V.beta_one(n3), n3, h))
    for field in V.FIELDS:
        beta = V.FIELDS[field](n3)
        bv.set_values(beta)
        for mean in MEANS:
            A.set_coefficient(bv, mean)
            yv.set(7.25)
            A.mult(xv, yv)
            assert np.array_equal(yv.get_values(), V.apply(x, beta, n3, h, mean)), (field, mean)
            A.diagonal_vec(yv)
            assert np.array_equal(yv.get_values(), V.diag(beta, n3, h, mean)), (field, mean)
    # the coefficient reads back as set; constants are in the null space to the bit
    assert A.coefficient(yv) == V.HARMONIC and np.array_equal(yv.get_values(), beta)
    xv.set(-3.7)
    A.mult(xv, yv)
    assert np.all(yv.get_values() == 0.0)
    with pytest.raises(pb.PbError) as e:
        A.diagonal()
    assert e.value.code == UNSUPPORTED
    # the constant kinds: the scalar diagonal broadcast
    S = pb.Mat(da, pb.STAR7, h)
    S.diagonal_vec(yv)
    assert np.all(yv.get_values() == S.diagonal())
    for o in (A, S, xv, yv, bv):
        o.destroy()
    da.destroy()


def test_set_deltas(ctx):
    n3 = (17, 12, 9)
    x, beta = O.fill_random(int(np.prod(n3)), SEED), V.beta_random(n3)
    da = pb.DA(ctx, n3)
    A = pb.Mat(da, pb.VARCOEF)
    xv, yv, bv = vec_of(da, x), pb.Vec(da), vec_of(da, beta)
    A.set_coefficient(bv, V.HARMONIC)
    A.set_deltas(DELTAS)
    A.mult(xv, yv)
    assert np.array_equal(yv.get_values(), V.apply(x, beta, n3, DELTAS, V.HARMONIC))
    A.diagonal_vec(yv)
    assert np.array_equal(yv.get_values(), V.diag(beta, n3, DELTAS, V.HARMONIC))


# ---------------------------------------------------------------------------------------------
# 2. N ranks over the host transport: every slab bit-identical to the one-rank result
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks,n3", [(2, (16, 16, 12)), (3, (20, 16, 7)), (2, (16, 16, 4))])
def test_ranks_bit_identical(ctx, nranks, n3):
    from test_gpu_parity import run_ranks
    h = spacing(n3, None)
    N = int(np.prod(n3))
    x = O.fill_random(N, SEED)
    cases = [(f, m) for f in V.FIELDS for m in MEANS]

    def one(c, rows):
        da = pb.DA(c, n3)
        A = pb.Mat(da, pb.VARCOEF, h)
        xv, yv, bv = vec_of(da, cut(x, n3, rows)), pb.Vec(da), pb.Vec(da)
        out = []
        for field, mean in cases:
            bv.set_values(cut(V.FIELDS[field](n3), n3, rows))
            A.set_coefficient(bv, mean)
            A.mult(xv, yv)
            y = yv.get_values()
            A.diagonal_vec(yv)
            out.append((y, yv.get_values()))
        return out

    whole = one(ctx, None)
    for (field, mean), (y, d) in zip(cases, whole):
        beta = V.FIELDS[field](n3)
        assert np.array_equal(y, V.apply(x, beta, n3, h, mean))
        assert np.array_equal(d, V.diag(beta, n3, h, mean))

    def body(c, rank):
        rows = pb.slab_partition(n3[2], nranks, rank)
        return rows, one(c, rows)

    for rows, slabs in run_ranks(nranks, body):
        for (field, mean), (y, d), (yw, dw) in zip(cases, slabs, whole):
            assert np.array_equal(y, cut(yw, n3, rows)), (rows, field, mean)
            assert np.array_equal(d, cut(dw, n3, rows)), (rows, field, mean)


# ---------------------------------------------------------------------------------------------
# 4. validation
# ---------------------------------------------------------------------------------------------
def test_validation_leaves_the_operator_as_it_was(ctx):
    n3 = (17, 12, 9)
    h = spacing(n3, None)
    N = int(np.prod(n3))
    x, beta = O.fill_random(N, SEED), V.beta_random(n3)
    da, other = pb.DA(ctx, n3), pb.DA(ctx, (16, 12, 9))
    A = pb.Mat(da, pb.VARCOEF, h)
    xv, yv, bv, bad = vec_of(da, x), pb.Vec(da), vec_of(da, beta), pb.Vec(da)
    A.set_coefficient(bv, V.HARMONIC)
    want = V.apply(x, beta, n3, h, V.HARMONIC)
    for value in (np.nan, np.inf, 0.0, -1.0):
        b2 = V.beta_sphere(n3).copy()
        b2[N // 3] = value
        bad.set_values(b2)
        with pytest.raises(pb.PbError) as e:
            A.set_coefficient(bad, V.ARITHMETIC)
        assert e.value.code == ARG, value
    ov = pb.Vec(other)
    ov.set(1.0)
    with pytest.raises(pb.PbError) as e:
        A.set_coefficient(ov, V.ARITHMETIC)
    assert e.value.code == ARG
    bad.set_values(V.beta_sphere(n3))
    for mean in (2, -1):
        with pytest.raises(pb.PbError) as e:
            A.set_coefficient(bad, mean)
        assert e.value.code == ARG
    A.mult(xv, yv)
    assert np.array_equal(yv.get_values(), want)
    assert A.coefficient(yv) == V.HARMONIC and np.array_equal(yv.get_values(), beta)
    # another kind, and inside a solve that holds the operator: PB_ERR_STATE
    S = pb.Mat(da, pb.STAR7, h)
    for call in (lambda: S.set_coefficient(bv, V.ARITHMETIC), lambda: S.coefficient()):
        with pytest.raises(pb.PbError) as e:
            call()
        assert e.value.code == STATE
    k = pb.KSP(A, A, pb.ksp_options(["-pc_type", "jacobi"]))
    rhs = vec_of(da, want)
    k.begin(rhs, yv)
    with pytest.raises(pb.PbError) as e:
        A.set_coefficient(bad, V.ARITHMETIC)
    assert e.value.code == STATE
    k.iterate(2)
    k.end()
    A.set_coefficient(bad, V.ARITHMETIC)  # free again
    A.mult(xv, yv)
    assert np.array_equal(yv.get_values(), V.apply(x, V.beta_sphere(n3), n3, h, V.ARITHMETIC))
    k.destroy()


# ---------------------------------------------------------------------------------------------
# KSP: one solve on the GPU against a restated run
# ---------------------------------------------------------------------------------------------
def gpu_solve(ctx, prob, b, argv, rows=None, keep=None):
    """One solve on ctx; rows = (k0, nk): this rank's planes of the global arrays. Returns (reason,
    its, history, x, rnorm0, rnorm, nhist), test_gpu_ksp_types.gpu_solve's tuple."""
    da = pb.DA(ctx, prob.n3, prob.L)
    P, A = prob.mats(pb, da)
    x, bv = pb.Vec(da), vec_of(da, cut(b, prob.n3, rows))
    x.set(7.25)  # (a zero-guess solve must overwrite whatever x holds)
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", prob.pc_argv] + list(argv)))
    try:
        reason, its, hist = k.solve(bv, x)
        res = k.result
        return (reason, its, np.asarray(hist), x.get_values(), res.rnorm0, res.rnorm, res.nhist)
    finally:
        k.destroy()
        for o in {A, P, x, bv}:
            o.destroy()
        da.destroy()


def true_residual(prob, b, x):
    return float(np.linalg.norm(b - prob.apply(x)) / np.linalg.norm(b))


def check_cg(prob, got, want, tag):
    reason, its, hist, xs, rnorm0, rnorm, nhist = got
    xo, ro, itso, ho, ref = want
    print(f"{tag}: gpu reason {reason} its {its} | restated reason {ro} its {itso}")
    assert (reason, its, nhist) == (ro, itso, len(ho)) and len(hist) == nhist
    bar = HIST_RTOL_PC if prob.pc in ("sor", "mg", "fft") else HIST_RTOL
    print(f"{tag}: history difference {check_history(hist, ho, bar=bar, tag=tag):.3e} (bar {bar:.0e})")
    print(f"{tag}: x difference {check_x(xs, xo, tag=tag):.3e} (bar {X_RTOL:.0e})")
    assert abs(rnorm0 - ref) <= HIST_RTOL * ref and rnorm == hist[-1]


CG_PCS = ["none", "jacobi", "sor", "mg", "fft", "var-none", "vjacobi"]
CG_FIELDS = [("sphere", V.HARMONIC), ("random", V.ARITHMETIC)]


@functools.lru_cache(maxsize=None)
def cg_fixed_case(n3, pc, field, mean):
    """(problem, b, the restated 6 iterations): computed once per case."""
    p = "var" if pc in ("var-none", "vjacobi") else "const"
    prob = V.VarProblem(n3, V.FIELDS[field](n3), mean, pc="none" if pc == "var-none" else pc, p=p)
    b = prob.rhs()
    want = NR.cg(prob, b, max_it=6, **FIXED_KW)
    assert (want[1], want[2], len(want[3])) == (-3, 6, 7)
    return prob, b, want


# 5. CG, fixed 6 iterations, every (P, pc)
@pytest.mark.parametrize("field,mean", CG_FIELDS, ids=[f[0] for f in CG_FIELDS])
@pytest.mark.parametrize("pc", CG_PCS)
def test_cg_fixed_iterations(ctx, pc, field, mean):
    for n3 in [(32, 32, 32)] + ([(32, 40, 48)] if pc == "fft" else []):
        prob, b, want = cg_fixed_case(n3, pc, field, mean)
        got = gpu_solve(ctx, prob, b, FIXED + ["-ksp_max_it", "6"])
        check_cg(prob, got, want, f"cg {pc} {field} {n3}")


# 6. CG to a tolerance: the contrast-10 sphere at 32^3, harmonic
@pytest.mark.parametrize("pc", ["vjacobi", "mg", "fft"])
def test_cg_to_a_tolerance(ctx, pc):
    n3, rtol = (32, 32, 32), 1e-8
    prob = V.VarProblem(n3, V.beta_sphere(n3, inside=0.1), V.HARMONIC, pc=pc)
    b = prob.rhs()
    xo, ro, itso, ho, ref = NR.cg(prob, b, rtol=rtol)
    assert ro == 2 and ttol_margin_ok(ho, rtol, ref), "the restatement stops too close to ttol"
    reason, its, hist, xs, rnorm0, rnorm, nhist = gpu_solve(ctx, prob, b, ["-ksp_rtol", repr(rtol)])
    res_gpu, res_ref = true_residual(prob, b, xs), true_residual(prob, b, xo)
    print(f"cg rtol {pc}: gpu reason {reason} its {its} | restated {ro} {itso}; ||b - A x|| / ||b|| "
          f"gpu {res_gpu:.3e} restated {res_ref:.3e}")
    assert (reason, its, nhist) == (ro, itso, itso + 1)
    assert res_gpu <= 10 * res_ref


@pytest.mark.parametrize("norm", ["unpreconditioned", "natural", "none"])
def test_cg_norm_types_with_the_variable_jacobi(ctx, norm):
    """The variable Jacobi is a stored-z PC to the residual-sum stages: the unpreconditioned norm
    takes its sum r^2 where r is formed, as with sor / mg / fft."""
    prob, b, _ = cg_fixed_case((32, 32, 32), "vjacobi", "sphere", V.HARMONIC)
    want = NR.cg(prob, b, norm_type=norm, max_it=6, **FIXED_KW)
    got = gpu_solve(ctx, prob, b, FIXED + ["-ksp_max_it", "6", "-ksp_norm_type", norm])
    assert (got[0], got[1], got[6]) == (want[1], want[2], len(want[3]))
    if norm != "none":
        check_history(got[2], want[3], tag=f"cg vjacobi {norm}")
    check_x(got[3], want[0], tag=f"cg vjacobi {norm}")


def test_cg_single_reduction_runs_the_cg_iteration(ctx):
    prob, b, want = cg_fixed_case((32, 32, 32), "vjacobi", "sphere", V.HARMONIC)
    argv = FIXED + ["-ksp_max_it", "6"]
    a = gpu_solve(ctx, prob, b, argv)
    s = gpu_solve(ctx, prob, b, argv + ["-ksp_cg_single_reduction"])
    assert a[:2] == s[:2] and np.array_equal(a[2], s[2]) and np.array_equal(a[3], s[3])


# ---------------------------------------------------------------------------------------------
# 7. one case per other type
# ---------------------------------------------------------------------------------------------
N32 = (32, 32, 32)


def sphere_problem(pc, n3=N32):
    prob = V.VarProblem(n3, V.beta_sphere(n3), V.HARMONIC, pc=pc)
    return prob, prob.rhs()


def test_richardson_mg(ctx):
    prob, b = sphere_problem("mg")
    want = KR.richardson(prob, b, max_it=6, **FIXED_KW)
    got = gpu_solve(ctx, prob, b, ["-ksp_type", "richardson"] + FIXED + ["-ksp_max_it", "6"])
    check(prob, got, want, tag="richardson mg")


def test_chebyshev_variable_jacobi(ctx):
    prob, b = sphere_problem("vjacobi")
    want = CR.chebyshev(prob, b, 0.05, 2.0, max_it=6, **FIXED_KW)
    got = gpu_solve(ctx, prob, b, ["-ksp_type", "chebyshev", "-ksp_chebyshev_eigenvalues",
                                   "0.05,2.0"] + FIXED + ["-ksp_max_it", "6"])
    check(prob, got, want, tag="chebyshev vjacobi")


def sensitivity_bars(run, floor_hist):
    """(history bar, x bar) of a case: 100 x the largest difference between two of the
    restatement's own runs under pairwise, sequential and exactly rounded sums, never below the CG
    bars; and the pairwise run."""
    outs = {s: run(s) for s in ("pairwise", "sequential", "exact")}
    assert len({(o[1], o[2]) for o in outs.values()}) == 1, "the variants end differently"
    dh = dx = 0.0
    for a in outs.values():
        for c in outs.values():
            dh = max(dh, float(np.max(np.abs(a[3] - c[3]) / c[3])))
            dx = max(dx, float(np.max(np.abs(a[0] - c[0])) / np.max(np.abs(c[0]))))
    return max(100 * dh, floor_hist), max(100 * dx, X_RTOL), outs["pairwise"]


def check_sensitive(got, want, hbar, xbar, tag):
    reason, its, hist, xs, rnorm0, rnorm, nhist = got
    xo, ro, itso, ho, ref = want
    print(f"{tag}: gpu reason {reason} its {its} | restated {ro} {itso}; bars history {hbar:.2e} "
          f"x {xbar:.2e}")
    assert (reason, its, nhist) == (ro, itso, len(ho))
    print(f"{tag}: history difference {check_history(hist, ho, bar=hbar, tag=tag):.3e}")
    print(f"{tag}: x difference {check_x(xs, xo, bar=xbar, tag=tag):.3e}")
    assert abs(rnorm0 - ref) <= HIST_RTOL * ref and rnorm == hist[-1]


def test_fgmres_fft(ctx):
    prob, b = sphere_problem("fft")
    hbar, xbar, want = sensitivity_bars(
        lambda s: FR.fgmres(prob, b, restart=3, max_it=7, sums=s, **FIXED_KW), HIST_RTOL_PC)
    got = gpu_solve(ctx, prob, b, ["-ksp_type", "fgmres", "-ksp_gmres_restart", "3"] + FIXED
                    + ["-ksp_max_it", "7"])
    check_sensitive(got, want, hbar, xbar, "fgmres fft")


def test_pipecg_variable_jacobi(ctx):
    prob, b = sphere_problem("vjacobi")
    hbar, xbar, want = sensitivity_bars(
        lambda s: PR.pipecg(prob, b, max_it=6, sums=s, **FIXED_KW), HIST_RTOL)
    got = gpu_solve(ctx, prob, b, ["-ksp_type", "pipecg"] + FIXED + ["-ksp_max_it", "6"])
    check_sensitive(got, want, hbar, xbar, "pipecg vjacobi")


def test_preonly_fft(ctx):
    prob, b = sphere_problem("fft")
    want = KR.preonly(prob, b)
    reason, its, hist, xs, rnorm0, rnorm, nhist = gpu_solve(ctx, prob, b, ["-ksp_type", "preonly"])
    assert (reason, its, rnorm, rnorm0, nhist) == (4, 1, 0.0, 0.0, 0)
    check_x(xs, want[0], tag="preonly fft")


def test_preonly_variable_jacobi(ctx):
    prob, b = sphere_problem("vjacobi")
    want = KR.preonly(prob, b + 0.5)
    got = gpu_solve(ctx, prob, b + 0.5, ["-ksp_type", "preonly"])
    assert got[:2] == (4, 1)
    check_x(got[3], want[0], tag="preonly vjacobi")


# ---------------------------------------------------------------------------------------------
# 8. p . Ap taken by the operator's own pass (tuning varcoef_dot_fused)
# ---------------------------------------------------------------------------------------------
def _dot_runs(c, prob, b, rows, tune):
    out = {}
    for fused in (0, 1):
        tune.set("varcoef_dot_fused", fused)
        c.reset_timing()
        c.set_timing(True)
        got = gpu_solve(c, prob, b, FIXED + ["-ksp_max_it", "6"], rows=rows)
        c.set_timing(False)
        out[fused] = (got, c.timing("cg_gen_dot")[1], c.timing("cg_gen_p")[1])
    return out


def _check_dot(out, prob, want, rows, tag):
    (g0, dot0, p0), (g1, dot1, p1) = out[0], out[1]
    print(f"{tag}: cg_gen_dot launches unfused {dot0} fused {dot1}; iterations enqueued {p0}")
    assert g0[:2] == g1[:2] == (want[1], want[2]) and g0[6] == g1[6]
    check_history(g1[2], g0[2], tag=tag)
    check_history(g1[2], want[3], tag=tag)
    check_x(g1[3], cut(want[0], prob.n3, rows), scale=float(np.max(np.abs(want[0]))), tag=tag)
    # one launch fewer per iteration enqueued: the dot kernel is gone
    assert p0 == p1 >= 6 and dot0 == p0 and dot1 == 0


@pytest.mark.parametrize("pc", ["vjacobi", "var-none", "mg"])
def test_fused_dot_one_rank(ctx, tune, pc):
    prob, b, want = cg_fixed_case((32, 32, 32), pc, "sphere", V.HARMONIC)
    _check_dot(_dot_runs(ctx, prob, b, None, tune), prob, want, None, f"fused dot {pc}")


@pytest.mark.parametrize("n3", [(16, 16, 12), (16, 16, 4)])
def test_fused_dot_two_ranks(tune, n3):
    """Under halo_overlap's split launches (interior, then the boundary planes behind it) and the
    single launch of a slab of fewer than three planes."""
    from test_gpu_parity import run_ranks
    prob, b, want = cg_fixed_case(n3, "vjacobi", "random", V.ARITHMETIC)
    results = {}
    for fused in (0, 1):
        tune.set("varcoef_dot_fused", fused)

        def body(c, rank):
            rows = pb.slab_partition(n3[2], 2, rank)
            c.set_timing(True)
            got = gpu_solve(c, prob, b, FIXED + ["-ksp_max_it", "6"], rows=rows)
            return rows, (got, c.timing("cg_gen_dot")[1], c.timing("cg_gen_p")[1])

        results[fused] = run_ranks(2, body)
    for (rows, r0), (_, r1) in zip(results[0], results[1]):
        _check_dot({0: r0, 1: r1}, prob, want, rows, f"fused dot 2 ranks {n3} rows {rows}")


# ---------------------------------------------------------------------------------------------
# 9. a KSP reused after pb_op_set_coefficient / pb_op_set_deltas behaves as a fresh one
# ---------------------------------------------------------------------------------------------
def _reuse(c, rows, argv):
    n3 = (16, 16, 12)
    h = spacing(n3, None)
    beta1, beta2 = V.beta_sphere(n3), V.beta_random(n3)
    b = V.apply(O.fill_random(int(np.prod(n3)), SEED), beta2, n3, h, V.HARMONIC)
    da = pb.DA(c, n3)
    bv, x, coef = vec_of(da, cut(b, n3, rows)), pb.Vec(da), pb.Vec(da)
    opts = pb.ksp_options(["-pc_type", "jacobi", "-ksp_rtol", "1e-8"] + argv)

    def solve(k):
        x.set(7.25)
        reason, its, hist = k.solve(bv, x)
        return reason, its, np.asarray(hist), x.get_values()

    A = pb.Mat(da, pb.VARCOEF, h)
    coef.set_values(cut(beta1, n3, rows))
    A.set_coefficient(coef, V.ARITHMETIC)
    k = pb.KSP(A, A, opts)
    first = solve(k)
    coef.set_values(cut(beta2, n3, rows))
    A.set_coefficient(coef, V.HARMONIC)
    again = solve(k)
    A.set_deltas(DELTAS)
    scaled = solve(k)
    k.destroy()
    F = pb.Mat(da, pb.VARCOEF, h)
    F.set_coefficient(coef, V.HARMONIC)
    kf = pb.KSP(F, F, opts)
    fresh = solve(kf)
    kf.destroy()
    G = pb.Mat(da, pb.VARCOEF, DELTAS)
    G.set_coefficient(coef, V.HARMONIC)
    kg = pb.KSP(G, G, opts)
    fresh_scaled = solve(kg)
    kg.destroy()
    return first, again, fresh, scaled, fresh_scaled


def _same(a, c):
    return a[:2] == c[:2] and np.array_equal(a[2], c[2]) and np.array_equal(a[3], c[3])


@pytest.mark.parametrize("ksp", ["cg", "richardson", "chebyshev"])
def test_reuse_after_set_coefficient(ctx, ksp):
    """(chebyshev: with estimated bounds, which belong to the coefficient they were estimated for)"""
    argv = ["-ksp_type", ksp] + {"richardson": ["-ksp_richardson_scale", "0.6", "-ksp_max_it", "40"],
                                 "chebyshev": ["-ksp_max_it", "40"]}.get(ksp, [])
    first, again, fresh, scaled, fresh_scaled = _reuse(ctx, None, argv)
    assert _same(again, fresh) and not np.array_equal(first[3], again[3])
    assert _same(scaled, fresh_scaled) and not np.array_equal(scaled[3], again[3])
    if ksp == "cg":
        assert again[0] == 2


def test_reuse_after_set_coefficient_two_ranks():
    from test_gpu_parity import run_ranks

    def body(c, rank):
        return _reuse(c, pb.slab_partition(12, 2, rank), ["-ksp_type", "cg"])

    for first, again, fresh, scaled, fresh_scaled in run_ranks(2, body):
        assert _same(again, fresh) and again[0] == 2
        assert _same(scaled, fresh_scaled)


# ---------------------------------------------------------------------------------------------
# 10. refusals
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["sor", "mg", "fft"])
def test_variable_p_refuses_sor_mg_fft(ctx, pc):
    da = pb.DA(ctx, (32, 32, 32))
    A = pb.Mat(da, pb.VARCOEF)
    with pytest.raises(pb.PbError) as e:
        pb.KSP(A, A, pb.ksp_options(["-pc_type", pc]))
    assert e.value.code == UNSUPPORTED
    assert "constant-coefficient P" in str(e.value) and "PB_OP_STAR7" in str(e.value)
    with pytest.raises(pb.PbError) as e:
        pb.KSP(A, None, pb.ksp_options(["-pc_type", pc]))  # P omitted: P = A
    assert e.value.code == UNSUPPORTED
    # the same PC from a constant P is the supported pairing
    P = pb.Mat(da, pb.STAR7)
    pb.KSP(A, P, pb.ksp_options(["-pc_type", pc])).destroy()
    for o in (A, P):
        o.destroy()
    da.destroy()
