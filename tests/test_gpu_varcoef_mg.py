"""GPU tier of the variable-coefficient -pc_type sor | mg (pb_ksp_pc_set_coefficient_from) against
its numpy restatement (tests/varcoef_mg_restatement.py, which defines it).

The preconditioner apply and every rank's slab must be bit-identical to the restatement: the same
operations in the same order, every one rounded (no FMA contraction, correctly rounded fp64
division). The kernels' variants, all covered by test_mg_apply_bit_identical,
test_sor_apply_bit_identical and test_variants_give_equal_bits:
  - the face mean (arithmetic | harmonic) in every kernel;
  - the half-sweep: from zero (a pair store, x not read) | in place; dinv stored | formed from the
    six faces (tuning mg_varcoef_dinv_stored); one plane per thread | a chunk of planes marched
    with a register queue (by the level's size; tuning mg_varcoef_kc forces chunks of 3 planes on
    16x12x8, whose last chunk is short, and of 5 on 24x20x16 -- without it only levels of more than
    256 Ki pair-planes march, 128x128x64 here);
  - the zero-start red + black pass | two launches (tuning mg_varcoef_pre_fused);
  - the residual: the operator's kernel, which picks by nx's parity and ny's divisibility by 4
    alone -- every level that has a residual has both extents divisible by 4, one variant;
  - the coarsening kernel and the transfers have none.
Shapes: the issue's (8^3: 2 levels, the smallest; 16x12x8: 2 levels, unequal extents; 24x20x16 with
deltas; 32^3: 4 levels; 64^3: several blocks per plane; 10x6x4 for sor: even, not a multiple of 4).

Bars under a KSP: tests/parity_bars.py as tests/test_gpu_varcoef.py uses them.

Every test here fails without the feature: the entry point does not exist.
"""
import functools

import numpy as np
import pytest

import poissbox_amd as pb
from oracle import oracle as O
import chebyshev_restatement as CR
import fgmres_restatement as FR
import ksp_types_restatement as KR
import mg_smoothers_restatement as M
import norm_type_restatement as NR
import pipecg_restatement as PR
import varcoef_mg_restatement as VM
import varcoef_restatement as V
from ksp_types_restatement import ttol_margin_ok
from parity_bars import HIST_RTOL, HIST_RTOL_PC
from test_gpu_ksp_types import FIXED, FIXED_KW, check
from test_gpu_varcoef import (check_cg, check_sensitive, cut, sensitivity_bars, spacing,
                              true_residual, vec_of)

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED, STATE = 1, 5, 6
SEED = 20231015
MEANS = [V.ARITHMETIC, V.HARMONIC]
DELTAS = (0.05, 0.03, 0.07)
FIELD_MEANS = [(f, m) for f in V.FIELDS for m in MEANS]
MG_SHAPES = [((8, 8, 8), None), ((16, 12, 8), None), ((24, 20, 16), DELTAS), ((32, 32, 32), None),
             ((64, 64, 64), None)]
SOR_SHAPES = MG_SHAPES + [((10, 6, 4), None)]
LEVELS = {(8, 8, 8): 2, (16, 12, 8): 2, (24, 20, 16): 2, (32, 32, 32): 4, (64, 64, 64): 5}


@functools.lru_cache(maxsize=None)
def rhs(n3):
    r = O.fill_random(int(np.prod(n3)), SEED)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def restated_apply(n3, deltas, pc, field, mean, nu=1, omega=1.0):
    vc = VM.VarVCycle(n3, spacing(n3, deltas), V.FIELDS[field](n3), mean, M.Smoother(nu=nu),
                      omega=omega, pc=pc)
    z = vc.apply(rhs(n3))
    z.setflags(write=False)
    return vc.L, z


def pc_argv(pc, nu=1, omega=1.0):
    argv = ["-pc_type", pc]
    if nu != 1:
        argv += M.Smoother(nu=nu).argv()
    if omega != 1.0:
        argv += ["-pc_sor_omega", repr(omega)]
    return argv


def gpu_applies(ctx, n3, deltas, argv, cases, rows=None, each=None):
    """pb_ksp_pc_apply of one KSP with its coefficient from A, for every (field, mean) of cases:
    [(levels, z)]. rows = (k0, nk): this rank's planes. each(k): called before every apply."""
    h = spacing(n3, deltas)
    da = pb.DA(ctx, n3)
    P, A = pb.Mat(da, pb.ASSEMBLED27, h), pb.Mat(da, pb.VARCOEF, h)
    rv, zv, bv = vec_of(da, cut(rhs(n3), n3, rows)), pb.Vec(da), pb.Vec(da)
    k = pb.KSP(A, P, pb.ksp_options(argv))
    out = []
    try:
        k.pc_set_coefficient_from(A)
        assert k.pc_coefficient_from() is A
        for field, mean in cases:
            bv.set_values(cut(V.FIELDS[field](n3), n3, rows))
            A.set_coefficient(bv, mean)
            zv.set(7.25)
            if each:
                each(k)
            k.pc_apply(rv, zv)
            out.append((k.pc_levels, zv.get_values()))
        return out
    finally:
        k.destroy()
        for o in (A, P, rv, zv, bv):
            o.destroy()
        da.destroy()


# ---------------------------------------------------------------------------------------------
# 1. the apply against the restatement
# ---------------------------------------------------------------------------------------------
def _check_applies(got, n3, deltas, pc, nu=1, omega=1.0):
    for (field, mean), (levels, z) in zip(FIELD_MEANS, got):
        L, want = restated_apply(n3, deltas, pc, field, mean, nu, omega)
        diff = float(np.max(np.abs(z - want)) / np.max(np.abs(want)))
        print(f"{pc} {n3} {field} mean {mean} nu {nu} omega {omega}: levels {levels}, max relative "
              f"difference {diff:.3e}")
        assert levels == L
        assert np.array_equal(z, want), (field, mean, diff)


@pytest.mark.parametrize("n3,deltas", MG_SHAPES, ids=[f"{s[0]}" for s in MG_SHAPES])
def test_mg_apply_bit_identical(ctx, n3, deltas):
    got = gpu_applies(ctx, n3, deltas, pc_argv("mg"), FIELD_MEANS)
    assert got[0][0] == LEVELS[n3]
    _check_applies(got, n3, deltas, "mg")


@pytest.mark.parametrize("n3,deltas", SOR_SHAPES, ids=[f"{s[0]}" for s in SOR_SHAPES])
def test_sor_apply_bit_identical(ctx, n3, deltas):
    got = gpu_applies(ctx, n3, deltas, pc_argv("sor"), FIELD_MEANS)
    assert got[0][0] == 1
    _check_applies(got, n3, deltas, "sor")


@pytest.mark.parametrize("pc,nu,omega", [("mg", 2, 1.3), ("mg", 3, 1.0), ("sor", 1, 1.3)])
def test_omega_and_sweep_count(ctx, pc, nu, omega):
    for n3, deltas in (((16, 12, 8), None), ((24, 20, 16), DELTAS)):
        got = gpu_applies(ctx, n3, deltas, pc_argv(pc, nu, omega), FIELD_MEANS)
        _check_applies(got, n3, deltas, pc, nu, omega)


def test_variants_give_equal_bits(ctx, tune):
    """mg_varcoef_pre_fused 0 and 1, dinv stored and formed, marched chunks of planes: the bits
    of the restatement every time."""
    for n3, deltas, kc in (((16, 12, 8), None, 3), ((24, 20, 16), DELTAS, 5)):
        for tuning in ({"mg_varcoef_pre_fused": 0}, {"mg_varcoef_pre_fused": 1},
                       {"mg_varcoef_dinv_stored": 1}, {"mg_varcoef_kc": kc},
                       {"mg_varcoef_kc": kc, "mg_varcoef_pre_fused": 0,
                        "mg_varcoef_dinv_stored": 1}):
            pb.tune_reset()
            for name, v in tuning.items():
                tune.set(name, v)
            for pc, nu in (("mg", 2), ("sor", 1)):
                got = gpu_applies(ctx, n3, deltas, pc_argv(pc, nu, 1.3), FIELD_MEANS)
                _check_applies(got, n3, deltas, pc, nu, 1.3)


def test_marched_chunks_on_a_large_level(ctx, tune):
    """128x128x64: 8192 columns of pairs, 32 chunks of 2 planes by the launcher's own choice. The
    restatement of this size takes too long for the suite; the reference is the same library with
    one plane per thread (whose bits the small shapes pin), both means."""
    n3 = (128, 128, 64)
    cases = [("random", V.ARITHMETIC), ("sphere", V.HARMONIC)]
    marched = gpu_applies(ctx, n3, None, pc_argv("mg"), cases)
    tune.set("mg_varcoef_kc", 1)
    single = gpu_applies(ctx, n3, None, pc_argv("mg"), cases)
    for (_, a), (_, c) in zip(marched, single):
        assert np.all(np.isfinite(a)) and np.array_equal(a, c)


# ---------------------------------------------------------------------------------------------
# 2. N ranks over the host transport: every slab bit-identical to the one-rank apply
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks,n3,levels", [(2, (16, 16, 16), 3), (3, (16, 16, 12), 2)])
def test_ranks_bit_identical(ctx, nranks, n3, levels):
    from test_gpu_parity import run_ranks
    whole = {pc: gpu_applies(ctx, n3, None, pc_argv(pc, nu, 1.3), FIELD_MEANS)
             for pc, nu in (("mg", 2), ("sor", 1))}
    assert whole["mg"][0][0] == levels
    _check_applies(whole["mg"], n3, None, "mg", 2, 1.3)

    def body(c, rank):
        rows = pb.slab_partition(n3[2], nranks, rank)
        return rows, {pc: gpu_applies(c, n3, None, pc_argv(pc, nu, 1.3), FIELD_MEANS, rows=rows)
                      for pc, nu in (("mg", 2), ("sor", 1))}

    for rows, slabs in run_ranks(nranks, body):
        for pc in slabs:
            for case, (lv, z), (lw, zw) in zip(FIELD_MEANS, slabs[pc], whole[pc]):
                assert lv == lw
                assert np.array_equal(z, cut(zw, n3, rows)), (pc, rows, case)


# ---------------------------------------------------------------------------------------------
# KSP: one solve on the GPU against a restated run
# ---------------------------------------------------------------------------------------------
def gpu_solve(ctx, prob, b, argv, before=False):
    """One solve on ctx with prob's hook applied to the KSP (before: also the solve of the same KSP
    before the hook, returned second). Returns test_gpu_ksp_types.gpu_solve's tuple."""
    da = pb.DA(ctx, prob.n3, prob.L)
    P, A = prob.mats(pb, da)
    x, bv = pb.Vec(da), vec_of(da, b)
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", prob.pc_argv] + list(argv)))

    def solve():
        x.set(7.25)  # (a zero-guess solve must overwrite whatever x holds)
        reason, its, hist = k.solve(bv, x)
        res = k.result
        return (reason, its, np.asarray(hist), x.get_values(), res.rnorm0, res.rnorm, res.nhist)

    try:
        first = solve() if before else None
        prob.after_create(k, P, A)
        got = solve()
        return (got, first) if before else got
    finally:
        k.destroy()
        for o in {A, P, x, bv}:
            o.destroy()
        da.destroy()


N32 = (32, 32, 32)
CG_FIELDS = [("sphere", V.HARMONIC), ("random", V.ARITHMETIC)]


@functools.lru_cache(maxsize=None)
def problem(pc, field, mean, inside=None):
    beta = V.beta_sphere(N32, inside=inside) if inside is not None else V.FIELDS[field](N32)
    prob = VM.VarMgProblem(N32, beta, mean, pc=pc)
    return prob, prob.rhs()


# 3. CG, fixed 6 iterations
@pytest.mark.parametrize("field,mean", CG_FIELDS, ids=[f[0] for f in CG_FIELDS])
@pytest.mark.parametrize("pc", ["vmg", "vsor"])
def test_cg_fixed_iterations(ctx, pc, field, mean):
    prob, b = problem(pc, field, mean)
    want = NR.cg(prob, b, max_it=6, **FIXED_KW)
    assert (want[1], want[2], len(want[3])) == (-3, 6, 7)
    got = gpu_solve(ctx, prob, b, FIXED + ["-ksp_max_it", "6"])
    check_cg(prob, got, want, f"cg {pc} {field}")


def test_richardson(ctx):
    prob, b = problem("vmg", "sphere", V.HARMONIC)
    want = KR.richardson(prob, b, max_it=6, **FIXED_KW)
    got = gpu_solve(ctx, prob, b, ["-ksp_type", "richardson"] + FIXED + ["-ksp_max_it", "6"])
    check(prob, got, want, tag="richardson vmg")


def test_chebyshev_given_bounds(ctx):
    prob, b = problem("vmg", "random", V.ARITHMETIC)
    want = CR.chebyshev(prob, b, 0.1, 1.1, max_it=6, **FIXED_KW)
    got = gpu_solve(ctx, prob, b, ["-ksp_type", "chebyshev", "-ksp_chebyshev_eigenvalues",
                                   "0.1,1.1"] + FIXED + ["-ksp_max_it", "6"])
    check(prob, got, want, tag="chebyshev vmg")


def test_fgmres(ctx):
    prob, b = problem("vmg", "sphere", V.HARMONIC)
    hbar, xbar, want = sensitivity_bars(
        lambda s: FR.fgmres(prob, b, restart=3, max_it=7, sums=s, **FIXED_KW), HIST_RTOL_PC)
    got = gpu_solve(ctx, prob, b, ["-ksp_type", "fgmres", "-ksp_gmres_restart", "3"] + FIXED
                    + ["-ksp_max_it", "7"])
    check_sensitive(got, want, hbar, xbar, "fgmres vmg")


def test_pipecg(ctx):
    prob, b = problem("vsor", "random", V.ARITHMETIC)
    hbar, xbar, want = sensitivity_bars(
        lambda s: PR.pipecg(prob, b, max_it=6, sums=s, **FIXED_KW), HIST_RTOL_PC)
    got = gpu_solve(ctx, prob, b, ["-ksp_type", "pipecg"] + FIXED + ["-ksp_max_it", "6"])
    check_sensitive(got, want, hbar, xbar, "pipecg vsor")


# 4. CG to a tolerance: the contrast-10 sphere at 32^3, harmonic
def test_cg_to_a_tolerance(ctx):
    rtol = 1e-8
    prob, b = problem("vmg", "sphere", V.HARMONIC, inside=0.1)
    xo, ro, itso, ho, ref = NR.cg(prob, b, rtol=rtol)
    assert ro == 2 and ttol_margin_ok(ho, rtol, ref), "the restatement stops too close to ttol"
    got, const = gpu_solve(ctx, prob, b, ["-ksp_rtol", repr(rtol)], before=True)
    reason, its, hist, xs, rnorm0, rnorm, nhist = got
    res_gpu, res_ref = true_residual(prob, b, xs), true_residual(prob, b, xo)
    print(f"cg rtol vmg: gpu reason {reason} its {its} | restated {ro} {itso}; before the call "
          f"{const[0]} {const[1]}; ||b - A x|| / ||b|| gpu {res_gpu:.3e} restated {res_ref:.3e}")
    assert (reason, its, nhist) == (ro, itso, itso + 1)
    assert res_gpu <= 10 * res_ref
    assert const[0] == 2 and its < const[1]


# ---------------------------------------------------------------------------------------------
# 5. a KSP reused after pb_op_set_coefficient / pb_op_set_deltas behaves as a fresh one; NULL
#    returns to the constant-coefficient PC
# ---------------------------------------------------------------------------------------------
def _same(a, c):
    return a[:2] == c[:2] and np.array_equal(a[2], c[2]) and np.array_equal(a[3], c[3])


@pytest.mark.parametrize("pc", ["mg", "sor"])
def test_reuse_and_unset(ctx, pc):
    n3 = (16, 16, 16)
    h = spacing(n3, None)
    beta1, beta2 = V.beta_sphere(n3), V.beta_random(n3)
    b = V.apply(O.fill_random(int(np.prod(n3)), SEED), beta2, n3, h, V.HARMONIC)
    da = pb.DA(ctx, n3)
    bv, x, coef = vec_of(da, b), pb.Vec(da), pb.Vec(da)
    opts = pb.ksp_options(["-pc_type", pc, "-ksp_rtol", "1e-8"])

    def solve(k):
        x.set(7.25)
        reason, its, hist = k.solve(bv, x)
        return reason, its, np.asarray(hist), x.get_values()

    P = pb.Mat(da, pb.STAR7, h)
    A = pb.Mat(da, pb.VARCOEF, h)
    coef.set_values(beta1)
    A.set_coefficient(coef, V.ARITHMETIC)
    k = pb.KSP(A, P, opts)
    const1 = solve(k)
    k.pc_set_coefficient_from(A)
    first = solve(k)
    coef.set_values(beta2)
    A.set_coefficient(coef, V.HARMONIC)
    again = solve(k)
    A.set_deltas(DELTAS)
    scaled = solve(k)
    k.pc_set_coefficient_from(None)
    assert k.pc_coefficient_from() is None
    unset = solve(k)
    k.destroy()

    F = pb.Mat(da, pb.VARCOEF, h)
    F.set_coefficient(coef, V.HARMONIC)
    kf = pb.KSP(F, P, opts)
    kf.pc_set_coefficient_from(F)
    fresh = solve(kf)
    kf.destroy()
    G = pb.Mat(da, pb.VARCOEF, DELTAS)
    G.set_coefficient(coef, V.HARMONIC)
    kg = pb.KSP(G, P, opts)
    fresh_const = solve(kg)  # the constant-coefficient PC of P on the scaled operator
    kg.pc_set_coefficient_from(G)
    fresh_scaled = solve(kg)
    kg.destroy()
    assert _same(again, fresh) and not np.array_equal(first[3], again[3]) and again[0] == 2
    assert _same(scaled, fresh_scaled) and not np.array_equal(scaled[3], again[3])
    assert _same(unset, fresh_const) and not np.array_equal(unset[3], scaled[3])
    assert not np.array_equal(const1[2], first[2])


# ---------------------------------------------------------------------------------------------
# 6. refusals and state
# ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_ksp_as_it_was(ctx):
    n3 = (32, 32, 32)  # (the smallest extent -pc_type fft takes)
    h = spacing(n3, None)
    da, other = pb.DA(ctx, n3), pb.DA(ctx, (32, 32, 16))
    P, S = pb.Mat(da, pb.ASSEMBLED27, h), pb.Mat(da, pb.STAR7, h)
    A, B, Q = pb.Mat(da, pb.VARCOEF, h), pb.Mat(da, pb.VARCOEF, h), pb.Mat(other, pb.VARCOEF)
    bv = vec_of(da, V.beta_random(n3))
    A.set_coefficient(bv, V.HARMONIC)
    B.set_coefficient(bv, V.ARITHMETIC)
    rv, zv = vec_of(da, rhs(n3)), pb.Vec(da)

    def raises(code, call):
        with pytest.raises(pb.PbError) as e:
            call()
        assert e.value.code == code, (e.value.code, str(e.value))

    def apply(k):
        zv.set(7.25)
        k.pc_apply(rv, zv)
        return zv.get_values()

    # a variable P is refused as before
    raises(UNSUPPORTED, lambda: pb.KSP(A, A, pb.ksp_options(["-pc_type", "mg"])))
    # the other PCs: PB_ERR_STATE
    for pc in ("fft", "jacobi", "none"):
        k = pb.KSP(A, S, pb.ksp_options(["-pc_type", pc]))
        z0 = apply(k)
        raises(STATE, lambda: k.pc_set_coefficient_from(A))
        assert k.pc_coefficient_from() is None and np.array_equal(apply(k), z0)
        k.destroy()
    for pc in ("mg", "sor"):
        k = pb.KSP(A, P, pb.ksp_options(["-pc_type", pc]))
        z_const = apply(k)
        # another kind, another grid
        raises(ARG, lambda: k.pc_set_coefficient_from(S))
        raises(ARG, lambda: k.pc_set_coefficient_from(Q))
        assert k.pc_coefficient_from() is None and np.array_equal(apply(k), z_const)
        k.pc_set_coefficient_from(A)
        z_var = apply(k)
        assert not np.array_equal(z_var, z_const)
        raises(ARG, lambda: k.pc_set_coefficient_from(Q))
        assert k.pc_coefficient_from() is A and np.array_equal(apply(k), z_var)
        # inside a solve: the call is PB_ERR_STATE, and the KSP holds C (here another operator than
        # A and P)
        k.pc_set_coefficient_from(B)
        z_b = apply(k)
        x = pb.Vec(da)
        k.begin(rv, x)
        raises(STATE, lambda: k.pc_set_coefficient_from(A))
        raises(STATE, lambda: k.pc_set_coefficient_from(None))
        raises(STATE, lambda: B.set_coefficient(bv, V.HARMONIC))
        raises(STATE, lambda: A.set_coefficient(bv, V.ARITHMETIC))
        k.iterate(2)
        k.end()
        B.set_coefficient(bv, V.ARITHMETIC)  # free again
        assert k.pc_coefficient_from() is B and np.array_equal(apply(k), z_b)
        x.destroy()
        k.destroy()
    # a Jacobi-type level smoother and a coefficient, in either order
    jac = pb.pc_mg_options(levels_ksp_type=pb.MG_LEVELS_CHEBYSHEV,
                           levels_pc_type=pb.MG_LEVELS_JACOBI, levels_ksp_max_it=2)
    sor3 = pb.pc_mg_options(levels_ksp_max_it=3)
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", "mg"]))
    k.pc_mg_set_opts(jac)
    z_jac = apply(k)
    raises(UNSUPPORTED, lambda: k.pc_set_coefficient_from(A))
    assert k.pc_coefficient_from() is None and np.array_equal(apply(k), z_jac)
    k.pc_mg_set_opts(sor3)
    k.pc_set_coefficient_from(A)
    z3 = apply(k)
    raises(UNSUPPORTED, lambda: k.pc_mg_set_opts(jac))
    assert k.pc_mg_get_opts().levels_pc_type == pb.MG_LEVELS_SOR
    assert k.pc_mg_get_opts().levels_ksp_max_it == 3 and np.array_equal(apply(k), z3)
    k.destroy()
    for o in (P, S, A, B, Q, bv, rv, zv):
        o.destroy()
    other.destroy()
    da.destroy()
