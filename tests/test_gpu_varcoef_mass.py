"""GPU tier of the mass term of PB_OP_VARCOEF (pb_op_set_mass: A = div(beta grad) - s m) against
its numpy restatement (tests/varcoef_mass_restatement.py, which defines it): the
apply, the diagonal, every rank's slab and the apply of the variable sor / mg preconditioner must be
bit-identical to the restatement -- the same operations in the same order, every one rounded.

Shapes of the apply: test_gpu_varcoef.py's six -- the kernel still picks its variants by nx's
parity and ny's divisibility by 4 / 2 alone, and the mass adds one variant axis (none | scalar |
field) that every shape runs. Shapes of the preconditioner: 16^3 (3 levels) and 24x20x16 with
unequal deltas (2 levels), under the four settings of (mg_varcoef_dinv_stored,
mg_varcoef_pre_fused).

Bars under a KSP: tests/parity_bars.py as tests/test_gpu_varcoef.py uses them -- HIST_RTOL_PC with
sor / mg, HIST_RTOL with the variable Jacobi, X_RTOL, exact reason and counts (the restatement's
last norms are further than 1e-6 from ttol: ttol_margin_ok, asserted). chebyshev (estimated
bounds), fgmres and pipecg: a converged reason and the true residual ||b - A x|| / ||b|| <=
10 rtol from the restatement's apply.

Every test here fails without the feature: pb_op_set_mass does not exist.
"""
import functools

import numpy as np
import pytest

import poissbox_amd as pb
from oracle import oracle as O
import ksp_types_restatement as KR
import mg_smoothers_restatement as M
import norm_type_restatement as NR
import varcoef_mass_restatement as VMS
import varcoef_restatement as V
from ksp_types_restatement import ttol_margin_ok
from parity_bars import HIST_RTOL, HIST_RTOL_PC, X_RTOL, check_history, check_x
from test_gpu_varcoef import SHAPES, cut, spacing, vec_of
from test_gpu_varcoef_mg import pc_argv, rhs

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 6
SEED = 20231015
MEANS = [V.ARITHMETIC, V.HARMONIC]
DELTAS = (0.05, 0.03, 0.07)
PC_SHAPES = [((16, 16, 16), None), ((24, 20, 16), DELTAS)]
RTOL = 1e-8


def masses(n3):
    """(name, m, s): scalar, field, the field zeroed on the lower half in z"""
    m = VMS.mass_uniform(n3)
    half = m.copy().reshape(n3[2], -1)
    half[:n3[2] // 2] = 0.0
    return [("scalar", None, 37.5), ("field", m, 100.0), ("half", half.reshape(-1), 100.0)]


def set_mass(da, A, m, s, n3, rows=None):
    if m is None:
        A.set_mass(None, s)
        return
    mv = vec_of(da, cut(m, n3, rows))
    A.set_mass(mv, s)
    mv.destroy()


# ---------------------------------------------------------------------------------------------
# 1. the apply and the diagonal
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n3,deltas", SHAPES, ids=[f"{s[0]}" for s in SHAPES])
def test_apply_and_diagonal_bit_identical(ctx, n3, deltas):
    h = spacing(n3, deltas)
    N = int(np.prod(n3))
    x = O.fill_random(N, SEED)
    da = pb.DA(ctx, n3)
    A = pb.Mat(da, pb.VARCOEF, h)
    xv, yv, bv = vec_of(da, x), pb.Vec(da), pb.Vec(da)
    # a fresh operator: m absent (reads back as ones), s = 0
    assert A.mass(yv) == 0.0 and np.all(yv.get_values() == 1.0)
    for field in ("random", "sphere"):
        beta = V.FIELDS[field](n3)
        bv.set_values(beta)
        for mean in MEANS:
            A.set_coefficient(bv, mean)
            for name, m, s in masses(n3):
                set_mass(da, A, m, s, n3)
                yv.set(7.25)
                A.mult(xv, yv)
                assert np.array_equal(yv.get_values(), VMS.apply(x, beta, n3, h, mean, m, s)), (
                    field, mean, name)
                A.diagonal_vec(yv)
                assert np.array_equal(yv.get_values(), VMS.diag(beta, n3, h, mean, m, s)), (
                    field, mean, name)
                assert A.mass(yv) == s
                assert np.array_equal(yv.get_values(), np.ones(N) if m is None else m), name
            # A 1 = -q to the bit (the last mass: the half-zeroed field)
            xv.set(1.0)
            A.mult(xv, yv)
            assert np.array_equal(yv.get_values(), -(s * m))
            xv.set_values(x)
            # the mass off: the bits of the operator without it
            A.set_mass(None, 0.0)
            assert A.mass(yv) == 0.0 and np.all(yv.get_values() == 1.0)
            A.mult(xv, yv)
            assert np.array_equal(yv.get_values(), V.apply(x, beta, n3, h, mean)), (field, mean)
            A.diagonal_vec(yv)
            assert np.array_equal(yv.get_values(), V.diag(beta, n3, h, mean)), (field, mean)
    for o in (A, xv, yv, bv):
        o.destroy()
    da.destroy()


# ---------------------------------------------------------------------------------------------
# 2. N ranks over the host transport
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks,n3", [(2, (16, 16, 12)), (3, (20, 16, 7)), (2, (16, 16, 4))])
def test_ranks_bit_identical(ctx, nranks, n3):
    from test_gpu_parity import run_ranks
    h = spacing(n3, None)
    x = O.fill_random(int(np.prod(n3)), SEED)
    _, m, s = masses(n3)[1]
    cases = [(f, mean) for f in ("random", "sphere") for mean in MEANS]

    def one(c, rows):
        da = pb.DA(c, n3)
        A = pb.Mat(da, pb.VARCOEF, h)
        xv, yv, bv = vec_of(da, cut(x, n3, rows)), pb.Vec(da), pb.Vec(da)
        set_mass(da, A, m, s, n3, rows)
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
        assert np.array_equal(y, VMS.apply(x, beta, n3, h, mean, m, s))
        assert np.array_equal(d, VMS.diag(beta, n3, h, mean, m, s))

    def body(c, rank):
        rows = pb.slab_partition(n3[2], nranks, rank)
        return rows, one(c, rows)

    for rows, slabs in run_ranks(nranks, body):
        for case, (y, d), (yw, dw) in zip(cases, slabs, whole):
            assert np.array_equal(y, cut(yw, n3, rows)), (rows, case)
            assert np.array_equal(d, cut(dw, n3, rows)), (rows, case)


# ---------------------------------------------------------------------------------------------
# 3. errors
# ---------------------------------------------------------------------------------------------
def raises(code, call):
    with pytest.raises(pb.PbError) as e:
        call()
    assert e.value.code == code, (e.value.code, str(e.value))
    return str(e.value)


def test_errors_leave_the_operator_as_it_was(ctx):
    n3 = (17, 12, 9)
    h = spacing(n3, None)
    N = int(np.prod(n3))
    x, beta = O.fill_random(N, SEED), V.beta_random(n3)
    _, m, s = masses(n3)[1]
    da, other = pb.DA(ctx, n3), pb.DA(ctx, (16, 12, 9))
    A = pb.Mat(da, pb.VARCOEF, h)
    xv, yv, bv, bad = vec_of(da, x), pb.Vec(da), vec_of(da, beta), pb.Vec(da)
    mv = vec_of(da, m)
    A.set_coefficient(bv, V.HARMONIC)
    A.set_mass(mv, s)
    want = VMS.apply(x, beta, n3, h, V.HARMONIC, m, s)

    def unchanged():
        yv.set(7.25)
        A.mult(xv, yv)
        assert np.array_equal(yv.get_values(), want)
        assert A.mass(yv) == s and np.array_equal(yv.get_values(), m)

    unchanged()
    for value in (np.nan, np.inf, -1.0):
        m2 = m.copy()
        m2[N // 3] = value
        bad.set_values(m2)
        raises(ARG, lambda: A.set_mass(bad, 1.0))
        unchanged()
    for s2 in (-1.0, np.nan, np.inf):
        raises(ARG, lambda: A.set_mass(mv, s2))
        raises(ARG, lambda: A.set_mass(None, s2))
        unchanged()
    ov = pb.Vec(other)
    ov.set(1.0)
    raises(ARG, lambda: A.set_mass(ov, 1.0))
    unchanged()
    # zero is a value of m: a region without mass
    m2 = m.copy()
    m2[N // 3] = 0.0
    bad.set_values(m2)
    A.set_mass(bad, s)
    A.mult(xv, yv)
    assert np.array_equal(yv.get_values(), VMS.apply(x, beta, n3, h, V.HARMONIC, m2, s))
    A.set_mass(mv, s)
    # another kind
    S = pb.Mat(da, pb.STAR7, h)
    raises(STATE, lambda: S.set_mass(None, 1.0))
    raises(STATE, lambda: S.mass())
    # inside a solve of a KSP that holds the operator
    k = pb.KSP(A, A, pb.ksp_options(["-pc_type", "jacobi"], nullspace=0))
    rhs_v, sol = vec_of(da, want), pb.Vec(da)
    k.begin(rhs_v, sol)
    raises(STATE, lambda: A.set_mass(None, 1.0))
    raises(STATE, lambda: A.set_mass(mv, 2.0))
    k.iterate(2)
    k.end()
    unchanged()
    A.set_mass(None, 2.0)  # free again
    k.destroy()
    for o in (A, S, xv, yv, bv, bad, mv, ov, rhs_v, sol):
        o.destroy()
    other.destroy()
    da.destroy()


def test_nullspace_rule(ctx):
    """A with the mass on and nullspace = 1: PB_ERR_STATE from solve and from begin, naming
    nullspace = 0; with the mass off again the same KSP gives the bits of a fresh one. A mass in
    the PC's coefficient operator alone is allowed."""
    n3 = (16, 16, 12)
    h = spacing(n3, None)
    beta = V.beta_random(n3)
    b = V.apply(O.fill_random(int(np.prod(n3)), SEED), beta, n3, h, V.HARMONIC)
    da = pb.DA(ctx, n3)
    bv, x, coef = vec_of(da, b), pb.Vec(da), vec_of(da, beta)

    def solve(k):
        x.set(7.25)
        reason, its, hist = k.solve(bv, x)
        return reason, its, np.asarray(hist), x.get_values()

    def same(a, c):
        return a[:2] == c[:2] and np.array_equal(a[2], c[2]) and np.array_equal(a[3], c[3])

    for argv in (["-pc_type", "jacobi"], ["-pc_type", "jacobi", "-ksp_type", "preonly"],
                 ["-pc_type", "jacobi", "-ksp_type", "fgmres"]):
        opts = pb.ksp_options(argv + ["-ksp_rtol", "1e-8"])
        A = pb.Mat(da, pb.VARCOEF, h)
        A.set_coefficient(coef, V.HARMONIC)
        k = pb.KSP(A, A, opts)
        A.set_mass(None, 3.0)
        assert "nullspace = 0" in raises(STATE, lambda: k.solve(bv, x))
        if "preonly" not in argv:
            assert "nullspace = 0" in raises(STATE, lambda: k.begin(bv, x))
        A.set_mass(None, 0.0)
        again = solve(k)
        k.destroy()
        F = pb.Mat(da, pb.VARCOEF, h)
        F.set_coefficient(coef, V.HARMONIC)
        kf = pb.KSP(F, F, opts)
        fresh = solve(kf)
        kf.destroy()
        assert same(again, fresh) and again[0] > 0, argv
        for o in (A, F):
            o.destroy()
    # the rule reads A only
    A, Cm = pb.Mat(da, pb.VARCOEF, h), pb.Mat(da, pb.VARCOEF, h)
    P = pb.Mat(da, pb.STAR7, h)
    for o in (A, Cm):
        o.set_coefficient(coef, V.HARMONIC)
    Cm.set_mass(None, 3.0)
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", "mg", "-ksp_rtol", "1e-8"]))
    k.pc_set_coefficient_from(Cm)
    assert solve(k)[0] == 2
    k.destroy()
    for o in (A, Cm, P, bv, x, coef):
        o.destroy()
    da.destroy()


# ---------------------------------------------------------------------------------------------
# 4. the preconditioner apply
# ---------------------------------------------------------------------------------------------
PC_CASES = [("random", V.ARITHMETIC), ("sphere", V.HARMONIC), ("random", V.HARMONIC)]
PC_MASSES = ["field", "scalar"]
NU, OMEGA = {"mg": 2, "sor": 1}, 1.3


@functools.lru_cache(maxsize=None)
def restated_pc(n3, deltas, pc, field, mean, mass):
    _, m, s = {name: (name, m, s) for name, m, s in masses(n3)}[mass]
    vc = VMS.MassVCycle(n3, spacing(n3, deltas), V.FIELDS[field](n3), mean, m, s,
                        M.Smoother(nu=NU[pc]), omega=OMEGA, pc=pc)
    z = vc.apply(rhs(n3))
    z.setflags(write=False)
    return z


def gpu_pc_applies(c, n3, deltas, pc, rows=None):
    """pb_ksp_pc_apply of one KSP with its levels from A: {(field, mean, mass): z}"""
    h = spacing(n3, deltas)
    da = pb.DA(c, n3)
    P, A = pb.Mat(da, pb.ASSEMBLED27, h), pb.Mat(da, pb.VARCOEF, h)
    rv, zv, bv = vec_of(da, cut(rhs(n3), n3, rows)), pb.Vec(da), pb.Vec(da)
    k = pb.KSP(A, P, pb.ksp_options(pc_argv(pc, NU[pc], OMEGA), nullspace=0))
    ms = {name: (m, s) for name, m, s in masses(n3)}
    out = {}
    try:
        k.pc_set_coefficient_from(A)
        for field, mean in PC_CASES:
            bv.set_values(cut(V.FIELDS[field](n3), n3, rows))
            A.set_coefficient(bv, mean)
            for mass in PC_MASSES:
                set_mass(da, A, *ms[mass], n3, rows)
                zv.set(7.25)
                k.pc_apply(rv, zv)
                out[(field, mean, mass)] = zv.get_values()
        return out
    finally:
        k.destroy()
        for o in (A, P, rv, zv, bv):
            o.destroy()
        da.destroy()


def check_pc(got, n3, deltas, pc, rows=None, tag=""):
    for (field, mean, mass), z in got.items():
        want = cut(restated_pc(n3, deltas, pc, field, mean, mass), n3, rows)
        diff = float(np.max(np.abs(z - want)) / np.max(np.abs(want)))
        print(f"{pc} {n3} {field} mean {mean} mass {mass} {tag}: max relative difference {diff:.3e}")
        assert np.array_equal(z, want), (pc, field, mean, mass, tag, diff)


@pytest.mark.parametrize("n3,deltas", PC_SHAPES, ids=[f"{s[0]}" for s in PC_SHAPES])
@pytest.mark.parametrize("pc", ["mg", "sor"])
def test_pc_apply_bit_identical(ctx, tune, pc, n3, deltas):
    for stored in (0, 1):
        for fused in (0, 1):
            tune.set("mg_varcoef_dinv_stored", stored)
            tune.set("mg_varcoef_pre_fused", fused)
            check_pc(gpu_pc_applies(ctx, n3, deltas, pc), n3, deltas, pc,
                     tag=f"dinv_stored {stored} pre_fused {fused}")


@pytest.mark.parametrize("n3,deltas", PC_SHAPES, ids=[f"{s[0]}" for s in PC_SHAPES])
def test_pc_apply_two_ranks(tune, n3, deltas):
    from test_gpu_parity import run_ranks
    for stored, fused in ((0, 0), (0, 1), (1, 0), (1, 1)):
        tune.set("mg_varcoef_dinv_stored", stored)
        tune.set("mg_varcoef_pre_fused", fused)

        def body(c, rank):
            rows = pb.slab_partition(n3[2], 2, rank)
            return rows, {pc: gpu_pc_applies(c, n3, deltas, pc, rows) for pc in ("mg", "sor")}

        for rows, got in run_ranks(2, body):
            for pc in got:
                check_pc(got[pc], n3, deltas, pc, rows,
                         tag=f"rows {rows} dinv_stored {stored} pre_fused {fused}")


# ---------------------------------------------------------------------------------------------
# 5. solves against the restatement
# ---------------------------------------------------------------------------------------------
def gpu_solve(c, prob, b, argv, rows=None):
    """One solve on c with nullspace = 0; rows = (k0, nk): this rank's planes. Returns
    test_gpu_ksp_types.gpu_solve's tuple."""
    da = pb.DA(c, prob.n3, prob.L)
    P, A = prob.mats(pb, da)
    x, bv = pb.Vec(da), vec_of(da, cut(b, prob.n3, rows))
    x.set(7.25)  # (a zero-guess solve must overwrite whatever x holds)
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", prob.pc_argv] + list(argv), nullspace=0))
    try:
        if hasattr(prob, "after_create"):
            prob.after_create(k, P, A)
        reason, its, hist = k.solve(bv, x)
        res = k.result
        return (reason, its, np.asarray(hist), x.get_values(), res.rnorm0, res.rnorm, res.nhist)
    finally:
        k.destroy()
        for o in {A, P, x, bv}:
            o.destroy()
        da.destroy()


def make_problem(n3, deltas, pc, mass="field"):
    beta, mean = (V.beta_random(n3), V.ARITHMETIC) if pc != "vsor" else (V.beta_sphere(n3),
                                                                         V.HARMONIC)
    _, m, s = {name: (name, m, s) for name, m, s in masses(n3)}[mass]
    if pc == "vjacobi":
        return VMS.MassProblem(n3, beta, mean, m, s, pc="vjacobi", deltas=deltas)
    return VMS.MassMgProblem(n3, beta, mean, m, s, pc=pc, deltas=deltas)


@functools.lru_cache(maxsize=None)
def cg_case(n3, deltas, pc):
    """(problem, b, the restated CG to RTOL): computed once, shared by 1 and 2 ranks."""
    prob = make_problem(n3, deltas, pc)
    b = prob.rhs()
    want = NR.cg(prob, b, rtol=RTOL)
    assert want[1] == 2 and ttol_margin_ok(want[3], RTOL, want[4]), (
        "the restatement stops too close to ttol", n3, pc)
    return prob, b, want


def check_solve(prob, got, want, rows, tag):
    reason, its, hist, xs, rnorm0, rnorm, nhist = got
    xo, ro, itso, ho, ref = want
    print(f"{tag}: gpu reason {reason} its {its} | restated reason {ro} its {itso}")
    assert (reason, its, nhist) == (ro, itso, len(ho)) and len(hist) == nhist
    bar = HIST_RTOL_PC if prob.pc in ("sor", "mg") else HIST_RTOL
    print(f"{tag}: history difference {check_history(hist, ho, bar=bar, tag=tag):.3e} (bar {bar:.0e})")
    dx = check_x(xs, cut(xo, prob.n3, rows), scale=float(np.max(np.abs(xo))), tag=tag)
    print(f"{tag}: x difference {dx:.3e} (bar {X_RTOL:.0e})")
    assert abs(rnorm0 - ref) <= HIST_RTOL * ref and rnorm == hist[-1]


@pytest.mark.parametrize("n3,deltas", PC_SHAPES, ids=[f"{s[0]}" for s in PC_SHAPES])
@pytest.mark.parametrize("pc", ["vjacobi", "vsor", "vmg"])
def test_cg_to_a_tolerance(ctx, tune, pc, n3, deltas):
    prob, b, want = cg_case(n3, deltas, pc)
    for fused in (1, 0):
        tune.set("varcoef_dot_fused", fused)
        got = gpu_solve(ctx, prob, b, ["-ksp_rtol", repr(RTOL)])
        check_solve(prob, got, want, None, f"cg {pc} {n3} dot_fused {fused}")


@pytest.mark.parametrize("n3,deltas", PC_SHAPES, ids=[f"{s[0]}" for s in PC_SHAPES])
def test_cg_to_a_tolerance_two_ranks(n3, deltas):
    from test_gpu_parity import run_ranks
    cases = {pc: cg_case(n3, deltas, pc) for pc in ("vjacobi", "vsor", "vmg")}

    def body(c, rank):
        rows = pb.slab_partition(n3[2], 2, rank)
        return rows, {pc: gpu_solve(c, prob, b, ["-ksp_rtol", repr(RTOL)], rows)
                      for pc, (prob, b, _) in cases.items()}

    for rows, got in run_ranks(2, body):
        for pc, (prob, b, want) in cases.items():
            check_solve(prob, got[pc], want, rows, f"cg {pc} {n3} rows {rows}")


def test_richardson_and_preonly_with_the_variable_mg(ctx):
    n3 = (16, 16, 16)
    prob = make_problem(n3, None, "vmg")
    b = prob.rhs()
    want = KR.richardson(prob, b, rtol=RTOL)
    assert want[1] == 2 and ttol_margin_ok(want[3], RTOL, want[4])
    got = gpu_solve(ctx, prob, b, ["-ksp_type", "richardson", "-ksp_rtol", repr(RTOL)])
    check_solve(prob, got, want, None, "richardson vmg")
    want = KR.preonly(prob, b + 0.5)
    got = gpu_solve(ctx, prob, b + 0.5, ["-ksp_type", "preonly"])
    assert got[:2] == (4, 1)
    print(f"preonly vmg: x difference {check_x(got[3], want[0], tag='preonly vmg'):.3e}")


@pytest.mark.parametrize("ksp", ["chebyshev", "fgmres", "pipecg"])
def test_other_types_with_the_variable_jacobi(ctx, ksp):
    n3 = (17, 12, 9)
    prob = make_problem(n3, None, "vjacobi")
    b = prob.rhs()
    reason, its, hist, xs, *_ = gpu_solve(ctx, prob, b, ["-ksp_type", ksp, "-ksp_rtol", repr(RTOL)])
    res = float(np.linalg.norm(b - prob.apply(xs)) / np.linalg.norm(b))
    print(f"{ksp} vjacobi {n3}: reason {reason} its {its} ||b - A x|| / ||b|| {res:.3e}")
    assert reason > 0 and res <= 10 * RTOL


# ---------------------------------------------------------------------------------------------
# 6. a time loop: set_mass(m, s) per step on one KSP
# ---------------------------------------------------------------------------------------------
def test_time_loop(ctx):
    n3 = (16, 16, 16)
    h = spacing(n3, None)
    beta, m = V.beta_random(n3), VMS.mass_uniform(n3)
    b = O.fill_random(int(np.prod(n3)), SEED)
    da = pb.DA(ctx, n3)
    bv, x, coef, mv = vec_of(da, b), pb.Vec(da), vec_of(da, beta), vec_of(da, m)
    P = pb.Mat(da, pb.STAR7, h)
    opts = pb.ksp_options(["-pc_type", "mg", "-ksp_rtol", "1e-8"], nullspace=0)

    def solve(k):
        x.set(7.25)
        reason, its, hist = k.solve(bv, x)
        return reason, its, np.asarray(hist), x.get_values()

    def make(s):
        A = pb.Mat(da, pb.VARCOEF, h)
        A.set_coefficient(coef, V.ARITHMETIC)
        A.set_mass(mv, s)
        k = pb.KSP(A, P, opts)
        k.pc_set_coefficient_from(A)
        return A, k

    A, k = make(10.0)
    steps = []
    for s in (10.0, 40.0, 10.0):
        A.set_mass(mv, s)
        steps.append(solve(k))
    k.destroy()
    A.destroy()
    for s, step in zip((10.0, 40.0, 10.0), steps):
        F, kf = make(s)
        fresh = solve(kf)
        kf.destroy()
        F.destroy()
        print(f"time loop s = {s}: reason {step[0]} its {step[1]}")
        assert step[0] == 2 and step[:2] == fresh[:2], s
        assert np.array_equal(step[2], fresh[2]) and np.array_equal(step[3], fresh[3]), s
    assert not np.array_equal(steps[0][3], steps[1][3])
    for o in (P, bv, x, coef, mv):
        o.destroy()
    da.destroy()
