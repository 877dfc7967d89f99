"""GPU tier: -ksp_norm_type unpreconditioned | natural | none against the numpy restatement
(tests/norm_type_restatement.py; semantics in DESIGN.md §3.1g, "parity unpinned": PETSc is not
available; the restatement is tied to the pinned oracle through the preconditioned norm, in
tests/test_norm_type_cpu.py).

Bars: tests/parity_bars.py -- HIST_RTOL (Jacobi / none), HIST_RTOL_PC (sor / mg), X_RTOL; with the
spectral PC test_gpu_ksp_types.check's rule (||.||_0 to 1e-12, the later rounding-noise norms to
1e-10 ||.||_0 absolute). No bar of this file's own. Iteration counts must match the restatement
exactly, so every stopping case asserts on the restatement's own norms that the last two are more
than 1e-6 (relative) from ttol. Richardson / Chebyshev recompute r = b - A x every update, so their
runs compared under the relative bars are fixed-count runs, and those taken to a tolerance carry
test_gpu_ksp_types' HIST_FLOOR (its docstring has the reasoning).

Every test here fails without the feature: the option is not parsed and pb_ksp_set_norm_type does
not exist. Reference: src/poissbox.f90:295 (KSPSetFromOptions).
"""
import functools

import numpy as np
import pytest

import poissbox_amd as pb
from oracle import oracle as O
import chebyshev_restatement as CR
import norm_type_restatement as NR
from norm_type_restatement import Problem, ttol_margin_ok
from parity_bars import HIST_RTOL, check_x
from test_gpu_ksp_types import FIXED, FIXED_KW, HIST_FLOOR, _multirank, check, gpu_solve, rich_argv

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED, STATE = 1, 5, 6
NT = ["-ksp_norm_type"]
PHASES = ("cg_init", "cg_init_guess", "cg_init_guess_vec", "cg_pass_a", "cg_pass_b",
          "cg_pass_b_even", "cg_pass_b_odd", "cg_pass_b_x4", "cg_sr1", "cg_sr_p", "cg_sr_p_x4",
          "cg_sr_s", "cg_finalize", "cg_gen_p", "cg_gen_dot", "cg_gen_xr", "cg_pc_xr", "cg_pc_sums",
          "cg_rr", "stencil", "compact_lapl_fast", "mg_apply", "mg_sor", "mg_sor_sweep2",
          "mg_post_sweep", "mg_presmooth_restrict", "mg_presmooth_residual", "mg_residual",
          "pc_fft", "rich_update", "rich_resid", "rich_resid_vec", "rich_axpy", "rich_sums",
          "rich_finalize", "cheb_update", "cheb_axpy", "allreduce", "halo")


def cg_argv(norm_type, rtol=None, max_it=None, sr=False, extra=()):
    a = ["-ksp_type", "cg"] + NT + [norm_type]
    if max_it is not None:
        a += FIXED + ["-ksp_max_it", str(max_it)]
    if rtol is not None:
        a += ["-ksp_rtol", repr(float(rtol))]
    return a + (["-ksp_cg_single_reduction"] if sr else []) + list(extra)


# ---------------------------------------------------------------------------------------------
# CG x {unpreconditioned, natural} x every operator / PC path
# ---------------------------------------------------------------------------------------------
CG_PATHS = {
    "none": (Problem((16, 16, 12), pc="none"), 1e-6),
    "jacobi": (Problem((24, 20, 12)), 1e-6),
    "jacobi_odd_x": (Problem((17, 18, 9)), 1e-6),
    "jacobi_two_segments": (Problem((130, 6, 33)), 1e-6),
    "sor": (Problem((16, 16, 12), pc="sor"), 1e-8),
    "mg": (Problem((32, 32, 32), pc="mg"), 1e-8),
    "mg_small": (Problem((16, 16, 12), pc="mg"), 1e-8),
    "fft": (Problem((32, 40, 48), pc="fft"), 1e-8),
    "compact_fft": (Problem((64, 64, 64), pc="fft", op="compact"), 1e-8),
    # (512-point x lines: the spectral PC fuses CG's r update into its first pass)
    "compact_fft_512": (Problem((512, 32, 32), pc="fft", op="compact"), 1e-8),
    "assembled_jacobi": (Problem((16, 16, 12), op="assembled"), 1e-6),
    "compact_jacobi": (Problem((16, 16, 16), op="compact"), 1e-6),
}
FUSED = ("none", "jacobi", "jacobi_odd_x", "jacobi_two_segments")


@functools.lru_cache(maxsize=None)
def cg_case(name, norm_type, sr=False):
    """(problem, b, rtol, restated solve): computed once; the margin to ttol checked here."""
    prob, rtol = CG_PATHS[name]
    b = prob.rhs()
    want = NR.cg(prob, b, norm_type=norm_type, single_reduction=sr, rtol=rtol)
    assert want[1] == 2, (name, norm_type, want[1:3])
    assert ttol_margin_ok(want[3], rtol, want[4]), (name, norm_type, "seed too close to ttol")
    return prob, b, rtol, want


@pytest.mark.parametrize("norm_type", ["unpreconditioned", "natural"])
@pytest.mark.parametrize("name", list(CG_PATHS))
def test_cg_every_path(ctx, name, norm_type):
    prob, b, rtol, want = cg_case(name, norm_type)
    got = gpu_solve(ctx, prob, b, cg_argv(norm_type, rtol=rtol))
    check(prob, got, want, tag=f"cg {name} {norm_type}")
    if norm_type == "unpreconditioned":  # the point of it: the logged number is ||b - A x||
        assert abs(got[4] - np.linalg.norm(b)) <= HIST_RTOL * got[4]
        true = float(np.linalg.norm(b - prob.apply(got[3])))
        assert true <= rtol * got[4] * 1.01 or prob.pc == "fft", (true, rtol * got[4])


@pytest.mark.parametrize("norm_type", ["unpreconditioned", "natural"])
@pytest.mark.parametrize("name", FUSED)
def test_single_reduction_cg(ctx, name, norm_type):
    prob, b, rtol, want = cg_case(name, norm_type, True)
    got = gpu_solve(ctx, prob, b, cg_argv(norm_type, rtol=rtol, sr=True))
    check(prob, got, want, tag=f"sr {name} {norm_type}")


@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("norm_type", ["unpreconditioned", "natural"])
def test_cg_folded_equals_unfolded(ctx, tune, norm_type, fold):
    """The stages run in the passes' prologues (cg_fold = 1, the default) or as launches of their
    own: the same bits, and the deferred x update at every depth."""
    prob, b, rtol, want = cg_case("jacobi", norm_type)
    tune.set("cg_fold", fold)
    outs = []
    for defer in (4, 2, 0):
        tune.set("cg_defer_x", defer)
        outs.append(gpu_solve(ctx, prob, b, cg_argv(norm_type, rtol=rtol)))
        check(prob, outs[-1], want, tag=f"fold {fold} defer {defer} {norm_type}")
        assert np.array_equal(outs[-1][2], outs[0][2])  # (x differs at rounding level by depth)


# ---------------------------------------------------------------------------------------------
# Richardson, Chebyshev: unpreconditioned
# ---------------------------------------------------------------------------------------------
def _stationary_case(solver, pc):
    n3 = {"jacobi": (24, 20, 12), "mg": (16, 16, 12), "fft": (32, 40, 48)}[pc]
    prob = Problem(n3, pc=pc)
    b = prob.rhs()
    if solver == "richardson":
        scale = 2.0 / 3.0 if pc == "jacobi" else 1.0
        argv = rich_argv(scale)
        run = functools.partial(NR.richardson, prob, b, scale=scale)
    else:
        lo, hi = CR.jacobi_spectrum(prob) if pc == "jacobi" else (0.1, 1.1)
        argv = ["-ksp_type", "chebyshev", "-ksp_chebyshev_eigenvalues", f"{lo!r},{hi!r}"]
        run = functools.partial(NR.chebyshev, prob, b, lo, hi)
    return prob, b, argv, run


@pytest.mark.parametrize("pc", ["jacobi", "mg", "fft"])
@pytest.mark.parametrize("solver", ["richardson", "chebyshev"])
def test_stationary_unpreconditioned(ctx, solver, pc):
    prob, b, argv, run = _stationary_case(solver, pc)
    nt = NT + ["unpreconditioned"]
    if pc != "fft":  # six updates under the relative bars
        want = run(norm_type="unpreconditioned", max_it=6, **FIXED_KW)
        got = gpu_solve(ctx, prob, b, argv + FIXED + ["-ksp_max_it", "6"] + nt)
        check(prob, got, want, tag=f"{solver} {pc} fixed")
    rtol = 1e-3 if pc == "jacobi" else 1e-8  # and to a tolerance: the stopping iteration
    want = run(norm_type="unpreconditioned", rtol=rtol)
    assert want[1] == 2 and ttol_margin_ok(want[3], rtol, want[4]), want[1:3]
    got = gpu_solve(ctx, prob, b, argv + ["-ksp_rtol", repr(rtol)] + nt)
    check(prob, got, want, tag=f"{solver} {pc} rtol", floor=0.0 if pc == "fft" else HIST_FLOOR)
    assert abs(got[4] - np.linalg.norm(b)) <= HIST_RTOL * got[4]
    assert abs(got[5] - np.linalg.norm(b - prob.apply(got[3]))) <= 1e-6 * got[5] + 1e-13 * got[4]


@pytest.mark.parametrize("pc", ["jacobi", "mg"])
def test_richardson_fused_equals_unfused(ctx, tune, pc):
    """rich_fused = 0 (vector kernel + the engine's residual pass) against 1 under
    unpreconditioned: the same bits."""
    prob, b, argv, run = _stationary_case("richardson", pc)
    want = run(norm_type="unpreconditioned", max_it=6, **FIXED_KW)
    out = {}
    for fused in (1, 0):
        tune.set("rich_fused", fused)
        out[fused] = gpu_solve(ctx, prob, b, argv + FIXED + ["-ksp_max_it", "6"]
                               + NT + ["unpreconditioned"])
    check(prob, out[0], want, tag=f"unfused {pc}")
    assert out[0][:2] == out[1][:2]
    assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])


# ---------------------------------------------------------------------------------------------
# nonzero guess, projected guess
# ---------------------------------------------------------------------------------------------
MODE_ARGV = {"default": [], "initial": ["-ksp_converged_use_initial_residual_norm"],
             "min": ["-ksp_converged_use_min_initial_residual_norm"]}


@pytest.mark.parametrize("norm_type", ["unpreconditioned", "natural"])
@pytest.mark.parametrize("mode", ["default", "initial", "min"])
@pytest.mark.parametrize("pc", ["jacobi", "mg"])
def test_cg_nonzero_guess(ctx, pc, mode, norm_type):
    prob = Problem((16, 16, 12), pc=pc)
    b, x0 = prob.rhs(), 1e-3 * O.fill_random(prob.N, 7)
    rtol = 1e-6
    want = NR.cg(prob, b, x0=x0, norm_type=norm_type, mode=mode, rtol=rtol)
    assert want[1] == 2 and ttol_margin_ok(want[3], rtol, want[4])
    argv = cg_argv(norm_type, rtol=rtol, extra=["-ksp_initial_guess_nonzero"] + MODE_ARGV[mode])
    got = gpu_solve(ctx, prob, b, argv, x0=x0)
    check(prob, got, want, tag=f"guess {pc} {mode} {norm_type}")
    if mode == "default" and norm_type == "unpreconditioned":
        assert abs(got[4] - np.linalg.norm(b)) <= HIST_RTOL * got[4] and got[4] != got[2][0]


@pytest.mark.parametrize("solver", ["richardson", "chebyshev"])
def test_stationary_nonzero_guess_mg(ctx, solver):
    prob, b, argv, run = _stationary_case(solver, "mg")
    x0 = 1e-3 * O.fill_random(prob.N, 7)
    want = run(x0=x0, norm_type="unpreconditioned", max_it=6, **FIXED_KW)
    got = gpu_solve(ctx, prob, b, argv + FIXED + ["-ksp_max_it", "6", "-ksp_initial_guess_nonzero"]
                    + NT + ["unpreconditioned"], x0=x0)
    check(prob, got, want, tag=f"{solver} guess mg")
    assert abs(got[4] - np.linalg.norm(b)) <= HIST_RTOL * got[4]


def _counts(ctx, names=PHASES):
    return {n: ctx.timing(n)[1] for n in names}


def _timed_split_solve(ctx, prob, b, argv, iters, x0=None):
    """begin / iterate(iters) / end with every phase timed: ({phase: launches}, result). Exactly
    `iters` iterations are enqueued (nothing stops these runs)."""
    da = pb.DA(ctx, prob.n3, prob.L)
    P, A = prob.mats(pb, da)
    x, bv = pb.Vec(da), pb.Vec(da)
    bv.set_values(b)
    x.set_values(x0 if x0 is not None else np.zeros(prob.N))
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", prob.pc] + list(argv)))
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        k.begin(bv, x)
        setup = _counts(ctx)
        k.iterate(iters)
        reason, its, hist = k.end()
        total = _counts(ctx)
    finally:
        ctx.set_timing(False)
        k.destroy()
        for o in {A, P, x, bv}:
            o.destroy()
        da.destroy()
    return setup, total, (reason, its, np.asarray(hist), None)


def test_mg_guess_setup_loses_its_pc_application(ctx):
    """From a nonzero guess the preconditioned norm applies the PC twice at setup (M^-1 b for the
    reference, M^-1 r_0); under unpreconditioned the reference is ||b||: one application."""
    prob = Problem((16, 16, 12), pc="mg")
    b, x0 = prob.rhs(), 1e-3 * O.fill_random(prob.N, 7)
    n = {}
    for t in ("preconditioned", "unpreconditioned", "none"):
        argv = cg_argv(t, max_it=4, extra=["-ksp_initial_guess_nonzero"])
        n[t] = _timed_split_solve(ctx, prob, b, argv, 0, x0=x0)[0]["mg_apply"]
    assert (n["preconditioned"], n["unpreconditioned"], n["none"]) == (2, 1, 1), n
    for solver in ("richardson", "chebyshev"):
        _, _, argv, _ = _stationary_case(solver, "mg")
        m = {t: _timed_split_solve(ctx, prob, b, argv + FIXED + ["-ksp_max_it", "4",
                                   "-ksp_initial_guess_nonzero"] + NT + [t], 0,
                                   x0=x0)[0]["mg_apply"]
             for t in ("preconditioned", "unpreconditioned")}
        assert (m["preconditioned"], m["unpreconditioned"]) == (2, 1), (solver, m)


def test_fischer_time_loop_unpreconditioned(ctx):
    """-ksp_guess_type fischer with -pc_type mg: every step stops on ||r|| <= rtol ||b_k||, the
    later ones in fewer iterations than the first."""
    prob = Problem((16, 16, 12), pc="mg")
    b, c = prob.rhs(), prob.rhs(seed=99)
    da = pb.DA(ctx, prob.n3)
    P, A = prob.mats(pb, da)
    x, bv = pb.Vec(da), pb.Vec(da)
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", "mg", "-ksp_guess_type", "fischer"]
                                    + cg_argv("unpreconditioned", rtol=1e-8)))
    assert k.norm_type == (pb.KSP_NORM_UNPRECONDITIONED, pb.KSP_NORM_UNPRECONDITIONED)
    its_all = []
    for step in range(3):
        bk = b + 0.01 * step * c
        bv.set_values(bk)
        reason, its, hist = k.solve(bv, x)
        ref = float(np.linalg.norm(bk))
        assert reason == 2 and len(hist) == its + 1
        assert abs(k.result.rnorm0 - ref) <= HIST_RTOL * ref
        true = float(np.linalg.norm(bk - prob.apply(x.get_values())))
        assert true <= 1e-8 * ref * (1 + 1e-3) and abs(true - hist[-1]) <= 1e-3 * hist[-1] + 1e-12 * ref
        its_all.append(its)
    k.destroy()
    assert its_all[1] < its_all[0] and its_all[2] < its_all[0], its_all


# ---------------------------------------------------------------------------------------------
# none
# ---------------------------------------------------------------------------------------------
def _solve_kw(ctx, prob, b, argv, **kw):
    da = pb.DA(ctx, prob.n3, prob.L)
    P, A = prob.mats(pb, da)
    x, bv = pb.Vec(da), pb.Vec(da)
    bv.set_values(b)
    x.set(7.25)
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", prob.pc] + list(argv), **kw))
    try:
        reason, its, hist = k.solve(bv, x)
        return reason, its, np.asarray(hist), x.get_values(), k.result.rnorm0, k.result.rnorm
    finally:
        k.destroy()
        for o in {A, P, x, bv}:
            o.destroy()
        da.destroy()


@pytest.mark.parametrize("check_every", [1, 8])
@pytest.mark.parametrize("max_it", [1, 2, 3, 4, 9])
@pytest.mark.parametrize("solver", ["cg", "sr", "richardson"])
def test_none_runs_max_it(ctx, tune, solver, max_it, check_every):
    """reason 4, its = max_it, zero history, and x to the bit of the preconditioned-norm run that
    max_it stops at the same count -- at every depth of the deferred x update."""
    prob = Problem((24, 20, 12))
    b = prob.rhs()
    base = {"cg": ["-ksp_type", "cg"], "sr": ["-ksp_type", "cg", "-ksp_cg_single_reduction"],
            "richardson": rich_argv(2.0 / 3.0)}[solver]
    for defer in ((4, 2, 0) if solver != "richardson" else (4,)):
        tune.set("cg_defer_x", defer)
        # (rtol = 0 would stop nothing either, but `none` must not need it)
        got = _solve_kw(ctx, prob, b, base + ["-ksp_max_it", str(max_it)] + NT + ["none"],
                        check_every=check_every)
        ref = _solve_kw(ctx, prob, b, base + FIXED + ["-ksp_max_it", str(max_it)],
                        check_every=check_every)
        assert ref[:2] == (-3, max_it)
        assert got[:2] == (4, max_it), (solver, defer, got[:2])
        assert got[4] == 0.0 and got[5] == 0.0
        assert len(got[2]) == max_it + 1 and np.all(got[2] == 0.0)
        assert np.array_equal(got[3], ref[3]), (solver, defer)


@pytest.mark.parametrize("pc,solver", [("mg", "cg"), ("mg", "richardson"), ("fft", "richardson")])
def test_none_stored_z(ctx, pc, solver):
    """(CG with the spectral PC is left out: its second iteration runs on rounding noise, where a
    breakdown exit, which `none` keeps, may come first.)"""
    prob = Problem((16, 16, 12) if pc == "mg" else (32, 40, 48), pc=pc)
    b = prob.rhs()
    base = ["-ksp_type", "cg"] if solver == "cg" else rich_argv(1.0)
    got = _solve_kw(ctx, prob, b, base + ["-ksp_max_it", "3"] + NT + ["none"])
    ref = _solve_kw(ctx, prob, b, base + FIXED + ["-ksp_max_it", "3"])
    assert ref[:2] == (-3, 3)
    assert got[:2] == (4, 3) and np.all(got[2] == 0.0) and len(got[2]) == 4
    assert np.array_equal(got[3], ref[3])


@pytest.mark.parametrize("solver", ["cg", "richardson", "preonly"])
def test_none_max_it_zero(ctx, solver):
    prob = Problem((16, 16, 12))
    b = prob.rhs()
    if solver == "preonly":
        got = _solve_kw(ctx, prob, b, ["-ksp_type", "preonly"] + NT + ["none"])
        assert got[:2] == (4, 1) and len(got[2]) == 0
        return
    base = ["-ksp_type", "cg"] if solver == "cg" else rich_argv()
    got = _solve_kw(ctx, prob, b, base + ["-ksp_max_it", "0"] + NT + ["none"])
    assert got[:2] == (4, 0) and list(got[2]) == [0.0] and np.all(got[3] == 0.0)


def test_none_nan_in_b_still_diverges(ctx):
    """The NaN checks on CG's dots stay (KSPCheckDot on beta): -9 at the setup."""
    prob = Problem((16, 16, 12))
    b = prob.rhs()
    b[37] = np.nan
    for sr in (False, True):
        got = _solve_kw(ctx, prob, b, cg_argv("none", sr=sr) + ["-ksp_max_it", "5"])
        assert got[:2] == (-9, 0), got[:2]


# ---------------------------------------------------------------------------------------------
# no added pass: launch counts per timed phase
# ---------------------------------------------------------------------------------------------
def prob_pc(name):
    return CG_PATHS[name][0].pc


def _more_iterations(ctx, prob, b, argv, lo, hi):
    """launches per phase that iterations lo .. hi - 1 add"""
    c_lo = _timed_split_solve(ctx, prob, b, argv, lo)[1]
    c_hi = _timed_split_solve(ctx, prob, b, argv, hi)[1]
    return {n: c_hi[n] - c_lo[n] for n in PHASES}


@pytest.mark.parametrize("solver,name", [(s, n) for s in ("cg", "richardson")
                                         for n in ("jacobi", "mg", "fft", "compact_fft_512")]
                         + [("sr", "jacobi")])
def test_no_launch_added_per_iteration(ctx, solver, name):
    """Three more iterations launch the same number of every timed phase under every norm type
    (allreduces and finalize launches included). The one exception: with the compact operator on
    512- or 1024-point x lines the spectral PC's fused r update gives way to cg_pc_xr under
    unpreconditioned (the preconditioned run launches none there). (CG with the
    spectral PC solves in one iteration and breaks down on rounding noise after it, where the
    polling types stop enqueuing and `none` goes on to max_it: there the first iteration is the
    one compared.)"""
    lo, hi = (0, 1) if (solver, prob_pc(name)) == ("cg", "fft") else (3, 6)
    prob = CG_PATHS[name][0]
    b = prob.rhs()
    base = {"cg": ["-ksp_type", "cg"], "sr": ["-ksp_type", "cg", "-ksp_cg_single_reduction"],
            "richardson": rich_argv(2.0 / 3.0 if name == "jacobi" else 1.0)}[solver]
    base = base + FIXED + ["-ksp_max_it", "50"]
    ref = _more_iterations(ctx, prob, b, base + NT + ["preconditioned"], lo, hi)
    assert sum(ref.values()) > 0
    types = ["unpreconditioned", "none"] + (["natural"] if solver != "richardson" else [])
    for t in types:
        got = _more_iterations(ctx, prob, b, base + NT + [t], lo, hi)
        if (name, solver, t) == ("compact_fft_512", "cg", "unpreconditioned"):
            assert got.pop("cg_pc_xr") == ref["cg_pc_xr"] + (hi - lo)
            assert {k: v for k, v in ref.items() if k != "cg_pc_xr"} == got
        else:
            assert got == ref, (t, {k: (ref[k], got[k]) for k in ref if ref[k] != got[k]})


def test_setup_reduction_is_setup_only(ctx):
    """Unpreconditioned with a stored-z PC from a zero guess: ||b|| takes one reduction pass of
    its own at setup (cg_rr), none in the iterations."""
    prob = CG_PATHS["mg_small"][0]
    b = prob.rhs()
    setup, total, _ = _timed_split_solve(
        ctx, prob, b, cg_argv("unpreconditioned", max_it=50), 4)
    assert setup["cg_rr"] == 1 and total["cg_rr"] == 1


# ---------------------------------------------------------------------------------------------
# the default is unchanged
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jacobi", "mg", "fft"])
def test_default_equals_preconditioned_to_the_bit(ctx, name):
    prob, rtol = CG_PATHS[name]
    b = prob.rhs()
    want = NR.cg(prob, b, rtol=rtol)
    unset = gpu_solve(ctx, prob, b, ["-ksp_type", "cg", "-ksp_rtol", repr(rtol)])
    named = gpu_solve(ctx, prob, b, cg_argv("preconditioned", rtol=rtol))
    dflt = gpu_solve(ctx, prob, b, cg_argv("default", rtol=rtol))
    for other in (named, dflt):
        assert unset[:2] == other[:2] and unset[4:] == other[4:]
        assert np.array_equal(unset[2], other[2]) and np.array_equal(unset[3], other[3])
    check(prob, unset, want, tag=f"default {name}")  # and the fields the existing tests expect
    xo, ro, itso, ho = O.cg_solve(b, prob.n3, prob.h, rtol=rtol, pc=prob.pc)
    assert (unset[0], unset[1], len(unset[2])) == (ro, itso, len(ho))


# ---------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------
def test_errors_leave_the_ksp_usable(ctx):
    da = pb.DA(ctx, (16, 16, 12))
    A = pb.Mat(da, pb.STAR7)
    x, b = pb.Vec(da), pb.Vec(da)
    b.set_values(Problem((16, 16, 12)).rhs())

    def refused(k, t, code):
        before = k.norm_type
        with pytest.raises(pb.PbError) as e:
            k.set_norm_type(t)
        assert e.value.code == code, (t, e.value.code)
        assert k.norm_type == before

    for ksp_type in ("richardson", "chebyshev"):
        k = pb.KSP(A, A, pb.ksp_options(["-ksp_type", ksp_type, "-ksp_max_it", "3",
                                         "-ksp_chebyshev_eigenvalues", "0.1,2.0"]))
        assert k.norm_type == (pb.KSP_NORM_DEFAULT, pb.KSP_NORM_PRECONDITIONED)
        refused(k, pb.KSP_NORM_NATURAL, UNSUPPORTED)
        refused(k, 4, ARG)
        refused(k, -2, ARG)
        k.set_norm_type(pb.KSP_NORM_UNPRECONDITIONED)
        refused(k, pb.KSP_NORM_NATURAL, UNSUPPORTED)
        assert k.norm_type == (2, 2)
        assert k.solve(b, x)[1] == 3  # still solves
        k.destroy()
        with pytest.raises(pb.PbError) as e:  # and through the options
            pb.KSP(A, A, pb.ksp_options(["-ksp_type", ksp_type] + NT + ["natural"]))
        assert e.value.code == UNSUPPORTED

    k = pb.KSP(A, A, pb.ksp_options(["-ksp_type", "preonly"]))
    assert k.norm_type == (pb.KSP_NORM_DEFAULT, pb.KSP_NORM_NONE)
    for t in (pb.KSP_NORM_PRECONDITIONED, pb.KSP_NORM_UNPRECONDITIONED, pb.KSP_NORM_NATURAL):
        refused(k, t, UNSUPPORTED)
    k.set_norm_type(pb.KSP_NORM_NONE)
    k.set_norm_type(pb.KSP_NORM_DEFAULT)
    assert k.solve(b, x)[:2] == (4, 1)
    k.destroy()

    k = pb.KSP(A, A, pb.ksp_options(["-ksp_type", "cg", "-ksp_rtol", "1e-6"]))
    k.begin(b, x)
    refused(k, pb.KSP_NORM_NATURAL, STATE)
    k.iterate(2)
    refused(k, pb.KSP_NORM_NONE, STATE)
    k.end()
    k.set_norm_type(pb.KSP_NORM_NATURAL)  # allowed again after the end
    assert k.norm_type == (3, 3)
    reason, its, hist = k.solve(b, x)
    assert reason == 2 and len(hist) == its + 1
    k.set_norm_type(pb.KSP_NORM_DEFAULT)
    assert k.norm_type == (pb.KSP_NORM_DEFAULT, pb.KSP_NORM_PRECONDITIONED)
    k.destroy()


def test_api_solve_honours_the_option(ctx):
    prob, b, rtol, want = cg_case("mg_small", "unpreconditioned")
    da = pb.DA(ctx, prob.n3)
    P, A = prob.mats(pb, da)
    x, bv = pb.Vec(da), pb.Vec(da)
    bv.set_values(b)
    reason, its, hist = pb.solve(P, A, x, bv, options=["-pc_type", "mg"]
                                 + cg_argv("unpreconditioned", rtol=rtol))
    assert (reason, its) == want[1:3] and abs(hist[0] - np.linalg.norm(b)) <= HIST_RTOL * hist[0]


# ---------------------------------------------------------------------------------------------
# two and three ranks over the host transport
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("norm_type", ["unpreconditioned", "natural"])
@pytest.mark.parametrize("nranks,pc", [(2, "jacobi"), (3, "jacobi"), (2, "mg"), (3, "mg")])
def test_multirank_cg(nranks, pc, norm_type):
    prob = Problem((16, 16, 12), pc=pc)
    b = prob.rhs(nranks=nranks)
    rtol = 1e-6
    want = NR.cg(prob, b, norm_type=norm_type, rtol=rtol, nranks=nranks)
    assert want[1] == 2 and ttol_margin_ok(want[3], rtol, want[4])
    _multirank(prob, b, want, cg_argv(norm_type, rtol=rtol), nranks,
               f"{nranks} ranks {pc} {norm_type}")


@pytest.mark.parametrize("nranks,pc", [(2, "jacobi"), (3, "mg")])
def test_multirank_richardson_unpreconditioned(nranks, pc):
    prob = Problem((16, 16, 12), pc=pc)
    b = prob.rhs(nranks=nranks)
    scale = 2.0 / 3.0 if pc == "jacobi" else 1.0
    want = NR.richardson(prob, b, scale=scale, norm_type="unpreconditioned", max_it=6,
                         nranks=nranks, **FIXED_KW)
    _multirank(prob, b, want, rich_argv(scale, max_it=6) + NT + ["unpreconditioned"], nranks,
               f"{nranks} ranks richardson {pc}")


def test_multirank_single_reduction_and_none():
    prob = Problem((16, 16, 12))
    b = prob.rhs()
    want = NR.cg(prob, b, norm_type="unpreconditioned", single_reduction=True, rtol=1e-6)
    assert want[1] == 2 and ttol_margin_ok(want[3], 1e-6, want[4])
    _multirank(prob, b, want, cg_argv("unpreconditioned", rtol=1e-6, sr=True), 2, "2 ranks sr")
    from test_gpu_parity import run_ranks

    def body(ctx, rank):
        k0, nk = pb.slab_partition(prob.n3[2], 2, rank)
        return gpu_solve(ctx, prob, b, cg_argv("none") + ["-ksp_max_it", "5"], rows=(k0, nk))

    for got in run_ranks(2, body):
        assert got[:2] == (4, 5) and np.all(got[2] == 0.0) and len(got[2]) == 6
