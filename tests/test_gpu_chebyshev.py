"""GPU tier: -ksp_type chebyshev against its numpy restatement (tests/chebyshev_restatement.py;
semantics in DESIGN.md §3.1f, "parity unpinned": PETSc is not available, so KSPSolve_Chebyshev is
pinned to the restatement only).

Bars: tests/parity_bars.py, used as tests/test_gpu_ksp_types.py uses them (its gpu_solve and check
are reused): HIST_RTOL for Jacobi / no PC, HIST_RTOL_PC for sor / mg, the spectral PC's handling,
X_RTOL, exact reason and iteration count after ttol_margin_ok on the restatement's own norms.
Chebyshev, like Richardson, recomputes the true residual every iteration, so the runs taken to a
tolerance add that file's floor of 1e-14 ||z_0|| (HIST_FLOOR) to the relative bar.

The eigenvalue estimate is compared with the restated Lanczos process. How far the restated
extremes move when every inner product and mean is summed in another order (reversed, sequential,
exactly rounded; Jacobi at 16x16x12 and 32x40x48 with unequal deltas, sor, mg, fft), relative:
the largest eigenvalue by at most 1.0e-15, the smallest by at most 3.5e-14. The bars are 100 x
that: EST_MAX_RTOL = 1e-13 (the default transform uses the largest alone), EST_MIN_RTOL = 3.5e-12.

Every test here fails without the feature: -ksp_type chebyshev is PB_ERR_UNSUPPORTED.
Reference: src/poissbox.f90:269-298 (solve -> KSPSetFromOptions -> KSPSolve).
"""
import functools

import numpy as np
import pytest

import poissbox_amd as pb
from oracle import oracle as O
from chebyshev_restatement import chebyshev, estimate, jacobi_spectrum, lanczos
from ksp_types_restatement import Problem, ttol_margin_ok
from parity_bars import HIST_RTOL
from test_gpu_ksp_types import FIXED, FIXED_KW, HIST_FLOOR, check, gpu_solve

pytestmark = pytest.mark.gpu

ARG, STATE = 1, 6
EST_MAX_RTOL, EST_MIN_RTOL = 1e-13, 3.5e-12  # (module docstring)


def cheb_argv(bounds=None, max_it=None, rtol=None, extra=()):
    a = ["-ksp_type", "chebyshev"]
    if bounds is not None:
        a += ["-ksp_chebyshev_eigenvalues", f"{bounds[0]!r},{bounds[1]!r}"]
    if max_it is not None:
        a += FIXED + ["-ksp_max_it", str(max_it)]
    if rtol is not None:
        a += ["-ksp_rtol", repr(float(rtol))]
    return a + list(extra)


def _paths():
    jac = Problem((16, 16, 12))
    lmin, lmax = jacobi_spectrum(jac)
    d = O.diag(jac.h)
    big = Problem((32, 40, 48), deltas=(0.05, 0.03, 0.07))
    return {
        "jacobi": (jac, (lmin, lmax)),
        # without a PC the spectrum is the Laplacian's: negative
        "none": (Problem((16, 16, 12), pc="none"), (d * lmax, d * lmin)),
        "jacobi_deltas": (big, jacobi_spectrum(big)),
        "sor": (Problem((16, 16, 12), pc="sor"), (0.05, 1.1)),
        "mg": (Problem((16, 16, 12), pc="mg"), (0.1, 1.1)),
        "fft": (Problem((32, 40, 48), pc="fft"), (0.1, 1.1)),
        "compact_fft": (Problem((32, 32, 32), pc="fft", op="compact"), (0.1, 1.1)),
        "assembled_jacobi": (Problem((16, 16, 12), op="assembled"), (lmin, lmax)),
    }


@functools.lru_cache(maxsize=None)
def fixed_run(name, n_updates=7):
    """(problem, bounds, b, restated run of n_updates updates without a stopping test, its
    iterates): computed once; every shorter run is a prefix of it."""
    prob, bounds = _paths()[name]
    b = prob.rhs()
    trace = []
    want = chebyshev(prob, b, *bounds, max_it=n_updates, trace=trace, **FIXED_KW)
    assert (want[1], want[2], len(want[3]), len(trace)) == (-3, n_updates, n_updates + 1,
                                                            n_updates + 1)
    return prob, bounds, b, want, trace


def prefix(want, trace, m):
    return trace[m], -3, m, want[3][:m + 1], want[4]


# ---------------------------------------------------------------------------------------------
# fixed numbers of updates: every residue of the three-buffer (y) and two-buffer (r) rotations and
# the special first update, on every operator / PC path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["jacobi", "none", "jacobi_deltas", "sor", "mg", "fft",
                                  "compact_fft", "assembled_jacobi"])
def test_fixed_updates(ctx, name):
    prob, bounds, b, want, trace = fixed_run(name)
    for m in range(1, 8):
        got = gpu_solve(ctx, prob, b, cheb_argv(bounds, max_it=m))  # (x pre-filled with 7.25)
        check(prob, got, prefix(want, trace, m), tag=f"fixed {name} {m} updates")


SHAPES = [((24, 20, 12), None), ((17, 18, 9), None), ((130, 6, 33), None), ((16, 16, 16), None),
          ((1024, 1024, 4), None), ((24, 20, 12), (0.05, 0.03, 0.07))]


@pytest.mark.parametrize("n3,deltas", SHAPES, ids=[f"{s[0]}-{s[1]}" for s in SHAPES])
def test_fused_pass_shapes(ctx, tune, n3, deltas):
    """The shapes of the Richardson fused-pass tests (even / odd x, 4 / 2 / 1 rows per wave, odd z,
    more than one x segment, 1024-wide planes with 8-row tiles, unequal spacing): 7 updates against
    the restatement, and cheb_fused = 0 (vector kernel + the engine's residual pass) gives the
    same bits."""
    prob = Problem(n3, deltas=deltas)
    b = prob.rhs()
    bounds = (0.05, 2.0)
    want = chebyshev(prob, b, *bounds, max_it=7, **FIXED_KW)
    out = {}
    for fused in (1, 0):
        tune.set("cheb_fused", fused)
        out[fused] = gpu_solve(ctx, prob, b, cheb_argv(bounds, max_it=7))
    check(prob, out[1], want, tag=f"fused {n3} {deltas}")
    assert out[0][:2] == out[1][:2]
    assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])


@pytest.mark.parametrize("name", ["none", "mg", "fft"])
def test_fused_equals_unfused(ctx, tune, name):
    prob, bounds, b, want, trace = fixed_run(name)
    out = {}
    for fused in (1, 0):
        tune.set("cheb_fused", fused)
        out[fused] = gpu_solve(ctx, prob, b, cheb_argv(bounds, max_it=7))
    check(prob, out[0], want, tag=f"unfused {name}")
    assert out[0][:2] == out[1][:2]
    assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])


# ---------------------------------------------------------------------------------------------
# stopping
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cube():
    prob = Problem((16, 16, 16))
    return prob, prob.rhs(), jacobi_spectrum(prob)


def test_jacobi_converges_like_the_restatement(ctx):
    prob, b, bounds = cube()
    want = chebyshev(prob, b, *bounds, rtol=1e-8)
    assert want[1] == 2 and ttol_margin_ok(want[3], 1e-8, want[4]), "seed too close to ttol"
    got = gpu_solve(ctx, prob, b, cheb_argv(bounds, rtol=1e-8))
    check(prob, got, want, tag="jacobi 16^3 rtol 1e-8", floor=HIST_FLOOR)
    res = np.linalg.norm(b - prob.apply(got[3])) / np.linalg.norm(b)
    assert res < 1e-7, res


def test_mg_estimated_bounds_converge_like_the_restatement(ctx):
    """The solve estimates its bounds; the restatement runs with the bounds the GPU reports."""
    prob = Problem((32, 32, 32), pc="mg")
    b = prob.rhs()
    da = pb.DA(ctx, prob.n3)
    P, A = prob.mats(pb, da)
    x, bv = pb.Vec(da), pb.Vec(da)
    bv.set_values(b)
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", "mg"] + cheb_argv(rtol=1e-8)))
    reason, its, hist = k.solve(bv, x)
    emin, emax, estimated = k.chebyshev_eigenvalues()
    assert estimated and 0.0 < emin < emax
    want = chebyshev(prob, b, emin, emax, rtol=1e-8)
    assert want[1] == 2 and ttol_margin_ok(want[3], 1e-8, want[4]), "seed too close to ttol"
    check(prob, (reason, its, np.asarray(hist), x.get_values(), k.result.rnorm0, k.result.rnorm,
                 k.result.nhist), want, tag="mg 32^3 estimated bounds", floor=HIST_FLOOR)
    k.destroy()


def test_converged_atol(ctx):
    prob, b, bounds = cube()
    z0 = chebyshev(prob, b, *bounds, max_it=0, **FIXED_KW)[3][0]
    kw = dict(rtol=0.0, atol=float(1e-3 * z0))
    want = chebyshev(prob, b, *bounds, **kw)
    assert want[1] == 3 and ttol_margin_ok(want[3], 0.0, want[4], atol=kw["atol"])
    argv = cheb_argv(bounds, extra=["-ksp_rtol", "0", "-ksp_atol", repr(kw["atol"])])
    check(prob, gpu_solve(ctx, prob, b, argv), want, tag="atol", floor=HIST_FLOOR)


def test_too_small_emax_diverges(ctx):
    prob, b, _ = cube()
    want = chebyshev(prob, b, 0.0254, 1.5)
    assert want[1] == -4 and want[3][-1] >= 1.001e5 * want[4] > 1e5 * want[4] > 1.001 * want[3][-2]
    check(prob, gpu_solve(ctx, prob, b, cheb_argv((0.0254, 1.5))), want, tag="dtol")


def test_diverged_its(ctx):
    prob, b, bounds = cube()
    want = chebyshev(prob, b, *bounds, rtol=1e-8, max_it=5)
    assert (want[1], want[2]) == (-3, 5)
    argv = cheb_argv(bounds, rtol=1e-8, extra=["-ksp_max_it", "5"])
    check(prob, gpu_solve(ctx, prob, b, argv), want, tag="its")
    want = chebyshev(prob, b, *bounds, max_it=0, **FIXED_KW)
    got = gpu_solve(ctx, prob, b, cheb_argv(bounds, max_it=0))
    check(prob, got, want, tag="max_it 0")
    assert np.all(got[3] == 0.0)


@pytest.mark.parametrize("pc", ["jacobi", "mg"])
def test_nan_in_b(ctx, pc):
    prob = Problem((16, 16, 12), pc=pc)
    b = prob.rhs()
    b[37] = np.nan
    reason, its, hist, _, _, _, nhist = gpu_solve(ctx, prob, b, cheb_argv((0.1, 1.1)))
    assert (reason, its, nhist) == (-9, 0, 1) and np.isnan(hist[0])


def test_long_run_stays_finite(ctx):
    """1500 updates with the default estimate's bounds at 16^3: PETSc's c_k recurrence is past
    1e78 after 290 of them and overflows near 1100; the ratio recurrence keeps every norm finite."""
    prob, b, _ = cube()
    reason, its, hist, xs, _, _, nhist = gpu_solve(ctx, prob, b, cheb_argv((0.196, 2.155),
                                                                           max_it=1500))
    assert (reason, its, nhist) == (-3, 1500, 1501)
    assert np.all(np.isfinite(hist)) and np.all(np.isfinite(xs))
    assert hist[-1] < 1e-10 * hist[0]


# ---------------------------------------------------------------------------------------------
# nonzero guess, projected guess, the split form, reuse
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc,mode", [("jacobi", "default"), ("mg", "default"), ("jacobi", "initial"),
                                     ("mg", "min")])
def test_nonzero_guess(ctx, pc, mode):
    prob, bounds = _paths()[pc]
    b, x0 = prob.rhs(), O.fill_random(prob.N, 7)
    want = chebyshev(prob, b, *bounds, x0=x0, mode=mode, max_it=6, **FIXED_KW)
    extra = ["-ksp_initial_guess_nonzero"] + {
        "default": [], "initial": ["-ksp_converged_use_initial_residual_norm"],
        "min": ["-ksp_converged_use_min_initial_residual_norm"]}[mode]
    got = gpu_solve(ctx, prob, b, cheb_argv(bounds, max_it=6, extra=extra), x0=x0)
    check(prob, got, want, tag=f"guess {pc} {mode}")
    if mode == "default":  # rnorm0 is the ||z_0|| a zero-guess solve of b logs
        zb = prob.remove(prob.pc_apply(b))
        ref = float(np.sqrt(np.sum(zb * zb)))
        assert abs(got[4] - ref) <= HIST_RTOL * ref and got[4] != got[2][0]


def test_fischer_time_loop(ctx):
    """-ksp_guess_type fischer through the solve wrapper: b_k = b + 0.01 k c; every step converges
    to the restated stopping rule, the later ones in fewer updates than the first."""
    prob = Problem((16, 16, 12), pc="mg")
    b, c = prob.rhs(), prob.rhs(seed=99)
    da = pb.DA(ctx, prob.n3)
    P, A = prob.mats(pb, da)
    x, bv = pb.Vec(da), pb.Vec(da)
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", "mg", "-ksp_guess_type", "fischer"]
                                    + cheb_argv(rtol=1e-8)))
    its_all = []
    for step in range(3):
        bk = b + 0.01 * step * c
        bv.set_values(bk)
        reason, its, hist = k.solve(bv, x)
        assert reason == 2 and len(hist) == its + 1
        zb = prob.remove(prob.pc_apply(bk))
        ref = float(np.sqrt(np.sum(zb * zb)))
        assert abs(k.result.rnorm0 - ref) <= HIST_RTOL * ref
        # the restated norm of the residual the solve left is the last norm it logged
        z = prob.remove(prob.pc_apply(bk - prob.apply(x.get_values())))
        zn = float(np.sqrt(np.sum(z * z)))
        assert zn <= 1e-8 * ref * (1 + 1e-3) and abs(zn - hist[-1]) <= 1e-3 * hist[-1] + 1e-12 * ref
        its_all.append(its)
    assert k.chebyshev_eigenvalues()[2]
    k.destroy()
    assert its_all[1] < its_all[0] and its_all[2] < its_all[0], its_all


@pytest.mark.parametrize("name", ["jacobi", "mg"])
@pytest.mark.parametrize("check_every", [1, 8])
def test_split_form_and_reuse(ctx, name, check_every):
    """pb_ksp_begin / iterate(3) / iterate(4) / end is the 7-update solve; a second solve on the
    same KSP (rho restarted, the buffers holding the first solve's iterates) is the first again."""
    prob, bounds, b, want, trace = fixed_run(name)
    da = pb.DA(ctx, prob.n3)
    P, A = prob.mats(pb, da)
    x, bv = pb.Vec(da), pb.Vec(da)
    bv.set_values(b)
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", prob.pc] + cheb_argv(bounds, max_it=7),
                                    check_every=check_every))
    runs = []
    for form in ("solve", "split", "solve"):
        x.set(3.0)
        if form == "solve":
            reason, its, hist = k.solve(bv, x)
        else:
            k.begin(bv, x)
            k.iterate(3)
            k.iterate(4)
            reason, its, hist = k.end()
        runs.append((reason, its, np.asarray(hist), x.get_values(), k.result.rnorm0,
                     k.result.rnorm, k.result.nhist))
    check(prob, runs[0], want, tag=f"reuse {name} check_every {check_every}")
    for r in runs[1:]:
        assert r[:2] == runs[0][:2]
        assert np.array_equal(r[2], runs[0][2]) and np.array_equal(r[3], runs[0][3])
    k.destroy()


def test_converged_early_with_updates_enqueued(ctx):
    """A solve that converges while later updates are enqueued: those exit at entry and rotate
    nothing (the result is copied from the buffer of the device's update count)."""
    prob = Problem((16, 16, 12), pc="mg")
    b = prob.rhs()
    for rtol in (1e-2, 1e-3, 1e-4):  # (stops after different numbers of updates)
        want = chebyshev(prob, b, 0.1, 1.1, rtol=rtol)
        assert want[1] == 2 and ttol_margin_ok(want[3], rtol, want[4])
        da = pb.DA(ctx, prob.n3)
        P, A = prob.mats(pb, da)
        x, bv = pb.Vec(da), pb.Vec(da)
        bv.set_values(b)
        k = pb.KSP(A, P, pb.ksp_options(["-pc_type", "mg"] + cheb_argv((0.1, 1.1), rtol=rtol),
                                        check_every=8))
        reason, its, hist = k.solve(bv, x)
        check(prob, (reason, its, np.asarray(hist), x.get_values(), k.result.rnorm0,
                     k.result.rnorm, k.result.nhist), want, tag=f"early rtol {rtol}")
        k.destroy()


# ---------------------------------------------------------------------------------------------
# the eigenvalue estimate
# ---------------------------------------------------------------------------------------------
def _ksp(ctx, prob, argv, **kw):
    da = pb.DA(ctx, prob.n3, prob.L)
    P, A = prob.mats(pb, da)
    return pb.KSP(A, P, pb.ksp_options(["-pc_type", prob.pc] + list(argv), **kw)), A, P, da


@pytest.mark.parametrize("name", ["jacobi", "jacobi_deltas", "sor", "mg", "fft"])
def test_estimate_against_restated_lanczos(ctx, name):
    prob = _paths()[name][0]
    lo, hi, m = lanczos(prob)
    assert m == (1 if name == "fft" else 10)
    # the default transform: 0.1 and 1.1 times the largest
    k = _ksp(ctx, prob, cheb_argv())[0]
    emin, emax, estimated = k.chebyshev_eigenvalues()
    print(f"estimate {name}: gpu {emin!r} {emax!r} restated {0.1 * hi!r} {1.1 * hi!r}")
    assert estimated
    assert abs(emax - 1.1 * hi) <= EST_MAX_RTOL * abs(1.1 * hi)
    assert abs(emin - 0.1 * hi) <= EST_MAX_RTOL * abs(0.1 * hi)
    assert k.chebyshev_eigenvalues() == (emin, emax, True)  # (kept, not run again)
    k.destroy()
    # the extremes themselves, and another step count
    k = _ksp(ctx, prob, cheb_argv(extra=["-ksp_chebyshev_esteig", "1,0,0,1"]))[0]
    if name == "fft":  # one step: min = max, no valid pair
        with pytest.raises(pb.PbError) as e:
            k.chebyshev_eigenvalues()
        assert e.value.code == ARG
        k.destroy()
        return
    emin, emax, _ = k.chebyshev_eigenvalues()
    assert abs(emin - lo) <= EST_MIN_RTOL * abs(lo) and abs(emax - hi) <= EST_MAX_RTOL * abs(hi)
    k.destroy()
    lo4, hi4, _ = lanczos(prob, steps=4)
    k = _ksp(ctx, prob, cheb_argv(extra=["-ksp_chebyshev_esteig_steps", "4"]))[0]
    assert abs(k.chebyshev_eigenvalues()[1] - 1.1 * hi4) <= EST_MAX_RTOL * 1.1 * hi4
    k.destroy()


def test_estimated_bounds_history_parity(ctx):
    """Jacobi on the engine path with estimated bounds: the restatement runs with the reported
    bounds; a changed spacing runs the estimate again."""
    prob = Problem((16, 16, 12))
    b = prob.rhs()
    da = pb.DA(ctx, prob.n3)
    P, A = prob.mats(pb, da)
    x, bv = pb.Vec(da), pb.Vec(da)
    bv.set_values(b)
    k = pb.KSP(A, P, pb.ksp_options(cheb_argv(max_it=6)))
    reason, its, hist = k.solve(bv, x)
    emin, emax, estimated = k.chebyshev_eigenvalues()
    assert estimated and abs(emax - estimate(prob)[1]) <= EST_MAX_RTOL * emax
    want = chebyshev(prob, b, emin, emax, max_it=6, **FIXED_KW)
    check(prob, (reason, its, np.asarray(hist), x.get_values(), k.result.rnorm0, k.result.rnorm,
                 k.result.nhist), want, tag="estimated bounds jacobi")
    other = Problem((16, 16, 12), deltas=(0.05, 0.03, 0.07))
    A.set_deltas(other.h)
    P.set_deltas(other.h)
    e2 = k.chebyshev_eigenvalues()
    assert e2[2] and abs(e2[1] - estimate(other)[1]) <= EST_MAX_RTOL * e2[1] and e2[1] != emax
    k.destroy()


def test_negative_spectrum_needs_bounds(ctx):
    """-pc_type none: the spectrum is negative and the default transform gives no valid pair; the
    solve says so and the KSP and the context stay usable."""
    prob = Problem((16, 16, 12), pc="none")
    b = prob.rhs()
    k, A, P, da = _ksp(ctx, prob, cheb_argv(max_it=3))
    x, bv = pb.Vec(da), pb.Vec(da)
    bv.set_values(b)
    for call in (lambda: k.solve(bv, x), lambda: k.begin(bv, x), k.chebyshev_eigenvalues):
        with pytest.raises(pb.PbError) as e:
            call()
        assert e.value.code == ARG and "estimate" in str(e.value)
    z = pb.Vec(da)
    k.pc_apply(bv, z)
    assert np.array_equal(z.get_values(), b)
    k.destroy()
    # a transform that keeps the order works: emin = 1.1 min, emax = 0.1 min
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", "none"] + cheb_argv(max_it=3),
                                    chebyshev_esteig=(1.1, 0.0, 0.1, 0.0)))
    lo = lanczos(prob)[0]
    emin, emax, estimated = k.chebyshev_eigenvalues()
    assert estimated and emin < emax < 0.0 and abs(emin - 1.1 * lo) <= EST_MIN_RTOL * abs(emin)
    want = chebyshev(prob, b, emin, emax, max_it=3, **FIXED_KW)
    reason, its, hist = k.solve(bv, x)
    check(prob, (reason, its, np.asarray(hist), x.get_values(), k.result.rnorm0, k.result.rnorm,
                 k.result.nhist), want, tag="none, estimated negative bounds")
    k.destroy()


def test_explicit_bounds_and_errors(ctx):
    prob = Problem((16, 16, 12))
    k, A, P, da = _ksp(ctx, prob, cheb_argv((0.05, 2.0)))
    assert k.chebyshev_eigenvalues() == (0.05, 2.0, False)
    x, b = pb.Vec(da), pb.Vec(da)
    b.set(1.0)
    with pytest.raises(pb.PbError) as e:
        k.solve(b, b)
    assert e.value.code == ARG
    k.destroy()
    for argv in (["-ksp_type", "cg"], ["-ksp_type", "richardson"]):
        k = pb.KSP(A, P, pb.ksp_options(argv))
        with pytest.raises(pb.PbError) as e:
            k.chebyshev_eigenvalues()
        assert e.value.code == STATE
        k.destroy()
    for kw in (dict(chebyshev_emin=2.0, chebyshev_emax=0.1), dict(chebyshev_emin=-1.0,
               chebyshev_emax=1.0), dict(chebyshev_emax=1.0), dict(chebyshev_esteig_steps=0),
               dict(chebyshev_esteig_steps=65), dict(chebyshev_emin=float("nan"),
               chebyshev_emax=1.0), dict(chebyshev_esteig=(0.0, 0.1, 0.0, float("inf")))):
        with pytest.raises(pb.PbError) as e:
            pb.KSP(A, P, pb.ksp_options(["-ksp_type", "chebyshev"], **kw))
        assert e.value.code == ARG, kw
    # -ksp_cg_single_reduction is ignored
    k = pb.KSP(A, P, pb.ksp_options(cheb_argv((0.05, 2.0), max_it=2)
                                    + ["-ksp_cg_single_reduction"]))
    b.set_values(prob.rhs())
    assert k.solve(b, x)[:2] == (-3, 2)
    k.destroy()


# ---------------------------------------------------------------------------------------------
# N ranks over the host transport (one GPU, one thread per rank)
# ---------------------------------------------------------------------------------------------
def _multirank(prob, b, want, argv, nranks, tag, est=None):
    from test_gpu_parity import run_ranks

    def body(ctx, rank):
        k0, nk = pb.slab_partition(prob.n3[2], nranks, rank)
        got = gpu_solve(ctx, prob, b, argv, rows=(k0, nk))
        bounds = None
        if est is not None:
            k = _ksp(ctx, prob, cheb_argv())[0]
            bounds = k.chebyshev_eigenvalues()
            k.destroy()
        return (k0, nk), got, bounds

    for rows, got, bounds in run_ranks(nranks, body):
        check(prob, got, want, rows=rows, tag=f"{tag} rows {rows}")
        if est is not None:
            assert bounds[2] and abs(bounds[1] - est[1]) <= EST_MAX_RTOL * est[1], (bounds, est)
            assert abs(bounds[0] - est[0]) <= EST_MAX_RTOL * est[0]


@pytest.mark.parametrize("nranks,n3", [(2, (16, 16, 12)), (3, (20, 16, 7))])
def test_multirank_jacobi(nranks, n3):
    prob = Problem(n3)
    b = prob.rhs()
    bounds = (0.05, 2.0)
    want = chebyshev(prob, b, *bounds, max_it=6, **FIXED_KW)
    _multirank(prob, b, want, cheb_argv(bounds, max_it=6), nranks, f"{nranks} ranks {n3}",
               est=estimate(prob) if nranks == 2 else None)


@pytest.mark.parametrize("nranks", [2, 3])
def test_multirank_mg(nranks):
    prob = Problem((16, 16, 12), pc="mg")
    b = prob.rhs(nranks=nranks)
    want = chebyshev(prob, b, 0.1, 1.1, max_it=6, nranks=nranks, **FIXED_KW)
    _multirank(prob, b, want, cheb_argv((0.1, 1.1), max_it=6), nranks, f"{nranks} ranks mg",
               est=estimate(prob, nranks=nranks) if nranks == 2 else None)
