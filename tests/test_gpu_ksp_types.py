"""GPU tier: -ksp_type preonly and -ksp_type richardson against their numpy restatement
(tests/ksp_types_restatement.py; semantics in DESIGN.md §3.1e, "parity unpinned": PETSc is not
available, so KSPSolve_PREONLY / KSPSolve_Richardson are pinned to the restatement only).

Bars: tests/parity_bars.py -- HIST_RTOL, HIST_RTOL_PC for sor / mg, X_RTOL (check_x's default).
With the spectral PC one update reaches rounding level: as test_gpu_initial_guess.check does, ||z_0|| is held to 1e-12
and the later (rounding-noise) norms to 1e-10 ||z_0|| absolute. Iteration counts must match the
restatement exactly, so the stopping cases assert on the restatement's own norms that the last two
are more than 1e-6 (relative) from ttol.

Richardson recomputes the true residual r = b - A x every iteration (CG updates it by recurrence),
so a norm far below ||z_0|| carries the rounding of x: two runs whose x differ in the last bit
(the mean is summed in another order) differ in r by about eps |A| |x|, whatever r's size. Measured
on the MI355X: the sor / mg runs of 6 or 8 updates stay inside HIST_RTOL_PC, the mg runs taken to
rtol 1e-8 (norms 1e-8 ||z_0||) differ from the restatement by up to 2.0e-9 relative, i.e. 2e-17
||z_0|| absolute. The paths compared under the parity bars therefore run their six updates; the
runs to rtol 1e-8, where the stopping iteration is the point, assert reason and count and hold
the history to HIST_RTOL_PC relative plus a floor of 1e-14 ||z_0|| (HIST_FLOOR: ~100 eps; a
perturbation of x by a few eps moves N(M^-1 (b - A x)) by a few eps ||M^-1 A|| ||x||, and with
multigrid ||M^-1 A|| is about 1 and ||x|| about ||z_0|| = ||M^-1 b||).

Every test here fails without the feature: -ksp_type preonly|richardson is PB_ERR_UNSUPPORTED.
Reference: src/poissbox.f90:269-298 (solve -> KSPSetFromOptions -> KSPSolve).
"""
import functools

import numpy as np
import pytest

import poissbox_amd as pb
from oracle import oracle as O
from ksp_types_restatement import Problem, preonly, richardson, ttol_margin_ok
from parity_bars import HIST_RTOL, HIST_RTOL_PC, check_history, check_x

pytestmark = pytest.mark.gpu

ARG, UNSUPPORTED = 1, 5
FIXED = ["-ksp_rtol", "0", "-ksp_atol", "0", "-ksp_divtol", "1e300"]
FIXED_KW = dict(rtol=0.0, atol=0.0, dtol=1e300)
HIST_FLOOR = 1e-14  # of ||z_0||, absolute, beside the relative bar (module docstring)


def gpu_solve(ctx, prob, b, argv, x0=None, rows=None):
    """One solve on ctx; rows = (k0, nk): this rank's planes of the global arrays.
    Returns (reason, its, history, x, rnorm0, rnorm, nhist)."""
    da = pb.DA(ctx, prob.n3, prob.L)
    P, A = prob.mats(pb, da)
    x, bv = pb.Vec(da), pb.Vec(da)
    cut = (lambda v: v) if rows is None else (
        lambda v: v.reshape(prob.n3[2], -1)[rows[0]:rows[0] + rows[1]])
    bv.set_values(cut(b))
    # (a zero-guess solve must overwrite whatever x holds)
    x.set_values(cut(x0 if x0 is not None else np.full(prob.N, 7.25)))
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", prob.pc] + list(argv)))
    try:
        reason, its, hist = k.solve(bv, x)
        res = k.result
        return (reason, its, np.asarray(hist), x.get_values(), res.rnorm0, res.rnorm, res.nhist)
    finally:
        k.destroy()
        for o in {A, P, x, bv}:
            o.destroy()
        da.destroy()


def check(prob, got, want, rows=None, tag="", floor=0.0):
    reason, its, hist, xs, rnorm0, rnorm, nhist = got
    xo, ro, itso, ho, ref = want
    print(f"{tag} gpu reason {reason} its {its} rnorm0 {rnorm0:.17g} | restated reason {ro} its "
          f"{itso} rnorm0 {ref:.17g}")
    assert (reason, its) == (ro, itso), (tag, reason, its, ro, itso)
    assert nhist == len(ho) == len(hist), (tag, nhist, len(ho))
    if len(ho):
        assert nhist == its + 1
        if prob.pc == "fft":
            assert abs(hist[0] - ho[0]) / ho[0] < 1e-12
            assert np.max(np.abs(hist[1:] - ho[1:]), initial=0.0) / ho[0] < 1e-10
        else:
            bar = HIST_RTOL_PC if prob.pc in ("mg", "sor") else HIST_RTOL
            if floor:
                excess = np.abs(hist - ho) - floor * ho[0]
                print(f"{tag} max relative ||z_k|| difference {np.max(np.abs(hist - ho) / ho):.3e}")
                assert np.all(excess < bar * ho), (tag, float(np.max(excess / ho)))
            else:
                check_history(hist, ho, bar=bar, tag=tag)
        assert abs(rnorm0 - ref) <= HIST_RTOL * ref, (tag, rnorm0, ref)
        assert rnorm == hist[-1]
    if rows is None:
        check_x(xs, xo, tag=tag)
    else:
        check_x(xs, xo.reshape(prob.n3[2], -1)[rows[0]:rows[0] + rows[1]].reshape(-1),
                scale=float(np.max(np.abs(xo))), tag=tag)


def rich_argv(scale=1.0, max_it=None, rtol=None, extra=()):
    a = ["-ksp_type", "richardson", "-ksp_richardson_scale", repr(float(scale))]
    if max_it is not None:
        a += FIXED + ["-ksp_max_it", str(max_it)]
    if rtol is not None:
        a += ["-ksp_rtol", repr(float(rtol))]
    return a + list(extra)


@functools.lru_cache(maxsize=None)
def fixed_case(n3, pc, deltas=None, max_it=6, scale=2.0 / 3.0):
    """(problem, b, restated damped iteration): computed once, shared by the tests that need it."""
    prob = Problem(n3, pc=pc, deltas=deltas)
    b = prob.rhs()
    want = richardson(prob, b, scale=scale, max_it=max_it, **FIXED_KW)
    assert (want[1], want[2], len(want[3])) == (-3, max_it, max_it + 1)
    return prob, b, want


# ---------------------------------------------------------------------------------------------
# preonly
# ---------------------------------------------------------------------------------------------
PREONLY = {"fft": Problem((32, 40, 48), pc="fft"),
           "compact_fft": Problem((32, 32, 32), pc="fft", op="compact"),
           "mg": Problem((16, 16, 12), pc="mg"), "sor": Problem((16, 16, 12), pc="sor"),
           "jacobi": Problem((16, 16, 12)), "none": Problem((16, 16, 12), pc="none")}


@pytest.mark.parametrize("name", list(PREONLY))
def test_preonly(ctx, name):
    prob = PREONLY[name]
    # a right-hand side with a mean: the null-space removal has something to remove
    b = prob.rhs() + (0.0 if prob.pc == "fft" else 0.5)
    want = preonly(prob, b)
    got = gpu_solve(ctx, prob, b, ["-ksp_type", "preonly"])
    reason, its, hist, xs, rnorm0, rnorm, nhist = got
    assert (reason, its, rnorm, rnorm0, nhist) == (4, 1, 0.0, 0.0, 0) and len(hist) == 0
    check(prob, got, want, tag=f"preonly {name}")
    if prob.pc == "fft":
        # the direct solve: the true residual of the mean-free system, against the oracle's own
        bm, nb = b - b.mean(), float(np.linalg.norm(b))
        res_gpu = float(np.linalg.norm(bm - prob.apply(xs))) / nb
        res_ref = float(np.linalg.norm(bm - prob.apply(want[0]))) / nb
        print(f"preonly {name}: ||(b - mean b) - A x|| / ||b|| gpu {res_gpu:.3e} oracle {res_ref:.3e}"
              f" |mean x| / max|x| {abs(xs.mean()) / np.max(np.abs(xs)):.3e}")
        assert res_gpu <= 10 * res_ref


def test_preonly_without_nullspace(ctx):
    prob = Problem((16, 16, 12), nullspace=0)
    b = prob.rhs() + 0.5
    da = pb.DA(ctx, prob.n3)
    P, A = prob.mats(pb, da)
    x, bv = pb.Vec(da), pb.Vec(da)
    bv.set_values(b)
    k = pb.KSP(A, P, pb.ksp_options(["-ksp_type", "preonly"], nullspace=0))
    k.solve(bv, x)
    check_x(x.get_values(), preonly(prob, b)[0], tag="preonly nullspace 0")
    # D^-1 (b + 0.5) keeps its mean 0.5 / diag
    assert abs(x.get_values().mean() - 0.5 / O.diag(prob.h)) <= 1e-12
    k.destroy()


def test_preonly_errors(ctx):
    da = pb.DA(ctx, (16, 16, 12))
    A = pb.Mat(da, pb.STAR7)
    x, b = pb.Vec(da), pb.Vec(da)
    b.set(1.0)
    for argv in (["-ksp_initial_guess_nonzero"], ["-ksp_guess_type", "fischer"]):
        with pytest.raises(pb.PbError) as e:
            pb.KSP(A, A, pb.ksp_options(["-ksp_type", "preonly"] + argv))
        assert e.value.code == ARG, argv
    with pytest.raises(pb.PbError) as e:
        pb.KSP(A, A, pb.ksp_options(ksp_type=7))
    assert e.value.code == UNSUPPORTED
    with pytest.raises(pb.PbError) as e:
        pb.KSP(A, A, pb.ksp_options(["-ksp_type", "richardson"], richardson_scale=float("nan")))
    assert e.value.code == ARG
    k = pb.KSP(A, A, pb.ksp_options(["-ksp_type", "preonly", "-ksp_cg_single_reduction"]))
    with pytest.raises(pb.PbError) as e:
        k.solve(b, b)
    assert e.value.code == ARG
    for call in (lambda: k.begin(b, x), lambda: k.iterate(1), lambda: k.end()):
        with pytest.raises(pb.PbError) as e:
            call()
        assert e.value.code == UNSUPPORTED
    assert k.solve(b, x)[:2] == (4, 1)  # still usable
    k.destroy()


# ---------------------------------------------------------------------------------------------
# richardson: the fused update + residual pass, its shapes
# ---------------------------------------------------------------------------------------------
SHAPES = [((24, 20, 12), None), ((17, 18, 9), None), ((130, 6, 33), None), ((16, 16, 16), None),
          ((1024, 1024, 4), None), ((24, 20, 12), (0.05, 0.03, 0.07))]


@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("n3,deltas", SHAPES, ids=[f"{s[0]}-{s[1]}" for s in SHAPES])
def test_fused_pass_shapes(ctx, n3, deltas, pc):
    """Even / odd x (two / one point per lane), 4 / 2 / 1 rows per wave, odd z, more than one x
    segment, 1024-wide planes (8-row tiles and the residency cap), non-uniform spacing: damped
    iteration, 6 updates, 7 norms. (Without a PC the iteration grows; nothing stops it here.)"""
    prob, b, want = fixed_case(n3, pc, deltas)
    got = gpu_solve(ctx, prob, b, rich_argv(2.0 / 3.0, max_it=6))
    assert len(got[2]) == 7
    check(prob, got, want, tag=f"fused {n3} {deltas} {pc}")


@pytest.mark.parametrize("n3,pc", [((24, 20, 12), "jacobi"), ((17, 18, 9), "jacobi"),
                                   ((130, 6, 33), "none"), ((16, 16, 12), "mg")])
def test_fused_equals_unfused(ctx, tune, n3, pc):
    """rich_fused = 0 (vector kernel + the engine's residual pass) against 1: the same bits."""
    prob, b, want = fixed_case(n3, pc)
    out = {}
    for fused in (1, 0):
        tune.set("rich_fused", fused)
        out[fused] = gpu_solve(ctx, prob, b, rich_argv(2.0 / 3.0, max_it=6))
    check(prob, out[0], want, tag=f"unfused {n3} {pc}")
    assert out[0][:2] == out[1][:2]
    assert np.array_equal(out[0][2], out[1][2]) and np.array_equal(out[0][3], out[1][3])


@pytest.mark.parametrize("check_every", [1, 8])
@pytest.mark.parametrize("max_it", [1, 2, 3, 4])
def test_buffer_parity(ctx, max_it, check_every):
    """x ping-pongs between the caller's vector and the KSP's: the caller's holds the result after
    an odd or an even number of updates, whatever was enqueued ahead of the poll."""
    prob, b, want = fixed_case((24, 20, 12), "jacobi", None, max_it)
    da = pb.DA(ctx, prob.n3)
    P, A = prob.mats(pb, da)
    x, bv = pb.Vec(da), pb.Vec(da)
    bv.set_values(b)
    x.set(3.0)
    k = pb.KSP(A, P, pb.ksp_options(rich_argv(2.0 / 3.0, max_it=max_it), check_every=check_every))
    reason, its, hist = k.solve(bv, x)
    got = (reason, its, np.asarray(hist), x.get_values(), k.result.rnorm0, k.result.rnorm,
           k.result.nhist)
    check(prob, got, want, tag=f"parity max_it {max_it} check_every {check_every}")
    # the split form, one update at a time
    k.begin(bv, x)
    for _ in range(max_it + 2):
        k.iterate(1)
    reason2, its2, hist2 = k.end()
    assert (reason2, its2) == (reason, its) and np.array_equal(hist2, hist)
    assert np.array_equal(x.get_values(), got[3])
    k.destroy()


def test_buffer_parity_converged_early(ctx):
    """A solve that converges while later updates are enqueued: those exit at entry and flip
    nothing."""
    prob = Problem((16, 16, 12), pc="mg")
    b = prob.rhs()
    for rtol in (1e-3, 1e-4):  # (stops after different numbers of updates)
        want = richardson(prob, b, rtol=rtol)
        assert want[1] == 2 and ttol_margin_ok(want[3], rtol, want[4])
        da = pb.DA(ctx, prob.n3)
        P, A = prob.mats(pb, da)
        x, bv = pb.Vec(da), pb.Vec(da)
        bv.set_values(b)
        k = pb.KSP(A, P, pb.ksp_options(["-pc_type", "mg"] + rich_argv(rtol=rtol), check_every=8))
        reason, its, hist = k.solve(bv, x)
        check(prob, (reason, its, np.asarray(hist), x.get_values(), k.result.rnorm0,
                     k.result.rnorm, k.result.nhist), want, tag=f"early rtol {rtol}")
        k.destroy()


# ---------------------------------------------------------------------------------------------
# stopping
# ---------------------------------------------------------------------------------------------
def test_mg_converges_like_the_restatement(ctx):
    prob = Problem((32, 32, 32), pc="mg")
    b = prob.rhs()
    want = richardson(prob, b, rtol=1e-8)
    assert (want[1], want[2]) == (2, 20), want[1:3]
    assert ttol_margin_ok(want[3], 1e-8, want[4]), "seed too close to ttol"
    check(prob, gpu_solve(ctx, prob, b, rich_argv(rtol=1e-8)), want, tag="mg 32^3", floor=HIST_FLOOR)


def test_overrelaxed_jacobi_diverges(ctx):
    prob = Problem((17, 18, 9))
    b = prob.rhs()
    want = richardson(prob, b, scale=2.5)
    assert (want[1], want[2], len(want[3])) == (-4, 10, 11)
    check(prob, gpu_solve(ctx, prob, b, rich_argv(2.5)), want, tag="dtol")


def test_sor_fixed_iterations(ctx):
    prob, b, want = fixed_case((32, 32, 32), "sor", None, 8, 1.0)
    check(prob, gpu_solve(ctx, prob, b, rich_argv(1.0, max_it=8)), want, tag="sor 32^3")


@pytest.mark.parametrize("pc", ["jacobi", "mg"])
def test_nan_in_b(ctx, pc):
    prob = Problem((16, 16, 12), pc=pc)
    b = prob.rhs()
    b[37] = np.nan
    reason, its, hist, _, _, _, nhist = gpu_solve(ctx, prob, b, rich_argv())
    assert (reason, its, nhist) == (-9, 0, 1) and np.isnan(hist[0])


def test_max_it_zero(ctx):
    prob = Problem((16, 16, 12))
    b = prob.rhs()
    want = richardson(prob, b, max_it=0, **FIXED_KW)
    assert (want[1], want[2]) == (-3, 0)
    got = gpu_solve(ctx, prob, b, rich_argv(max_it=0))
    check(prob, got, want, tag="max_it 0")
    assert np.all(got[3] == 0.0)


# ---------------------------------------------------------------------------------------------
# every operator / PC path
# ---------------------------------------------------------------------------------------------
def _paths():
    none = Problem((16, 16, 12), pc="none")
    return {
        # without a PC the damping carries the diagonal (a negative scale: diag(P) < 0)
        "none": (none, dict(scale=(2.0 / 3.0) / O.diag(none.h), max_it=6)),
        "jacobi": (Problem((16, 16, 12)), dict(scale=2.0 / 3.0, max_it=6)),
        "sor": (Problem((16, 16, 12), pc="sor"), dict(max_it=6)),
        "mg": (Problem((16, 16, 12), pc="mg"), dict(max_it=6)),
        "fft": (Problem((32, 40, 48), pc="fft"), dict(rtol=1e-8)),
        "compact_fft": (Problem((64, 64, 64), pc="fft", op="compact"), dict(rtol=1e-8)),
        "assembled_jacobi": (Problem((16, 16, 12), op="assembled"), dict(scale=2.0 / 3.0, max_it=6)),
        "compact_jacobi": (Problem((16, 16, 16), op="compact"), dict(scale=0.5, max_it=6)),
    }


@pytest.mark.parametrize("name", ["none", "jacobi", "sor", "mg", "fft", "compact_fft",
                                  "assembled_jacobi", "compact_jacobi"])
def test_every_path(ctx, name):
    prob, kw = _paths()[name]
    b = prob.rhs()
    scale, max_it, rtol = kw.get("scale", 1.0), kw.get("max_it"), kw.get("rtol")
    if max_it is not None:
        want = richardson(prob, b, scale=scale, max_it=max_it, **FIXED_KW)
    else:
        want = richardson(prob, b, scale=scale, rtol=rtol)
        assert want[1] == 2 and ttol_margin_ok(want[3], rtol, want[4])
    if name == "fft":  # the direct solve plus one residual check
        assert want[2] == 1 and want[3][1] < 1e-12 * want[3][0], want[3]
    check(prob, gpu_solve(ctx, prob, b, rich_argv(scale, max_it=max_it, rtol=rtol)), want,
          tag=f"path {name}")


# ---------------------------------------------------------------------------------------------
# nonzero guess, projected guess
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc,mode", [("jacobi", "default"), ("mg", "default"), ("jacobi", "initial"),
                                     ("mg", "min")])
def test_nonzero_guess(ctx, pc, mode):
    prob = Problem((16, 16, 12), pc=pc)
    b, x0 = prob.rhs(), O.fill_random(prob.N, 7)
    scale = 2.0 / 3.0 if pc == "jacobi" else 1.0
    want = richardson(prob, b, x0=x0, scale=scale, mode=mode, max_it=6, **FIXED_KW)
    extra = ["-ksp_initial_guess_nonzero"] + {
        "default": [], "initial": ["-ksp_converged_use_initial_residual_norm"],
        "min": ["-ksp_converged_use_min_initial_residual_norm"]}[mode]
    argv = rich_argv(scale, max_it=6, extra=extra)
    got = gpu_solve(ctx, prob, b, argv, x0=x0)
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
                                    + rich_argv(rtol=1e-8)))
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
    k.destroy()
    assert its_all[1] < its_all[0] and its_all[2] < its_all[0], its_all


# ---------------------------------------------------------------------------------------------
# N ranks over the host transport (one GPU, one thread per rank)
# ---------------------------------------------------------------------------------------------
def _multirank(prob, b, want, argv, nranks, tag, floor=0.0):
    from test_gpu_parity import run_ranks

    def body(ctx, rank):
        k0, nk = pb.slab_partition(prob.n3[2], nranks, rank)
        return (k0, nk), gpu_solve(ctx, prob, b, argv, rows=(k0, nk))

    for rows, got in run_ranks(nranks, body):
        check(prob, got, want, rows=rows, tag=f"{tag} rows {rows}", floor=floor)


@pytest.mark.parametrize("nranks,n3", [(2, (16, 16, 12)), (3, (20, 16, 7)), (2, (16, 16, 4))])
def test_multirank_jacobi(nranks, n3):
    prob, b, want = fixed_case(n3, "jacobi")
    _multirank(prob, b, want, rich_argv(2.0 / 3.0, max_it=6), nranks, f"{nranks} ranks {n3}")


@pytest.mark.parametrize("nranks", [2, 3])
def test_multirank_mg(nranks):
    prob = Problem((16, 16, 12), pc="mg")
    b = prob.rhs(nranks=nranks)
    want = richardson(prob, b, max_it=6, nranks=nranks, **FIXED_KW)
    _multirank(prob, b, want, rich_argv(max_it=6), nranks, f"{nranks} ranks mg")
    # and to rtol 1e-8: the same stopping iteration on every rank
    want = richardson(prob, b, rtol=1e-8, nranks=nranks)
    assert want[1] == 2 and ttol_margin_ok(want[3], 1e-8, want[4])
    _multirank(prob, b, want, rich_argv(rtol=1e-8), nranks, f"{nranks} ranks mg rtol",
               floor=HIST_FLOOR)


def test_multirank_preonly_fft():
    prob = Problem((64, 64, 64), pc="fft")
    b = prob.rhs()
    _multirank(prob, b, preonly(prob, b), ["-ksp_type", "preonly"], 2, "2 ranks preonly fft")
