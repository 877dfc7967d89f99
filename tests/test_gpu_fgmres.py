"""GPU tier: -ksp_type fgmres against its numpy restatement (tests/fgmres_restatement.py; semantics
in DESIGN.md §3.1h, "parity unpinned": PETSc is not available, so KSPSolve_FGMRES is pinned to the
restatement only). The cases and their restated runs are tests/fgmres_cases.py's, computed once.

Bars. Classical Gram-Schmidt without refinement is more sensitive to the summation order than CG,
so the CG bars are not assumed: scripts/fgmres_sensitivity.py runs the restatement of every case on
the CPU under pairwise, left-to-right and exactly rounded sums and records the largest difference d
between two variants (profiles/ksp_fgmres/sensitivity.json). A case's history bar is 100 d -- the
two orders of margin parity_bars.py states -- and never below HIST_RTOL (HIST_RTOL_PC with sor /
mg; with the spectral PC the entries after the first are rounding noise and held to 1e-10 of
||r_0||, as test_gpu_ksp_types.check holds them); x likewise against X_RTOL. Measured d
(history, x), the largest of each group:
  fixed counts m = 1..7 at restart 3:  jacobi 2.0e-14, 4.9e-15; none 1.6e-14, 4.6e-15;
    jacobi_deltas 3.3e-14, 7.5e-15; sor 5.7e-14, 5.3e-15; mg 4.3e-13, 2.2e-15;
    fft 1.5e-15, 4.4e-15; compact_fft 2.2e-15, 5.1e-15; assembled_jacobi 2.0e-14, 5.0e-15
  shapes, 7 iterations at restart 4, jacobi and none: 7.8e-13, 6.2e-14 (the largest:
    1024x1024x4; the others at most 7.0e-14, 3.4e-15)
  two ranks, 7 iterations at restart 3: jacobi 2.0e-14, 1.1e-15; mg 4.3e-13, 1.2e-15
  to a tolerance: 32^3 jacobi rtol 1e-8 restart 30 (121 iterations): 1.2e-10, 1.3e-15; restart 5
    (307): 3.3e-10, 1.6e-15; 32^3 mg rtol 1e-10 (12): 9.3e-8, 7.9e-15; 32x40x48 fft (1):
    1.5e-15, 4.4e-15; refine_always (121) 2.2e-10, 1.4e-15; nonzero guess (66) 9.1e-12, 9.9e-16;
    32^3 mg rtol 1e-12 (15, the enqueue-ahead case) 1.8e-4, 7.8e-15
so x sits at X_RTOL everywhere, the fixed-count, shape and two-rank histories sit at the CG bars
but for 1024x1024x4 (7.8e-11), and the sensitivity sets the history bars of the runs to a
tolerance: 1.2e-8 and 3.3e-8 (jacobi), 9.3e-6 (mg to 1e-10) and 1.8e-2 (mg to 1e-12). With
multigrid a dozen steps take the estimate 10 to 12 orders down; |g_(k+1)| is a product of the
rotations' sines, and what the unrefined Gram-Schmidt loses of the basis' orthogonality moves its
last entries by far more than it moves x or the true residual. Reason and iteration count must be
exact where ttol_margin_ok holds on the restatement's own norms; every variant of the restatement
ends alike on every case (same_outcome in the json).

The true residual ||b - A x|| / ||b|| (O.stencil) of the runs to a tolerance may exceed the last
logged estimate by the factor the restatement itself shows on that case, times 10; the recorded
factors (||b - A x|| over the last estimate): jacobi restart 30 1.0000000001, restart 5
1.00000000004, mg 1.0000000006, fft 0.988 -- so the allowed factor is 10 on each.

On the 7-point operator with Jacobi / no PC (one rank) a step starts with one engine pass; the
null-space shift of these two paths comes from the sum of the unnormalised direction (the
multi-axpy takes it), not from a sum over z as the restatement forms it: equal in exact
arithmetic, a rounding-level difference that the bars above hold.

Every test here fails without the feature: -ksp_type fgmres is PB_ERR_UNSUPPORTED.
Reference: src/poissbox.f90:269-298 (solve -> KSPSetFromOptions -> KSPSolve).
"""
import numpy as np
import pytest

import poissbox_amd as pb
import fgmres_cases as F
from ksp_types_restatement import ttol_margin_ok
from test_gpu_ksp_types import FIXED, gpu_solve

pytestmark = pytest.mark.gpu

UNSUPPORTED, STATE = 5, 6


def argv_of(cid, extra=()):
    _, kw, ex = F.CASES[cid]
    a = ["-ksp_type", "fgmres", "-ksp_gmres_restart", str(kw.get("restart", 30))]
    if kw.get("rtol") == 0.0:
        a += FIXED
    elif "rtol" in kw:
        a += ["-ksp_rtol", repr(float(kw["rtol"]))]
    if "max_it" in kw:
        a += ["-ksp_max_it", str(kw["max_it"])]
    if kw.get("refine"):
        a += ["-ksp_gmres_cgs_refinement_type", "refine_always"]
    if kw.get("norm_none"):
        a += ["-ksp_norm_type", "none"]
    if "x0" in ex:
        a += ["-ksp_initial_guess_nonzero"]
    if kw.get("mode") == "initial":
        a += ["-ksp_converged_use_initial_residual_norm"]
    return a + list(extra)


def fg_check(cid, got, rows=None, tag=None):
    """history, x, reason, count and the result fields of one GPU solve against the case's
    restated run, within the case's bars; every figure is printed before it is asserted."""
    tag = tag or cid
    prob, b, _ = F.setup(cid)
    kw = F.CASES[cid][1]
    xo, ro, itso, ho, ref = F.restated(cid)
    reason, its, hist, xs, rnorm0, rnorm, nhist = got
    hbar, xbar, _ = F.bars(cid)
    print(f"{tag}: gpu reason {reason} its {its} | restated reason {ro} its {itso}; bars history "
          f"{hbar:.2e} x {xbar:.2e}")
    stopping = kw.get("rtol", 1e-5) > 0.0 and not kw.get("norm_none")
    if not stopping or ttol_margin_ok(ho, kw.get("rtol", 1e-5), ref):
        assert (reason, its) == (ro, itso), (tag, reason, its, ro, itso)
    assert nhist == len(hist) == its + 1, (tag, nhist, len(hist), its)
    n = min(len(hist), len(ho))
    dh = F.hist_diff(prob, hist[:n], ho[:n])
    print(f"{tag}: history difference {dh:.3e}")
    assert dh < hbar, (tag, dh, hbar)
    assert abs(rnorm0 - ref) <= 1e-11 * ref, (tag, rnorm0, ref)
    # (a solve that a restart's recomputed norm ended returns that norm, which is not logged)
    if its % kw.get("restart", 30) != 0:
        assert rnorm == hist[-1]
    if rows is not None:
        xo = xo.reshape(prob.n3[2], -1)[rows[0]:rows[0] + rows[1]].reshape(-1)
        dx = float(np.max(np.abs(xs - xo))) / float(np.max(np.abs(F.restated(cid)[0])))
    else:
        dx = F.x_diff(xs, xo)
    print(f"{tag}: x difference {dx:.3e}")
    assert np.all(np.isfinite(xs)) and dx <= xbar, (tag, dx, xbar)


def solve_case(ctx, cid, extra=(), rows=None):
    prob, b, x0 = F.setup(cid)
    return gpu_solve(ctx, prob, b, argv_of(cid, extra), x0=x0, rows=rows)


# ---------------------------------------------------------------------------------------------
# fixed iteration counts: every cycle position (restart 3: a restart at 3 and at 6, max_it inside
# a cycle) on every path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(1, 8))
@pytest.mark.parametrize("name", list(F.PATHS))
def test_fixed_counts(ctx, name, m):
    cid = f"fixed-{name}-{m}"
    got = solve_case(ctx, cid)
    assert (got[0], got[1]) == (-3, m)
    fg_check(cid, got)


@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("n3,deltas", F.SHAPES, ids=[F.shape_id(*s) for s in F.SHAPES])
def test_fused_pass_shapes(ctx, tune, n3, deltas, pc):
    """The engine pass that starts a step (v = s wt, z = D^-1 v - mean formed on load, A z
    written) on even / odd x (two / one point per lane), 4 / 2 / 1 rows per wave, odd z, more
    than one x segment, 1024-wide planes, non-uniform spacing: 7 iterations at restart 4 against
    the restatement, and the unfused sequence (fgmres_fused = 0: scale pass, Jacobi + shift pass,
    standalone operator) gives the same bits."""
    cid = F.shape_id(n3, deltas) + ("" if pc == "jacobi" else "-none")
    got = solve_case(ctx, cid)
    assert (got[0], got[1]) == (-3, 7)
    fg_check(cid, got)
    tune.set("fgmres_fused", 0)
    unfused = solve_case(ctx, cid)
    assert unfused[:2] == got[:2]
    assert np.array_equal(unfused[2], got[2]) and np.array_equal(unfused[3], got[3])


def test_fused_pass_without_nullspace(ctx, tune):
    """nullspace = 0: the loader's add is absent (not + 0.0); fused and unfused agree bit for bit
    and the run matches the restatement."""
    from fgmres_restatement import fgmres
    from ksp_types_restatement import Problem
    prob = Problem((24, 20, 12), nullspace=0)
    b = prob.rhs()
    want = fgmres(prob, b, restart=4, max_it=7, **F.FIXED_KW)
    runs = []
    for fused in (1, 0):
        tune.set("fgmres_fused", fused)
        da = pb.DA(ctx, prob.n3)
        P, A = prob.mats(pb, da)
        x, bv = pb.Vec(da), pb.Vec(da)
        bv.set_values(b)
        k = pb.KSP(A, P, pb.ksp_options(["-ksp_type", "fgmres", "-ksp_gmres_restart", "4",
                                         "-ksp_max_it", "7"] + FIXED, nullspace=0))
        reason, its, hist = k.solve(bv, x)
        runs.append((reason, its, hist, x.get_values()))
        k.destroy()
    assert runs[0][:2] == (-3, 7) == runs[1][:2]
    assert np.array_equal(runs[0][2], runs[1][2]) and np.array_equal(runs[0][3], runs[1][3])
    assert F.hist_diff(prob, runs[0][2], want[3]) < 1e-11
    assert F.x_diff(runs[0][3], want[0]) <= 1e-10


# ---------------------------------------------------------------------------------------------
# to a tolerance
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["tol-jacobi-r30", "tol-jacobi-r5", "tol-mg", "tol-fft"])
def test_to_tolerance(ctx, cid):
    prob, b, _ = F.setup(cid)
    xo, ro, itso, ho, _ = F.restated(cid)
    assert ro == 2 and (cid != "tol-jacobi-r5" or itso > 10)  # several restarts
    assert cid != "tol-fft" or itso <= 2  # the near-breakdown column
    got = solve_case(ctx, cid)
    fg_check(cid, got)
    nb = float(np.linalg.norm(b))
    res = F.true_residual(prob, b, got[3])
    est = got[2][-1] / nb
    factor = F.bars(cid)[2]
    print(f"{cid}: ||b - A x|| / ||b|| {res:.3e}, last estimate / ||b|| {est:.3e}, allowed factor "
          f"{factor:.2f}")
    assert res <= factor * est, (cid, res, est, factor)


def test_refine_always(ctx):
    got = solve_case(ctx, "refine-jacobi")
    fg_check("refine-jacobi", got)
    # the second pass shows: refined and unrefined histories differ (on the restatement too)
    assert not np.array_equal(F.restated("refine-jacobi")[3], F.restated("tol-jacobi-r30")[3])


@pytest.mark.parametrize("cid", ["guess-jacobi", "guess-jacobi-initial"])
def test_initial_guess_nonzero(ctx, cid):
    got = solve_case(ctx, cid)
    assert got[0] == 2
    fg_check(cid, got)
    # the reference norms differ: ||b|| against ||r_0||
    assert F.restated("guess-jacobi")[4] != F.restated("guess-jacobi-initial")[4]


def test_zero_rhs(ctx):
    got = solve_case(ctx, "zero-rhs")
    xo, ro, itso, ho, _ = F.restated("zero-rhs")
    assert (got[0], got[1], got[6]) == (ro, itso, 1) == (3, 0, 1)
    assert np.all(np.isfinite(got[3])) and not np.any(got[3])


def test_norm_none(ctx):
    got = solve_case(ctx, "none-jacobi")
    assert (got[0], got[1]) == (4, 7)
    fg_check("none-jacobi", got)
    # the same iterations as the tested fixed-count run: the same x, bit for bit
    same = solve_case(ctx, "fixed-jacobi-7")
    assert np.array_equal(got[3], same[3]) and np.array_equal(got[2], same[2])


def test_errors(ctx):
    da = pb.DA(ctx, (16, 16, 12))
    A = pb.Mat(da, pb.STAR7)
    x, b = pb.Vec(da), pb.Vec(da)
    b.set_random(3)
    for nt in ("preconditioned", "natural"):
        with pytest.raises(pb.PbError) as e:
            pb.KSP(A, A, pb.ksp_options(["-ksp_type", "fgmres", "-ksp_norm_type", nt]))
        assert e.value.code == UNSUPPORTED, nt
    with pytest.raises(pb.PbError) as e:
        pb.KSP(A, A, pb.ksp_options(["-ksp_type", "fgmres", "-ksp_guess_type", "fischer"]))
    assert e.value.code == UNSUPPORTED
    k = pb.KSP(A, A, pb.ksp_options(["-ksp_type", "fgmres", "-ksp_gmres_restart", "5"]))
    assert k.norm_type == (pb.KSP_NORM_DEFAULT, pb.KSP_NORM_UNPRECONDITIONED)
    assert k.fgmres_get_opts().restart == 5
    k.begin(b, x)
    with pytest.raises(pb.PbError) as e:
        k.fgmres_set_opts(restart=7)
    assert e.value.code == STATE
    k.iterate(3)
    k.end()
    k.fgmres_set_opts(restart=7)
    assert k.fgmres_get_opts().restart == 7
    k.destroy()
    k = pb.KSP(A, A, pb.ksp_options(["-ksp_type", "cg"]))
    with pytest.raises(pb.PbError) as e:
        k.fgmres_set_opts(restart=7)
    assert e.value.code == STATE
    k.destroy()


def _objects(ctx, prob):
    da = pb.DA(ctx, prob.n3, prob.L)
    P, A = prob.mats(pb, da)
    return da, P, A, pb.Vec(da), pb.Vec(da)


def test_enqueue_ahead(ctx):
    """begin / iterate(200) / end on a case that converges in about 20 iterations: the steps
    enqueued behind the one that set the done flag change nothing -- the bits of solve()."""
    cid = "ahead-mg"
    prob, b, _ = F.setup(cid)
    assert 10 <= F.restated(cid)[2] <= 30
    whole = solve_case(ctx, cid)
    fg_check(cid, whole)
    da, P, A, x, bv = _objects(ctx, prob)
    bv.set_values(b)
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", prob.pc] + argv_of(cid)))
    k.begin(bv, x)
    k.iterate(200)
    reason, its, hist = k.end()
    assert (reason, its) == (whole[0], whole[1])
    assert np.array_equal(hist, whole[2]) and np.array_equal(x.get_values(), whole[3])
    k.destroy()


def test_reuse_after_nan(ctx):
    """One KSP, restart 30: a solve whose b holds a NaN (DIVERGED_NANORINF, its 0), then a normal
    solve that converges early in its first cycle -- its solution build must touch no basis
    vector this solve never formed. Equal to a fresh KSP's result, bit for bit, and finite."""
    cid = "tol-mg"
    prob, b, _ = F.setup(cid)
    fresh = solve_case(ctx, cid)
    assert fresh[1] < 30
    da, P, A, x, bv = _objects(ctx, prob)
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", prob.pc] + argv_of(cid)))
    bad = b.copy()
    bad[prob.N // 3] = np.nan
    bv.set_values(bad)
    reason, its, _ = k.solve(bv, x)
    assert (reason, its) == (-9, 0)
    bv.set_values(b)
    reason, its, hist = k.solve(bv, x)
    xs = x.get_values()
    assert np.all(np.isfinite(xs))
    assert (reason, its) == (fresh[0], fresh[1])
    assert np.array_equal(hist, fresh[2]) and np.array_equal(xs, fresh[3])
    k.destroy()


@pytest.mark.parametrize("cid", ["ranks2-jacobi", "ranks2-mg"])
def test_two_ranks(cid):
    from test_gpu_parity import run_ranks
    prob = F.setup(cid)[0]

    def body(ctx, rank):
        k0, nk = pb.slab_partition(prob.n3[2], 2, rank)
        return (k0, nk), solve_case(ctx, cid, rows=(k0, nk))

    for rows, got in run_ranks(2, body):
        assert (got[0], got[1]) == (-3, 7)
        fg_check(cid, got, rows=rows, tag=f"{cid} rows {rows}")
