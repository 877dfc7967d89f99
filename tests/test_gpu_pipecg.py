"""GPU tier: -ksp_type pipecg against its numpy restatement (tests/pipecg_restatement.py; semantics
in DESIGN.md §3.1i, "parity unpinned": PETSc is not available, so KSPSolve_PIPECG is pinned to the
restatement only). The cases and their restated runs are tests/pipecg_cases.py's, computed once.

Bars. Pipelined CG never recomputes r, u = M^-1 r and w = A u from x: they are recurrences, and
deep into a solve its histories are more sensitive to the summation order than CG's. So the CG
bars are not assumed: scripts/pipecg_sensitivity.py runs the restatement of every case on the CPU
under pairwise, left-to-right and exactly rounded sums and records the largest difference d
between two variants (profiles/ksp_pipecg/sensitivity.json). A case's history bar is 100 d -- the
two orders of margin parity_bars.py states -- and never below HIST_RTOL (HIST_RTOL_PC with sor /
mg; with the spectral PC the entries after the first are rounding noise and held to 1e-10 of the
first, as fgmres_cases.hist_diff holds them); x likewise against X_RTOL. Measured d (history, x),
the largest of each group:
  fixed counts m = 1..6: jacobi 1.4e-14, 4.9e-15; none 9.6e-15, 5.1e-15; jacobi_deltas 1.9e-14,
    6.6e-15; sor 8.7e-15, 1.2e-14; mg 3.2e-13, 7.3e-15; fft 3.2e-15, 8.9e-16; compact_fft
    3.5e-15, 2.5e-14; assembled_jacobi 9.4e-15, 3.8e-15
  shapes, 7 iterations, jacobi and none: 2.1e-13, 3.5e-14 (1024x1024x4; the others at most
    4.4e-14, 1.3e-14)
  norm types, 6 iterations: 2.1e-13, 7.3e-15 (mg); two ranks, 7 iterations: 2.1e-12, 8.9e-15 (mg)
  to a tolerance: 32^3 jacobi rtol 1e-8 (89 iterations): 2.6e-9, 8.5e-13; 32^3 mg rtol 1e-10
    (13): 1.1e-6, 2.4e-14; 32x40x48 fft (1): 3.2e-15, 4.4e-16; nonzero guess rtol 1e-6 (37):
    8.5e-11, 1.8e-13; unpreconditioned rtol 1e-6 (37): 1.7e-10, 1.2e-13
so x sits at X_RTOL everywhere, the fixed-count, shape and norm-type histories sit at the CG bars
(but 1024x1024x4, 2.1e-11, and the two-rank mg run, 2.1e-10), and the sensitivity sets the bars of
the runs to a tolerance: 2.6e-7 (jacobi), 1.1e-4 (mg), 8.5e-9 and 1.7e-8. Reason and iteration
count must be exact where the restatement's last two norms lie further from ttol than the case's
own bar (pipecg_cases.stop_margin_ok: asserted, it holds on every such case); every variant of the
restatement ends alike on every case (same_outcome in the json).

The true residual ||b - A x|| / ||b|| of the runs to a tolerance must be no more than 10 x the
restatement's own.

On the 7-point operator with Jacobi / no PC (one rank) the iteration is one engine pass and the
finalize; tuning pipecg_fused = 0 runs the sequence it replaces (Jacobi + shift kernel, standalone
operator, update pass from stored m and n in the engine's tiles) and must give the same bits.

Every test here fails without the feature: -ksp_type pipecg is PB_ERR_UNSUPPORTED.
Reference: src/poissbox.f90:269-298 (solve -> KSPSetFromOptions -> KSPSolve).
"""
import numpy as np
import pytest

import poissbox_amd as pb
import pipecg_cases as F
from parity_bars import _record
from test_gpu_ksp_types import FIXED, gpu_solve

pytestmark = pytest.mark.gpu

UNSUPPORTED = 5


def argv_of(cid, extra=()):
    _, kw, ex = F.CASES[cid]
    a = ["-ksp_type", "pipecg"]
    if kw.get("rtol") == 0.0:
        a += FIXED
    elif "rtol" in kw:
        a += ["-ksp_rtol", repr(float(kw["rtol"]))]
    if "max_it" in kw:
        a += ["-ksp_max_it", str(kw["max_it"])]
    if "norm" in kw:
        a += ["-ksp_norm_type", kw["norm"]]
    if "x0" in ex:
        a += ["-ksp_initial_guess_nonzero"]
    if kw.get("mode") == "initial":
        a += ["-ksp_converged_use_initial_residual_norm"]
    return a + list(extra)


def pcg_check(cid, got, rows=None, tag=None):
    """history, x, reason, count and the result fields of one GPU solve against the case's
    restated run, within the case's bars; every figure is printed before it is asserted."""
    tag = tag or cid
    prob, b, _ = F.setup(cid)
    kw = F.CASES[cid][1]
    xo, ro, itso, ho, ref = F.restated(cid)
    reason, its, hist, xs, rnorm0, rnorm, nhist = got
    hbar, xbar = F.bars(cid)
    print(f"{tag}: gpu reason {reason} its {its} | restated reason {ro} its {itso}; bars history "
          f"{hbar:.2e} x {xbar:.2e}")
    stopping = kw.get("rtol", 1e-5) > 0.0 and kw.get("norm") != "none"
    if stopping:
        assert F.stop_margin_ok(cid), (tag, "the restatement's last norms are too close to ttol")
    assert (reason, its) == (ro, itso), (tag, reason, its, ro, itso)
    assert nhist == len(hist) == its + 1, (tag, nhist, len(hist), its)
    dh = F.hist_diff(prob, hist, ho)
    print(f"{tag}: history difference {dh:.3e}")
    _record("history", dh, hbar, tag)
    assert dh < hbar, (tag, dh, hbar)
    assert abs(rnorm0 - ref) <= 1e-11 * ref, (tag, rnorm0, ref)
    assert rnorm == hist[-1]
    if rows is not None:
        xo = xo.reshape(prob.n3[2], -1)[rows[0]:rows[0] + rows[1]].reshape(-1)
        dx = float(np.max(np.abs(xs - xo))) / float(np.max(np.abs(F.restated(cid)[0])))
    else:
        dx = F.x_diff(xs, xo)
    print(f"{tag}: x difference {dx:.3e}")
    _record("x", dx, xbar, tag)
    assert np.all(np.isfinite(xs)) and dx <= xbar, (tag, dx, xbar)


def solve_case(ctx, cid, extra=(), rows=None):
    prob, b, x0 = F.setup(cid)
    return gpu_solve(ctx, prob, b, argv_of(cid, extra), x0=x0, rows=rows)


def same_bits(a, b):
    return a[:2] == b[:2] and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


# ---------------------------------------------------------------------------------------------
# fixed iteration counts: the i = 0 branch alone (1), the recurrence (2..6), an odd and an even
# number of w ping-pong flips, on every path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", range(1, 7))
@pytest.mark.parametrize("name", list(F.PATHS))
def test_fixed_counts(ctx, name, m):
    cid = f"fixed-{name}-{m}"
    got = solve_case(ctx, cid)
    assert (got[0], got[1]) == (-3, m)
    pcg_check(cid, got)


@pytest.mark.parametrize("pc", ["jacobi", "none"])
@pytest.mark.parametrize("n3,deltas", F.SHAPES, ids=[F.shape_id(*s) for s in F.SHAPES])
def test_fused_pass_shapes(ctx, tune, n3, deltas, pc):
    """The engine pass (m = D^-1 w - mean formed on load, A m, the eight updates, the five sums)
    on even / odd x (two / one point per lane), 4 / 2 / 1 rows per wave, odd z, more than one x
    segment, 1024-wide planes, non-uniform spacing: 7 iterations against the restatement, and the
    unfused sequence (pipecg_fused = 0) gives the same bits."""
    cid = F.shape_id(n3, deltas) + ("" if pc == "jacobi" else "-none")
    got = solve_case(ctx, cid)
    assert (got[0], got[1]) == (-3, 7)
    pcg_check(cid, got)
    tune.set("pipecg_fused", 0)
    assert same_bits(solve_case(ctx, cid), got)


def test_fused_pass_without_nullspace(ctx, tune):
    """nullspace = 0: the loader's add is absent (not + 0.0); fused and unfused agree bit for bit
    and the run matches the restatement."""
    from ksp_types_restatement import Problem
    from pipecg_restatement import pipecg
    prob = Problem((24, 20, 12), nullspace=0)
    b = prob.rhs()
    want = pipecg(prob, b, max_it=5, **F.FIXED_KW)
    runs = []
    for fused in (1, 0):
        tune.set("pipecg_fused", fused)
        da = pb.DA(ctx, prob.n3)
        P, A = prob.mats(pb, da)
        x, bv = pb.Vec(da), pb.Vec(da)
        bv.set_values(b)
        k = pb.KSP(A, P, pb.ksp_options(["-ksp_type", "pipecg", "-ksp_max_it", "5"] + FIXED,
                                        nullspace=0))
        reason, its, hist = k.solve(bv, x)
        runs.append((reason, its, np.asarray(hist), x.get_values()))
        k.destroy()
    assert runs[0][:2] == (-3, 5) and same_bits(runs[0], runs[1])
    assert F.hist_diff(prob, runs[0][2], want[3]) < 1e-11
    assert F.x_diff(runs[0][3], want[0]) <= 1e-10


# ---------------------------------------------------------------------------------------------
# to a tolerance
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["tol-jacobi", "tol-mg", "tol-fft"])
def test_to_tolerance(ctx, cid):
    prob, b, _ = F.setup(cid)
    xo, ro, itso, ho, _ = F.restated(cid)
    assert ro == 2
    got = solve_case(ctx, cid)
    pcg_check(cid, got)
    res, want = F.true_residual(prob, b, got[3]), F.true_residual(prob, b, xo)
    print(f"{cid}: ||b - A x|| / ||b|| {res:.3e}, the restatement's {want:.3e}")
    assert res <= 10.0 * want, (cid, res, want)


# ---------------------------------------------------------------------------------------------
# norm types, nonzero guess, the split form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["jacobi", "mg"])
@pytest.mark.parametrize("nt", F.NORMS)
def test_norm_types(ctx, nt, pc):
    cid = f"norm-{nt}-{pc}"
    got = solve_case(ctx, cid)
    assert (got[0], got[1]) == ((4, 6) if nt == "none" else (-3, 6))
    pcg_check(cid, got)
    # the same iterations under every norm type: the same x, bit for bit
    assert np.array_equal(got[3], solve_case(ctx, f"fixed-{pc}-6")[3])
    if nt == "none":
        assert not np.any(got[2])


def test_unpreconditioned_to_tolerance(ctx):
    got = solve_case(ctx, "norm-unpreconditioned-tol")
    assert got[0] == 2
    pcg_check("norm-unpreconditioned-tol", got)


@pytest.mark.parametrize("cid", ["guess-jacobi", "guess-jacobi-initial"])
def test_initial_guess_nonzero(ctx, cid):
    got = solve_case(ctx, cid)
    assert got[0] == 2
    pcg_check(cid, got)
    # the reference norms differ: ||N(M^-1 b)|| against ||u_0||
    assert F.restated("guess-jacobi")[4] != F.restated("guess-jacobi-initial")[4]


def _objects(ctx, prob):
    da = pb.DA(ctx, prob.n3, prob.L)
    P, A = prob.mats(pb, da)
    return da, P, A, pb.Vec(da), pb.Vec(da)


@pytest.mark.parametrize("cid", ["tol-jacobi", "tol-mg"])
def test_split_form_equals_solve(ctx, cid):
    """begin, iterate in uneven batches (an odd batch first: the w ping-pong's parity carries
    over), end: the bits of solve()."""
    prob, b, _ = F.setup(cid)
    whole = solve_case(ctx, cid)
    da, P, A, x, bv = _objects(ctx, prob)
    bv.set_values(b)
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", prob.pc] + argv_of(cid)))
    k.begin(bv, x)
    for batch in (1, 3, 2, 7, 200):
        k.iterate(batch)
    reason, its, hist = k.end()
    assert same_bits((reason, its, np.asarray(hist), x.get_values()), whole)
    k.destroy()


def test_enqueue_ahead(ctx):
    """The same converging solve with the flag polled every 1, 8 and 32 iterations: whatever was
    enqueued past the stopping iteration touches neither x nor the history."""
    cid = "tol-jacobi"
    prob, b, _ = F.setup(cid)
    whole = solve_case(ctx, cid)
    pcg_check(cid, whole)
    runs = [whole]
    for ce in (1, 8, 32):
        da, P, A, x, bv = _objects(ctx, prob)
        bv.set_values(b)
        k = pb.KSP(A, P, pb.ksp_options(["-pc_type", prob.pc] + argv_of(cid), check_every=ce))
        reason, its, hist = k.solve(bv, x)
        runs.append((reason, its, np.asarray(hist), x.get_values()))
        k.destroy()
    assert all(same_bits(runs[0], r) for r in runs[1:])


# ---------------------------------------------------------------------------------------------
# non-finite input, errors
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["tol-jacobi", "tol-mg"])
def test_reuse_after_nan(ctx, cid):
    """One KSP: a solve whose b holds a NaN (DIVERGED_NANORINF, its 0), then a normal solve --
    z, q, s, p still hold the first solve's NaNs and must be set, not read, by the first update.
    Equal to a fresh KSP's result, bit for bit, and finite."""
    prob, b, _ = F.setup(cid)
    fresh = solve_case(ctx, cid)
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
    assert same_bits((reason, its, np.asarray(hist), xs), fresh)
    k.destroy()


def test_errors(ctx):
    da = pb.DA(ctx, (16, 16, 12))
    A = pb.Mat(da, pb.STAR7)
    with pytest.raises(pb.PbError) as e:
        pb.KSP(A, A, pb.ksp_options(["-ksp_type", "pipecg", "-ksp_guess_type", "fischer"]))
    assert e.value.code == UNSUPPORTED
    k = pb.KSP(A, A, pb.ksp_options(["-ksp_type", "pipecg", "-ksp_cg_single_reduction"]))
    assert k.norm_type == (pb.KSP_NORM_DEFAULT, pb.KSP_NORM_PRECONDITIONED)
    v = pb.Vec(da)
    v.set_random(3)
    with pytest.raises(pb.PbError):
        k.solve(v, v)  # b and x must be distinct
    k.destroy()


# ---------------------------------------------------------------------------------------------
# two ranks over the host transport
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["ranks2-jacobi", "ranks2-mg"])
def test_two_ranks(cid):
    from test_gpu_parity import run_ranks
    prob = F.setup(cid)[0]

    def body(ctx, rank):
        k0, nk = pb.slab_partition(prob.n3[2], 2, rank)
        return (k0, nk), solve_case(ctx, cid, rows=(k0, nk))

    for rows, got in run_ranks(2, body):
        assert (got[0], got[1]) == (-3, 7)
        pcg_check(cid, got, rows=rows, tag=f"{cid} rows {rows}")


# ---------------------------------------------------------------------------------------------
# launches per iteration
# ---------------------------------------------------------------------------------------------
PHASES = ("pipecg_pass", "pipecg_finalize", "pipecg_update", "pipecg_pc", "stencil")


def _launches(ctx, nt, iters):
    """launches per timed phase of begin / iterate(iters) / end (the facility of
    test_gpu_norm_type._timed_split_solve); nothing stops these runs"""
    prob, b, _ = F.setup("fixed-jacobi-6")
    da, P, A, x, bv = _objects(ctx, prob)
    bv.set_values(b)
    k = pb.KSP(A, P, pb.ksp_options(["-ksp_type", "pipecg", "-ksp_max_it", "50",
                                     "-ksp_norm_type", nt] + FIXED))
    ctx.set_timing(True)
    ctx.reset_timing()
    try:
        k.begin(bv, x)
        k.iterate(iters)
        k.end()
        return {n: ctx.timing(n)[1] for n in PHASES}
    finally:
        ctx.set_timing(False)
        k.destroy()


def test_fused_iteration_is_two_launches(ctx):
    """Three more fused Jacobi iterations add three engine passes and three finalize launches and
    nothing else of the type's phases or the operator's, under every norm type."""
    for nt in ("preconditioned",) + F.NORMS:
        lo, hi = _launches(ctx, nt, 2), _launches(ctx, nt, 5)
        more = {n: hi[n] - lo[n] for n in PHASES}
        assert more == {"pipecg_pass": 3, "pipecg_finalize": 3, "pipecg_update": 0,
                        "pipecg_pc": 0, "stencil": 0}, (nt, more)
