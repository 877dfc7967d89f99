"""GPU tier: KSPSolve from a nonzero initial guess (-ksp_initial_guess_nonzero).

Semantics (PETSc KSPSolve_CG + KSPConvergedDefault, restated; PETSc itself is not available, so
this behaviour is pinned to this restatement only -- DESIGN.md "parity unpinned"):
r0 = b - A x0 with x0 taken as it is, the iteration unchanged, x accumulating onto x0; the
stopping reference rnorm0 is the preconditioned, null-space-removed norm of the right-hand side
||N(M^-1 b)|| (= the ||z_0|| a zero-guess solve of b logs), ||z_0|| of the actual initial residual
when that is exactly 0 or with -ksp_converged_use_initial_residual_norm, the smaller of the two
with -ksp_converged_use_min_initial_residual_norm; ttol = max(rtol rnorm0, atol).

The oracle (oracle/pb_oracle.c) starts from zero, and needs no change: a guess solve of (b, x0)
is the zero-guess solve of b' = b - A x0 with x = x0 + d, and its stopping reference ||z_0(b')||
is moved to rnorm0 by handing it rtol' = rtol rnorm0 / ||z_0(b')|| (both norms from oracle runs
with max_it = 1). The iteration count must match exactly, so every case asserts on the oracle's
own values that its last two logged norms are more than 1e-6 (relative) away from ttol.
Bars: tests/parity_bars.py (HIST_RTOL, HIST_RTOL_PC for mg, X_RTOL). With the spectral PC one
iteration reaches rounding level: as in test_gpu_parity's fft tests, ||z_0|| is held to 1e-12 and
the later (rounding-noise) norms to 1e-10 ||z_0|| absolute.
Reference: src/poissbox.f90:295-296 (KSPSetFromOptions before KSPSolve).
"""
import numpy as np
import pytest

import poissbox_amd as pb
from oracle import oracle as O
from parity_bars import HIST_RTOL, HIST_RTOL_PC, X_RTOL, check_history, check_x

pytestmark = pytest.mark.gpu

SEED = 20231015
GUESS = ["-ksp_initial_guess_nonzero"]
MODE_ARGV = {"default": [], "initial": ["-ksp_converged_use_initial_residual_norm"],
             "min": ["-ksp_converged_use_min_initial_residual_norm"]}
TWO_PI = 2 * np.pi


class Case:
    """One (operator, PC, options) configuration and how the oracle is told about it."""

    def __init__(self, n3, pc="jacobi", op="star7", rtol=1e-8, max_it=None, sr=0, mode="default",
                 deltas=None, its_range=None):
        self.n3, self.pc, self.op, self.rtol, self.max_it = tuple(n3), pc, op, rtol, max_it
        self.sr, self.mode, self.its_range = sr, mode, its_range
        self.N = int(np.prod(n3))
        # config 5 (compact A = P, spectral PC) lives on the 2 pi box, as in test_gpu_parity
        self.L = (TWO_PI,) * 3 if (op, pc) == ("compact", "fft") else (1.0, 1.0, 1.0)
        self.h = tuple(deltas) if deltas else tuple(l / m for l, m in zip(self.L, n3))

    def apply(self, x, nranks=1):
        if self.op == "compact":
            return O.lapl(x, self.n3, self.h)
        if self.op == "assembled":
            return O.assembled(x, self.n3, self.h, nranks=nranks)
        return O.stencil(x, self.n3, self.h)

    def rhs(self, seed=SEED, nranks=1):
        return self.apply(O.fill_random(self.N, seed), nranks)

    def oracle_kw(self, nranks=1):
        kw = dict(pc=self.pc, op=self.op, nranks=nranks, single_reduction=self.sr)
        if self.max_it is not None:
            kw.update(atol=0.0, dtol=1e300, max_it=self.max_it)
        return kw

    def argv(self, guess=True):
        a = ["-pc_type", self.pc, "-ksp_rtol", repr(float(self.rtol))]
        if self.max_it is not None:
            a += ["-ksp_atol", "0", "-ksp_divtol", "1e300", "-ksp_max_it", str(self.max_it)]
        if self.sr:
            a += ["-ksp_cg_single_reduction"]
        return a + (GUESS + MODE_ARGV[self.mode] if guess else [])

    def mats(self, da):
        if self.op == "compact":
            A = pb.Mat(da, pb.COMPACT, self.h)
            # (other PCs take their diagonal / smoother from the 7-point P, src/poissbox.f90:226-228)
            return (A if self.pc == "fft" else pb.Mat(da, pb.ASSEMBLED27, self.h)), A
        if self.op == "assembled":
            P = pb.Mat(da, pb.ASSEMBLED27, self.h)
            return P, P
        if self.pc == "fft":  # the spectral PC inverts P's symbol: P = A = the 7-point operator
            A = pb.Mat(da, pb.STAR7, self.h)
            return A, A
        return pb.Mat(da, pb.ASSEMBLED27, self.h), pb.Mat(da, pb.STAR7, self.h)


def first_norm(case, v, nranks=1):
    """||N(M^-1 v)||: the ||z_0|| a zero-guess solve of v logs."""
    kw = dict(case.oracle_kw(nranks), max_it=1)
    return float(O.cg_solve(v, case.n3, case.h, rtol=0.0, **kw)[3][0])


def restate(case, b, x0, nranks=1):
    """The oracle's restatement of the guess solve of (b, x0): (x, reason, its, history, rnorm0).
    Asserts the margin of its last two logged norms to ttol."""
    bp = b - case.apply(x0, nranks)
    nb, nbp = first_norm(case, b, nranks), first_norm(case, bp, nranks)
    ref = {"default": nb if nb != 0.0 else nbp, "initial": nbp, "min": min(nb, nbp)}[case.mode]
    rtol = 0.0 if case.max_it is not None else case.rtol
    rtol_p = rtol * ref / nbp if nbp > 0.0 else rtol
    d, reason, its, hist = O.cg_solve(bp, case.n3, case.h, rtol=rtol_p, **case.oracle_kw(nranks))
    ttol = max(rtol * ref, 0.0 if case.max_it is not None else 1e-50)
    for v in hist[-2:]:
        assert abs(v - ttol) > 1e-6 * ttol or ttol == 0.0, (v, ttol, "seed too close to ttol")
    if case.its_range:
        assert case.its_range[0] <= its <= case.its_range[1], its
    return x0 + d, reason, its, np.asarray(hist), ref


def gpu_solve(ctx, case, b, x0, guess=True, rows=None, argv=None):
    """One solve on ctx; rows = (k0, nk): this rank's planes of the global arrays."""
    da = pb.DA(ctx, case.n3, case.L)
    P, A = case.mats(da)
    x, bv = pb.Vec(da), pb.Vec(da)
    cut = (lambda v: v) if rows is None else (
        lambda v: v.reshape(case.n3[2], -1)[rows[0]:rows[0] + rows[1]])
    bv.set_values(cut(b))
    x.set_values(cut(x0))
    k = pb.KSP(A, P, pb.ksp_options(argv or case.argv(guess)))
    reason, its, hist = k.solve(bv, x)
    out = (reason, its, np.asarray(hist), x.get_values(), k.result.rnorm0)
    k.destroy()
    for o in {A, P, x, bv}:
        o.destroy()
    da.destroy()
    return out


def check(case, got, want, rows=None, tag=""):
    reason, its, hist, xs, rnorm0 = got
    xo, ro, itso, ho, ref = want
    print(f"{tag} gpu reason {reason} its {its} rnorm0 {rnorm0:.17g} | oracle reason {ro} its "
          f"{itso} rnorm0 {ref:.17g}")
    assert (reason, its) == (ro, itso), (tag, reason, its, ro, itso)
    if case.pc == "fft":
        assert hist.shape == ho.shape
        assert abs(hist[0] - ho[0]) / ho[0] < 1e-12
        assert np.max(np.abs(hist[1:] - ho[1:]), initial=0.0) / ho[0] < 1e-10
    else:
        check_history(hist, ho, bar=HIST_RTOL_PC if case.pc == "mg" else HIST_RTOL, tag=tag)
    if rows is None:
        check_x(xs, xo, tag=tag)
    else:
        check_x(xs, xo.reshape(case.n3[2], -1)[rows[0]:rows[0] + rows[1]].reshape(-1),
                scale=float(np.max(np.abs(xo))), tag=tag)
    assert abs(rnorm0 - ref) <= HIST_RTOL * ref, (tag, rnorm0, ref)


def guess_of(case, seed=7, scale=1.0):
    return scale * O.fill_random(case.N, seed)


# ---------------------------------------------------------------------------------------------
# warm start (fails without the feature: the option is ignored and the guess destroyed)
# ---------------------------------------------------------------------------------------------
WARM = Case((32, 32, 32), rtol=1e-10)


def test_warm_start_fewer_iterations(ctx):
    """x0 = x* + 1e-6 max|x*| random: reason, its and history of the oracle on b' with rtol', x
    within X_RTOL of x0 + d_oracle, and strictly fewer iterations than the cold solve."""
    b = WARM.rhs()
    cold = gpu_solve(ctx, WARM, b, np.zeros(WARM.N), guess=False)
    assert cold[0] == 2
    xstar = cold[3]
    x0 = xstar + 1e-6 * np.max(np.abs(xstar)) * O.fill_random(WARM.N, 11)
    want = restate(WARM, b, x0)
    got = gpu_solve(ctx, WARM, b, x0)
    check(WARM, got, want, tag="warm")
    assert 0 < got[1] < cold[1], (got[1], cold[1])
    # the reference norm is the cold solve's ||z_0||
    assert abs(got[4] - cold[2][0]) <= HIST_RTOL * cold[2][0]


# ---------------------------------------------------------------------------------------------
# every setup / x-update path, from a random x0 of O(1)
# ---------------------------------------------------------------------------------------------
PATHS = {
    "jacobi": Case((16, 16, 16), rtol=1e-6, its_range=(20, 40)),
    "none": Case((16, 16, 16), pc="none", rtol=1e-6, its_range=(20, 40)),
    "single_reduction": Case((16, 16, 16), rtol=1e-6, sr=1, its_range=(20, 40)),
    "sr_none": Case((16, 16, 16), pc="none", rtol=1e-6, sr=1, its_range=(20, 40)),
    # stored-z PCs converge in fewer iterations than 20 at any tolerance above rounding
    "mg": Case((16, 16, 16), pc="mg", rtol=1e-10),
    "sor": Case((16, 16, 16), pc="sor", rtol=1e-10),
    "fft": Case((64, 64, 64), pc="fft", rtol=1e-10),
    "compact_fft": Case((64, 64, 64), pc="fft", op="compact", rtol=1e-10),
    "assembled": Case((16, 16, 16), op="assembled", rtol=1e-6, its_range=(20, 40)),
    # compact A with the Jacobi PC: the vector-kernel setup with its six sums
    "compact_jacobi": Case((16, 16, 16), op="compact", rtol=1e-6),
}


@pytest.mark.parametrize("name", list(PATHS))
def test_paths_random_guess(ctx, name):
    case = PATHS[name]
    b, x0 = case.rhs(), guess_of(case)
    want = restate(case, b, x0)
    check(case, gpu_solve(ctx, case, b, x0), want, tag=name)


@pytest.mark.parametrize("sr", [0, 1])
@pytest.mark.parametrize("defer", [0, 2, 4])
@pytest.mark.parametrize("max_it", [1, 3, 4, 5, 9])
def test_deferred_x_lands_on_the_guess(ctx, tune, defer, max_it, sr):
    """Stopping at every position of the deferred-x cycle: the in-pass updates and the flushes of
    1 to 3 pending alpha p terms all add to x0."""
    tune.set("cg_defer_x", defer)
    case = Case((32, 24, 16), rtol=0.0, max_it=max_it, sr=sr)
    b, x0 = case.rhs(), guess_of(case)
    want = restate(case, b, x0)
    assert (want[1], want[2]) == (-3, max_it)
    check(case, gpu_solve(ctx, case, b, x0), want, tag=f"defer{defer} max_it{max_it} sr{sr}")


# ---------------------------------------------------------------------------------------------
# shapes of the fused setup pass (the single-reduction tests' small odd ones)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deltas", [None, (0.05, 0.05, 0.05), (0.05, 0.03, 0.07)],
                         ids=["grid", "uniform", "nonuniform"])
@pytest.mark.parametrize("n3", [(24, 20, 12), (17, 18, 9), (130, 6, 33), (16, 16, 16)])
def test_setup_pass_shapes(ctx, n3, deltas):
    """Even / odd x (two / one point per lane), 4 / 2 / 1 rows per wave, odd z, more than one x
    segment; spacing 1/n, uniform and non-uniform."""
    case = Case(n3, rtol=0.0, max_it=3, deltas=deltas)
    b, x0 = case.rhs(), guess_of(case)
    want = restate(case, b, x0)
    check(case, gpu_solve(ctx, case, b, x0), want, tag=f"{n3} {deltas}")


def test_setup_pass_wide_planes(ctx):
    """1024-point-wide planes: more 4-row columns than CUs, so the pass takes its 8-row tiles and
    the residency cap (the launch shape of pass B, which it shares)."""
    case = Case((1024, 1024, 4), rtol=0.0, max_it=3)
    b, x0 = case.rhs(), guess_of(case)
    want = restate(case, b, x0)
    check(case, gpu_solve(ctx, case, b, x0), want, tag="1024x1024x4")


def test_setup_pass_residual_is_reference_order(ctx):
    """r0 = b - A x0 with A x0 summed in the reference order: max_it 0 leaves ||z_0|| of exactly
    the oracle's b' = b - stencil(x0) (to the sums' rounding) and x untouched."""
    case = Case((24, 20, 12), rtol=0.0, max_it=0)
    b, x0 = case.rhs(), guess_of(case)
    reason, its, hist, xs, _ = gpu_solve(ctx, case, b, x0)
    assert (reason, its) == (-3, 0) and len(hist) == 1
    nbp = first_norm(case, b - case.apply(x0))
    assert abs(hist[0] - nbp) <= 1e-13 * nbp
    assert np.array_equal(xs, x0)


# ---------------------------------------------------------------------------------------------
# stopping reference
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale,order", [(1e-3, "initial_smaller"), (30.0, "rhs_smaller")])
def test_stopping_modes(ctx, scale, order):
    """Default, use_initial_residual_norm and use_min each stop where the restatement says, and
    report its rnorm0. min(a, b) is one of a and b, so one (b, x0) pair gives at most two distinct
    iteration counts; two pairs put the minimum on either side: a guess near the solution
    (||z_0|| << ||N M^-1 b||: min = initial) and one far from it (min = default)."""
    n3 = (16, 16, 16)
    base = Case(n3, rtol=1e-6)
    b = base.rhs()
    xstar = restate(base, b, np.zeros(base.N))[0]
    x0 = xstar + scale * np.max(np.abs(xstar)) * O.fill_random(base.N, 11)
    res = {}
    for mode in MODE_ARGV:
        case = Case(n3, rtol=1e-6, mode=mode)
        want = restate(case, b, x0)
        got = gpu_solve(ctx, case, b, x0)
        check(case, got, want, tag=f"{order} {mode}")
        res[mode] = (got[1], got[4])
    assert res["default"][0] != res["initial"][0], res
    small = "initial" if order == "initial_smaller" else "default"
    assert res[small][1] < res["default" if small == "initial" else "initial"][1]
    assert res["min"] == res[small], res


def test_both_reference_switches_rejected_at_create(ctx):
    da = pb.DA(ctx, (8, 8, 8))
    A = pb.Mat(da, pb.STAR7)
    o = pb.ksp_options(GUESS, converged_use_initial_residual_norm=1,
                       converged_use_min_initial_residual_norm=1)
    with pytest.raises(pb.PbError) as e:
        pb.KSP(A, A, o)
    assert e.value.code == 1  # PB_ERR_ARG


# ---------------------------------------------------------------------------------------------
# edges
# ---------------------------------------------------------------------------------------------
EXACT = {"jacobi": Case((16, 16, 16), rtol=1e-8), "mg": Case((16, 16, 16), pc="mg", rtol=1e-8),
         # compact + fft: the path that leaves r0 = b, x0 = 0 implicit from a zero guess
         "compact_fft": Case((64, 64, 64), pc="fft", op="compact", rtol=1e-8)}


@pytest.mark.parametrize("name", list(EXACT))
def test_exact_guess_returns_x0_untouched(ctx, name):
    """x0 = x* of a solve converged two orders further: converged at its 0, x bit-identical."""
    case = EXACT[name]
    b = case.rhs()
    tight = Case(case.n3, pc=case.pc, op=case.op, rtol=1e-10)
    cold = gpu_solve(ctx, tight, b, np.zeros(case.N), guess=False)
    assert cold[0] == 2
    x0 = cold[3]
    reason, its, hist, xs, rnorm0 = gpu_solve(ctx, case, b, x0)
    assert reason in (2, 3) and its == 0 and len(hist) == 1, (reason, its, hist)
    assert np.array_equal(xs, x0)
    assert hist[0] <= case.rtol * rnorm0
    assert abs(rnorm0 - cold[2][0]) <= HIST_RTOL * cold[2][0]


@pytest.mark.parametrize("name", ["jacobi", "mg"])
def test_zero_rhs_falls_back_to_initial_residual(ctx, name):
    """b = 0: ||N M^-1 b|| is exactly 0 and the reference falls back to ||z_0||; the solve removes
    x0's non-constant part and keeps its mean."""
    case = Case((16, 16, 16), pc=name, rtol=1e-10)
    b, x0 = np.zeros(case.N), guess_of(case)
    want = restate(case, b, x0)
    got = gpu_solve(ctx, case, b, x0)
    check(case, got, want, tag=f"zero rhs {name}")
    reason, its, hist, xs, rnorm0 = got
    assert rnorm0 == hist[0] and reason == 2 and its > 0
    s = float(np.max(np.abs(x0)))
    assert abs(xs.mean() - x0.mean()) <= X_RTOL * s
    # converged to rtol 1e-10 in the preconditioned norm; the 16^3 operator's condition number is
    # ~1e2 (Jacobi) or less: what is left of x0's non-constant part is below 1e-7 of it
    assert np.max(np.abs(xs - xs.mean())) < 1e-7 * s


@pytest.mark.parametrize("name", ["jacobi", "single_reduction", "mg", "compact_fft"])
def test_nan_in_guess_is_nanorinf(ctx, name):
    case = PATHS[name]
    b, x0 = case.rhs(), guess_of(case)
    x0[37] = np.nan
    reason, its, hist, _, _ = gpu_solve(ctx, case, b, x0)
    assert (reason, its) == (-9, 0) and len(hist) == 1 and np.isnan(hist[0])


@pytest.mark.parametrize("name", ["jacobi", "single_reduction", "mg", "compact_fft"])
def test_flag_off_ignores_x(ctx, name):
    """No flag: a nonzero x passed in is overwritten, the result the cold solve's bit for bit."""
    case = PATHS[name]
    b = case.rhs()
    cold = gpu_solve(ctx, case, b, np.zeros(case.N), guess=False)
    full = gpu_solve(ctx, case, b, guess_of(case), guess=False)
    assert cold[:2] == full[:2] and cold[4] == full[4]
    assert np.array_equal(cold[2], full[2]) and np.array_equal(cold[3], full[3])
    expl = gpu_solve(ctx, case, b, guess_of(case), argv=case.argv(False) + GUESS + ["false"])
    assert cold[:2] == expl[:2] and np.array_equal(cold[2], expl[2])
    assert np.array_equal(cold[3], expl[3])


@pytest.mark.parametrize("name", ["jacobi", "mg"])
def test_ksp_reuse_time_loop(ctx, name):
    """One KSP, three solves with b_k = b + 0.01 k c, each starting from the previous x: every
    solve matches its own restatement, and solves 2 and 3 take fewer iterations than solve 1."""
    case = Case((16, 16, 16), pc=name, rtol=1e-8)
    b, c = case.rhs(), case.rhs(seed=99)
    da = pb.DA(ctx, case.n3, case.L)
    P, A = case.mats(da)
    x, bv = pb.Vec(da), pb.Vec(da)
    x.set(0.0)
    k = pb.KSP(A, P, pb.ksp_options(case.argv()))
    its_all = []
    for step in range(3):
        bk = b + 0.01 * step * c
        x0 = x.get_values()
        want = restate(case, bk, x0)
        bv.set_values(bk)
        reason, its, hist = k.solve(bv, x)
        check(case, (reason, its, np.asarray(hist), x.get_values(), k.result.rnorm0), want,
              tag=f"reuse {name} step {step}")
        its_all.append(its)
    k.destroy()
    assert its_all[1] < its_all[0] and its_all[2] < its_all[0], its_all


# ---------------------------------------------------------------------------------------------
# N ranks over the host transport (one GPU, one thread per rank)
# ---------------------------------------------------------------------------------------------
def _multirank(case, nranks, tag):
    from test_gpu_parity import run_ranks
    b, x0 = case.rhs(nranks=nranks), guess_of(case)
    want = restate(case, b, x0, nranks)

    def body(ctx, rank):
        k0, nk = pb.slab_partition(case.n3[2], nranks, rank)
        return (k0, nk), gpu_solve(ctx, case, b, x0, rows=(k0, nk))

    for rows, got in run_ranks(nranks, body):
        check(case, got, want, rows=rows, tag=f"{tag} rows {rows}")


@pytest.mark.parametrize("variant", ["jacobi", "single_reduction"])
@pytest.mark.parametrize("nranks,n3", [(2, (16, 16, 12)), (3, (16, 16, 12)), (3, (20, 16, 7)),
                                       # two-plane slabs: the non-overlapped halo exchange
                                       (2, (16, 16, 4))])
def test_multirank_guess(nranks, n3, variant):
    """x0's boundary planes are exchanged under the setup pass's interior planes (or before it on
    slabs of fewer than three planes); the six sums are allreduced once."""
    case = Case(n3, rtol=1e-8, sr=int(variant == "single_reduction"))
    _multirank(case, nranks, f"{nranks} ranks {n3} {variant}")


@pytest.mark.parametrize("nranks", [2, 3])
def test_multirank_guess_mg(nranks):
    case = Case((16, 16, 12), pc="mg", rtol=1e-8)
    _multirank(case, nranks, f"{nranks} ranks mg")


def test_multirank_guess_compact_fft():
    """Config 5 on two ranks (all-to-all callback): A x0 by the decomposed compact operator."""
    _multirank(Case((64, 64, 64), pc="fft", op="compact", rtol=1e-10), 2, "2 ranks compact fft")
