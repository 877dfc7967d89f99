"""GPU tier: the projected initial guess (-ksp_guess_type fischer) and the two multi-vector
operations under it (pb_vec_mdot, pb_vec_maxpy).

PETSc is not available: the guess is held to the numpy restatement of KSPGuessFischer model 1 in
tests/fischer_restatement.py, and each solve to the oracle's restatement of a solve from a nonzero
guess (test_gpu_initial_guess.restate) started from the guess the library itself formed -- the
solve's own form is deterministic, so it starts from the same bits (DESIGN.md "parity unpinned").

Bars. Multi-dot: (N + 1) 2^-53 sum|x_j y_ij| per output against math.fsum of the products, N = the
smallest local length -- the a-priori bound of any summation order (one rounding per product, N - 1
per sum, one for the reference's own products). Multi-axpy: 2 nv 2^-53 (|y| + sum|alpha_i x_i|)
per element, one rounding per product and per sum. Guesses: parity_bars.X_RTOL of max|guess| (the
restatement against itself sits at 1e-16; the inputs are independent random fields, so the basis
is well conditioned). Solves: the bars of test_gpu_initial_guess.check.
"""
import math

import numpy as np
import pytest

import poissbox_amd as pb
from fischer_restatement import Fischer
from oracle import oracle as O
from parity_bars import X_RTOL
from test_gpu_initial_guess import PATHS, Case, check, restate
from test_gpu_parity import run_ranks

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
SHAPES = [(8, 8, 8), (16, 16, 16), (17, 17, 9), (130, 6, 33)]
NVS = (1, 2, 3, 8, 16)
FISCHER = ["-ksp_guess_type", "fischer"]
ERR_ARG, ERR_STATE = 1, 6


def _rows(n3, rows, v):
    return v if rows is None else v.reshape(n3[2], -1)[rows[0]:rows[0] + rows[1]].reshape(-1)


def _vecs(da, arrays, n3, rows=None):
    out = []
    for a in arrays:
        v = pb.Vec(da)
        v.set_values(_rows(n3, rows, a))
        out.append(v)
    return out


def _check_mdot(got, x, ys, nmin, tag):
    for i, y in enumerate(ys):
        prod = x * y
        exact = math.fsum(prod)
        bar = (nmin + 1) * U * float(np.sum(np.abs(prod)))
        print(f"{tag} mdot[{i}] err {abs(got[i] - exact):.3e} bar {bar:.3e}")
        assert abs(got[i] - exact) <= bar, (tag, i, got[i], exact, bar)


def _check_maxpy(got, y, alphas, xs, tag):
    ld = np.longdouble
    ref, mag = y.astype(ld), np.abs(y)
    for a, x in zip(alphas, xs):
        ref = ref + ld(a) * x.astype(ld)
        mag = mag + np.abs(a * x)
    err = np.abs(got.astype(ld) - ref).astype(np.float64)
    bar = 2 * len(xs) * U * mag
    print(f"{tag} maxpy max err/bar {float(np.max(err / bar)):.3e}")
    assert np.all(err <= bar), (tag, float(np.max(err / bar)))


def _fields(N, count, seed):
    return [O.fill_random(N, seed + i) for i in range(count)]


# ---------------------------------------------------------------------------------------------
# 1, 2: the multi-vector operations on one rank
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n3", SHAPES)
def test_mdot(ctx, n3):
    N = int(np.prod(n3))
    da = pb.DA(ctx, n3)
    arrs = _fields(N, 17, 100)
    vs = _vecs(da, arrs, n3)
    for nv in NVS:
        got = vs[0].mdot(vs[1:1 + nv])
        _check_mdot(got, arrs[0], arrs[1:1 + nv], N, f"{n3} nv{nv}")
        assert np.array_equal(got, vs[0].mdot(vs[1:1 + nv]))  # deterministic run to run
    # y[i] == x is allowed
    got = vs[0].mdot([vs[1], vs[0], vs[2]])
    _check_mdot(got, arrs[0], [arrs[1], arrs[0], arrs[2]], N, f"{n3} self")
    assert abs(math.sqrt(got[1]) - vs[0].norm()) <= 1e-14 * vs[0].norm()
    for v in vs:
        v.destroy()
    da.destroy()


def test_mdot_arguments(ctx):
    da, db = pb.DA(ctx, (8, 8, 8)), pb.DA(ctx, (8, 8, 9))
    x, y, z = pb.Vec(da), pb.Vec(da), pb.Vec(db)
    x.set_random(1)
    assert x.mdot([]).size == 0  # nv = 0 returns at once
    with pytest.raises(pb.PbError) as e:
        x.mdot([y] * 17)
    assert e.value.code == ERR_ARG
    with pytest.raises(pb.PbError) as e:
        x.mdot([y, z])
    assert e.value.code == ERR_ARG
    for o in (x, y, z):
        o.destroy()
    da.destroy()
    db.destroy()


@pytest.mark.parametrize("n3", SHAPES)
def test_maxpy(ctx, n3):
    N = int(np.prod(n3))
    da = pb.DA(ctx, n3)
    arrs = _fields(N, 17, 200)
    vs = _vecs(da, arrs, n3)
    alphas = np.array([(-1.0) ** i * (0.3 + 0.17 * i) for i in range(16)])
    for nv in NVS:
        vs[0].set_values(arrs[0])
        vs[0].maxpy(alphas[:nv], vs[1:1 + nv])
        _check_maxpy(vs[0].get_values(), arrs[0], alphas[:nv], arrs[1:1 + nv], f"{n3} nv{nv}")
    for v in vs:
        v.destroy()
    da.destroy()


def test_maxpy_arguments(ctx):
    da, db = pb.DA(ctx, (17, 17, 9)), pb.DA(ctx, (8, 8, 9))
    y, x, z = pb.Vec(da), pb.Vec(da), pb.Vec(db)
    y.set_random(1)
    x.set_random(2)
    y0 = y.get_values()
    y.maxpy([], [])  # nv = 0 leaves y as it is
    assert np.array_equal(y.get_values(), y0)
    for bad in ([x, y], [y], [x, z], [x] * 17):
        with pytest.raises(pb.PbError) as e:
            y.maxpy([1.0] * len(bad), bad)
        assert e.value.code == ERR_ARG
    assert np.array_equal(y.get_values(), y0)
    for o in (x, y, z):
        o.destroy()
    da.destroy()
    db.destroy()


# ---------------------------------------------------------------------------------------------
# 3: both on N ranks over the host transport
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nranks,n3", [(2, (16, 16, 12)), (3, (16, 16, 12)), (3, (20, 16, 7))])
def test_multirank_mdot_maxpy(nranks, n3):
    N = int(np.prod(n3))
    arrs = _fields(N, 17, 300)
    alphas = np.array([(-1.0) ** i * (0.3 + 0.17 * i) for i in range(16)])

    def body(ctx, rank):
        rows = pb.slab_partition(n3[2], nranks, rank)
        da = pb.DA(ctx, n3)
        vs = _vecs(da, arrs, n3, rows)
        dots, ys = {}, {}
        for nv in NVS:
            vs[0].set_values(_rows(n3, rows, arrs[0]))
            dots[nv] = vs[0].mdot(vs[1:1 + nv])
            vs[0].maxpy(alphas[:nv], vs[1:1 + nv])
            ys[nv] = vs[0].get_values()
        return rows, dots, ys

    res = run_ranks(nranks, body)
    nmin = min(rows[1] for rows, _, _ in res) * n3[0] * n3[1]
    for rows, dots, ys in res:
        for nv in NVS:
            assert np.array_equal(dots[nv], res[0][1][nv])  # every rank: the same bits
            _check_mdot(dots[nv], arrs[0], arrs[1:1 + nv], nmin, f"{nranks} ranks {n3} nv{nv}")
            _check_maxpy(ys[nv], _rows(n3, rows, arrs[0]), alphas[:nv],
                         [_rows(n3, rows, a) for a in arrs[1:1 + nv]], f"rows {rows} nv{nv}")


# ---------------------------------------------------------------------------------------------
# a KSP with the guess, kept over several solves
# ---------------------------------------------------------------------------------------------
def plain(case):
    """The case without the iteration-count window of its random-guess test."""
    return Case(case.n3, pc=case.pc, op=case.op, rtol=case.rtol, sr=case.sr)


class Loop:
    def __init__(self, ctx, case, maxl=10, rows=None, argv=None):
        self.case, self.rows = case, rows
        self.da = pb.DA(ctx, case.n3, case.L)
        self.P, self.A = case.mats(self.da)
        self.x, self.b, self.tmp = pb.Vec(self.da), pb.Vec(self.da), pb.Vec(self.da)
        if argv is None:
            argv = case.argv(False) + FISCHER + ["-ksp_guess_fischer_model", f"1,{maxl}"]
        self.ksp = pb.KSP(self.A, self.P, pb.ksp_options(argv))

    def cut(self, v):
        return _rows(self.case.n3, self.rows, v)

    def form(self, b):
        """The library's guess for b (this rank's rows)."""
        self.b.set_values(self.cut(b))
        self.ksp.guess_form(self.b, self.tmp)
        return self.tmp.get_values()

    def update(self, b, x):
        self.b.set_values(self.cut(b))
        self.tmp.set_values(self.cut(x))
        self.ksp.guess_update(self.b, self.tmp)
        return self.ksp.guess_size()[0]

    def mult(self, x):
        self.tmp.set_values(self.cut(x))
        self.A.mult(self.tmp, self.b)
        return self.b.get_values()

    def solve(self, b, x_in=None):
        """(the guess the solve starts from, the solve's results as gpu_solve returns them)."""
        x0 = self.form(b)
        if x_in is not None:
            self.x.set_values(self.cut(x_in))
        reason, its, hist = self.ksp.solve(self.b, self.x)
        return x0, (reason, its, np.asarray(hist), self.x.get_values(), self.ksp.result.rnorm0)

    def destroy(self):
        self.ksp.destroy()
        for o in {self.A, self.P, self.x, self.b, self.tmp}:
            o.destroy()
        self.da.destroy()


def mean_free(N, seed):
    x = O.fill_random(N, seed)
    return x - x.mean()


def family(case, t, nranks=1):
    """The right-hand sides of a time loop: three fields in A's range, slowly mixed."""
    r = [case.rhs(seed=s, nranks=nranks) for s in (41, 42, 43)]
    return r[0] + math.sin(0.3 * t) * r[1] + 0.5 * math.cos(0.2 * t) * r[2]


# ---------------------------------------------------------------------------------------------
# 4, 5: the guess against the restatement
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["star7", "compact"])
def test_guess_matches_restatement(ctx, op):
    """Seven form / update cycles with maxl 4 (sizes 1, 2, 3, 4, 1, 2, 3: one restart); after each
    the guess for a fresh random b is the restatement's."""
    case = Case((16, 16, 16), op=op)
    lp = Loop(ctx, case, maxl=4)
    ref = Fischer(case.apply, maxl=4)
    assert lp.ksp.guess_size() == (0, 4)
    sizes = []
    for k in range(7):
        xk = mean_free(case.N, 500 + k)
        bk = lp.mult(xk)
        lp.form(bk)
        ref.form(bk)
        sizes.append(lp.update(bk, xk))
        assert ref.update(xk) == sizes[-1]
        bf = O.fill_random(case.N, 600 + k)
        got, want = lp.form(bf), ref.form(bf)
        err = float(np.max(np.abs(got - want))) / float(np.max(np.abs(want)))
        print(f"{op} cycle {k} curl {sizes[-1]} guess err {err:.3e}")
        assert err <= X_RTOL, (k, err)
    assert sizes == [1, 2, 3, 4, 1, 2, 3]
    lp.destroy()


def test_span_exact_and_projection(ctx):
    case = Case((16, 16, 16), rtol=1e-8)
    lp = Loop(ctx, case, maxl=10)
    xs = [mean_free(case.N, 700 + k) for k in range(3)]
    bs = []
    for xk in xs:
        bs.append(lp.mult(xk))
        lp.form(bs[-1])
        lp.update(bs[-1], xk)
    assert lp.ksp.guess_size() == (3, 10)
    c = (0.7, -1.3, 0.4)
    b = sum(ck * bk for ck, bk in zip(c, bs))
    want = sum(ck * xk for ck, xk in zip(c, xs))
    g = lp.form(b)
    err = float(np.max(np.abs(g - want))) / float(np.max(np.abs(want)))
    print(f"span err {err:.3e}")
    assert err <= X_RTOL
    # b lies in the span: the solve has nothing left to do
    x0, (reason, its, hist, xs_, _) = lp.solve(b)
    assert reason in (2, 3) and its == 0, (reason, its)
    assert np.array_equal(xs_, x0)
    assert lp.ksp.guess_size() == (3, 10)  # the new direction is exactly 0: not added
    # the guess is an orthogonal projection in the residual
    for seed in (801, 802):
        br = O.fill_random(case.N, seed)
        gr = lp.form(br)
        res = float(np.linalg.norm(br - case.apply(gr)))
        assert res <= float(np.linalg.norm(br)) * (1 + 1e-12), (res, np.linalg.norm(br))
    lp.destroy()


# ---------------------------------------------------------------------------------------------
# 6: a time loop
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pc", ["jacobi", "mg"])
def test_time_loop(ctx, pc):
    """12 steps of the three-field family, maxl 10: every solve is the restatement's solve from
    the guess the library formed, and from step 3 on it takes at most a quarter of the iterations
    of a warm start from the previous x (measured on the oracle: at most 3 against at least 42
    with jacobi, at most 1 against 9 with mg)."""
    case = Case((16, 16, 16), pc=pc, rtol=1e-8)
    lp = Loop(ctx, case, maxl=10)
    warm = Loop(ctx, case, argv=case.argv(False) + ["-ksp_initial_guess_nonzero"])
    warm.x.set(0.0)
    for t in range(12):
        b = family(case, t)
        x0, got = lp.solve(b)
        check(case, got, restate(case, b, x0), tag=f"loop {pc} step {t}")
        warm.b.set_values(b)
        _, its_warm, _ = warm.ksp.solve(warm.b, warm.x)
        print(f"{pc} step {t}: fischer its {got[1]} warm its {its_warm} "
              f"curl {lp.ksp.guess_size()[0]}")
        if t >= 3:
            assert 4 * got[1] <= its_warm, (t, got[1], its_warm)
    lp.destroy()
    warm.destroy()


# ---------------------------------------------------------------------------------------------
# 7: every setup / iteration path
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["none", "single_reduction", "sor", "assembled",
                                  "compact_jacobi", "fft", "compact_fft"])
def test_paths_three_steps(ctx, name):
    case = plain(PATHS[name])
    lp = Loop(ctx, case, maxl=2)
    for t in range(3):
        b = family(case, t)
        x0, got = lp.solve(b)
        check(case, got, restate(case, b, x0), tag=f"{name} step {t}")
    lp.destroy()


# ---------------------------------------------------------------------------------------------
# 8: edges
# ---------------------------------------------------------------------------------------------
def test_zero_rhs_adds_nothing(ctx):
    case = Case((16, 16, 16), rtol=1e-8)
    lp = Loop(ctx, case, maxl=4)
    _, (reason, its, hist, xs, _) = lp.solve(np.zeros(case.N))
    assert reason > 0 and its == 0 and not np.any(xs)
    assert lp.ksp.guess_size() == (0, 4)
    lp.destroy()


def test_nan_rhs_leaves_the_basis(ctx):
    case = Case((16, 16, 16), rtol=1e-8)
    lp = Loop(ctx, case, maxl=4)
    x0, got = lp.solve(family(case, 0))
    assert got[0] == 2 and lp.ksp.guess_size()[0] == 1
    bad = family(case, 1)
    bad[37] = np.nan
    _, (reason, its, hist, _, _) = lp.solve(bad)
    assert reason == -9
    assert lp.ksp.guess_size()[0] == 1
    b = family(case, 2)
    x0, got = lp.solve(b)
    assert np.all(np.isfinite(x0)) and np.any(x0)
    check(case, got, restate(case, b, x0), tag="after nan")
    assert lp.ksp.guess_size()[0] == 2
    lp.destroy()


def test_reset(ctx):
    case = Case((16, 16, 16), rtol=1e-8)
    lp = Loop(ctx, case, maxl=4)
    lp.solve(family(case, 0))
    lp.solve(family(case, 1))
    assert lp.ksp.guess_size()[0] == 2
    lp.ksp.guess_reset()
    assert lp.ksp.guess_size() == (0, 4)
    b = family(case, 2)
    x0, got = lp.solve(b)
    assert not np.any(x0)
    check(case, got, restate(case, b, np.zeros(case.N)), tag="after reset")
    lp.destroy()


def test_nonzero_x_passed_in_is_ignored(ctx):
    case = Case((16, 16, 16), rtol=1e-8)
    res = []
    for x_in in (None, O.fill_random(case.N, 9)):
        lp = Loop(ctx, case, maxl=4)
        for t in range(2):
            _, got = lp.solve(family(case, t), x_in=x_in)
        res.append(got)
        lp.destroy()
    assert res[0][:2] == res[1][:2] and res[0][4] == res[1][4]
    assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])


@pytest.mark.parametrize("name", ["jacobi", "mg"])
def test_without_the_option_nothing_changes(ctx, name):
    """No option, or -ksp_guess_type none: the plain solve bit for bit (which the parity tests hold
    to the oracle), and the guess calls are out of order."""
    case = plain(PATHS[name])
    b = case.rhs()
    res = []
    for extra in ([], ["-ksp_guess_type", "none", "-ksp_guess_fischer_model", "1,3"]):
        lp = Loop(ctx, case, argv=case.argv(False) + extra)
        lp.b.set_values(b)
        lp.x.set_values(O.fill_random(case.N, 9))
        reason, its, hist = lp.ksp.solve(lp.b, lp.x)
        res.append((reason, its, np.asarray(hist), lp.x.get_values()))
        for call in (lambda: lp.ksp.guess_form(lp.b, lp.tmp),
                     lambda: lp.ksp.guess_update(lp.b, lp.tmp), lp.ksp.guess_reset,
                     lp.ksp.guess_size):
            with pytest.raises(pb.PbError) as e:
                call()
            assert e.value.code == ERR_STATE
        lp.destroy()
    want = restate(Case(case.n3, pc=case.pc, rtol=case.rtol), b, np.zeros(case.N))
    assert (res[0][0], res[0][1]) == (want[1], want[2])
    assert res[0][:2] == res[1][:2]
    assert np.array_equal(res[0][2], res[1][2]) and np.array_equal(res[0][3], res[1][3])


def test_one_shot_solve_has_no_memory(ctx):
    """pb_solve accepts the option; its KSP lives for one call, so every solve is the nonzero-guess
    solve from x = 0, whatever came before."""
    case = Case((16, 16, 16), rtol=1e-8)
    lp = Loop(ctx, case, argv=case.argv(False))
    for t in range(2):
        b = family(case, t)
        lp.b.set_values(b)
        lp.x.set_values(O.fill_random(case.N, 9))
        reason, its, hist = pb.solve(lp.P, lp.A, lp.x, lp.b, case.argv(False) + FISCHER)
        want = restate(case, b, np.zeros(case.N))
        assert (reason, its) == (want[1], want[2])
        assert np.max(np.abs(lp.x.get_values() - want[0])) <= X_RTOL * np.max(np.abs(want[0]))
    lp.destroy()


def test_bad_maxl_rejected_at_create(ctx):
    da = pb.DA(ctx, (8, 8, 8))
    A = pb.Mat(da, pb.STAR7)
    for maxl, code in ((0, ERR_ARG), (17, ERR_ARG)):
        with pytest.raises(pb.PbError) as e:
            pb.KSP(A, A, pb.ksp_options(FISCHER, guess_fischer_maxl=maxl))
        assert e.value.code == code
    with pytest.raises(pb.PbError) as e:
        pb.KSP(A, A, pb.ksp_options(FISCHER, guess_fischer_model=2))
    assert e.value.code == 5  # PB_ERR_UNSUPPORTED
    A.destroy()
    da.destroy()


# ---------------------------------------------------------------------------------------------
# 9: the loop on N ranks over the host transport
# ---------------------------------------------------------------------------------------------
def _multirank_loop(case, nranks, steps, maxl, tag):
    bs = [family(case, t, nranks) for t in range(steps)]

    def body(ctx, rank):
        rows = pb.slab_partition(case.n3[2], nranks, rank)
        lp = Loop(ctx, case, maxl=maxl, rows=rows)
        out = [lp.solve(b) for b in bs]
        lp.destroy()
        return rows, out

    res = run_ranks(nranks, body)
    for t, b in enumerate(bs):
        x0 = np.concatenate([out[t][0] for _, out in res])  # rank order = natural order
        want = restate(case, b, x0, nranks)
        for rows, out in res:
            check(case, out[t][1], want, rows=rows, tag=f"{tag} step {t} rows {rows}")
    return [res[0][1][t][1][1] for t in range(steps)]


@pytest.mark.parametrize("nranks,n3", [(2, (16, 16, 12)), (3, (16, 16, 12)), (3, (20, 16, 7))])
def test_multirank_loop(nranks, n3):
    case = Case(n3, rtol=1e-8)
    its = _multirank_loop(case, nranks, 4, 10, f"{nranks} ranks {n3}")
    assert its[3] < its[0], its


def test_multirank_compact_fft():
    """Config 5 on two ranks: the new direction's A-image by the decomposed compact operator."""
    case = plain(PATHS["compact_fft"])
    _multirank_loop(case, 2, 2, 2, "2 ranks compact fft")
