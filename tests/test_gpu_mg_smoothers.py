"""GPU tier: the -mg_levels_* level smoothers of -pc_type mg against their numpy restatement
(tests/mg_smoothers_restatement.py, itself bit-identical to the pinned oracle for the default
smoother: tests/test_mg_smoothers_cpu.py; semantics in DESIGN.md §3.3).

The preconditioner apply is compared bit for bit: the library is built without FMA contraction,
every kernel (engine pass, pair kernel, vector kernel + residual pass) evaluates the restated
expressions in the restated order, and the smoother takes no sums. CG / Richardson / Chebyshev
around it are held to tests/parity_bars.py as tests/test_gpu_ksp_types.py holds them (the bars were
measured with a bit-identical PC apply, which is the situation here).

Grids: 16^3 (levels 16, 8, 4: the pair kernels), 24x16x32 with unequal spacings, and for the engine
pass -- whose launcher takes any grid on one rank -- the smallest hierarchy there is (8^3: one row
per wave, one x segment) beside 16^3, the anisotropic grid and 256x32x8 (two x segments, four rows
per wave), with mg_engine_min_plane tuned down to 0.

Every test here fails without the feature: the options and entry points do not exist.
"""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import poissbox_amd as pb
from oracle import oracle as O
from chebyshev_restatement import chebyshev
from ksp_types_restatement import richardson, ttol_margin_ok
from mg_smoothers_restatement import MgProblem, Smoother, VCycle, cg
from test_gpu_ksp_types import FIXED, FIXED_KW, check, gpu_solve

pytestmark = pytest.mark.gpu

STATE, UNSUPPORTED = 6, 5
CUBE8 = ((8, 8, 8), (1 / 8,) * 3)
CUBE16 = ((16, 16, 16), (1 / 16,) * 3)
CUBE32 = ((32, 32, 32), (1 / 32,) * 3)
ANISO = ((24, 16, 32), (1 / 24, 1 / 20, 1 / 40))
WIDE = ((256, 32, 8), (1 / 256, 1 / 32, 1 / 8))
PAIRS = {"sor": ("richardson", "sor", 1.0), "rich": ("richardson", "jacobi", 6.0 / 7.0),
         "cheb": ("chebyshev", "jacobi", 1.0)}
ENGINE = {"mg_engine_min_plane": 0}
PAIRK = {"mg_engine_min_plane": 10 ** 9}


def smoother(pair, nu):
    ksp, pc, scale = PAIRS[pair]
    return Smoother(ksp, pc, nu, scale)


@functools.lru_cache(maxsize=None)
def rhs(n):
    return O.fill_random(int(np.prod(n)), 20231015)


@functools.lru_cache(maxsize=None)
def restated_apply(n, h, pair, nu):
    z = VCycle(n, h, smoother(pair, nu)).apply(rhs(n))
    z.setflags(write=False)
    return z


def gpu_apply(ctx, n, h, argv, r, rows=None, set_default=False):
    """pb_ksp_pc_apply of -pc_type mg with argv's level smoother; rows = (k0, nk): this rank's
    planes. set_default: a KSP created without -mg_levels_* is given pb_pc_mg_opts_default."""
    da = pb.DA(ctx, n)
    P, A = pb.Mat(da, pb.ASSEMBLED27, h), pb.Mat(da, pb.STAR7, h)
    rv, zv = pb.Vec(da), pb.Vec(da)
    if rows is None:
        (_, _, k0), (_, _, nk) = da.get_corners()
        rows = (k0, nk)
    rv.set_values(r.reshape(n[2], -1)[rows[0]:rows[0] + rows[1]])
    zv.set_values(np.full(rows[1] * n[0] * n[1], 7.25))
    k = pb.KSP(A, P, pb.ksp_options(["-pc_type", "mg"] + list(argv)))
    try:
        if set_default:
            k.pc_mg_set_opts(pb.pc_mg_options())
        k.pc_apply(rv, zv)
        return rows, zv.get_values()
    finally:
        k.destroy()
        for o in (A, P, rv, zv):
            o.destroy()
        da.destroy()


# ---------------------------------------------------------------------------------------------
# the preconditioner apply against the restatement
# ---------------------------------------------------------------------------------------------
CASES = [("pair", CUBE16, {}), ("pair", ANISO, {}), ("engine", CUBE8, ENGINE),
         ("engine", CUBE16, ENGINE), ("engine", ANISO, ENGINE), ("engine", WIDE, ENGINE)]


@pytest.mark.parametrize("nu", [1, 2, 3])
@pytest.mark.parametrize("pair", list(PAIRS))
@pytest.mark.parametrize("kern,grid,tuning", CASES,
                         ids=[f"{c[0]}-{'x'.join(map(str, c[1][0]))}" for c in CASES])
def test_pc_apply_bit_identical_to_restatement(ctx, tune, kern, grid, tuning, pair, nu):
    n, h = grid
    for name, v in tuning.items():
        tune.set(name, v)
    _, z = gpu_apply(ctx, n, h, smoother(pair, nu).argv(), rhs(n))
    want = restated_apply(n, h, pair, nu)
    diff = float(np.max(np.abs(z - want)) / np.max(np.abs(want)))
    print(f"{kern} {n} {pair} nu={nu}: max relative difference {diff:.3e}")
    assert np.array_equal(z, want), diff


@pytest.mark.parametrize("grid", [CUBE16, ANISO, CUBE32], ids=["16", "aniso", "32"])
def test_default_options_keep_the_default_bits(ctx, grid):
    """A KSP given pb_pc_mg_opts_default (or the reference README's command line) returns the bits
    of a KSP given nothing: the oracle's V(1,1)."""
    n, h = grid
    r = rhs(n)
    _, z0 = gpu_apply(ctx, n, h, [], r)
    _, z1 = gpu_apply(ctx, n, h, [], r, set_default=True)
    _, z2 = gpu_apply(ctx, n, h, ["-mg_coarse_sub_pc_type", "svd", "-mg_levels_ksp_rtol", "1.0e-4",
                                  "-mg_levels_ksp_type", "richardson", "-mg_levels_pc_type",
                                  "sor"], r)
    assert np.array_equal(z0, O.mg_apply(r, n, h))
    assert np.array_equal(z0, z1) and np.array_equal(z0, z2)


@pytest.mark.parametrize("pair", ["rich", "cheb"])
def test_engine_pass_equals_pair_kernel_equals_unfused(ctx, tune, pair):
    """mg_engine_min_plane high and low, mg_poly_fused 0 and 1, on a grid whose fine planes are
    1024 wide with more 4-row columns than CUs (the engine's 8-row tiles) and on 256x32x8."""
    for n in ((1024, 528, 8), (256, 32, 8)):
        h = tuple(1.0 / m for m in n)
        r = rhs(n)
        out = []
        for tuning in (ENGINE, PAIRK, dict(ENGINE, mg_poly_fused=0), dict(PAIRK, mg_poly_fused=0)):
            pb.tune_reset()
            for name, v in tuning.items():
                tune.set(name, v)
            out.append(gpu_apply(ctx, n, h, smoother(pair, 3).argv(), r)[1])
        assert np.all(np.isfinite(out[0]))
        for z in out[1:]:
            assert np.array_equal(out[0], z), n


@pytest.mark.parametrize("nranks", [2, 4])
@pytest.mark.parametrize("pair", ["cheb", "sor"])
def test_split_grid_bit_identical_to_one_rank(pair, nranks):
    """32^3 on 2 and 4 ranks over the host transport (16- and 8-plane slabs): the Jacobi-type
    smoothers run the vector kernel + ghost exchange + residual pass there."""
    from test_gpu_parity import run_ranks
    n, h = CUBE32
    want = restated_apply(n, h, pair, 2).reshape(n[2], -1)
    argv = smoother(pair, 2).argv()

    def body(ctx, rank):
        return gpu_apply(ctx, n, h, argv, rhs(n))

    for (k0, nk), z in run_ranks(nranks, body):
        assert nk == n[2] // nranks
        assert np.array_equal(z, want[k0:k0 + nk].reshape(-1)), (pair, nranks, k0)


# ---------------------------------------------------------------------------------------------
# solves around the new preconditioner settings
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def cg_case(n, h, pair, nu):
    prob = MgProblem(n, h, smoother(pair, nu))
    b = prob.rhs()
    x, reason, its, hist = cg(prob, b, rtol=1e-10)
    assert reason == 2 and ttol_margin_ok(hist, 1e-10, hist[0])
    return prob, b, (x, reason, its, hist, float(hist[0]))


@pytest.mark.parametrize("pair", ["cheb", "rich", "sor"])
@pytest.mark.parametrize("grid", [CUBE32, ANISO], ids=["32", "aniso"])
def test_cg_solves_match_restatement(ctx, grid, pair):
    prob, b, want = cg_case(grid[0], grid[1], pair, 2)
    got = gpu_solve(ctx, prob, b, ["-ksp_type", "cg", "-ksp_rtol", "1e-10"] + prob.vc.sm.argv())
    check(prob, got, want, tag=f"cg {grid[0]} {pair} nu=2")


@pytest.mark.parametrize("pair", ["cheb", "sor"])
@pytest.mark.parametrize("outer", ["richardson", "chebyshev"])
def test_stationary_outer_solvers_run_with_the_settings(ctx, outer, pair):
    n, h = CUBE16
    prob = MgProblem(n, h, smoother(pair, 2))
    b = prob.rhs()
    if outer == "richardson":
        want = richardson(prob, b, scale=0.75, max_it=6, **FIXED_KW)
        argv = ["-ksp_type", "richardson", "-ksp_richardson_scale", "0.75"]
    else:
        want = chebyshev(prob, b, 0.1, 1.1, max_it=6, **FIXED_KW)
        argv = ["-ksp_type", "chebyshev", "-ksp_chebyshev_eigenvalues", "0.1,1.1"]
    got = gpu_solve(ctx, prob, b, argv + FIXED + ["-ksp_max_it", "6"] + prob.vc.sm.argv())
    check(prob, got, want, tag=f"{outer} {pair}")


@pytest.mark.parametrize("pair", ["cheb", "rich", "sor"])
def test_nan_rhs_ends_with_nanorinf(ctx, pair):
    n, h = CUBE16
    prob = MgProblem(n, h, smoother(pair, 2))
    b = prob.rhs()
    b[37] = np.nan
    reason, its, hist = gpu_solve(ctx, prob, b, ["-ksp_rtol", "1e-8"] + prob.vc.sm.argv())[:3]
    assert (reason, its) == (-9, 0) and len(hist) == 1 and not np.isfinite(hist[0])


def test_set_opts_errors_and_get(ctx):
    da = pb.DA(ctx, (16, 16, 16))
    P, A, _, _ = pb.initialise_linear_system(da, (1 / 16,) * 3)
    kj = pb.KSP(A, P, ["-pc_type", "jacobi"])
    km = pb.KSP(A, P, ["-pc_type", "mg"])
    try:
        with pytest.raises(pb.PbError) as e:
            kj.pc_mg_set_opts(pb.pc_mg_options())
        assert e.value.code == STATE
        with pytest.raises(pb.PbError) as e:
            kj.pc_mg_get_opts()
        assert e.value.code == STATE
        assert km.pc_mg_get_opts().levels_ksp_max_it == 1
        bad = pb.pc_mg_options(levels_ksp_type=pb.MG_LEVELS_CHEBYSHEV)
        with pytest.raises(pb.PbError) as e:
            km.pc_mg_set_opts(bad)
        assert e.value.code == UNSUPPORTED
        assert km.pc_mg_get_opts().levels_ksp_type == pb.MG_LEVELS_RICHARDSON  # left as it was
        km.pc_mg_set_opts(pb.pc_mg_options(levels_ksp_type=pb.MG_LEVELS_CHEBYSHEV,
                                           levels_pc_type=pb.MG_LEVELS_JACOBI,
                                           levels_ksp_max_it=2))
        got = km.pc_mg_get_opts()
        assert (got.levels_ksp_type, got.levels_pc_type, got.levels_ksp_max_it) == (1, 1, 2)
    finally:
        for o in (kj, km, A, P):
            o.destroy()
        da.destroy()
