"""CPU tier: -ksp_type chebyshev through the option parsers, the pb_ksp_chebyshev_opts struct,
pb_tridiag_extreme_eigenvalues, and the properties of the numpy restatement the GPU tests compare
against (tests/chebyshev_restatement.py).
"""
import ctypes as C
import math

import numpy as np
import pytest

import poissbox_amd as pb
from oracle import oracle as O
from poissbox_amd import _lib as L
from chebyshev_restatement import (chebyshev, coefficients, estimate, jacobi_spectrum, lanczos,
                                   petsc_c_recurrence)
from ksp_types_restatement import Problem, richardson

UNSUPPORTED, ARG = 5, 1


def test_enum_and_defaults():
    assert pb.KSP_CHEBYSHEV == 3
    o = pb.ksp_options()
    assert o.ksp_type == pb.KSP_CG
    assert (o.chebyshev_emin, o.chebyshev_emax) == (0.0, 0.0)
    assert list(o.chebyshev_esteig) == [0.0, 0.1, 0.0, 1.1]
    assert o.chebyshev_esteig_steps == 10


def test_settings_struct_matches_header(tmp_path):
    """pb_ksp_opts keeps its layout (tests/test_ksp_types_cpu.py pins richardson_scale as its last
    field): the Chebyshev settings are a struct of their own, whose ctypes mirror has the C size
    and offsets (gcc on include/poissbox_gpu.h, as tests/test_abi.py does for the other structs)."""
    import os
    import subprocess
    assert [f[0] for f in L.KspOpts._fields_][-1] == "richardson_scale"
    assert C.sizeof(pb.ksp_options()) == C.sizeof(L.KspOpts)
    py = L.KspChebyshevOpts
    assert [f[0] for f in py._fields_] == ["emin", "emax", "esteig", "esteig_steps"]
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "poissbox_gpu.h"',
             'int main(void) {', '  printf("size %zu\\n", sizeof(pb_ksp_chebyshev_opts));']
    for f in py._fields_:
        lines.append(f'  printf("{f[0]} %zu\\n", offsetof(pb_ksp_chebyshev_opts, {f[0]}));')
    lines.append('  return 0; }')
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines) + "\n")
    exe = tmp_path / "layout"
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run(["gcc", "-I", os.path.join(repo, "include"), str(src), "-o", str(exe)],
                   check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], check=True, capture_output=True,
                                                 text=True).stdout.splitlines())
    assert int(got["size"]) == C.sizeof(py)
    for f in py._fields_:
        assert int(got[f[0]]) == getattr(py, f[0]).offset, f[0]
    major, minor = C.c_int(), C.c_int()
    L.call("pb_version", C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == (0, 2)


def test_c_level_parse_and_defaults():
    c = L.KspChebyshevOpts()
    L.call("pb_ksp_chebyshev_opts_default", C.byref(c))
    assert (c.emin, c.emax, list(c.esteig), c.esteig_steps) == (0.0, 0.0, [0.0, 0.1, 0.0, 1.1], 10)
    argv = ["-ksp_rtol", "1e-3", "-ksp_chebyshev_eigenvalues", "-8,-0.5", "-ksp_type", "cg"]
    arr = (C.c_char_p * len(argv))(*[a.encode() for a in argv])
    L.call("pb_ksp_chebyshev_opts_parse", C.byref(c), len(argv), arr)
    assert (c.emin, c.emax, c.esteig_steps) == (-8.0, -0.5, 10)
    # pb_ksp_opts_parse reports the same errors without keeping the values
    o = L.KspOpts()
    L.call("pb_ksp_opts_default", C.byref(o))
    bad = ["-ksp_chebyshev_eigenvalues", "2,1"]
    arr = (C.c_char_p * 2)(*[a.encode() for a in bad])
    for fn, st in (("pb_ksp_opts_parse", o), ("pb_ksp_chebyshev_opts_parse", c)):
        with pytest.raises(pb.PbError) as e:
            L.call(fn, C.byref(st), 2, arr)
        assert e.value.code == ARG


def test_every_option_parsed():
    o = pb.ksp_options(["-ksp_type", "chebyshev", "-ksp_chebyshev_eigenvalues", "0.05,2.0",
                        "-ksp_chebyshev_esteig", "0,0.25,0.5,1.2", "-ksp_chebyshev_esteig_steps",
                        "17", "-ksp_chebyshev_esteig_noisy", "-pc_type", "mg", "-ksp_max_it", "9"])
    assert o.ksp_type == pb.KSP_CHEBYSHEV and o.pc_type == pb.PC_MG and o.max_it == 9
    assert (o.chebyshev_emin, o.chebyshev_emax) == (0.05, 2.0)
    assert list(o.chebyshev_esteig) == [0.0, 0.25, 0.5, 1.2]
    assert o.chebyshev_esteig_steps == 17
    # negative pairs are legal (-pc_type none: the Laplacian is negative semi-definite)
    o = pb.ksp_options(["-ksp_chebyshev_eigenvalues", "-8e3,-1.5e1"])
    assert (o.chebyshev_emin, o.chebyshev_emax) == (-8000.0, -15.0)
    # bounds alone leave the type
    assert o.ksp_type == pb.KSP_CG
    for v in ("true", "1", "yes"):
        pb.ksp_options(["-ksp_chebyshev_esteig_noisy", v, "-ksp_max_it", "3"])
    for steps in (1, 64):
        assert pb.ksp_options(["-ksp_chebyshev_esteig_steps",
                               str(steps)]).chebyshev_esteig_steps == steps
    o = pb.ksp_options(chebyshev_esteig=(0.0, 0.2, 0.0, 1.05), chebyshev_emax=2.0,
                       chebyshev_emin=0.1)
    assert list(o.chebyshev_esteig) == [0.0, 0.2, 0.0, 1.05] and o.chebyshev_emax == 2.0


def test_later_ksp_type_wins():
    assert pb.ksp_options(["-ksp_type", "chebyshev", "-ksp_type", "cg"]).ksp_type == pb.KSP_CG
    assert pb.ksp_options(["-ksp_type", "richardson", "-ksp_type",
                           "chebyshev"]).ksp_type == pb.KSP_CHEBYSHEV


@pytest.mark.parametrize("name", ["gmres", "bcgs", "Chebyshev", "cheby"])
def test_other_types_stay_unsupported(name):
    with pytest.raises(pb.PbError) as e:
        pb.ksp_options(["-ksp_type", name])
    assert e.value.code == UNSUPPORTED


@pytest.mark.parametrize("v", ["1.0,1.0", "2.0,0.1", "-0.5,2.0", "0,2.0", "0.1,0", "0,0",
                               "nan,2.0", "0.1,nan", "0.1,inf", "-inf,-1", "1.5", "0.1,2.0,3.0",
                               "abc", "0.1;2.0", "-1.0,-2.0"])
def test_invalid_bounds_at_parse(v):
    with pytest.raises(pb.PbError) as e:
        pb.ksp_options(["-ksp_chebyshev_eigenvalues", v])
    assert e.value.code == ARG


@pytest.mark.parametrize("steps", ["0", "65", "-3"])
def test_invalid_steps_at_parse(steps):
    with pytest.raises(pb.PbError) as e:
        pb.ksp_options(["-ksp_chebyshev_esteig_steps", steps])
    assert e.value.code == ARG


@pytest.mark.parametrize("v", ["0,0.1,0", "0,0.1,0,nan", "0,0.1,0,1.1,2"])
def test_invalid_transform_at_parse(v):
    with pytest.raises(pb.PbError) as e:
        pb.ksp_options(["-ksp_chebyshev_esteig", v])
    assert e.value.code == ARG


def test_esteig_noisy_false_unsupported():
    for argv in (["-ksp_chebyshev_esteig_noisy", "false"], ["-ksp_chebyshev_esteig_noisy", "0"],
                 ["-ksp_type", "chebyshev", "-ksp_chebyshev_esteig_noisy", "no", "-ksp_rtol",
                  "1e-3"]):
        with pytest.raises(pb.PbError) as e:
            pb.ksp_options(argv)
        assert e.value.code == UNSUPPORTED


# ---------------------------------------------------------------------------------------------
# pb_tridiag_extreme_eigenvalues (host code)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 10, 64])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_tridiag_extremes(n, seed):
    rng = np.random.default_rng(100 * n + seed)
    d = rng.standard_normal(n) * (10.0 ** rng.integers(-3, 4))
    e = rng.standard_normal(n - 1) * (10.0 ** rng.integers(-3, 4))
    T = np.diag(d) + np.diag(e, 1) + np.diag(e, -1)
    ev = np.linalg.eigvalsh(T)
    lo, hi = pb.tridiag_extreme_eigenvalues(d, e)
    radius = float(np.max(np.abs(ev)))
    assert abs(lo - ev[0]) <= 1e-12 * radius and abs(hi - ev[-1]) <= 1e-12 * radius


def test_tridiag_special_cases():
    assert pb.tridiag_extreme_eigenvalues([3.5]) == (3.5, 3.5)
    # zero off-diagonals: the diagonal itself; a Lanczos matrix of the 1-D Laplacian
    lo, hi = pb.tridiag_extreme_eigenvalues([2.0, -1.0, 5.0], [0.0, 0.0])
    assert abs(lo + 1.0) <= 1e-14 and abs(hi - 5.0) <= 1e-14
    n = 20
    lo, hi = pb.tridiag_extreme_eigenvalues([2.0] * n, [-1.0] * (n - 1))
    k = np.arange(1, n + 1)
    ev = 2.0 - 2.0 * np.cos(np.pi * k / (n + 1))
    assert abs(lo - ev.min()) <= 1e-13 and abs(hi - ev.max()) <= 1e-13


def test_tridiag_argument_errors():
    for n in (0, 65):
        with pytest.raises(pb.PbError) as e:
            pb.tridiag_extreme_eigenvalues(np.ones(n), np.ones(max(n - 1, 0)))
        assert e.value.code == ARG
    with pytest.raises(pb.PbError) as e:
        pb.tridiag_extreme_eigenvalues([1.0, float("nan")], [0.5])
    assert e.value.code == ARG


# ---------------------------------------------------------------------------------------------
# the restatement's own properties (oracle blocks on the CPU)
# ---------------------------------------------------------------------------------------------
def _exact_case():
    prob = Problem((16, 16, 16))
    return prob, prob.rhs(), jacobi_spectrum(prob)


def test_restatement_converges_with_exact_bounds():
    prob, b, (lmin, lmax) = _exact_case()
    assert abs(lmax - 2.0) < 1e-14
    x, reason, its, hist, rn0 = chebyshev(prob, b, lmin, lmax, rtol=1e-8)
    print("jacobi 16^3 exact bounds", lmin, lmax, "its", its)
    assert reason == 2 and len(hist) == its + 1 and 60 <= its <= 110
    assert hist[-1] <= 1e-8 * rn0 < hist[-2]
    assert np.linalg.norm(b - prob.apply(x)) / np.linalg.norm(b) < 1e-7
    # Richardson with the same scale needs far more updates
    slow = richardson(prob, b, scale=coefficients(lmin, lmax)[0], rtol=1e-8, max_it=4 * its)
    assert slow[1] == -3


def test_restatement_negative_pair_without_pc():
    """M^-1 A = A is negative: the pair (diag lmax, diag lmin) gives the same iterates."""
    prob, b, (lmin, lmax) = _exact_case()
    its = chebyshev(prob, b, lmin, lmax, rtol=1e-8)[2]
    none = Problem((16, 16, 16), pc="none")
    d = O.diag(none.h)
    assert d < 0
    x, reason, its_n, hist, _ = chebyshev(none, b, d * lmax, d * lmin, rtol=1e-8)
    assert (reason, its_n) == (2, its)


def test_restatement_first_update_is_richardson():
    prob, b, (lmin, lmax) = _exact_case()
    scale = coefficients(lmin, lmax)[0]
    one = chebyshev(prob, b, lmin, lmax, rtol=0.0, atol=0.0, max_it=1)
    ref = richardson(prob, b, scale=scale, rtol=0.0, atol=0.0, max_it=1)
    assert np.array_equal(one[0], ref[0]) and np.array_equal(one[3], ref[3])


def test_restatement_too_small_emax_diverges():
    prob, b, _ = _exact_case()
    x, reason, its, hist, rn0 = chebyshev(prob, b, 0.0254, 1.5)
    assert reason == -4 and hist[-1] >= 1e5 * rn0 > hist[-2] and len(hist) == its + 1


def test_restatement_long_run_stays_finite():
    """1500 updates: PETSc's c_k recurrence has overflowed long before, the ratio form has not."""
    prob, b, _ = _exact_case()
    x, reason, its, hist, _ = chebyshev(prob, b, 0.196, 2.155, rtol=0.0, atol=0.0, dtol=1e300,
                                        max_it=1500)
    assert (reason, its, len(hist)) == (-3, 1500, 1501)
    assert np.all(np.isfinite(hist)) and np.all(np.isfinite(x))
    assert petsc_c_recurrence(0.196, 2.155, 290) > 1e70
    assert not math.isfinite(petsc_c_recurrence(0.196, 2.155, 1500))


@pytest.mark.parametrize("n3", [(16, 16, 16), (24, 20, 18), (16, 16, 12), (32, 40, 48)])
def test_restated_estimate_covers_the_spectrum(n3):
    """1.1 x the 10-step estimate covers the true largest eigenvalue (2 for even extents) in every
    Jacobi case the tests use."""
    prob = Problem(n3)
    lo, hi, m = lanczos(prob)
    print(n3, "estimated extremes", lo, hi)
    assert m == 10 and 0.0 < lo < hi <= 2.0 + 1e-12
    assert 1.1 * hi >= jacobi_spectrum(prob)[1]
    emin, emax = estimate(prob)
    assert (emin, emax) == (0.1 * hi, 1.1 * hi)


def test_restated_estimate_fft_is_one_step():
    prob = Problem((16, 16, 16), pc="fft")
    lo, hi, m = lanczos(prob)
    assert m == 1 and lo == hi and abs(hi - 1.0) < 1e-12


def test_restated_estimate_without_pc_is_negative():
    lo, hi, m = lanczos(Problem((16, 16, 12), pc="none"))
    assert m == 10 and lo < hi < 0.0
