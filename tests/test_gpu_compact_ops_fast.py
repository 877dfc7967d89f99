"""GPU tier: the factorised compact grad / div / interp (pb_compact_{grad,div,interp}_fast,
half-operator line passes) against the flang-built reference's fixtures and the oracle.

The bar is the fast Laplacian's FAST_RTOL = 1e-12 relative to max|reference| per output field
(grad: per component). The operation order differs from the reference's Thomas + Sherman-Morrison
sweeps; an independent (spectral) evaluation of the same circulant operators differs from the
oracle by 5.8e-16 .. 9.9e-16 of max|ref|, so the bar leaves three orders of magnitude for a correct
kernel and none for a wrong neighbour, coefficient or carry.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

import poissbox_amd as pb
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FAST_RTOL = 1e-12
EPS = np.finfo(float).eps

# the Laplacian's list (test_gpu_parity.py) plus three that target the new passes
SHAPES = [(64, 48, 40),      # x in registers, y and z on the LDS-PCR kernel
          (33, 17, 9),       # every axis on the fallback
          (128, 128, 64),
          (256, 192, 64),    # C = 4, 3
          (1024, 64, 64),    # C = 16
          (64, 768, 64),     # C = 12
          (128, 64, 384),    # C = 6
          (512, 64, 64),     # C = 8
          (40, 64, 64),      # register Y and Z passes, ragged last tile of 8 lines; x on the fallback
          (33, 64, 128)]     # odd row length: the strided register passes take their 8-byte moves


def _cases(golden, prefix):
    names = sorted({k.rsplit("__", 1)[0] for k in golden.files})
    return [n for n in names if n.split("__")[0] == prefix]


def _h(n3):
    return tuple(2 * np.pi / m for m in n3)


def _vecs(da, arrays):
    out = []
    for a in arrays:
        v = pb.Vec(da)
        if a is not None:
            v.set_values(a)
        out.append(v)
    return out


def _free(da, *vecs):
    for v in vecs:
        v.destroy()
    da.destroy()


def _grad_fast(ctx, n3, h3, f):
    da = pb.DA(ctx, n3)
    fv, d1, d2, d3 = _vecs(da, [f, None, None, None])
    pb.compact_grad_fast(da, h3, fv, [d1, d2, d3])
    got = [v.get_values() for v in (d1, d2, d3)]
    _free(da, fv, d1, d2, d3)
    return got


def _div_fast(ctx, n3, h3, f3):
    da = pb.DA(ctx, n3)
    f1, f2, f3v, out = _vecs(da, [f3[0], f3[1], f3[2], None])
    pb.compact_div_fast(da, h3, [f1, f2, f3v], out)
    got = out.get_values()
    _free(da, f1, f2, f3v, out)
    return got


def _interp_fast(ctx, n3, stagger, f):
    da = pb.DA(ctx, n3)
    fv, out = _vecs(da, [f, None])
    pb.compact_interp_fast(da, stagger, fv, out)
    got = out.get_values()
    _free(da, fv, out)
    return got


def _check(got, ref, what):
    err = float(np.max(np.abs(got - ref)))
    scale = float(np.max(np.abs(ref)))
    print(f"{what}: max|diff| {err:.3e} = {err / scale:.3e} of max|ref|")
    assert err <= FAST_RTOL * scale, (what, err, scale)


# ---------------------------------------------------------------------------------------------
# 1. the reference's own outputs
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("op", ["grad", "div", "interp", "interp_div"])
def test_fast_matches_reference_fixtures(ctx, golden, op):
    names = _cases(golden, op)
    assert names
    for name in names:
        m = golden[name + "__meta"]
        n3, h3 = tuple(int(v) for v in m[:3]), tuple(float(v) for v in m[3:])
        N = int(np.prod(n3))
        inp, ref = golden[name + "__in"], golden[name + "__out"]
        if op == "grad":
            got = _grad_fast(ctx, n3, h3, inp)
            for c in range(3):
                _check(got[c], ref[c * N:(c + 1) * N], f"{name} df{c + 1}")
        elif op == "div":
            _check(_div_fast(ctx, n3, h3, [inp[c * N:(c + 1) * N] for c in range(3)]), ref, name)
        else:
            _check(_interp_fast(ctx, n3, -1 if op == "interp" else 1, inp), ref, name)


# ---------------------------------------------------------------------------------------------
# 2. the oracle, by shape (one random field and one oracle evaluation per shape and operator)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _field(n3, ncomp=1):
    N = int(np.prod(n3))
    f = O.fill_random(ncomp * N, 77 + ncomp)
    f.setflags(write=False)
    return f


@pytest.mark.parametrize("n3", SHAPES)
def test_grad_fast_vs_oracle(ctx, n3):
    N = int(np.prod(n3))
    f = _field(n3)
    ref = O.grad(f, n3, _h(n3))
    got = _grad_fast(ctx, n3, _h(n3), f)
    for c in range(3):
        _check(got[c], ref[c * N:(c + 1) * N], f"grad {n3} df{c + 1}")


@pytest.mark.parametrize("n3", SHAPES)
def test_div_fast_vs_oracle(ctx, n3):
    N = int(np.prod(n3))
    f = _field(n3, 3)
    ref = O.div(f, n3, _h(n3))
    _check(_div_fast(ctx, n3, _h(n3), [f[c * N:(c + 1) * N] for c in range(3)]), ref, f"div {n3}")


@pytest.mark.parametrize("stagger", [-1, 1])
@pytest.mark.parametrize("n3", SHAPES)
def test_interp_fast_vs_oracle(ctx, n3, stagger):
    f = _field(n3)
    ref = O.interp(f, n3, stagger)
    _check(_interp_fast(ctx, n3, stagger, f), ref, f"interp {n3} stagger {stagger}")


def test_compact_lines_off_takes_the_fallback(ctx, tune):
    """The `compact_lines` tuning entry applies as for the Laplacian: 0 sends 64*C lines to the
    LDS-PCR kernel's half-operator term too (same bar)."""
    n3 = (128, 64, 64)
    N = int(np.prod(n3))
    tune.set("compact_lines", 0)
    f, f3 = _field(n3), _field(n3, 3)
    ref = O.grad(f, n3, _h(n3))
    for c, g in enumerate(_grad_fast(ctx, n3, _h(n3), f)):
        _check(g, ref[c * N:(c + 1) * N], f"grad, lines off, df{c + 1}")
    _check(_div_fast(ctx, n3, _h(n3), [f3[c * N:(c + 1) * N] for c in range(3)]),
           O.div(f3, n3, _h(n3)), "div, lines off")
    _check(_interp_fast(ctx, n3, 1, f), O.interp(f, n3, 1), "interp, lines off")


# ---------------------------------------------------------------------------------------------
# 3. composition: div_fast(grad_fast f) is the Laplacian (the oracle's own div(grad f) equals its
# lapl bit for bit)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n3", [(64, 64, 64), (64, 48, 40)])
def test_div_of_grad_is_lapl(ctx, n3):
    f = _field(n3)
    h3 = _h(n3)
    ref = O.lapl(f, n3, h3)
    da = pb.DA(ctx, n3)
    fv, d1, d2, d3, out = _vecs(da, [f, None, None, None, None])
    pb.compact_grad_fast(da, h3, fv, [d1, d2, d3])
    pb.compact_div_fast(da, h3, [d1, d2, d3], out)
    got = out.get_values()
    _free(da, fv, d1, d2, d3, out)
    _check(got, ref, f"div(grad) {n3}")


# ---------------------------------------------------------------------------------------------
# 4. constant field (the form of the Laplacian's constant test)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n3", [(64, 64, 64), (33, 17, 9)])
def test_constant_field(ctx, n3):
    c = 2.8170923
    h3 = _h(n3)
    f = np.full(int(np.prod(n3)), c)
    for comp, g in enumerate(_grad_fast(ctx, n3, h3, f)):
        worst = float(np.max(np.abs(g)))
        print(f"grad(const) {n3} df{comp + 1}: max {worst:.3e}")
        assert worst <= 100 * EPS * abs(c) / min(h3)
    for stagger in (-1, 1):
        worst = float(np.max(np.abs(_interp_fast(ctx, n3, stagger, f) - c)))
        print(f"interp(const) {n3} stagger {stagger}: max |fi - c| {worst:.3e}")
        assert worst <= 100 * EPS * abs(c)


# ---------------------------------------------------------------------------------------------
# 5. aliasing, 6. line lengths the fast path refuses
# ---------------------------------------------------------------------------------------------
PB_ERR_ARG = 1


def test_aliased_arguments_are_refused(ctx):
    n3 = (64, 16, 8)
    da = pb.DA(ctx, n3)
    a, b, c, d = _vecs(da, [_field(n3), None, None, None])
    bad = [lambda: pb.compact_grad_fast(da, _h(n3), a, [a, b, c]),
           lambda: pb.compact_grad_fast(da, _h(n3), a, [b, c, a]),
           lambda: pb.compact_grad_fast(da, _h(n3), a, [b, b, c]),
           lambda: pb.compact_grad_fast(da, _h(n3), a, [b, c, b]),
           lambda: pb.compact_div_fast(da, _h(n3), [a, b, c], a),
           lambda: pb.compact_div_fast(da, _h(n3), [a, b, c], c),
           lambda: pb.compact_div_fast(da, _h(n3), [a, a, c], d),
           lambda: pb.compact_div_fast(da, _h(n3), [a, b, b], d),
           lambda: pb.compact_interp_fast(da, -1, a, a),
           lambda: pb.compact_interp_fast(da, 1, a, a)]
    for i, call in enumerate(bad):
        with pytest.raises(pb.PbError) as e:
            call()
        assert e.value.code == PB_ERR_ARG, i
    # the same vectors, distinct: accepted
    pb.compact_grad_fast(da, _h(n3), a, [b, c, d])
    _free(da, a, b, c, d)


@pytest.mark.parametrize("n3", [(4100, 4, 4), (4, 4100, 4), (4, 4, 4100)])
def test_refused_line_length_gives_the_laplacians_error(ctx, n3):
    da = pb.DA(ctx, n3)
    a, b, c, d = _vecs(da, [np.ones(int(np.prod(n3))), None, None, None])
    with pytest.raises(pb.PbError) as e0:
        pb.compact_lapl_fast(da, _h(n3), a, b)
    for call in (lambda: pb.compact_grad_fast(da, _h(n3), a, [b, c, d]),
                 lambda: pb.compact_div_fast(da, _h(n3), [a, b, c], d),
                 lambda: pb.compact_interp_fast(da, -1, a, b),
                 lambda: pb.compact_interp_fast(da, 1, a, b)):
        with pytest.raises(pb.PbError) as e:
            call()
        assert e.value.code == e0.value.code
    _free(da, a, b, c, d)


# ---------------------------------------------------------------------------------------------
# 7. the Laplacian's passes and the batched solve compute what they computed before this change
# ---------------------------------------------------------------------------------------------
def test_existing_paths_unchanged(ctx):
    """tests/golden/compact_unchanged.npz was written by scripts/record_compact_unchanged.py on the
    commit before the compact host path was reduced to one line geometry, one length dispatch and
    one tiled launcher (its first twelve entries came out as the commit before the half-operator
    passes had recorded them); the same script's record() on this build must reproduce every
    digest and every sampled value."""
    spec = importlib.util.spec_from_file_location(
        "record_compact_unchanged", os.path.join(REPO, "scripts", "record_compact_unchanged.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    want = np.load(os.path.join(REPO, "tests", "golden", "compact_unchanged.npz"))
    got = mod.record(ctx)
    assert sorted(got) == sorted(want.files) and len(got) == 120
    for k in sorted(got):
        assert np.array_equal(got[k], want[k]), k
