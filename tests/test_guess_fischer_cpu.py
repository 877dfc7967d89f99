"""CPU tier of the projected initial guess (-ksp_guess_type fischer): the options through
pb_ksp_opts_parse, and the numpy restatement (tests/fischer_restatement.py) against itself.

PETSc names: -ksp_guess_type none|fischer, -ksp_guess_fischer_model <model>[,<maxl>] (default
"1,10"). Only model 1 exists here; maxl is 1..16 (the multi-vector kernels' width).
"""
import numpy as np
import pytest

import poissbox_amd as pb
from fischer_restatement import Fischer
from oracle import oracle as O

UNSUPPORTED, ARG = 5, 1


def _guess(o):
    return o.guess_type, o.guess_fischer_model, o.guess_fischer_maxl


def test_defaults():
    assert _guess(pb.ksp_options()) == (0, 1, 10)
    # other options leave them alone
    assert _guess(pb.ksp_options(["-pc_type", "mg", "-ksp_initial_guess_nonzero"])) == (0, 1, 10)


def test_guess_type():
    assert _guess(pb.ksp_options(["-ksp_guess_type", "fischer"])) == (1, 1, 10)
    assert _guess(pb.ksp_options(["-ksp_guess_type", "fischer", "-ksp_guess_type", "none"])) == \
        (0, 1, 10)
    with pytest.raises(pb.PbError) as e:
        pb.ksp_options(["-ksp_guess_type", "pod"])
    assert e.value.code == UNSUPPORTED


def test_model_and_maxl():
    o = pb.ksp_options(["-ksp_guess_type", "fischer", "-ksp_guess_fischer_model", "1,4"])
    assert _guess(o) == (1, 1, 4)
    # a bare model keeps maxl
    assert _guess(pb.ksp_options(["-ksp_guess_fischer_model", "1"])) == (0, 1, 10)
    assert _guess(pb.ksp_options(["-ksp_guess_fischer_model", "1,4",
                                  "-ksp_guess_fischer_model", "1"])) == (0, 1, 4)
    assert _guess(pb.ksp_options(["-ksp_guess_fischer_model", "1,16"])) == (0, 1, 16)
    assert _guess(pb.ksp_options(["-ksp_guess_fischer_model", "1,1"])) == (0, 1, 1)


@pytest.mark.parametrize("value", ["2,10", "3,10", "2", "3"])
def test_other_models_unsupported(value):
    with pytest.raises(pb.PbError) as e:
        pb.ksp_options(["-ksp_guess_fischer_model", value])
    assert e.value.code == UNSUPPORTED


@pytest.mark.parametrize("value", ["1,0", "1,17", "1,-3"])
def test_maxl_out_of_range(value):
    with pytest.raises(pb.PbError) as e:
        pb.ksp_options(["-ksp_guess_fischer_model", value])
    assert e.value.code == ARG


def test_other_options_unaffected():
    o = pb.ksp_options(["-ksp_rtol", "1e-9", "-ksp_guess_type", "fischer", "-pc_type", "mg",
                        "-ksp_guess_fischer_model", "1,7", "-ksp_max_it", "77",
                        "-ksp_initial_guess_nonzero"])
    assert _guess(o) == (1, 1, 7)
    assert (o.rtol, o.pc_type, o.max_it, o.initial_guess_nonzero) == (1e-9, pb.PC_MG, 77, 1)
    # a following option is not eaten as the value
    o = pb.ksp_options(["-ksp_guess_fischer_model", "-ksp_rtol", "1e-7"])
    assert _guess(o) == (0, 1, 10) and o.rtol == 1e-7
    o = pb.ksp_options(["-ksp_guess_type", "fischer", "-ksp_rtol", "1e-7"])
    assert _guess(o) == (1, 1, 10) and o.rtol == 1e-7
    # the keyword form sets the fields
    assert _guess(pb.ksp_options(guess_type=1, guess_fischer_maxl=3)) == (1, 1, 3)


# ---------------------------------------------------------------------------------------------
# the restatement against itself (passes without the library's feature)
# ---------------------------------------------------------------------------------------------
N3 = (16, 16, 16)
H = tuple(1.0 / m for m in N3)


def _mean_free(seed):
    x = O.fill_random(int(np.prod(N3)), seed)
    return x - x.mean()


def _apply(x):
    return O.stencil(x, N3, H)


def test_restatement_orthonormal_and_span_exact():
    xs = [_mean_free(s) for s in (1, 2, 3)]
    bs = [_apply(x) for x in xs]
    f = Fischer(_apply, maxl=10)
    for k, (x, b) in enumerate(zip(xs, bs)):
        f.form(b)
        assert f.update(x) == k + 1
    gram = np.array([[np.dot(p, q) for q in f.btilde] for p in f.btilde])
    err = float(np.max(np.abs(gram - np.eye(3))))
    print("gram error", err)
    assert err <= 1e-14
    c = (0.7, -1.3, 0.4)
    g = f.form(sum(ck * bk for ck, bk in zip(c, bs)))
    want = sum(ck * xk for ck, xk in zip(c, xs))
    err = float(np.max(np.abs(g - want))) / float(np.max(np.abs(want)))
    print("span error", err)
    assert err <= 1e-14


def test_restatement_restart_cycle():
    f = Fischer(_apply, maxl=4)
    sizes = []
    for k in range(7):
        x = _mean_free(10 + k)
        f.form(_apply(x))
        sizes.append(f.update(x))
    assert sizes == [1, 2, 3, 4, 1, 2, 3]
