"""GPU tier: every user of the 7-point engine (pb_star7.hpp) computes the bits it computed on the
commit tests/golden/engine_unchanged.npz was recorded on -- the commit before the engine was split
from its solvers' passes.

scripts/record_engine_unchanged.py wrote the file (its docstring lists the users, the shapes --
one per tile shape the launch path can choose -- and the pairs multigrid refuses); the same
script's record_shape() runs here and must reproduce every history, (reason, its) pair, digest and
sampled value by np.array_equal. Identical device code does not settle this: a launch-descriptor
field set wrongly changes the z-chunks or the march direction and with them the partial sums.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location(
    "record_engine_unchanged", os.path.join(REPO, "scripts", "record_engine_unchanged.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

USERS = ["apply"] + list(R.USERS)
MG_USERS = {"mg_sor", "mg_rich", "mg_cheb"}
ODD_SHAPES = {(63, 30, 17), (66, 33, 16)}


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "engine_unchanged.npz"))


def keys_of(n3, user):
    pre = f"{R.shape_tag(n3)}__{user}"
    return sorted(k for k in golden().files if k.startswith(pre + "__") or
                  (user == "apply" and k.startswith(pre)))


def test_file_holds_every_pair():
    """5 shapes x (2 apply digests + 14 solves): 4 arrays per solve, 1 per refused pair, and the
    refused pairs are multigrid on the odd shapes and nothing else."""
    want = golden()
    assert len(R.SHAPES) == 5 and len(R.USERS) == 14
    refused = sorted(k for k in want.files if k.endswith("__error"))
    assert refused == sorted(f"{R.shape_tag(n)}__{u}__error" for n in ODD_SHAPES for u in MG_USERS)
    assert len(want.files) == 5 * 2 + (5 * 14 - 6) * 4 + 6
    for n3 in R.SHAPES:
        for user in USERS:
            assert keys_of(n3, user), (n3, user)


@pytest.mark.parametrize("user", USERS)
@pytest.mark.parametrize("n3", R.SHAPES, ids=[R.shape_tag(n) for n in R.SHAPES])
def test_engine_user_unchanged(ctx, n3, user):
    want = golden()
    got = R.record_shape(ctx, n3, users=[user])
    assert sorted(got) == keys_of(n3, user)
    for k in sorted(got):
        assert np.array_equal(got[k], want[k]), k
