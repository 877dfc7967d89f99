"""GPU tier: the CG host enqueue paths compute the bits they computed on the commit
tests/golden/cg_enqueue_unchanged.npz was recorded on -- the commit before CG's host code moved into
pb_ksp_cg.cpp behind one pass descriptor and one halo-overlap helper.

scripts/record_cg_enqueue_unchanged.py wrote the file (its docstring lists the topologies and their
cases); the same script's record_topology() runs here and must reproduce every history, (reason,
its) pair, digest and sampled value of every rank by np.array_equal. Every solve runs as begin,
iterate(3), iterate(7), end, so the batch tails and the state slots across calls are compared too.
tests/golden/engine_unchanged.npz pins one rank and pb_ksp_solve only, and the multi-rank tests
compare with the oracle to 1e-11: a wrong partial offset or a reduction missing on a boundary launch
can hide under that, not under this.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location(
    "record_cg_enqueue_unchanged", os.path.join(REPO, "scripts", "record_cg_enqueue_unchanged.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

ONE_RANK = [(t, c) for t in ("one", "one64") for c in R.TOPOLOGIES[t][3]]


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "cg_enqueue_unchanged.npz"))


def keys_of(topo, case=None):
    pre = f"{topo}__" + (f"{case}__" if case else "")
    return sorted(k for k in golden().files if k.startswith(pre))


def compare(got, want_keys):
    want = golden()
    assert sorted(got) == want_keys
    differing = [k for k in want_keys if not np.array_equal(got[k], want[k])]
    assert not differing, differing


def test_file_holds_every_case():
    """per rank 2 digests per apply and 4 arrays per solve; no case was refused or dropped"""
    want = golden()
    n = 0
    for topo, (nranks, _, _, cases) in R.TOPOLOGIES.items():
        for case in cases:
            for rank in range(nranks):
                pre = f"{topo}__{case}__r{rank}__"
                what = ["digest0", "digest1"] if case == "apply" else ["digest", "history",
                                                                       "sample", "status"]
                assert sorted(k[len(pre):] for k in want.files if k.startswith(pre)) == what, pre
                n += len(what)
    assert len(want.files) == n == 196
    # Jacobi CG and the single reduction, folded and unfolded, are there on every topology
    for topo in ("one", "host2", "host3", "comm"):
        for case in ("cg", "cg_c1", "cg_sr"):
            assert keys_of(topo, case), (topo, case)


@pytest.mark.parametrize("topo,case", ONE_RANK, ids=[f"{t}-{c}" for t, c in ONE_RANK])
def test_one_rank_enqueue_unchanged(ctx, topo, case):
    compare(R.record_topology(topo, [case], ctx), keys_of(topo, case))


@pytest.mark.parametrize("topo", ["host2", "host3"])
def test_host_transport_enqueue_unchanged(topo):
    """2 ranks with two planes each (the nzl < 3 branch), 3 ranks with four (the overlap)"""
    compare(R.record_topology(topo), keys_of(topo))


def test_one_rank_communicator_enqueue_unchanged(tune):
    """force_comm: the decomposed paths with the boundary launches on the comm stream"""
    compare(R.record_topology("comm"), keys_of("comm"))
