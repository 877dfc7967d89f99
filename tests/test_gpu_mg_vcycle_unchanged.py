"""GPU tier: the multigrid host path computes the bits, and launches the passes, of the commit
tests/golden/mg_vcycle_unchanged.npz was recorded on -- the commit before the V-cycle's host code
moved into pb_mg.cpp behind one level plan, one driver and one launcher per pass.

scripts/record_mg_vcycle_unchanged.py wrote the file (its docstring lists the topologies and their
cases); the same script's record_topology() runs here and must reproduce, of every rank, the digest
of one PC application, every history, (reason, its) pair, digest and sampled value of a CG solve
run as begin, iterate(3), iterate(7), end, and the launch count of every multigrid phase, by
np.array_equal. The oracle comparisons (test_pc_apply_bit_exact and the others) pin the V-cycle's
output; the launch counts here also pin which kernels produced it.
"""
import functools
import importlib.util
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location(
    "record_mg_vcycle_unchanged", os.path.join(REPO, "scripts", "record_mg_vcycle_unchanged.py"))
R = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(R)

ONE_RANK = [(t, c) for t in ("one128", "one32") for c in R.TOPOLOGIES[t][3]]
HOST = [(t, c) for t in ("host2", "host3") for c in R.TOPOLOGIES[t][3]]


@functools.lru_cache(maxsize=None)
def golden():
    return np.load(os.path.join(REPO, "tests", "golden", "mg_vcycle_unchanged.npz"))


def keys_of(topo, case=None):
    pre = f"{topo}__" + (f"{case}__" if case else "")
    return sorted(k for k in golden().files if k.startswith(pre))


def compare(got, want_keys):
    want = golden()
    assert sorted(got) == want_keys
    differing = [k for k in want_keys if not np.array_equal(got[k], want[k])]
    assert not differing, differing


def test_file_holds_every_case():
    """per rank six arrays per case; no case was refused or dropped, and the cases reach the
    passes they are there for"""
    want = golden()
    n = 0
    for topo, (nranks, _, _, cases) in R.TOPOLOGIES.items():
        for case in cases:
            for rank in range(nranks):
                pre = f"{topo}__{case}__r{rank}__"
                assert sorted(k[len(pre):] for k in want.files if k.startswith(pre)) == R.WHAT, pre
                n += len(R.WHAT)
                custom = R.case_of(case)[2]
                assert len(want[pre + "launches"]) == len(R.PHASES) - (4 if custom else 0)
                assert len(want[pre + "history"]) == R.E.ITS + 1
    assert len(want.files) == n == 330

    def launches(topo, case, phase):
        return int(want[f"{topo}__{case}__r0__launches"][R.PHASES.index(phase)])

    # one PC application and 11 in the solve, one launch of each fused pass per application
    assert launches("one128", "mg_engine", "mg_apply") == 12
    assert launches("one128", "mg_engine", "mg_presmooth_restrict") == 12
    assert launches("one128", "mg_engine", "mg_post_sweep") == 12
    assert launches("one32", "mg_engine", "mg_post_sweep") == 0
    for topo in ("host2", "host3"):
        assert launches(topo, "mg_nosplitfused", "mg_presmooth_residual") == 12
        assert launches(topo, "mg_nosplitfused", "mg_sor_sweep2") == 12
        assert launches(topo, "mg_splitfused", "mg_post_sweep") == 12
    assert launches("one128", "cheb_e1_f1", "mg_poly") > 0
    assert launches("one128", "cheb_e1_f0", "mg_poly") == 0


@pytest.mark.parametrize("topo,case", ONE_RANK, ids=[f"{t}-{c}" for t, c in ONE_RANK])
def test_one_rank_vcycle_unchanged(ctx, topo, case):
    compare(R.record_topology(topo, [case], ctx), keys_of(topo, case))


@pytest.mark.parametrize("topo,case", HOST, ids=[f"{t}-{c}" for t, c in HOST])
def test_host_transport_vcycle_unchanged(topo, case):
    """2 ranks with 16 planes each, 3 ranks with four: the decomposed V-cycle with the coarse
    levels gathered, with halo exchanges on every level, and on the fused passes with deep ghosts"""
    compare(R.record_topology(topo, [case]), keys_of(topo, case))


def test_one_rank_communicator_vcycle_unchanged():
    """force_comm: the decomposed paths over a one-rank RCCL communicator"""
    compare(R.record_topology("comm"), keys_of("comm"))
