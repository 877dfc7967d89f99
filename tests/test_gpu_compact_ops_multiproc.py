"""GPU tier, N processes on the one GPU (gloo host transport, as test_gpu_multiproc.py): the
factorised compact grad / div / interp on a z-slab decomposition. Their Z passes run on y-slabs
behind all-to-all transposes; on three ranks both the z split (22 / 21 / 21 planes) and the y split
(11 / 11 / 10 rows) of 64x32x64 are uneven.

Every rank's slab must be bit-identical to the one-rank result of the same call (a per-line
kernel whose arithmetic changes with the decomposition is a bug) and within FAST_RTOL = 1e-12 of
max|oracle| per output field."""
import functools

import numpy as np
import pytest

from test_dist_cpu import _run

pytestmark = pytest.mark.gpu

N3 = (64, 32, 64)
FAST_RTOL = 1e-12
FIELDS = ("grad1", "grad2", "grad3", "div", "interp-1", "interp+1")


def _inputs():
    from oracle import oracle as O
    N = int(np.prod(N3))
    return O.fill_random(N, 5), O.fill_random(3 * N, 6)


def _all_ops(rank, world, tr):
    """every fast call on this rank's slab: (k0, nk, {field: values})"""
    import poissbox_amd as pb
    ctx = pb.Context(0, rank, world)
    if world > 1:
        ctx.set_host_transport(tr.sendrecv, tr.allreduce, tr.alltoallv)
    da = pb.DA(ctx, N3, (2 * np.pi,) * 3)
    (_, _, k0), (_, _, nk) = da.get_corners()
    f, f3 = _inputs()
    N = int(np.prod(N3))
    slab = lambda a: a.reshape(N3[2], -1)[k0:k0 + nk]
    fv, v1, v2, v3, o1, o2, o3 = (pb.Vec(da) for _ in range(7))
    h = da.spacing
    res = {}
    fv.set_values(slab(f))
    pb.compact_grad_fast(da, h, fv, [o1, o2, o3])
    for c, o in enumerate((o1, o2, o3)):
        res[f"grad{c + 1}"] = o.get_values()
    for c, v in enumerate((v1, v2, v3)):
        v.set_values(slab(f3[c * N:(c + 1) * N]))
    pb.compact_div_fast(da, h, [v1, v2, v3], o1)
    res["div"] = o1.get_values()
    for s in (-1, 1):
        pb.compact_interp_fast(da, s, fv, o2)
        res[f"interp{s:+d}"] = o2.get_values()
    ctx.destroy()
    return k0, nk, res


@functools.lru_cache(maxsize=None)
def _references():
    """(one-rank GPU result, oracle) per field, whole grid as [k][j * i]; computed once"""
    from oracle import oracle as O
    f, f3 = _inputs()
    N = int(np.prod(N3))
    h = tuple(2 * np.pi / m for m in N3)
    g = O.grad(f, N3, h)
    orc = {f"grad{c + 1}": g[c * N:(c + 1) * N] for c in range(3)}
    orc["div"] = O.div(f3, N3, h)
    orc["interp-1"] = O.interp(f, N3, -1)
    orc["interp+1"] = O.interp(f, N3, 1)
    (_, _, one), = _run(1, _all_ops)  # a fresh process, like the ranks
    plane = lambda a: a.reshape(N3[2], -1)
    return {k: plane(one[k]) for k in FIELDS}, {k: plane(orc[k]) for k in FIELDS}


def test_one_rank_matches_oracle():
    one, orc = _references()
    for k in FIELDS:
        err = float(np.max(np.abs(one[k] - orc[k])))
        assert err <= FAST_RTOL * np.max(np.abs(orc[k])), (k, err)


@pytest.mark.parametrize("world", [2, 3])
def test_multiprocess_compact_ops(world):
    one, orc = _references()
    for k0, nk, res in _run(world, _all_ops):
        assert sorted(res) == sorted(FIELDS)
        for k in FIELDS:
            got = res[k].reshape(nk, -1)
            assert np.array_equal(got, one[k][k0:k0 + nk]), (world, k0, k)
            err = float(np.max(np.abs(got - orc[k][k0:k0 + nk])))
            assert err <= FAST_RTOL * np.max(np.abs(orc[k])), (world, k0, k, err)
