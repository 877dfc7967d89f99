"""Record what pb_compact_lapl_fast and pb_pcr_alpha_batched compute, bit for bit, so that a later
change can be checked against the commit this ran on (tests/test_gpu_compact_ops_fast.py,
test_existing_paths_unchanged, compares a fresh run with the file by np.array_equal).

Two random fields (oracle fill_random): 64^3 and 128x64x192. For each: the fast Laplacian, the
batched (3/10, 1, 3/10) solve along x (contiguous lines) and along z (interleaved lines). The
outputs are 2 to 12 MiB each, so the file keeps of every output its blake2b digest (as bytes) and
every STRIDE-th value (the places a digest mismatch can be looked at).

usage (on the commit to record, with a GPU): python scripts/record_compact_unchanged.py [OUT.npz]
default OUT: tests/golden/compact_unchanged.npz"""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
import poissbox_amd as pb  # noqa: E402
from oracle import oracle as O  # noqa: E402

SHAPES = [(64, 64, 64), (128, 64, 192)]
SEED = 4242
STRIDE = 257
ALPHA = 3.0 / 10.0


def digest(a):
    return np.frombuffer(hashlib.blake2b(np.ascontiguousarray(a).tobytes()).digest(), dtype=np.uint8)


def outputs(ctx, n3):
    """name -> full output array, for one shape"""
    nx, ny, nz = n3
    N = nx * ny * nz
    f = O.fill_random(N, SEED + N)
    h3 = tuple(2 * np.pi / m for m in n3)
    da = pb.DA(ctx, n3)
    fv, out = pb.Vec(da), pb.Vec(da)
    fv.set_values(f)
    pb.compact_lapl_fast(da, h3, fv, out)
    res = {"lapl_fast": out.get_values()}
    for name, (n, nb, ls, es) in (("pcr_x", (nx, ny * nz, nx, 1)), ("pcr_z", (nz, nx * ny, 1, nx * ny))):
        out.set_values(f)
        p, _ = out.device_ptr()
        pb.pcr_alpha_batched(ctx, n, nb, ls, es, ALPHA, C.c_void_p(p))
        res[name] = out.get_values()
    for v in (fv, out):
        v.destroy()
    da.destroy()
    return res


def record(ctx):
    rec = {}
    for n3 in SHAPES:
        tag = "x".join(str(m) for m in n3)
        for name, a in outputs(ctx, n3).items():
            rec[f"{tag}__{name}__digest"] = digest(a)
            rec[f"{tag}__{name}__sample"] = a[::STRIDE].copy()
    return rec


if __name__ == "__main__":
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden",
                                                             "compact_unchanged.npz")
    ctx = pb.Context(0)
    np.savez_compressed(dst, **record(ctx))
    ctx.destroy()
    print("wrote", dst)
