"""Record what the fast compact operators and pb_pcr_alpha_batched compute, bit for bit, so that a
later change can be checked against the commit this ran on (tests/test_gpu_compact_ops_fast.py,
test_existing_paths_unchanged, compares a fresh run with the file by np.array_equal).

Two random fields (oracle fill_random): 64^3 and 128x64x192. For each: the fast Laplacian, the
batched (3/10, 1, 3/10) solve along x (contiguous lines) and along z (interleaved lines), at
STRIDE. At these two and at OPS_SHAPES (every host path of the line passes: PCR fallback on every
axis, ragged last tile, 8-byte moves, C = 8 with 8-byte moves, C = 12, and 64*C lines sent to the
PCR builders by compact_lines = 0): the fast grad (three components), div, interp at both staggers
and, where not recorded already, the fast Laplacian, at OPS_STRIDE. The outputs are up to 25 MiB
each, so the file keeps of every output its blake2b digest (as bytes) and every STRIDE-th value
(the places a digest mismatch can be looked at).

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
# (shape, tuning entries, tag suffix)
OPS_SHAPES = [((33, 17, 9), {}, ""),
              ((40, 64, 64), {}, ""),
              ((33, 64, 128), {}, ""),
              ((33, 512, 64), {}, ""),
              ((64, 768, 64), {}, ""),
              ((128, 64, 64), {"compact_lines": 0}, "_lines0")]
OPS_STRIDE = 4099


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


def ops_outputs(ctx, n3, lapl):
    """name -> full output array of the fast grad / div / interp (and Laplacian), for one shape"""
    N = n3[0] * n3[1] * n3[2]
    f = O.fill_random(3 * N, SEED + 3 * N)
    h3 = tuple(2 * np.pi / m for m in n3)
    da = pb.DA(ctx, n3)
    v = [pb.Vec(da) for _ in range(4)]
    res = {}
    v[0].set_values(f[:N])
    pb.compact_grad_fast(da, h3, v[0], v[1:])
    for c in range(3):
        res[f"grad_fast{c + 1}"] = v[1 + c].get_values()
    for stagger, name in ((-1, "interp_fast_m"), (1, "interp_fast_p")):
        pb.compact_interp_fast(da, stagger, v[0], v[1])
        res[name] = v[1].get_values()
    if lapl:
        pb.compact_lapl_fast(da, h3, v[0], v[1])
        res["lapl_fast"] = v[1].get_values()
    for c in range(3):
        v[c].set_values(f[c * N:(c + 1) * N])
    pb.compact_div_fast(da, h3, v[:3], v[3])
    res["div_fast"] = v[3].get_values()
    for u in v:
        u.destroy()
    da.destroy()
    return res


def record(ctx):
    rec = {}

    def keep(tag, res, stride):
        for name, a in res.items():
            rec[f"{tag}__{name}__digest"] = digest(a)
            rec[f"{tag}__{name}__sample"] = a[::stride].copy()

    for n3 in SHAPES:
        keep("x".join(str(m) for m in n3), outputs(ctx, n3), STRIDE)
    for n3, tuning, suffix in [(n3, {}, "") for n3 in SHAPES] + OPS_SHAPES:
        pb.tune_reset()
        for name, value in tuning.items():
            pb.tune_set(name, value)
        try:
            keep("x".join(str(m) for m in n3) + suffix, ops_outputs(ctx, n3, n3 not in SHAPES),
                 OPS_STRIDE)
        finally:
            pb.tune_reset()
    return rec


if __name__ == "__main__":
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden",
                                                             "compact_unchanged.npz")
    ctx = pb.Context(0)
    np.savez_compressed(dst, **record(ctx))
    ctx.destroy()
    print("wrote", dst)
