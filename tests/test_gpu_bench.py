"""GPU tier: bench.py's plain run (one GPU, no --full) at a small grid -- the result line's
headline fields and --dump-outputs, whose files two runs with the same arguments must write alike."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from parity_bars import check_history, check_x

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir):
    env = {k: v for k, v in os.environ.items()
           if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT")}
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1", "--steps", "6",
           "--warmup", "2", "--base", "48", "--dump-outputs", str(out_dir)]
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=env, cwd=REPO)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_plain_run_line_and_dumped_outputs(tmp_path):
    from oracle import oracle as O
    d = _plain_run(tmp_path / "a")
    assert d["unit"] == "DoF-updates/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    assert d["steps"] == 6 and d["warmup"] == 2 and d["ms_per_step"] > 0
    assert abs(d["value"] - 48 ** 3 / (d["ms_per_step"] * 1e-3)) <= 1e-9 * d["value"]
    assert d["ksp_state"]["its"] == 8          # the timed steps really ran: 2 + 6 iterations
    # a plain run carries nothing that needs a run of its own
    for k in ("kernels", "variants", "cpu_baseline", "secondary", "matvec_star7_sustained"):
        assert k not in d
    assert sorted(os.listdir(tmp_path / "a")) == ["residual_history.npy", "x.npy"]
    hist, x = np.load(tmp_path / "a" / "residual_history.npy"), np.load(tmp_path / "a" / "x.npy")
    assert hist.dtype == np.float64 and hist.shape == (9,)
    assert x.dtype == np.float64 and x.shape == (48 ** 3,)
    # the dumped arrays are the solve's: 8 CG + Jacobi iterations of the oracle on the same system
    n, h = (48, 48, 48), (1 / 48,) * 3
    b = O.stencil(O.fill_random(48 ** 3, 20231015), n, h)
    xo, _, _, ho = O.cg_solve(b, n, h, rtol=0.0, atol=0.0, dtol=1e300, max_it=8)
    check_history(hist, ho)
    check_x(x, xo)
    # the same arguments again: the same inputs, so the same outputs, bit for bit
    _plain_run(tmp_path / "b")
    for f in ("residual_history.npy", "x.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f))
