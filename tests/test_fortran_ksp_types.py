"""The Fortran host side with -ksp_type preonly -pc_type fft: the reference's options path
(src/poissbox.f90:295 KSPSetFromOptions) reaches the direct solve through the iso_c_binding module,
whose pb_ksp_opts carries the appended richardson_scale field."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_fortran import DEMO, FDIR, FLANG


def _demo(args):
    if not os.path.exists(DEMO):
        if not os.path.exists(FLANG):
            pytest.skip("no Fortran demo and no flang in this image")
        subprocess.run(["make", "-s", "-C", FDIR], check=True)
    out = subprocess.run([DEMO, "-n", "64", "-ksp_converged_reason"] + args, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


@pytest.mark.gpu
def test_fortran_demo_preonly_fft():
    from oracle import oracle as O
    txt = _demo(["-ksp_type", "preonly", "-pc_type", "fft"])
    assert re.search(r"converged due to CONVERGED_ITS iterations 1\b", txt), txt[-2000:]
    n3, h = (64, 64, 64), (1 / 64,) * 3
    b = O.stencil(O.fill_random(64 ** 3, 20231015), n3, h)
    res = float(re.search(r"Solution residual \(L2 norm\):\s+(\S+)", txt).group(1))
    # the direct solve: rounding level (the oracle's own P^+ leaves 5.6e-16 ||b|| at 32x40x48),
    # against 1e-4 ||b|| for the demo's iterative solves in test_fortran.py
    assert res < 1e-12 * np.linalg.norm(b), res


@pytest.mark.gpu
def test_fortran_demo_richardson_mg():
    from ksp_types_restatement import Problem, richardson, ttol_margin_ok
    txt = _demo(["-ksp_type", "richardson", "-pc_type", "mg", "-ksp_rtol", "1e-6"])
    prob = Problem((64, 64, 64), pc="mg")
    _, reason, its, hist, rn0 = richardson(prob, prob.rhs(), rtol=1e-6)
    assert ttol_margin_ok(hist, 1e-6, rn0), "seed too close to ttol"
    m = re.search(r"converged due to CONVERGED_RTOL iterations (\d+)", txt)
    assert reason == 2 and m and int(m.group(1)) == its, txt[-2000:]
