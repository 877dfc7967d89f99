"""The Fortran host side with -ksp_type chebyshev: the reference's options path
(src/poissbox.f90:295 KSPSetFromOptions) reaches the Chebyshev solve through the iso_c_binding
module: solve parses the pb_ksp_chebyshev_opts settings beside pb_ksp_opts."""
import os
import re
import subprocess

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
def test_fortran_demo_chebyshev_mg():
    from chebyshev_restatement import chebyshev
    from ksp_types_restatement import Problem, ttol_margin_ok
    txt = _demo(["-ksp_type", "chebyshev", "-ksp_chebyshev_eigenvalues", "0.1,1.1", "-pc_type",
                 "mg", "-ksp_rtol", "1e-6"])
    prob = Problem((64, 64, 64), pc="mg")
    _, reason, its, hist, rn0 = chebyshev(prob, prob.rhs(), 0.1, 1.1, rtol=1e-6)
    assert ttol_margin_ok(hist, 1e-6, rn0), "seed too close to ttol"
    m = re.search(r"converged due to CONVERGED_RTOL iterations (\d+)", txt)
    assert reason == 2 and m and int(m.group(1)) == its, txt[-2000:]


@pytest.mark.gpu
def test_fortran_demo_chebyshev_estimated_bounds():
    """Without bounds the solve estimates them (10 Lanczos steps with the multigrid PC)."""
    from chebyshev_restatement import chebyshev, estimate
    from ksp_types_restatement import Problem, ttol_margin_ok
    txt = _demo(["-ksp_type", "chebyshev", "-pc_type", "mg", "-ksp_rtol", "1e-6"])
    prob = Problem((64, 64, 64), pc="mg")
    # (the library's estimate agrees with the restated one to 1e-13: tests/test_gpu_chebyshev.py)
    _, reason, its, hist, rn0 = chebyshev(prob, prob.rhs(), *estimate(prob), rtol=1e-6)
    assert ttol_margin_ok(hist, 1e-6, rn0), "seed too close to ttol"
    m = re.search(r"converged due to CONVERGED_RTOL iterations (\d+)", txt)
    assert reason == 2 and m and int(m.group(1)) == its, txt[-2000:]
