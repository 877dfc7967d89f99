"""The Fortran demo (src/example.f90's flow) with a -mg_levels_* level smoother: the options reach
the library through the module's solve(), and the run converges in the Python run's iterations."""
import os
import re
import subprocess

import numpy as np
import pytest

import poissbox_amd as pb
from oracle import oracle as O
from mg_smoothers_restatement import MgProblem, Smoother, cg

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FDIR = os.path.join(REPO, "poissbox_amd", "fortran")
DEMO = os.path.join(FDIR, "build", "poissbox_demo")
SMOOTHER = ["-mg_levels_ksp_type", "chebyshev", "-mg_levels_pc_type", "jacobi",
            "-mg_levels_ksp_max_it", "2"]


@pytest.mark.gpu
def test_fortran_demo_with_chebyshev_jacobi_levels(ctx):
    if not os.path.exists(DEMO):
        subprocess.run(["make", "-s", "-C", FDIR], check=True)
    opts = ["-ksp_type", "cg", "-pc_type", "mg", "-ksp_rtol", "1e-8"] + SMOOTHER
    out = subprocess.run([DEMO, "-n", "32"] + opts + ["-ksp_converged_reason"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    m = re.search(r"converged due to CONVERGED_RTOL iterations (\d+)", out.stdout)
    assert m, out.stdout
    # the Python run of the demo's system (src/example.f90:175-195: b = A x_random)
    n, h = (32, 32, 32), (1 / 32,) * 3
    b = O.stencil(O.fill_random(32 ** 3, 20231015), n, h)
    da = pb.DA(ctx, n)
    P, A, x, bv = pb.initialise_linear_system(da, h)
    bv.set_values(b)
    reason, its, _ = pb.solve(P, A, x, bv, opts)
    for o in (P, A, x, bv):
        o.destroy()
    da.destroy()
    assert reason == 2 and int(m.group(1)) == its
    # ... which is the restatement's count, and not the default smoother's
    want = cg(MgProblem(n, h, Smoother("chebyshev", "jacobi", 2)), b, rtol=1e-8)
    assert (want[1], want[2]) == (2, its)
    assert its != O.cg_solve(b, n, h, rtol=1e-8, pc="mg")[2]
