"""The Fortran host side with -ksp_type fgmres: the reference's options path
(src/poissbox.f90:295 KSPSetFromOptions) reaches the flexible GMRES solve through the
iso_c_binding module: solve parses the pb_ksp_fgmres_opts settings beside pb_ksp_opts and sets
them on the KSP."""
import os
import re
import subprocess

import pytest

from test_fortran import DEMO, FDIR, FLANG


def _demo(args, check=True):
    if not os.path.exists(DEMO):
        if not os.path.exists(FLANG):
            pytest.skip("no Fortran demo and no flang in this image")
        subprocess.run(["make", "-s", "-C", FDIR], check=True)
    out = subprocess.run([DEMO, "-n", "32", "-ksp_converged_reason"] + args, capture_output=True,
                         text=True, timeout=300)
    if check:
        assert out.returncode == 0, out.stdout + out.stderr
    return out


@pytest.mark.gpu
def test_fortran_demo_fgmres_jacobi_restart():
    """-ksp_gmres_restart reaches the KSP: the count is the restatement's with that restart, and
    not the default restart's."""
    from fgmres_restatement import fgmres
    from ksp_types_restatement import Problem, ttol_margin_ok
    txt = _demo(["-ksp_type", "fgmres", "-pc_type", "jacobi", "-ksp_gmres_restart", "5",
                 "-ksp_rtol", "1e-6"]).stdout
    prob = Problem((32, 32, 32))
    b = prob.rhs()
    _, reason, its, hist, rn0 = fgmres(prob, b, restart=5, rtol=1e-6)
    assert ttol_margin_ok(hist, 1e-6, rn0), "seed too close to ttol"
    m = re.search(r"converged due to CONVERGED_RTOL iterations (\d+)", txt)
    assert reason == 2 and m and int(m.group(1)) == its, txt[-2000:]
    assert its != fgmres(prob, b, restart=30, rtol=1e-6)[2]


@pytest.mark.gpu
def test_fortran_demo_fgmres_mg_and_errors():
    from fgmres_restatement import fgmres
    from ksp_types_restatement import Problem, ttol_margin_ok
    txt = _demo(["-ksp_type", "fgmres", "-pc_type", "mg", "-ksp_rtol", "1e-8"]).stdout
    prob = Problem((32, 32, 32), pc="mg")
    _, reason, its, hist, rn0 = fgmres(prob, prob.rhs(), rtol=1e-8)
    assert ttol_margin_ok(hist, 1e-8, rn0), "seed too close to ttol"
    m = re.search(r"converged due to CONVERGED_RTOL iterations (\d+)", txt)
    assert reason == 2 and m and int(m.group(1)) == its, txt[-2000:]
    for args in (["-ksp_gmres_modifiedgramschmidt"], ["-ksp_gmres_restart", "65"],
                 ["-ksp_norm_type", "preconditioned"]):
        out = _demo(["-ksp_type", "fgmres"] + args, check=False)
        assert out.returncode != 0 and "failed" in out.stdout, out.stdout[-800:]
