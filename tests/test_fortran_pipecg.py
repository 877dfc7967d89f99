"""The Fortran host side with -ksp_type pipecg: the reference's options path
(src/poissbox.f90:295 KSPSetFromOptions) reaches the pipelined CG solve through the iso_c_binding
module -- the type has no options of its own, the name alone routes it."""
import re

import pytest

from test_fortran_fgmres import _demo


def _restated(pc, rtol):
    import pipecg_cases as F
    from ksp_types_restatement import Problem, ttol_margin_ok
    from pipecg_restatement import pipecg
    prob = Problem((32, 32, 32), pc=pc)
    _, reason, its, hist, rn0 = pipecg(prob, prob.rhs(), rtol=rtol)
    # (the same solves as the cases tol-jacobi / tol-mg, whose margin is the case's own bar)
    assert ttol_margin_ok(hist, rtol, rn0) and F.stop_margin_ok("tol-" + pc)
    return reason, its


@pytest.mark.gpu
@pytest.mark.parametrize("pc,rtol", [("jacobi", 1e-8), ("mg", 1e-10)])
def test_fortran_demo_pipecg(pc, rtol):
    txt = _demo(["-ksp_type", "pipecg", "-pc_type", pc, "-ksp_rtol", repr(rtol)]).stdout
    reason, its = _restated(pc, rtol)
    m = re.search(r"converged due to CONVERGED_RTOL iterations (\d+)", txt)
    assert reason == 2 and m and int(m.group(1)) == its, txt[-2000:]


@pytest.mark.gpu
def test_fortran_demo_pipecg_unsupported_combination():
    out = _demo(["-ksp_type", "pipecg", "-ksp_guess_type", "fischer"], check=False)
    assert out.returncode != 0 and "failed" in out.stdout, out.stdout[-800:]
    # the library's own message (list-directed output wraps it: compare without white space)
    assert "-ksp_guess_typefischerwith-ksp_typepipecg" in re.sub(r"\s+", "", out.stdout)
