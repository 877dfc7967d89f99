"""The Fortran host side with -ksp_norm_type: the reference's options path (src/poissbox.f90:295
KSPSetFromOptions) reaches the option through the iso_c_binding module -- `solve` parses it beside
pb_ksp_opts and sets it on a KSP of its own -- and the module's set / get calls
(≙ KSPSetNormType / KSPGetNormType) work from a Fortran program."""
import os
import re
import subprocess

import pytest

from test_fortran import DEMO, FDIR, FLANG, REPO

SETGET = """
program norm_type_calls
  use iso_c_binding
  use poissbox_gpu
  implicit none
  integer :: ierr
  integer(c_int) :: rc, nset, neff
  type(tDM) :: da
  type(tMat) :: P, A
  type(tVec) :: x, b
  type(mat_ctx) :: ctx
  type(pb_ksp_opts) :: o
  type(c_ptr) :: ksp
  call PoissboxInitialize(0, ierr)
  if (ierr /= 0) stop 1
  call initialise_grid([16, 16, 12], da, ierr)
  ctx%da = da
  ctx%grid_deltas = [1.0_pb_dp / 16, 1.0_pb_dp / 16, 1.0_pb_dp / 12]
  call initialise_linear_system(da, ctx, P, A, x, b, ierr)
  if (ierr /= 0) stop 1
  rc = c_pb_ksp_opts_default(o)
  o%ksp_type = 2  ! richardson
  rc = c_pb_ksp_create(A%h, P%h, o, ksp)
  if (rc /= 0) stop 2
  rc = c_pb_ksp_get_norm_type(ksp, nset, neff)
  print *, "created:", rc, nset, neff
  rc = c_pb_ksp_set_norm_type(ksp, PB_KSP_NORM_UNPRECONDITIONED)
  print *, "set unpreconditioned:", rc
  rc = c_pb_ksp_get_norm_type(ksp, nset, neff)
  print *, "now:", rc, nset, neff
  rc = c_pb_ksp_set_norm_type(ksp, PB_KSP_NORM_NATURAL)
  print *, "set natural on richardson:", rc
  rc = c_pb_ksp_set_norm_type(ksp, 7_c_int)
  print *, "set 7:", rc
  rc = c_pb_ksp_get_norm_type(ksp, nset, neff)
  print *, "still:", rc, nset, neff
  rc = c_pb_ksp_set_norm_type(ksp, PB_KSP_NORM_NONE)
  rc = c_pb_ksp_get_norm_type(ksp, nset, neff)
  print *, "none:", rc, nset, neff
  rc = c_pb_ksp_destroy(ksp)
  call PoissboxFinalize(ierr)
end program norm_type_calls
"""


def _built():
    if not os.path.exists(DEMO):
        if not os.path.exists(FLANG):
            pytest.skip("no Fortran demo and no flang in this image")
        subprocess.run(["make", "-s", "-C", FDIR], check=True)


def _demo(args):
    _built()
    out = subprocess.run([DEMO, "-n", "64", "-ksp_converged_reason"] + args, capture_output=True,
                         text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout


@pytest.mark.gpu
def test_fortran_demo_unpreconditioned_mg():
    """The solve wrapper's option list carries -ksp_norm_type unpreconditioned: the restatement's
    stopping iteration, and the norm it returns is the true residual the demo prints."""
    from norm_type_restatement import Problem, cg, ttol_margin_ok
    txt = _demo(["-ksp_type", "cg", "-pc_type", "mg", "-ksp_rtol", "1e-6", "-ksp_norm_type",
                 "unpreconditioned"])
    prob = Problem((64, 64, 64), pc="mg")
    _, reason, its, hist, rn0 = cg(prob, prob.rhs(), norm_type="unpreconditioned", rtol=1e-6)
    assert ttol_margin_ok(hist, 1e-6, rn0), "seed too close to ttol"
    m = re.search(r"converged due to CONVERGED_RTOL iterations (\d+)", txt)
    assert reason == 2 and m and int(m.group(1)) == its, txt[-2000:]
    rnorm = float(re.search(r"\|\|z\|\|:\s+(\S+)", txt).group(1))
    true = float(re.search(r"Solution residual \(L2 norm\):\s+(\S+)", txt).group(1))
    assert abs(rnorm - hist[-1]) <= 5e-11 * hist[-1] + 1e-6 * rnorm  # (printed digits)
    assert abs(rnorm - true) <= 1e-3 * rnorm and rnorm <= 1e-6 * rn0
    # and the same list without the option stops on ||z||: another number
    txt = _demo(["-ksp_type", "cg", "-pc_type", "mg", "-ksp_rtol", "1e-6"])
    rz = float(re.search(r"\|\|z\|\|:\s+(\S+)", txt).group(1))
    assert abs(rz - rnorm) > 0.1 * rnorm


@pytest.mark.gpu
def test_fortran_demo_none_and_errors():
    txt = _demo(["-ksp_type", "richardson", "-pc_type", "mg", "-ksp_max_it", "4", "-ksp_norm_type",
                 "none"])
    assert re.search(r"converged due to CONVERGED_ITS iterations 4", txt), txt[-2000:]
    _built()
    for args in (["-ksp_norm_type", "frobenius"],
                 ["-ksp_type", "chebyshev", "-ksp_norm_type", "natural"]):
        out = subprocess.run([DEMO, "-n", "16"] + args, capture_output=True, text=True, timeout=300)
        assert out.returncode != 0 and "failed" in out.stdout and "norm" in out.stdout, out.stdout[-800:]


@pytest.mark.gpu
@pytest.mark.skipif(not os.path.exists(FLANG), reason="flang not in this image")
def test_fortran_module_set_get(tmp_path):
    _built()
    (tmp_path / "norm_type_calls.f90").write_text(SETGET)
    build = os.path.join(FDIR, "build")
    lib = os.path.join(REPO, "poissbox_amd")
    out = subprocess.run([FLANG, "-O1", "-I", build, "-o", "norm_type_calls", "norm_type_calls.f90",
                          os.path.join(build, "libpoissbox_f.a"), f"-L{lib}", "-lpoissbox_gpu",
                          f"-Wl,-rpath,{lib}", "-Wl,-rpath,/opt/rocm/lib"], cwd=tmp_path,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    run = subprocess.run([str(tmp_path / "norm_type_calls")], capture_output=True, text=True,
                         timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    nums = {k: [int(v) for v in vals.split()] for k, vals in
            re.findall(r"^\s*([a-z 7]+):((?:\s+-?\d+)+)\s*$", run.stdout, re.M)}
    assert nums["created"] == [0, -1, 1], run.stdout
    assert nums["set unpreconditioned"] == [0] and nums["now"] == [0, 2, 2]
    assert nums["set natural on richardson"] == [5] and nums["set 7"] == [1]
    assert nums["still"] == [0, 2, 2] and nums["none"] == [0, 0, 0]
