"""CPU tier of the factorised compact grad / div / interp: the built library exports the three entry
points, the ctypes signatures mirror the header's declarations, and the ABI version is unchanged
(the change is additive). Without the feature the names do not exist."""
import ctypes as C
import os
import re

import pytest

from poissbox_amd import _lib as L

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("pb_compact_grad_fast", "pb_compact_div_fast", "pb_compact_interp_fast")
# the bit-exact call each one mirrors in arguments
MIRRORS = {"pb_compact_grad_fast": "pb_compact_grad", "pb_compact_div_fast": "pb_compact_div",
           "pb_compact_interp_fast": "pb_compact_interp"}


def _ctype(param):
    """ctypes type of one C parameter declaration of include/poissbox_gpu.h"""
    p = " ".join(param.replace("const", " ").split())
    if re.fullmatch(r"pb_grid ?\* ?\w+", p) or re.fullmatch(r"pb_vec ?\* ?\w+", p):
        return L.c_p
    if re.fullmatch(r"double \w+\[3\]", p):
        return L.P_d
    if re.fullmatch(r"pb_vec ?\* ?\w+\[3\]", p):
        return C.POINTER(L.c_p)
    if re.fullmatch(r"int \w+", p):
        return C.c_int
    raise AssertionError(f"unexpected parameter {param!r}")


def _declared(name):
    header = open(os.path.join(REPO, "include", "poissbox_gpu.h")).read()
    m = re.search(r"^int " + name + r"\((.*?)\);", header, re.S | re.M)
    assert m, f"{name} is not declared in the header"
    return [_ctype(a) for a in m.group(1).split(",")]


@pytest.mark.parametrize("name", NAMES)
def test_library_exports_the_symbol(name):
    lib = C.CDLL(L.LIB_PATH)
    assert getattr(lib, name) is not None
    assert name in L.EXPORTED


@pytest.mark.parametrize("name", NAMES)
def test_ctypes_signature_matches_the_header(name):
    assert L._SIGS[name] == _declared(name)
    assert L._SIGS[name] == L._SIGS[MIRRORS[name]] == _declared(MIRRORS[name])


def test_python_wrappers_exist():
    import poissbox_amd as pb
    for fn in ("compact_grad_fast", "compact_div_fast", "compact_interp_fast"):
        assert callable(getattr(pb, fn))


def test_version_is_unchanged():
    major, minor = C.c_int(), C.c_int()
    L.call("pb_version", C.byref(major), C.byref(minor))
    assert (major.value, minor.value) == (0, 2)
