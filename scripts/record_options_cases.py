"""Record tests/golden/options_cases.json: what the three option parsers (pb_ksp_opts_parse,
pb_ksp_chebyshev_opts_parse, pb_pc_mg_opts_parse) return for a list of argv lines. Host code only:
no GPU is needed. Run it on the commit whose behaviour is to be pinned (PB_LIB selects another
build of the library); tests/test_options_recorded.py then holds every later commit to it.

For each line and parser, starting from that parser's defaults: the return code; for 0 every field
of the resulting struct; else whether the struct was left as it was given ("unchanged").

usage: python scripts/record_options_cases.py [OUT.json]"""
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
from poissbox_amd import _lib as L  # noqa: E402

PARSERS = {"ksp": ("pb_ksp_opts", L.KspOpts), "chebyshev": ("pb_ksp_chebyshev_opts", L.KspChebyshevOpts),
           "mg": ("pb_pc_mg_opts", L.PcMgOpts)}
TRUE = ["true", "1", "yes", "True", "on", "YES"]    # the spellings of tests/test_abi.py
FALSE = ["false", "0", "no", "FALSE", "OFF", "No"]
JAC = ["-mg_levels_pc_type", "jacobi"]
CHEB_JAC = ["-mg_levels_ksp_type", "chebyshev"] + JAC
LISTS2 = ["1", "1,2,3", "1,2,", "1,x", "x", "1,inf", "nan,2", "2,1", "1,1", "-1,2", "0,0", ""]
LISTS4 = ["0,0.1,0", "0,0.1,0,1.1,2", "0,0.1,0,1.1,", "0,a,0,1", "0,inf,0,1", "0,nan,0,1", ""]


def lines():
    out = [
        [],
        # the README's solver line (tests/test_mg_smoothers_cpu.py) and the suite's other lines
        ["-ksp_type", "cg", "-pc_type", "gamg", "-mg_coarse_sub_pc_type", "svd",
         "-mg_levels_ksp_rtol", "1.0e-4", "-mg_levels_ksp_type", "richardson",
         "-mg_levels_pc_type", "sor"],
        ["-pc_type", "mg", "-mg_levels_ksp_type", "chebyshev", "-mg_levels_pc_type", "jacobi",
         "-mg_levels_ksp_max_it", "3", "-mg_levels_ksp_chebyshev_eigenvalues", "0.25,2.5",
         "-mg_levels_ksp_chebyshev_esteig", "0,0.2,0,1.05", "-mg_levels_ksp_rtol", "1e-4",
         "-mg_coarse_sub_pc_type", "svd", "-ksp_rtol", "1e-9"],
        ["-ksp_type", "cg", "-pc_type", "none", "-ksp_rtol", "1e-10", "-ksp_atol", "1e-30",
         "-ksp_divtol", "1e9", "-ksp_max_it", "77", "-ksp_monitor", "-ksp_converged_reason", "-foo"],
        ["-pc_type", "mg", "-pc_mg_levels", "5", "-pc_mg_coarse_its", "3", "-pc_sor_omega", "1.3"],
        ["-pc_type", "gamg", "-mg_coarse_ksp_max_it", "2", "-ksp_converged_reason"],
        ["-ksp_rtol", "1e-3", "-ksp_rtol", "1e-4"],
        ["-ksp_rtol", "-ksp_monitor"],
        ["-ksp_rtol", "abc", "-ksp_max_it", "3.7", "-pc_mg_levels", "x"],
        ["x" * 4096, "-pc_type", "sor"],
        ["-ksp_initial_guess_nonzero", "-ksp_converged_use_initial_residual_norm"],
        ["-ksp_initial_guess_nonzero", "true", "-ksp_converged_use_min_initial_residual_norm"],
        ["-ksp_converged_use_initial_residual_norm", "-ksp_converged_use_min_initial_residual_norm"],
        ["-ksp_converged_use_initial_residual_norm", "-ksp_converged_use_min_initial_residual_norm",
         "false"],
        ["-ksp_cg_single_reduction"],
        ["-ksp_cg_single_reduction", "maybe", "-ksp_max_it", "5"],
        ["-ksp_cg_single_reduction", "-ksp_rtol", "1e-9"],
        ["-ksp_richardson_self_scale"],
        ["-ksp_chebyshev_esteig_noisy"],
        ["-ksp_type", "richardson", "-ksp_richardson_scale", "0.75"],
        ["-ksp_type", "richardson", "-ksp_richardson_scale", "-1.5", "-pc_type", "fft"],
        ["-ksp_richardson_scale", "inf"],
        ["-ksp_richardson_scale", "nan"],
        ["-ksp_type", "chebyshev", "-ksp_chebyshev_eigenvalues", "0.1,1.1", "-ksp_chebyshev_esteig",
         "0,0.2,0,1.05", "-ksp_chebyshev_esteig_steps", "9"],
        ["-ksp_chebyshev_eigenvalues", "-2,-0.5"],
        ["-ksp_chebyshev_eigenvalues", " 0.5 , 1.5"],
        ["-ksp_guess_type", "fischer"],
        ["-ksp_guess_type", "none"],
        ["-ksp_guess_type", "fischer", "-ksp_guess_fischer_model", "1,5", "-ksp_guess_fischer_model",
         "1"],
        ["-ksp_guess_fischer_model", "1,0"],
        ["-ksp_guess_fischer_model", "3"],
        ["-ksp_guess_fischer_model", "1,"],
        JAC + ["-mg_levels_ksp_richardson_scale", "0.75", "-mg_levels_ksp_max_it", "8"],
        CHEB_JAC,
        CHEB_JAC + ["-mg_levels_ksp_chebyshev_esteig", "0,0,0,1"],
        CHEB_JAC + ["-mg_levels_ksp_chebyshev_esteig", "0,0.25,0.5,1.0"],
        ["-mg_levels_ksp_type", "chebyshev", "-mg_levels_pc_type", "sor"],
        ["-mg_levels_ksp_type", "chebyshev"],
        ["-mg_levels_ksp_richardson_scale", "0.5"],
        ["-mg_levels_ksp_richardson_scale", "1"],
        ["-mg_unknown", "3", "-mg_levels_ksp_max_it", "2"],
        # which error is reported when a line has several
        ["-mg_levels_ksp_max_it", "0", "-mg_levels_ksp_type", "gmres"],
        ["-mg_levels_ksp_type", "chebyshev", "-mg_levels_ksp_max_it", "0"],
        ["-ksp_chebyshev_esteig_steps", "0", "-mg_levels_pc_type", "ilu", "-ksp_type", "gmres"],
        ["-ksp_chebyshev_esteig_steps", "0", "-mg_levels_pc_type", "ilu"],
        ["-ksp_converged_use_initial_residual_norm", "-ksp_converged_use_min_initial_residual_norm",
         "-mg_levels_pc_type", "ilu"],
        ["-ksp_chebyshev_esteig_steps", "65", "-ksp_chebyshev_eigenvalues", "x"],
        ["-ksp_type", "richardson", "-pc_type", "ilu"],
    ]
    for opt, vals in (("-ksp_type", ["cg", "preonly", "richardson", "chebyshev", "gmres", "CG", ""]),
                      ("-pc_type", ["none", "jacobi", "sor", "mg", "gamg", "fft", "ilu"]),
                      ("-ksp_guess_type", ["bogus"]),
                      ("-ksp_guess_fischer_model", ["1", "1,5", "2", "4", "1,99", "x", "1,16", "1,17"]),
                      ("-mg_levels_ksp_type", ["richardson", "gmres"]),
                      ("-mg_levels_pc_type", ["sor", "jacobi", "ilu"]),
                      ("-mg_levels_ksp_max_it", ["0", "1", "8", "9", "65", "abc"]),
                      ("-ksp_chebyshev_esteig_steps", ["0", "1", "9", "64", "65", "-3"]),
                      ("-ksp_chebyshev_eigenvalues", LISTS2),
                      ("-mg_levels_ksp_chebyshev_eigenvalues", LISTS2 + ["-2,-0.5"]),
                      ("-ksp_chebyshev_esteig", LISTS4),
                      ("-mg_levels_ksp_chebyshev_esteig", LISTS4)):
        out += [[opt, v] for v in vals]
    for v in ("nan", "inf", "-1", "0"):
        out.append(JAC + ["-mg_levels_ksp_richardson_scale", v])
    for flag in ("-ksp_cg_single_reduction", "-ksp_richardson_self_scale",
                 "-ksp_chebyshev_esteig_noisy"):
        out += [[flag, v, "-ksp_max_it", "5"] for v in TRUE + FALSE]
    # an option as the last token, without its value
    for opt in ("-ksp_type", "-pc_type", "-ksp_rtol", "-ksp_atol", "-ksp_divtol", "-ksp_max_it",
                "-pc_mg_levels", "-pc_mg_coarse_its", "-mg_coarse_ksp_max_it", "-pc_sor_omega",
                "-ksp_richardson_scale", "-ksp_guess_type", "-ksp_guess_fischer_model",
                "-ksp_chebyshev_eigenvalues", "-ksp_chebyshev_esteig", "-ksp_chebyshev_esteig_steps",
                "-mg_levels_ksp_type", "-mg_levels_pc_type", "-mg_levels_ksp_max_it",
                "-mg_levels_ksp_richardson_scale", "-mg_levels_ksp_chebyshev_eigenvalues",
                "-mg_levels_ksp_chebyshev_esteig", "-mg_levels_ksp_rtol", "-mg_coarse_sub_pc_type"):
        out.append(["-pc_type", "sor", opt])
    return out


def fields(st):
    return {name: (list(getattr(st, name)) if hasattr(getattr(st, name), "__len__")
                   else getattr(st, name)) for name, _ in st._fields_}


def run(parser, argv):
    """-> (return code, fields after the call, fields before it)"""
    cname, cls = PARSERS[parser]
    st = cls()
    lib = L.load()
    assert getattr(lib, cname + "_default")(C.byref(st)) == 0
    before = fields(st)
    arr = (C.c_char_p * max(len(argv), 1))(*[a.encode() for a in argv])
    rc = getattr(lib, cname + "_parse")(C.byref(st), len(argv), arr)
    return rc, fields(st), before


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden",
                                                             "options_cases.json")
    cases = []
    for argv in lines():
        case = {"argv": argv}
        for parser in PARSERS:
            rc, after, before = run(parser, argv)
            case[parser] = {"rc": rc, "fields": after} if rc == 0 else \
                {"rc": rc, "unchanged": after == before}
        cases.append(case)
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(c) for c in cases) + "\n]\n")
    print(f"{len(cases)} lines -> {out}")


if __name__ == "__main__":
    main()
