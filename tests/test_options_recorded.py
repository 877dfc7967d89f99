"""CPU tier: the three option parsers against tests/golden/options_cases.json, recorded by
scripts/record_options_cases.py from the library as it was before the parsers moved into
poissbox_amd/csrc/pb_options.cpp. For every recorded argv line and every parser: the return code
is the recorded one; on 0 every field of the struct is the recorded value; on an error the struct
is left as it was given (the defaults).

Fixed defects. The recording marks with "unchanged": false the rejected lines after which the old
parsers had already written into the caller's struct: -ksp_richardson_scale inf / nan (assigned
before its check), and the values of earlier options of a line whose error came later (from a
later option, from the final pb_pc_mg_opts check, or from the chebyshev / mg parsers that
pb_ksp_opts_parse runs last). All of them are held to the new behaviour here: nothing is written.
"""
import json
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "scripts"))
import record_options_cases as R  # noqa: E402

CASES = json.load(open(os.path.join(REPO, "tests", "golden", "options_cases.json")))
SOURCE = os.path.join(REPO, "poissbox_amd", "csrc", "pb_options.cpp")
README_LINE = ["-ksp_type", "cg", "-pc_type", "gamg", "-mg_coarse_sub_pc_type", "svd",
               "-mg_levels_ksp_rtol", "1.0e-4", "-mg_levels_ksp_type", "richardson",
               "-mg_levels_pc_type", "sor"]
# the options whose value (alone or with another option's) a parser can reject
REJECTABLE = {
    "-ksp_type", "-pc_type", "-ksp_guess_type", "-ksp_guess_fischer_model", "-ksp_richardson_scale",
    "-ksp_richardson_self_scale", "-ksp_converged_use_initial_residual_norm",
    "-ksp_converged_use_min_initial_residual_norm", "-ksp_chebyshev_eigenvalues",
    "-ksp_chebyshev_esteig", "-ksp_chebyshev_esteig_steps", "-ksp_chebyshev_esteig_noisy",
    "-mg_levels_ksp_type", "-mg_levels_pc_type", "-mg_levels_ksp_max_it",
    "-mg_levels_ksp_richardson_scale", "-mg_levels_ksp_chebyshev_eigenvalues",
    "-mg_levels_ksp_chebyshev_esteig"}
ARG, UNSUPPORTED = 1, 5


def accepted(case):
    return all(case[p]["rc"] == 0 for p in R.PARSERS)


@pytest.mark.parametrize("parser", list(R.PARSERS))
def test_parsers_match_the_recording(parser):
    for case in CASES:
        want = case[parser]
        rc, after, before = R.run(parser, case["argv"])
        assert rc == want["rc"], (parser, case["argv"], rc, want)
        if rc == 0:
            assert after == want["fields"], (parser, case["argv"])
        else:
            assert after == before, (parser, case["argv"], "an error wrote into the struct")


def test_recording_is_current():
    """The committed fixture holds exactly the lines the recording script would record."""
    assert [c["argv"] for c in CASES] == R.lines()


def test_richardson_scale_defect_is_recorded_and_fixed():
    case = next(c for c in CASES if c["argv"] == ["-ksp_richardson_scale", "inf"])
    assert case["ksp"] == {"rc": ARG, "unchanged": False}
    rc, after, before = R.run("ksp", case["argv"])
    assert rc == ARG and after == before


def test_every_option_is_covered():
    """Every option named in pb_options.cpp occurs in an accepted line, and every option a parser
    can reject in a rejected one."""
    text = open(SOURCE).read()
    options = set(re.findall(r'"(-[a-z][a-z0-9_]*[a-z0-9])"', text))
    assert REJECTABLE <= options and len(options) >= 30, sorted(REJECTABLE - options)
    in_accepted = {a for c in CASES if accepted(c) for a in c["argv"]}
    in_rejected = {a for c in CASES if not accepted(c) for a in c["argv"]}
    assert not options - in_accepted, sorted(options - in_accepted)
    assert not REJECTABLE - in_rejected, sorted(REJECTABLE - in_rejected)
    # an option as the last token, without its value, is skipped
    valued = options - {"-ksp_monitor", "-ksp_converged_reason", "-ksp_cg_single_reduction",
                        "-ksp_initial_guess_nonzero", "-ksp_richardson_self_scale",
                        "-ksp_chebyshev_esteig_noisy", "-ksp_converged_use_initial_residual_norm",
                        "-ksp_converged_use_min_initial_residual_norm"}
    last = {c["argv"][-1] for c in CASES if c["argv"] and accepted(c)}
    assert not valued - last, sorted(valued - last)


def test_required_lines_are_recorded():
    by_argv = {tuple(c["argv"]): c for c in CASES}

    def rcs(*argv):
        c = by_argv[argv]
        return tuple(c[p]["rc"] for p in R.PARSERS)

    assert rcs(*README_LINE) == (0, 0, 0)
    # each enum with an unknown value
    for opt, v in (("-ksp_type", "gmres"), ("-pc_type", "ilu"), ("-ksp_guess_type", "bogus"),
                   ("-mg_levels_ksp_type", "gmres"), ("-mg_levels_pc_type", "ilu")):
        assert rcs(opt, v)[0] == UNSUPPORTED, (opt, v)
    # every bool spelling of tests/test_abi.py, accepted and rejected, and a bare flag at the end
    abi = open(os.path.join(REPO, "tests", "test_abi.py")).read()
    spellings = re.findall(r'\("(\w+)", ([01])\)',
                           re.search(r"for v, want in \((.*?)\):\n", abi, re.S).group(1))
    assert len(spellings) == 12 and {s for s, _ in spellings} == set(R.TRUE + R.FALSE)
    for word, value in spellings:
        c = by_argv[("-ksp_cg_single_reduction", word, "-ksp_max_it", "5")]
        assert c["ksp"]["fields"]["cg_single_reduction"] == int(value)
        assert c["ksp"]["fields"]["max_it"] == 5
        assert rcs("-ksp_richardson_self_scale", word, "-ksp_max_it", "5")[0] == \
            (UNSUPPORTED if value == "1" else 0)
        assert rcs("-ksp_chebyshev_esteig_noisy", word, "-ksp_max_it", "5")[1] == \
            (0 if value == "1" else UNSUPPORTED)
    assert rcs("-ksp_richardson_self_scale")[0] == UNSUPPORTED
    assert by_argv[("-ksp_cg_single_reduction",)]["ksp"]["fields"]["cg_single_reduction"] == 1
    # lists: too few, too many, a trailing comma, a non-number, inf, nan
    for opt, p, bad in (("-ksp_chebyshev_eigenvalues", 1, R.LISTS2[:7]),
                        ("-mg_levels_ksp_chebyshev_eigenvalues", 2, R.LISTS2[:7]),
                        ("-ksp_chebyshev_esteig", 1, R.LISTS4[:6]),
                        ("-mg_levels_ksp_chebyshev_esteig", 2, R.LISTS4[:6])):
        for v in bad:
            assert rcs(opt, v)[p] == ARG and rcs(opt, v)[0] == ARG, (opt, v)
    # 0, 9 and 65 against 1..8 and 1..64
    assert [rcs("-mg_levels_ksp_max_it", v)[2] for v in ("0", "1", "8", "9", "65")] == \
        [ARG, 0, 0, ARG, ARG]
    assert [rcs("-ksp_chebyshev_esteig_steps", v)[1] for v in ("0", "1", "9", "64", "65")] == \
        [ARG, 0, 0, 0, ARG]
    # a negative Chebyshev pair is legal, a mixed-sign pair is not
    assert rcs("-ksp_chebyshev_eigenvalues", "-2,-0.5") == (0, 0, 0)
    assert rcs("-ksp_chebyshev_eigenvalues", "-1,2")[:2] == (ARG, ARG)
    # mg: chebyshev over sor, sor with a scale other than 1
    assert rcs("-mg_levels_ksp_type", "chebyshev", "-mg_levels_pc_type", "sor")[2] == UNSUPPORTED
    assert rcs("-mg_levels_ksp_richardson_scale", "0.5")[2] == UNSUPPORTED
    # the Fischer model values
    assert [rcs("-ksp_guess_fischer_model", v)[0] for v in ("1", "1,5", "2", "4", "1,99", "x")] == \
        [0, 0, UNSUPPORTED, ARG, ARG, 0]
    c = by_argv[("-ksp_guess_fischer_model", "1")]["ksp"]["fields"]
    assert (c["guess_fischer_model"], c["guess_fischer_maxl"]) == (1, 10)
    c = by_argv[("-ksp_guess_fischer_model", "1,5")]["ksp"]["fields"]
    assert (c["guess_fischer_model"], c["guess_fischer_maxl"]) == (1, 5)
