"""CPU tier: the options of the nonzero initial guess (-ksp_initial_guess_nonzero and PETSc's two
KSPConvergedDefault reference-norm switches) through pb_ksp_opts_parse.

PetscOptionsBool: a bare flag is true, an explicit value may follow (PetscOptionsStringToBool:
case-insensitive true/yes/on/1, false/no/off/0). KSPConvergedDefaultSetUIRNorm and SetUMIRNorm
exclude each other (PETSc errors on the second): both set is PB_ERR_ARG.
"""
import pytest

import poissbox_amd as pb

GUESS = "-ksp_initial_guess_nonzero"
UIR = "-ksp_converged_use_initial_residual_norm"
UMIR = "-ksp_converged_use_min_initial_residual_norm"
FIELDS = {GUESS: "initial_guess_nonzero", UIR: "converged_use_initial_residual_norm",
          UMIR: "converged_use_min_initial_residual_norm"}
SPELLINGS = (("true", 1), ("1", 1), ("yes", 1), ("on", 1), ("True", 1), ("YES", 1), ("ON", 1),
             ("false", 0), ("0", 0), ("no", 0), ("off", 0), ("FALSE", 0), ("No", 0), ("OFF", 0))


def _flags(o):
    return tuple(getattr(o, f) for f in FIELDS.values())


def test_defaults_are_zero():
    assert _flags(pb.ksp_options()) == (0, 0, 0)
    # other options leave them alone
    assert _flags(pb.ksp_options(["-pc_type", "mg", "-ksp_cg_single_reduction"])) == (0, 0, 0)


@pytest.mark.parametrize("opt", list(FIELDS))
def test_bare_flag_is_true(opt):
    o = pb.ksp_options([opt])
    assert getattr(o, FIELDS[opt]) == 1
    assert sum(_flags(o)) == 1
    # a following option is not eaten as the value
    o = pb.ksp_options([opt, "-ksp_rtol", "1e-9"])
    assert getattr(o, FIELDS[opt]) == 1 and o.rtol == 1e-9


@pytest.mark.parametrize("opt", list(FIELDS))
def test_bool_spellings(opt):
    for v, want in SPELLINGS:
        o = pb.ksp_options([opt, v, "-ksp_max_it", "5"])
        assert getattr(o, FIELDS[opt]) == want, (opt, v)
        assert o.max_it == 5, (opt, v)


def test_later_value_wins():
    assert pb.ksp_options([GUESS, GUESS, "false"]).initial_guess_nonzero == 0
    assert pb.ksp_options([GUESS, "false", GUESS]).initial_guess_nonzero == 1


def test_both_reference_norm_switches_rejected():
    with pytest.raises(pb.PbError) as e:
        pb.ksp_options([UIR, UMIR])
    assert e.value.code == 1  # PB_ERR_ARG
    with pytest.raises(pb.PbError):
        pb.ksp_options([GUESS, UMIR, "true", UIR, "yes"])
    # one switched off again is fine
    o = pb.ksp_options([UIR, UMIR, "false"])
    assert _flags(o) == (0, 1, 0)
    o = pb.ksp_options([UIR, "off", UMIR])
    assert _flags(o) == (0, 0, 1)


def test_unknown_options_still_ignored():
    o = pb.ksp_options(["-foo", GUESS, "-ksp_initial_guess", "-bar", "7", UMIR, "-pc_type", "none"])
    assert _flags(o) == (1, 0, 1) and o.pc_type == pb.PC_NONE
    assert _flags(pb.ksp_options(["-ksp_initial_guess_nonzeros", "-ksp_converged_use"])) == (0, 0, 0)


def test_keyword_form_sets_the_fields():
    o = pb.ksp_options(["-ksp_rtol", "1e-7"], initial_guess_nonzero=1,
                       converged_use_min_initial_residual_norm=1)
    assert _flags(o) == (1, 0, 1) and o.rtol == 1e-7
