// pb_options.cpp -- the option structs pb_ksp_opts, pb_ksp_chebyshev_opts and pb_pc_mg_opts: their
// defaults, their range and compatibility rules (the check_* functions, also behind the *_set_opts
// calls, pb_ksp_create and pb_solve*) and their parsers (PETSc options database names,
// src/poissbox.f90:295 KSPSetFromOptions).
//
// A parser works on a copy of the caller's struct: it converts a token, stores it in the copy and
// runs the struct's check; the copy is committed only when the whole line gave PB_OK, so an error
// leaves the caller's struct as it was. Unknown options are skipped, and so is an option that is
// the last token, without its value.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <strings.h>
#include <string>

#include "pb_ksp.hpp"

using namespace pb;

// ---------------------------------------------------------------------------------------------
// Defaults
// ---------------------------------------------------------------------------------------------
// KSPChebyshevEstEigSet's default transform
static const double kEsteigDefault[4] = {0.0, 0.1, 0.0, 1.1};

extern "C" {

int pb_ksp_opts_default(pb_ksp_opts* o) {
  PB_CHECK_ARG(o, "opts is NULL");
  o->rtol = 1e-5;
  o->atol = 1e-50;
  o->dtol = 1e5;
  o->max_it = 10000;
  o->ksp_type = PB_KSP_CG;
  o->pc_type = PB_PC_JACOBI;
  o->nullspace = 1;
  o->monitor = 0;
  o->converged_reason = 0;
  o->check_every = 8;
  o->mg_levels = 0;
  o->mg_coarse_its = 8;
  o->sor_omega = 1.0;
  o->cg_single_reduction = 0;
  o->initial_guess_nonzero = 0;
  o->converged_use_initial_residual_norm = 0;
  o->converged_use_min_initial_residual_norm = 0;
  o->guess_type = PB_GUESS_NONE;
  o->guess_fischer_model = 1;  // PETSc's -ksp_guess_fischer_model default "1,10"
  o->guess_fischer_maxl = 10;
  o->richardson_scale = 1.0;  // KSPRichardsonSetScale's default
  return PB_OK;
}

int pb_ksp_chebyshev_opts_default(pb_ksp_chebyshev_opts* o) {
  PB_CHECK_ARG(o, "opts is NULL");
  o->emin = 0.0;  // 0, 0: estimate
  o->emax = 0.0;
  for (int i = 0; i < 4; ++i) o->esteig[i] = kEsteigDefault[i];
  o->esteig_steps = 10;
  return PB_OK;
}

int pb_pc_mg_opts_default(pb_pc_mg_opts* o) {
  PB_CHECK_ARG(o, "opts is NULL");
  o->levels_ksp_type = PB_MG_LEVELS_RICHARDSON;
  o->levels_pc_type = PB_MG_LEVELS_SOR;
  o->levels_ksp_max_it = 1;
  o->levels_richardson_scale = 1.0;
  o->levels_eigenvalues[0] = o->levels_eigenvalues[1] = 0.0;  // 0, 0: the transform of (0, 2)
  for (int i = 0; i < 4; ++i) o->levels_esteig[i] = kEsteigDefault[i];
  return PB_OK;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Checks: every range and compatibility rule, once
// ---------------------------------------------------------------------------------------------
// Chebyshev's interval: finite, non-zero, of one sign (negative pairs are legal, as in PETSc: A is
// negative semi-definite, so M^-1 A is negative without a PC), emax > emin
int pb::check_cheb_pair(double emin, double emax, const char* what) {
  if (!std::isfinite(emin) || !std::isfinite(emax) || emin == 0.0 || emax == 0.0 ||
      (emin < 0.0) != (emax < 0.0) || !(emax > emin))
    return set_error(PB_ERR_ARG,
                     "%s: emin %g, emax %g are no finite, non-zero bounds of one sign with "
                     "emax > emin", what, emin, emax);
  return PB_OK;
}

int pb::check_cheb_opts(const pb_ksp_chebyshev_opts* o) {
  if (o->emin != 0.0 || o->emax != 0.0)
    PB_TRY(check_cheb_pair(o->emin, o->emax, "-ksp_chebyshev_eigenvalues"));
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(o->esteig[i]))
      return set_error(PB_ERR_ARG, "-ksp_chebyshev_esteig: weight %d, %g, is not finite", i,
                       o->esteig[i]);
  if (o->esteig_steps < 1 || o->esteig_steps > 64)
    return set_error(PB_ERR_ARG, "-ksp_chebyshev_esteig_steps %d outside 1..64", o->esteig_steps);
  return PB_OK;
}

// the level smoother's Chebyshev interval: D^-1 A is positive semi-definite
static int check_mg_pair(double emin, double emax, const char* what) {
  if (!std::isfinite(emin) || !std::isfinite(emax) || !(emin > 0.0) || !(emax > emin))
    return set_error(PB_ERR_ARG, "%s: emin %g, emax %g are no finite bounds with 0 < emin < emax",
                     what, emin, emax);
  return PB_OK;
}

void pb::mg_levels_bounds(const pb_pc_mg_opts* o, double* emin, double* emax) {
  if (o->levels_eigenvalues[0] != 0.0 || o->levels_eigenvalues[1] != 0.0) {
    *emin = o->levels_eigenvalues[0];
    *emax = o->levels_eigenvalues[1];
    return;
  }
  const double lo = 0.0, hi = 2.0;
  *emin = o->levels_esteig[0] * lo + o->levels_esteig[1] * hi;
  *emax = o->levels_esteig[2] * lo + o->levels_esteig[3] * hi;
}

// the rules of pb_pc_mg_opts that concern one field each (the parser runs them after every token:
// the first bad option of a line is the one reported)
static int check_mg_fields(const pb_pc_mg_opts* o) {
  const int kt = o->levels_ksp_type, pt = o->levels_pc_type;
  if (kt != PB_MG_LEVELS_RICHARDSON && kt != PB_MG_LEVELS_CHEBYSHEV)
    return set_error(PB_ERR_ARG, "unknown mg levels_ksp_type %d", kt);
  if (pt != PB_MG_LEVELS_SOR && pt != PB_MG_LEVELS_JACOBI)
    return set_error(PB_ERR_ARG, "unknown mg levels_pc_type %d", pt);
  if (o->levels_ksp_max_it < 1 || o->levels_ksp_max_it > 8)
    return set_error(PB_ERR_ARG, "-mg_levels_ksp_max_it %d outside 1..8", o->levels_ksp_max_it);
  if (!std::isfinite(o->levels_richardson_scale) || !(o->levels_richardson_scale > 0.0))
    return set_error(PB_ERR_ARG, "-mg_levels_ksp_richardson_scale %g is not finite and > 0",
                     o->levels_richardson_scale);
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(o->levels_esteig[i]))
      return set_error(PB_ERR_ARG, "-mg_levels_ksp_chebyshev_esteig: weight %d, %g, is not finite",
                       i, o->levels_esteig[i]);
  if (o->levels_eigenvalues[0] != 0.0 || o->levels_eigenvalues[1] != 0.0)
    PB_TRY(check_mg_pair(o->levels_eigenvalues[0], o->levels_eigenvalues[1],
                         "-mg_levels_ksp_chebyshev_eigenvalues"));
  return PB_OK;
}

int pb::check_mg_opts(const pb_pc_mg_opts* o) {
  PB_TRY(check_mg_fields(o));
  const int kt = o->levels_ksp_type, pt = o->levels_pc_type;
  if (kt == PB_MG_LEVELS_CHEBYSHEV) {
    if (pt == PB_MG_LEVELS_SOR)
      return set_error(PB_ERR_UNSUPPORTED,
                       "-mg_levels_ksp_type chebyshev with -mg_levels_pc_type sor: the polynomial "
                       "smoother runs over jacobi only");
    double emin, emax;
    mg_levels_bounds(o, &emin, &emax);
    PB_TRY(check_mg_pair(emin, emax, "-mg_levels_ksp_chebyshev_esteig transform of (0, 2)"));
  }
  if (pt == PB_MG_LEVELS_SOR && o->levels_richardson_scale != 1.0)
    return set_error(PB_ERR_UNSUPPORTED,
                     "-mg_levels_ksp_richardson_scale %g with -mg_levels_pc_type sor: only 1 "
                     "(the relaxation factor is -pc_sor_omega)", o->levels_richardson_scale);
  return PB_OK;
}

int pb::check_guess_opts(int model, int maxl) {
  if (model == 2 || model == 3)
    return set_error(PB_ERR_UNSUPPORTED, "-ksp_guess_fischer_model %d: only model 1", model);
  if (model != 1) return set_error(PB_ERR_ARG, "-ksp_guess_fischer_model %d: no such model", model);
  if (maxl < 1 || maxl > kMaxVecs)
    return set_error(PB_ERR_ARG, "-ksp_guess_fischer_model: maxl %d outside 1..%d", maxl, kMaxVecs);
  return PB_OK;
}

// KSPConvergedDefaultSetUIRNorm / SetUMIRNorm exclude each other (PETSc errors on the second)
int pb::check_ref_norm_opts(const pb_ksp_opts* o) {
  if (o->converged_use_initial_residual_norm && o->converged_use_min_initial_residual_norm)
    return set_error(PB_ERR_ARG,
                     "-ksp_converged_use_initial_residual_norm and "
                     "-ksp_converged_use_min_initial_residual_norm exclude each other");
  return PB_OK;
}

int pb::check_richardson_scale(double scale) {
  if (!std::isfinite(scale))
    return set_error(PB_ERR_ARG, "-ksp_richardson_scale %g is not finite", scale);
  return PB_OK;
}

// ---------------------------------------------------------------------------------------------
// Token conversion
// ---------------------------------------------------------------------------------------------
// PetscOptionsBool at argv[*i]: a bare flag is true; an explicit value may follow and is consumed
// (PetscOptionsStringToBool: case-insensitive true/yes/on/1 and false/no/off/0)
static void opt_bool(const char* const* argv, int argc, int* i, int* out) {
  const char* v = *i + 1 < argc ? argv[*i + 1] : nullptr;
  *out = 1;
  if (!v) return;
  static const struct {
    const char* word;
    int value;
  } kWords[] = {{"true", 1}, {"yes", 1}, {"on", 1}, {"1", 1},
                {"false", 0}, {"no", 0}, {"off", 0}, {"0", 0}};
  for (const auto& w : kWords)
    if (!strcasecmp(v, w.word)) {
      *out = w.value;
      ++*i;
      return;
    }
}

// exactly n comma-separated finite reals
static int opt_reals(const char* opt, const char* v, int n, double* out) {
  const char* s = v;
  for (int i = 0; i < n; ++i) {
    char* end = nullptr;
    out[i] = strtod(s, &end);
    if (end == s || *end != (i + 1 < n ? ',' : '\0') || !std::isfinite(out[i]))
      return set_error(PB_ERR_ARG, "%s %s: expected %d comma-separated finite numbers", opt, v, n);
    s = end + 1;  // (past the comma: not read after the last number)
  }
  return PB_OK;
}

// an enum-valued option: the names it takes, ended by a nullptr name
struct EnumName {
  const char* name;
  int value;
};
static const EnumName kKspTypes[] = {{"cg", PB_KSP_CG}, {"preonly", PB_KSP_PREONLY},
                                     {"richardson", PB_KSP_RICHARDSON},
                                     {"chebyshev", PB_KSP_CHEBYSHEV},
                                     {"fgmres", PB_KSP_FGMRES}, {"pipecg", PB_KSP_PIPECG},
                                     {nullptr, 0}};
static const EnumName kPcTypes[] = {{"none", PB_PC_NONE}, {"jacobi", PB_PC_JACOBI},
                                    {"sor", PB_PC_SOR}, {"mg", PB_PC_MG}, {"gamg", PB_PC_MG},
                                    {"fft", PB_PC_FFT}, {nullptr, 0}};
static const EnumName kGuessTypes[] = {{"none", PB_GUESS_NONE}, {"fischer", PB_GUESS_FISCHER},
                                       {nullptr, 0}};
static const EnumName kMgKspTypes[] = {{"richardson", PB_MG_LEVELS_RICHARDSON},
                                       {"chebyshev", PB_MG_LEVELS_CHEBYSHEV}, {nullptr, 0}};
static const EnumName kMgPcTypes[] = {{"sor", PB_MG_LEVELS_SOR}, {"jacobi", PB_MG_LEVELS_JACOBI},
                                      {nullptr, 0}};

static int opt_enum(const char* opt, const char* v, const EnumName* table, int* out) {
  std::string names;
  for (const EnumName* t = table; t->name; ++t) {
    if (!strcmp(v, t->name)) {
      *out = t->value;
      return PB_OK;
    }
    names += names.empty() ? "" : ", ";
    names += t->name;
  }
  return set_error(PB_ERR_UNSUPPORTED, "%s %s: only %s", opt, v, names.c_str());
}

// ---------------------------------------------------------------------------------------------
// Parsers
// ---------------------------------------------------------------------------------------------
extern "C" {

int pb_pc_mg_opts_parse(pb_pc_mg_opts* o, int argc, const char* const* argv) {
  PB_CHECK_ARG(o, "opts is NULL");
  pb_pc_mg_opts t = *o;
  for (int i = 0; i < argc; ++i) {
    const char* a = argv[i];
    const char* v = i + 1 < argc ? argv[i + 1] : nullptr;
    if (!a || strncmp(a, "-mg_", 4) || !v) continue;
    if (!strcmp(a, "-mg_levels_ksp_type")) {
      PB_TRY(opt_enum(a, v, kMgKspTypes, &t.levels_ksp_type));
    } else if (!strcmp(a, "-mg_levels_pc_type")) {
      PB_TRY(opt_enum(a, v, kMgPcTypes, &t.levels_pc_type));
    } else if (!strcmp(a, "-mg_levels_ksp_max_it")) {
      t.levels_ksp_max_it = atoi(v);
    } else if (!strcmp(a, "-mg_levels_ksp_richardson_scale")) {
      t.levels_richardson_scale = atof(v);
    } else if (!strcmp(a, "-mg_levels_ksp_chebyshev_eigenvalues")) {
      double e[2];
      PB_TRY(opt_reals(a, v, 2, e));
      PB_TRY(check_mg_pair(e[0], e[1], a));  // (here 0,0 is a pair like any other: not valid)
      t.levels_eigenvalues[0] = e[0];
      t.levels_eigenvalues[1] = e[1];
    } else if (!strcmp(a, "-mg_levels_ksp_chebyshev_esteig")) {
      PB_TRY(opt_reals(a, v, 4, t.levels_esteig));
    } else if (!strcmp(a, "-mg_levels_ksp_rtol") || !strcmp(a, "-mg_coarse_sub_pc_type")) {
      // accepted, no effect: fixed sweep counts, SOR sweeps on the coarsest level
    } else {
      continue;
    }
    ++i;
    PB_TRY(check_mg_fields(&t));
  }
  PB_TRY(check_mg_opts(&t));
  *o = t;
  return PB_OK;
}

int pb_ksp_chebyshev_opts_parse(pb_ksp_chebyshev_opts* o, int argc, const char* const* argv) {
  PB_CHECK_ARG(o, "opts is NULL");
  pb_ksp_chebyshev_opts t = *o;
  for (int i = 0; i < argc; ++i) {
    const char* a = argv[i];
    const char* v = i + 1 < argc ? argv[i + 1] : nullptr;
    if (!a) continue;
    if (!strcmp(a, "-ksp_chebyshev_esteig_noisy")) {
      int noisy = 1;
      opt_bool(argv, argc, &i, &noisy);
      if (!noisy)
        return set_error(PB_ERR_UNSUPPORTED,
                         "-ksp_chebyshev_esteig_noisy %s: the estimate starts from noise", v);
      continue;
    }
    if (!v) continue;
    if (!strcmp(a, "-ksp_chebyshev_eigenvalues")) {
      double e[2];
      PB_TRY(opt_reals(a, v, 2, e));
      PB_TRY(check_cheb_pair(e[0], e[1], a));  // (here 0,0 is a pair like any other: not valid)
      t.emin = e[0];
      t.emax = e[1];
    } else if (!strcmp(a, "-ksp_chebyshev_esteig")) {
      PB_TRY(opt_reals(a, v, 4, t.esteig));
    } else if (!strcmp(a, "-ksp_chebyshev_esteig_steps")) {
      t.esteig_steps = atoi(v);
    } else {
      continue;
    }
    ++i;
    PB_TRY(check_cheb_opts(&t));
  }
  *o = t;
  return PB_OK;
}

int pb_ksp_opts_parse(pb_ksp_opts* o, int argc, const char* const* argv) {
  PB_CHECK_ARG(o, "opts is NULL");
  pb_ksp_opts t = *o;
  for (int i = 0; i < argc; ++i) {
    const char* a = argv[i];
    const char* v = i + 1 < argc ? argv[i + 1] : nullptr;
    if (!a) continue;
    // the flags (none of them is a name of the second chain: they end at its `continue`)
    if (!strcmp(a, "-ksp_richardson_self_scale")) {
      int self_scale = 0;
      opt_bool(argv, argc, &i, &self_scale);
      if (self_scale)
        return set_error(PB_ERR_UNSUPPORTED, "-ksp_richardson_self_scale true: only false");
    } else if (!strcmp(a, "-ksp_cg_single_reduction")) {
      opt_bool(argv, argc, &i, &t.cg_single_reduction);
    } else if (!strcmp(a, "-ksp_initial_guess_nonzero")) {
      opt_bool(argv, argc, &i, &t.initial_guess_nonzero);
    } else if (!strcmp(a, "-ksp_converged_use_initial_residual_norm")) {
      opt_bool(argv, argc, &i, &t.converged_use_initial_residual_norm);
    } else if (!strcmp(a, "-ksp_converged_use_min_initial_residual_norm")) {
      opt_bool(argv, argc, &i, &t.converged_use_min_initial_residual_norm);
    } else if (!strcmp(a, "-ksp_monitor")) {
      t.monitor = 1;
    } else if (!strcmp(a, "-ksp_converged_reason")) {
      t.converged_reason = 1;
    }
    if (!v) continue;
    // the options with a value
    if (!strcmp(a, "-ksp_type")) {
      PB_TRY(opt_enum(a, v, kKspTypes, &t.ksp_type));
    } else if (!strcmp(a, "-pc_type")) {
      PB_TRY(opt_enum(a, v, kPcTypes, &t.pc_type));
    } else if (!strcmp(a, "-ksp_guess_type")) {
      PB_TRY(opt_enum(a, v, kGuessTypes, &t.guess_type));
    } else if (!strcmp(a, "-ksp_richardson_scale")) {
      t.richardson_scale = atof(v);
      PB_TRY(check_richardson_scale(t.richardson_scale));
    } else if (!strcmp(a, "-ksp_rtol")) {
      t.rtol = atof(v);
    } else if (!strcmp(a, "-ksp_atol")) {
      t.atol = atof(v);
    } else if (!strcmp(a, "-ksp_divtol")) {
      t.dtol = atof(v);
    } else if (!strcmp(a, "-ksp_max_it")) {
      t.max_it = atoll(v);
    } else if (!strcmp(a, "-pc_mg_levels")) {
      t.mg_levels = atoi(v);
    } else if (!strcmp(a, "-pc_mg_coarse_its") || !strcmp(a, "-mg_coarse_ksp_max_it")) {
      t.mg_coarse_its = atoi(v);
    } else if (!strcmp(a, "-pc_sor_omega")) {
      t.sor_omega = atof(v);
    } else if (!strcmp(a, "-ksp_guess_fischer_model") && v[0] >= '0' && v[0] <= '9') {
      // <model>[,<maxl>] (PetscOptionsIntArray: a bare model keeps maxl)
      t.guess_fischer_model = atoi(v);
      const char* comma = strchr(v, ',');
      if (comma) t.guess_fischer_maxl = atoi(comma + 1);
      PB_TRY(check_guess_opts(t.guess_fischer_model, t.guess_fischer_maxl));
    } else {
      continue;
    }
    ++i;
  }
  // the -ksp_chebyshev_* options: their errors are reported here too (the values belong to
  // pb_ksp_chebyshev_opts_parse)
  pb_ksp_chebyshev_opts co;
  pb_ksp_chebyshev_opts_default(&co);
  PB_TRY(pb_ksp_chebyshev_opts_parse(&co, argc, argv));
  // likewise the -mg_levels_* options (pb_pc_mg_opts_parse keeps the values)
  pb_pc_mg_opts mo;
  pb_pc_mg_opts_default(&mo);
  PB_TRY(pb_pc_mg_opts_parse(&mo, argc, argv));
  PB_TRY(check_ref_norm_opts(&t));
  *o = t;
  return PB_OK;
}

}  // extern "C"
