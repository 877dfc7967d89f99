// pb_norm_type.cpp -- -ksp_norm_type (PETSc KSPSetNormType / KSPGetNormType): the option's parser
// and the KSP's setter and getter. The value lives on the KSP object, not in pb_ksp_opts (whose
// layout and parser stay as they are: pb_ksp_opts_parse skips the option as unknown). What the
// types mean on the device is in pb_cg_device.hpp (cg_dp, the CG stages) and
// pb_ksp_stationary.hip (rich_stage); DESIGN.md §3.1g. -ksp_type pipecg takes all four (its default
// is preconditioned): every one comes out of its one reduction (pcg_dp, pb_ksp_pipecg.hip).
#include <cstring>

#include "pb_ksp.hpp"

using namespace pb;

extern "C" {

int pb_ksp_norm_type_parse(int* type, int argc, const char* const* argv) {
  PB_CHECK_ARG(type && (argc == 0 || argv), "bad parse args");
  static const struct {
    const char* word;
    int value;
  } words[] = {{"none", PB_KSP_NORM_NONE},
               {"preconditioned", PB_KSP_NORM_PRECONDITIONED},
               {"unpreconditioned", PB_KSP_NORM_UNPRECONDITIONED},
               {"natural", PB_KSP_NORM_NATURAL},
               {"default", PB_KSP_NORM_DEFAULT}};
  int found = *type;
  for (int i = 0; i + 1 < argc; ++i) {  // (the option as the last token has no value: skipped)
    if (!argv[i] || strcmp(argv[i], "-ksp_norm_type") != 0) continue;
    const char* v = argv[++i];
    bool known = false;
    for (const auto& w : words)
      if (v && strcmp(v, w.word) == 0) {
        found = w.value;
        known = true;
      }
    if (!known)
      return set_error(PB_ERR_UNSUPPORTED, "unknown -ksp_norm_type %s (none, preconditioned, "
                                           "unpreconditioned, natural, default)", v ? v : "(null)");
  }
  *type = found;
  return PB_OK;
}

int pb_ksp_set_norm_type(pb_ksp* k, int type) {
  PB_CHECK_ARG(k, "ksp is NULL");
  PB_CHECK_ARG(type >= PB_KSP_NORM_DEFAULT && type <= PB_KSP_NORM_NATURAL,
               "norm type outside pb_ksp_norm_type");
  if (k->begun) return set_error(PB_ERR_STATE, "pb_ksp_set_norm_type inside a solve");
  const int kt = k->opts.ksp_type;
  if (kt == PB_KSP_PREONLY && type != PB_KSP_NORM_DEFAULT && type != PB_KSP_NORM_NONE)
    return set_error(PB_ERR_UNSUPPORTED, "-ksp_type preonly takes no norm: -ksp_norm_type none");
  if (k->rich() && type == PB_KSP_NORM_NATURAL)
    return set_error(PB_ERR_UNSUPPORTED, "-ksp_type %s does not support the natural norm",
                     k->cheb() ? "chebyshev" : "richardson");
  if (k->fgmres() && (type == PB_KSP_NORM_PRECONDITIONED || type == PB_KSP_NORM_NATURAL))
    return set_error(PB_ERR_UNSUPPORTED, "-ksp_type fgmres is right-preconditioned: "
                                         "-ksp_norm_type unpreconditioned or none");
  k->norm_type = type;
  return PB_OK;
}

int pb_ksp_get_norm_type(const pb_ksp* k, int* set, int* effective) {
  PB_CHECK_ARG(k, "ksp is NULL");
  if (set) *set = k->norm_type;
  if (effective) *effective = k->norm();
  return PB_OK;
}

}  // extern "C"
