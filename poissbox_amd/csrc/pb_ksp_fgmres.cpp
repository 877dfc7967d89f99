// pb_ksp_fgmres.cpp -- the host part of -ksp_type fgmres: restarted flexible
// GMRES, PETSc KSPSolve_FGMRES / KSPFGMRESCycle with classical Gram-Schmidt and right
// preconditioning, kept on the device. Its options (pb_ksp_fgmres_opts: parser, setter, getter,
// pb_solve_fgmres), pb_ksp_begin's setup, one Arnoldi step of pb_ksp_iterate with the restart
// sequence the host enqueues at the cycle's fixed end, and pb_ksp_end's solution build. The
// kernels are in pb_ksp_fgmres.hip; the orthogonalisation is the multi-dot / multi-axpy pair of
// pb_guess.hip with device-side coefficients; the done flags, history and polling are CG's
// (pb_solver.cpp).
#include <cmath>
#include <cstddef>
#include <cstdlib>
#include <cstring>
#include <string>
#include <strings.h>

#include "pb_ksp.hpp"
#include "pb_cg_device.hpp"  // REF_*

using namespace pb;

// basis memory comes in chunks of this many pairs (v_j, z_j)
static constexpr int kFgChunk = 4;

int pb::check_fgmres_opts(const pb_ksp_fgmres_opts* o) {
  if (o->restart < 1 || o->restart > kFgMaxRestart)
    return set_error(PB_ERR_ARG, "-ksp_gmres_restart %d outside 1..%d", o->restart, kFgMaxRestart);
  if (!std::isfinite(o->haptol) || !(o->haptol > 0.0))
    return set_error(PB_ERR_ARG, "-ksp_gmres_haptol %g: must be finite and > 0", o->haptol);
  if (o->cgs_refinement == 1)
    return set_error(PB_ERR_UNSUPPORTED,
                     "-ksp_gmres_cgs_refinement_type refine_ifneeded: only refine_never and "
                     "refine_always");
  if (o->cgs_refinement != PB_FGMRES_REFINE_NEVER && o->cgs_refinement != PB_FGMRES_REFINE_ALWAYS)
    return set_error(PB_ERR_ARG, "cgs_refinement %d is no refinement type", o->cgs_refinement);
  return PB_OK;
}

int pb::fgmres_create(pb_ksp* k) {
  pb_ksp_fgmres_opts_default(&k->fgm.opts);
  if (!k->fgmres()) return PB_OK;
  if (k->opts.guess_type != PB_GUESS_NONE)
    return set_error(PB_ERR_UNSUPPORTED, "-ksp_guess_type fischer with -ksp_type fgmres");
  if (hipMalloc(&k->fgm.d, sizeof(FgState)) != hipSuccess)
    return set_error(PB_ERR_ALLOC, "fgmres state: out of device memory");
  PB_HIP(hipMemsetAsync(k->fgm.d, 0, sizeof(FgState), k->A->grid->ctx->stream));
  k->fgm.v.assign(kFgMaxRestart, nullptr);
  k->fgm.z.assign(kFgMaxRestart, nullptr);
  return PB_OK;
}

void pb::fgmres_destroy(pb_ksp* k) {
  for (double* p : k->fgm.v) field_free(p);
  for (double* p : k->fgm.z) field_free(p);
  if (k->fgm.d) (void)hipFree(k->fgm.d);
}

// v[j], z[j] exist for every j <= upto: a chunk at a time, cleared as they are allocated (the
// build reads live directions only; a cleared vector keeps the ones a done state leaves unformed
// finite for the multi-dots enqueued ahead)
static int fg_reserve(pb_ksp* k, int upto) {
  pb_grid* g = k->A->grid;
  const size_t vb = (size_t)g->nlocal * sizeof(double);
  if (k->fgm.v[upto]) return PB_OK;
  const int end = std::min(k->fgm.opts.restart, (upto / kFgChunk + 1) * kFgChunk);
  for (int j = 0; j < end; ++j) {
    if (k->fgm.v[j]) continue;
    if (field_alloc(&k->fgm.v[j], vb) != hipSuccess || field_alloc(&k->fgm.z[j], vb) != hipSuccess)
      return set_error(PB_ERR_ALLOC, "fgmres basis: vectors %d of 2 x %d: out of device memory",
                       j, k->fgm.opts.restart);
    PB_HIP(hipMemsetAsync(k->fgm.v[j], 0, vb, g->ctx->stream));
    PB_HIP(hipMemsetAsync(k->fgm.z[j], 0, vb, g->ctx->stream));
  }
  return PB_OK;
}

// sum y^2 of a field as it is, left in *d_out (the multi-axpy of no vectors); with_sum: the plain
// sum behind it (FgState::nrm2, wsum)
static int fg_norm2(pb_ctx* ctx, const double* y, int64_t n, double* d_out, bool with_sum) {
  const VecTable none{};
  const MCoef c{};
  return launch_maxpy(ctx, const_cast<double*>(y), nullptr, 0, none, c, n, false, d_out, with_sum);
}
static_assert(offsetof(FgState, wsum) == offsetof(FgState, nrm2) + sizeof(double),
              "the multi-axpy leaves sum w^2 and sum w side by side");

// the 7-point operator on one rank with Jacobi / no PC: a step starts with the engine pass
// (tuning fgmres_fused = 0: the three passes it replaces, bit-identical)
static bool fg_engine(const pb_ksp* k) {
  return fused_kind(k->A->kind) && !k->A->grid->ctx->split && !k->stored_z();
}

// KSPSolve_FGMRES's setup: r_0 = b (x = 0) or b - A x_0 into w, its norm, the reference norm of
// -ksp_norm_type unpreconditioned, history[0] and the first test (the first step forms
// v_0 = r_0 / ||r_0|| from it)
int pb::fgmres_begin(pb_ksp* k, const pb_vec* b, pb_vec* x) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const int64_t n = g->nlocal;
  const size_t vb = (size_t)n * sizeof(double);
  // b is read again at every restart (r = b - A x) while x is written
  PB_CHECK_ARG(b != x, "fgmres needs distinct b and x");
  k->sr.on = false;
  k->pst = false;
  k->lazy0 = false;
  k->defer_x = 0;
  k->b = b;
  k->x = x;
  k->fgm.pos = 0;
  k->fgm.cur = 0;
  PB_TRY(fg_reserve(k, 0));
  double* w = k->pb[0];
  FgState* fs = k->fgm.d;
  int ref = REF_ZERO_GUESS;
  if (!k->opts.initial_guess_nonzero) {
    PB_HIP(hipMemsetAsync(x->d, 0, vb, ctx->stream));
    PB_HIP(hipMemcpyAsync(w, b->d, vb, hipMemcpyDeviceToDevice, ctx->stream));
  } else {
    PB_TRY(check_ref_norm_opts(&k->opts));
    ref = k->ref_norm();
    if (ref != REF_INITIAL && !k->norm_none()) PB_TRY(fg_norm2(ctx, b->d, n, &fs->bsq, false));
    PB_TRY(op_apply_raw(k->A, x->d, k->r));
    PB_TRY(launch_guess_diff(ctx, b->d, k->r, w, n));
  }
  PB_TRY(fg_norm2(ctx, w, n, &fs->nrm2, true));
  return launch_fg_start(ctx, k->log(), fs, 0, ref, k->fgm.opts.restart, k->fgm.opts.haptol, -1);
}

// w -= sum_j <w, v_j> v_j over the nv basis vectors, in groups of at most kMaxVecs: every group's
// dots are of w as it came (classical Gram-Schmidt), the multi-axpys chain; the last leaves
// sum w^2 and sum w. dots: where the nv sums go
static int fg_orthogonalise(pb_ksp* k, double* w, int nv, double* dots) {
  pb_ctx* ctx = k->A->grid->ctx;
  const int64_t n = k->A->grid->nlocal;
  for (int j0 = 0; j0 < nv; j0 += kMaxVecs) {
    const int m = std::min(kMaxVecs, nv - j0);
    VecTable t{};
    for (int j = 0; j < m; ++j) t.p[j] = k->fgm.v[j0 + j];
    PB_TRY(launch_mdot(ctx, w, m, t, n, dots + j0));
  }
  for (int j0 = 0; j0 < nv; j0 += kMaxVecs) {
    const int m = std::min(kMaxVecs, nv - j0);
    VecTable t{};
    for (int j = 0; j < m; ++j) t.p[j] = k->fgm.v[j0 + j];
    MCoef c{};
    c.dev = dots + j0;
    c.sign = -1.0;
    PB_TRY(launch_maxpy(ctx, w, nullptr, m, t, c, n, false,
                        j0 + m == nv ? &k->fgm.d->nrm2 : nullptr, true));
  }
  return PB_OK;
}

// One Arnoldi step at the host's cycle position (the device's while the state is not done; every
// kernel that writes v, z, x or the state exits at entry once it is): v_k = s wt from the
// unnormalised direction the last step (or the cycle's start) left, z_k = N(M^-1 v_k), w = A z_k,
// the orthogonalisation, the scalar part; after the cycle's last step the restart: the solution
// build, r = b - A x, its norm, the next cycle's start
int pb::enqueue_fgmres_iteration(pb_ksp* k) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const int64_t n = g->nlocal;
  const int pos = k->fgm.pos, R = k->fgm.opts.restart;
  FgState* fs = k->fgm.d;
  CgState* st = k->d_st;
  const double* wt = k->pb[k->fgm.cur];
  double* w = k->pb[k->fgm.cur ^ 1];
  k->fgm.cur ^= 1;
  PB_TRY(fg_reserve(k, pos));
  double* v = k->fgm.v[pos];
  double* z = k->fgm.z[pos];
  const bool ns = k->opts.nullspace != 0;
  if (fg_engine(k) && tune("fgmres_fused", 1) != 0) {
    PB_TRY(launch_fg_fused(g, star_of(k->A), wt, v, z, w, fs, st, ns));
  } else {
    PB_TRY(launch_fg_scale(ctx, wt, v, fs, st, n));
    // z_k = N(M^-1 v_k), stored
    if (k->stored_z()) {
      PB_TRY(pc_stored_apply(k, v, z, &st->done));
      if (ns) {
        PB_TRY(launch_fg_zsum(ctx, z, fs, st, n));
        PB_TRY(launch_fg_shift(ctx, z, fs, st, n));
      }
    } else {
      // (Jacobi / none: the shift is in the state already, from the sum of wt)
      PB_TRY(launch_fg_pcshift(ctx, v, z, fs, st, n, ns));
    }
    OpApplySkip guard(ctx, &st->done);
    PB_TRY(op_apply_raw(k->A, z, w));
  }
  const int passes = k->fgm.opts.cgs_refinement == PB_FGMRES_REFINE_ALWAYS ? 2 : 1;
  PB_TRY(fg_orthogonalise(k, w, pos + 1, fs->dots));
  if (passes == 2) PB_TRY(fg_orthogonalise(k, w, pos + 1, fs->dots2));
  PB_TRY(launch_fg_step(ctx, k->log(), fs, passes, k->host_iter));
  if (pos + 1 < R) {
    k->fgm.pos = pos + 1;
    return PB_OK;
  }
  FgTable zt{};
  for (int j = 0; j < R; ++j) zt.p[j] = k->fgm.z[j];
  PB_TRY(launch_fg_trisolve(ctx, st, fs, false));
  PB_TRY(launch_fg_build(ctx, k->x->d, zt, fs, st, false, n));
  {
    OpApplySkip guard(ctx, &st->done);
    PB_TRY(op_apply_raw(k->A, k->x->d, k->r));
  }
  PB_TRY(launch_guess_diff(ctx, k->b->d, k->r, w, n));
  PB_TRY(fg_norm2(ctx, w, n, &fs->nrm2, true));
  k->fgm.pos = 0;
  return launch_fg_start(ctx, k->log(), fs, 1, 0, R, k->fgm.opts.haptol, k->host_iter);
}

// the solution of the cycle the solve ended in (the stream is idle: the state is final). The live
// count is the device's: a cycle that a restart completed, or a solve that ended at its setup,
// has none
int pb::fgmres_finish(pb_ksp* k) {
  pb_ctx* ctx = k->A->grid->ctx;
  FgTable zt{};
  for (int j = 0; j < kFgMaxRestart; ++j) zt.p[j] = k->fgm.z[j];
  PB_TRY(launch_fg_trisolve(ctx, k->d_st, k->fgm.d, true));
  return launch_fg_build(ctx, k->x->d, zt, k->fgm.d, k->d_st, true, k->A->grid->nlocal);
}

// PetscOptionsBool at argv[*i], as pb_options.cpp reads it: a bare flag is true, an explicit
// value may follow and is consumed
static int fg_opt_bool(const char* const* argv, int argc, int* i) {
  const char* v = *i + 1 < argc ? argv[*i + 1] : nullptr;
  if (!v) return 1;
  static const struct {
    const char* word;
    int value;
  } kWords[] = {{"true", 1}, {"yes", 1}, {"on", 1}, {"1", 1},
                {"false", 0}, {"no", 0}, {"off", 0}, {"0", 0}};
  for (const auto& w : kWords)
    if (!strcasecmp(v, w.word)) {
      ++*i;
      return w.value;
    }
  return 1;
}

extern "C" {

int pb_ksp_fgmres_opts_default(pb_ksp_fgmres_opts* o) {
  PB_CHECK_ARG(o, "opts is NULL");
  o->restart = 30;
  o->haptol = 1e-30;
  o->cgs_refinement = PB_FGMRES_REFINE_NEVER;
  return PB_OK;
}

int pb_ksp_fgmres_opts_parse(pb_ksp_fgmres_opts* o, int argc, const char* const* argv) {
  PB_CHECK_ARG(o && (argc == 0 || argv), "bad parse args");
  pb_ksp_fgmres_opts t = *o;
  for (int i = 0; i < argc; ++i) {
    const char* a = argv[i];
    const char* v = i + 1 < argc ? argv[i + 1] : nullptr;
    if (!a || strncmp(a, "-ksp_gmres_", 11)) continue;
    // the flags
    if (!strcmp(a, "-ksp_gmres_classicalgramschmidt") || !strcmp(a, "-ksp_gmres_preallocate")) {
      (void)fg_opt_bool(argv, argc, &i);  // no effect either way
      continue;
    }
    if (!strcmp(a, "-ksp_gmres_modifiedgramschmidt")) {
      if (fg_opt_bool(argv, argc, &i))
        return set_error(PB_ERR_UNSUPPORTED,
                         "-ksp_gmres_modifiedgramschmidt: only classical Gram-Schmidt");
      continue;
    }
    if (!v) continue;
    if (!strcmp(a, "-ksp_gmres_restart")) {
      t.restart = atoi(v);
    } else if (!strcmp(a, "-ksp_gmres_haptol")) {
      char* end = nullptr;
      t.haptol = strtod(v, &end);
      if (end == v || *end) return set_error(PB_ERR_ARG, "-ksp_gmres_haptol %s: not a number", v);
    } else if (!strcmp(a, "-ksp_gmres_cgs_refinement_type")) {
      if (!strcmp(v, "refine_never")) t.cgs_refinement = PB_FGMRES_REFINE_NEVER;
      else if (!strcmp(v, "refine_always")) t.cgs_refinement = PB_FGMRES_REFINE_ALWAYS;
      else if (!strcmp(v, "refine_ifneeded")) t.cgs_refinement = 1;  // (refused by the check)
      else
        return set_error(PB_ERR_UNSUPPORTED, "-ksp_gmres_cgs_refinement_type %s: only "
                                             "refine_never, refine_always", v);
    } else {
      continue;
    }
    ++i;
    PB_TRY(check_fgmres_opts(&t));
  }
  *o = t;
  return PB_OK;
}

int pb_ksp_fgmres_set_opts(pb_ksp* k, const pb_ksp_fgmres_opts* o) {
  PB_CHECK_ARG(k && o, "bad args");
  if (!k->fgmres()) return set_error(PB_ERR_STATE, "KSP created without -ksp_type fgmres");
  if (k->begun) return set_error(PB_ERR_STATE, "pb_ksp_fgmres_set_opts inside a solve");
  PB_TRY(check_fgmres_opts(o));
  k->fgm.opts = *o;
  return PB_OK;
}

int pb_ksp_fgmres_get_opts(const pb_ksp* k, pb_ksp_fgmres_opts* o) {
  PB_CHECK_ARG(k && o, "bad args");
  if (!k->fgmres()) return set_error(PB_ERR_STATE, "KSP created without -ksp_type fgmres");
  *o = k->fgm.opts;
  return PB_OK;
}

int pb_solve_fgmres(pb_op* A, pb_op* P, const pb_ksp_opts* opts, const pb_ksp_fgmres_opts* fg,
                    const pb_vec* b, pb_vec* x, pb_ksp_result* res, double* history, int64_t cap) {
  pb_ksp* k = nullptr;
  PB_TRY(pb_ksp_create(A, P, opts, &k));
  int rc = fg && k->fgmres() ? pb_ksp_fgmres_set_opts(k, fg) : PB_OK;
  if (rc == PB_OK) rc = pb_ksp_solve(k, b, x, res, history, cap);
  const std::string msg = rc != PB_OK ? pb_last_error() : "";
  pb_ksp_destroy(k);
  return rc != PB_OK ? set_error(rc, "%s", msg.c_str()) : PB_OK;
}

}  // extern "C"
