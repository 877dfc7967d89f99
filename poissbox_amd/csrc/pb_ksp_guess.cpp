// pb_ksp_guess.cpp -- the host driver of the projected initial guess (-ksp_guess_type fischer:
// PETSc KSPGuessFischer, model 1; DESIGN.md "Projected initial guess"). Its kernels are in
// pb_guess.hip; the basis (pb_ksp::Fischer) is allocated by pb_ksp_create.
#include <cmath>

#include "pb_ksp.hpp"

using namespace pb;

// x = sum_i (b . bt[i]) xt[i], and the same into f->guess: one multi-dot, one two-output
// multi-axpy onto 0 reading its coefficients from the device (no host round trip)
static int fischer_form(pb_ksp* k, const double* b, double* x) {
  pb_ksp::Fischer* f = k->fg;
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const size_t vb = (size_t)g->nlocal * sizeof(double);
  if (f->curl == 0) {
    PB_HIP(hipMemsetAsync(x, 0, vb, ctx->stream));
    PB_HIP(hipMemsetAsync(f->guess, 0, vb, ctx->stream));
    return PB_OK;
  }
  VecTable t;
  for (int i = 0; i < kMaxVecs; ++i) t.p[i] = i < f->curl ? f->bt[i] : nullptr;
  PB_TRY(launch_mdot(ctx, b, f->curl, t, g->nlocal, f->d_coef));
  for (int i = 0; i < f->curl; ++i) t.p[i] = f->xt[i];
  MCoef c{};
  c.dev = f->d_coef;
  c.sign = 1.0;
  return launch_maxpy(ctx, x, f->guess, f->curl, t, c, g->nlocal, true, nullptr);
}

// the norm the last pass left in d_coef[16] as its square: the one host read of an update
static int fischer_norm(pb_ksp* k, double* norm) {
  pb_ctx* ctx = k->A->grid->ctx;
  PB_HIP(hipMemcpyAsync(ctx->h_scalars, k->fg->d_coef + kMaxVecs, sizeof(double),
                        hipMemcpyDeviceToHost, ctx->stream));
  PB_SYNC(ctx, "projected guess update");
  *norm = sqrt(ctx->h_scalars[0]);
  return PB_OK;
}

static int fischer_matvec(pb_ksp* k, const double* x, double* y) {
  ScopedTimer tm(k->A->grid->ctx, "guess_matvec");
  return op_apply_raw(k->A, x, y);
}

// after a solve from f->guess: the new direction x - guess, its A-image orthonormalised against
// the stored ones; a direction that is 0 or not finite is not added
static int fischer_update(pb_ksp* k, const double* x) {
  pb_ksp::Fischer* f = k->fg;
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const int64_t n = g->nlocal;
  VecTable t;
  for (int i = 0; i < kMaxVecs; ++i) t.p[i] = nullptr;
  MCoef c{};
  double* nrm2 = f->d_coef + kMaxVecs;
  double norm = 0.0;
  if (f->curl == f->maxl) {  // space full: restart from this solution alone
    PB_TRY(fischer_matvec(k, x, f->bt[0]));
    PB_TRY(launch_maxpy(ctx, f->bt[0], nullptr, 0, t, c, n, false, nrm2));
    PB_TRY(fischer_norm(k, &norm));
    f->curl = 0;
    if (!std::isfinite(norm) || norm == 0.0) return PB_OK;
    PB_TRY(launch_guess_scale(ctx, f->bt[0], x, f->xt[0], 1.0 / norm, n));
    f->curl = 1;
    return PB_OK;
  }
  const int l = f->curl;
  double* xn = f->xt[l];
  double* bn = f->bt[l];
  if (l == 0)
    PB_HIP(hipMemcpyAsync(xn, x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  else
    PB_TRY(launch_guess_diff(ctx, x, f->guess, xn, n));
  PB_TRY(fischer_matvec(k, xn, bn));
  if (l > 0) {
    // alpha[i] = -(bn . bt[i]); bn += sum alpha[i] bt[i] (its norm^2 in the same pass);
    // xn += sum alpha[i] xt[i]
    for (int i = 0; i < l; ++i) t.p[i] = f->bt[i];
    PB_TRY(launch_mdot(ctx, bn, l, t, n, f->d_coef));
    c.dev = f->d_coef;
    c.sign = -1.0;
    PB_TRY(launch_maxpy(ctx, bn, nullptr, l, t, c, n, false, nrm2));
    for (int i = 0; i < l; ++i) t.p[i] = f->xt[i];
    PB_TRY(launch_maxpy(ctx, xn, nullptr, l, t, c, n, false, nullptr));
  } else {
    PB_TRY(launch_maxpy(ctx, bn, nullptr, 0, t, c, n, false, nrm2));
  }
  PB_TRY(fischer_norm(k, &norm));
  if (!std::isfinite(norm) || norm == 0.0) return PB_OK;
  PB_TRY(launch_guess_scale(ctx, bn, xn, xn, 1.0 / norm, n));
  f->curl = l + 1;
  return PB_OK;
}

static int fischer_check(const pb_ksp* k, const pb_vec* b, const pb_vec* x) {
  PB_CHECK_ARG(k, "ksp is NULL");
  if (!k->fg) return set_error(PB_ERR_STATE, "KSP created without -ksp_guess_type fischer");
  PB_CHECK_ARG(b && x && b != x, "the projected guess needs distinct b and x");
  PB_CHECK_ARG(b->grid == k->A->grid && x->grid == k->A->grid, "vector/operator grid mismatch");
  return PB_OK;
}

extern "C" {

int pb_ksp_guess_form(pb_ksp* k, const pb_vec* b, pb_vec* x) {
  PB_TRY(fischer_check(k, b, x));
  return fischer_form(k, b->d, x->d);
}

int pb_ksp_guess_update(pb_ksp* k, const pb_vec* b, const pb_vec* x) {
  PB_TRY(fischer_check(k, b, x));
  return fischer_update(k, x->d);
}

int pb_ksp_guess_reset(pb_ksp* k) {
  PB_CHECK_ARG(k, "ksp is NULL");
  if (!k->fg) return set_error(PB_ERR_STATE, "KSP created without -ksp_guess_type fischer");
  k->fg->curl = 0;
  return PB_OK;
}

int pb_ksp_guess_size(const pb_ksp* k, int* curl, int* maxl) {
  PB_CHECK_ARG(k, "ksp is NULL");
  if (!k->fg) return set_error(PB_ERR_STATE, "KSP created without -ksp_guess_type fischer");
  if (curl) *curl = k->fg->curl;
  if (maxl) *maxl = k->fg->maxl;
  return PB_OK;
}

}  // extern "C"

// form, the solve exactly as with initial_guess_nonzero = 1 (also while the space is empty and
// x = 0: PETSc's guess_zero is false once the guess object touched x), update
int pb::solve_projected(pb_ksp* k, const pb_vec* b, pb_vec* x, pb_ksp_result* res,
                        double* history, int64_t cap) {
  PB_TRY(fischer_check(k, b, x));
  PB_TRY(fischer_form(k, b->d, x->d));
  const int user_flag = k->opts.initial_guess_nonzero;
  k->opts.initial_guess_nonzero = 1;
  const int rc = pb_ksp_begin(k, b, x);
  k->opts.initial_guess_nonzero = user_flag;
  PB_TRY(rc);
  PB_TRY(pb_ksp_iterate(k, k->solve_iters()));
  pb_ksp_result r;
  PB_TRY(pb_ksp_end(k, &r, history, cap));
  if (res) *res = r;
  // a non-finite direction must never enter the basis
  if (r.reason == PB_KSP_DIVERGED_NANORINF) return PB_OK;
  return fischer_update(k, x->d);
}
