// pb_ksp_stationary.cpp -- the host drivers of the stationary solves:
// -ksp_type richardson, chebyshev (with its eigenvalue estimate) and preonly. Their kernels and
// launchers and the fused update passes are in pb_ksp_stationary.hip; the
// device-resident state, done flags, history and polling are CG's (pb_solver.cpp).
#include <cmath>
#include <cstdio>
#include <cstring>

#include "pb_ksp.hpp"

using namespace pb;

// the 7-point operator on one rank: the engine pass reads the periodic wrap planes in place
static bool rich_engine(const pb_ksp* k) {
  return fused_kind(k->A->kind) && !k->A->grid->ctx->split;
}

// the unpreconditioned norm with a stored-z PC: the residual pass takes its two sums of
// t = r - mean (dinv = 1) after all, into the second partial region (the PC's own follow below it)
static bool rich_rr(const pb_ksp* k) { return k->stored_z() && k->norm_unp(); }

// r_out = b - A x (+ the sums of dinv r_out - mean with Jacobi / no PC: *np blocks, else 0; rr:
// the same sums into the second region instead, rich_rr)
static int rich_residual(pb_ksp* k, const double* x, double* r_out, bool skip, int* np,
                         RrParts* rr) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const bool sums = !k->stored_z();
  const bool aside = rich_rr(k);
  int n2 = 0;
  *np = 0;
  if (rich_engine(k)) {
    const Star s = star_of(k->A);
    const StencilPlanes gp = wrap_planes();
    PB_TRY(launch_rich_update(g, s, x, nullptr, k->b->d, nullptr, r_out, gp, k->d_st, 0.0,
                              sums || aside, skip, aside ? &n2 : np,
                              aside ? rr_part_off(ctx, 2) : 0));
  } else {
    {
      OpApplySkip guard(ctx, skip ? &k->d_st->done : nullptr);
      PB_TRY(op_apply_raw(k->A, x, k->w));
    }
    PB_TRY(launch_rich_resid(g, k->b->d, k->w, r_out, k->d_st, skip,
                             aside ? &n2 : (sums ? np : nullptr),
                             aside ? rr_region(ctx) : nullptr));
  }
  if (aside) *rr = RrParts{rr_region(ctx), n2, 2};
  return PB_OK;
}

// z = M^-1 r of a stored-z PC with the sums of z - mean (4 wide: the PC's own, or CG's sum kernel)
static int rich_pc(pb_ksp* k, const double* r, const int* skip, int* np) {
  PB_TRY(pc_apply_dev(k, r, k->z, skip, np));
  if (*np == 0) PB_TRY(launch_cg_pc_sums(k->A->grid, k->z, r, k->d_st, np));
  return PB_OK;
}

// ---------------------------------------------------------------------------------------------
// Chebyshev's interval
// ---------------------------------------------------------------------------------------------
// z = N(M^-1 r) with the KSP's PC and null space, host-driven (setup cost, not a hot path)
static int cheb_pc_n(pb_ksp* k, const double* r, double* z) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  if (k->stored_z()) {
    PB_TRY(pc_stored_apply(k, r, z));
  } else {
    PB_HIP(hipMemcpyAsync(z, r, (size_t)g->nlocal * sizeof(double), hipMemcpyDeviceToDevice,
                          ctx->stream));
    if (k->opts.pc_type == PB_PC_JACOBI)
      PB_TRY(vec_update(ctx, 2, z, nullptr, g->nlocal, 1.0 / k->P->cc));
  }
  if (!k->opts.nullspace) return PB_OK;
  int np = 0;
  PB_TRY(launch_pre_scale_sum(g, z, nullptr, 1.0, &np));
  PB_TRY(rich_reduce(ctx, np, 2, nullptr));
  return launch_pre_shift(g, z, (double)(g->n[0] * g->n[1] * g->n[2]));
}

// The extreme eigenvalues of M^-1 A on the range of N from `steps` steps of preconditioned
// CG-Lanczos (poissbox_gpu.h, pb_ksp_chebyshev_get_eigenvalues). Uses r, pb[0], pb[1] and x2:
// nothing of a solve may be in them. *n_out = the steps the tridiagonal holds (0: none)
static int cheb_lanczos(pb_ksp* k, double* lo, double* hi, int* n_out) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const int64_t n = g->nlocal;
  const size_t vb = (size_t)n * sizeof(double);
  if (!k->ri.x2 && field_alloc(&k->ri.x2, vb) != hipSuccess)
    return set_error(PB_ERR_ALLOC, "Chebyshev solution buffer: out of device memory");
  double *r = k->r, *p = k->pb[0], *w = k->pb[1], *z = k->ri.x2;
  const int steps = k->ch.opts.esteig_steps;
  double diag[64], off[64], alpha_prev = 0.0, beta_prev = 0.0;
  int m = 0;
  PB_TRY(vec_random(ctx, r, n, PB_CHEBYSHEV_ESTEIG_SEED, g->k0 * g->plane));
  if (k->opts.nullspace) {  // r_0 = N(v): r then stays in A's range
    int np = 0;
    PB_TRY(launch_pre_scale_sum(g, r, nullptr, 1.0, &np));
    PB_TRY(rich_reduce(ctx, np, 2, nullptr));
    PB_TRY(launch_pre_shift(g, r, (double)(g->n[0] * g->n[1] * g->n[2])));
  }
  PB_TRY(cheb_pc_n(k, r, z));
  PB_HIP(hipMemcpyAsync(p, z, vb, hipMemcpyDeviceToDevice, ctx->stream));
  double rz = 0.0, rz0 = 0.0;
  PB_TRY(vec_reduce(ctx, 1, r, z, n, &rz));
  rz0 = rz;
  for (int j = 0; j < steps; ++j) {
    double pw = 0.0;
    PB_TRY(op_apply_raw(k->A, p, w));
    PB_TRY(vec_reduce(ctx, 1, p, w, n, &pw));
    const double alpha = rz / pw;
    if (!std::isfinite(alpha) || alpha == 0.0) break;
    diag[j] = 1.0 / alpha + (j > 0 ? beta_prev / alpha_prev : 0.0);
    m = j + 1;
    if (m == steps) break;
    PB_TRY(vec_update(ctx, 0, r, w, n, -alpha));
    PB_TRY(cheb_pc_n(k, r, z));
    double rz_new = 0.0;
    PB_TRY(vec_reduce(ctx, 1, r, z, n, &rz_new));
    const double beta = rz_new / rz;
    // the Krylov space is exhausted (-pc_type fft with A = P after one step), or the PC is not
    // definite on it
    if (!std::isfinite(beta) || beta <= 0.0 || std::fabs(rz_new) <= 1e-24 * std::fabs(rz0)) break;
    off[j] = std::sqrt(beta) / alpha;
    PB_TRY(vec_update(ctx, 1, p, z, n, beta));
    alpha_prev = alpha;
    beta_prev = beta;
    rz = rz_new;
  }
  *n_out = m;
  if (m == 0) return PB_OK;
  return pb_tridiag_extreme_eigenvalues(m, diag, off, lo, hi);
}

// the bounds of the next solve into k->ch: the caller's, or the estimate (run once per pair of
// deltas) through the transform; an invalid pair is PB_ERR_ARG and leaves the KSP usable
static int cheb_bounds(pb_ksp* k) {
  const pb_ksp_chebyshev_opts& o = k->ch.opts;
  double emin = o.emin, emax = o.emax;
  const bool given = emin != 0.0 || emax != 0.0;
  double dl[6];
  for (int d = 0; d < 3; ++d) {
    dl[d] = k->A->deltas[d];
    dl[3 + d] = k->P->deltas[d];
  }
  if (given) {
    PB_TRY(check_cheb_pair(emin, emax, "chebyshev eigenvalues"));
    k->ch.state = 1;
  } else if (k->ch.state != 2 || memcmp(dl, k->ch.deltas, sizeof(dl)) != 0 ||
             k->ch.change[0] != k->A->change || k->ch.change[1] != k->P->change) {
    if (k->begun) return set_error(PB_ERR_STATE, "Chebyshev eigenvalue estimate inside a solve");
    double lo = 0.0, hi = 0.0;
    int m = 0;
    k->ch.state = 0;
    PB_TRY(cheb_lanczos(k, &lo, &hi, &m));
    if (m == 0)
      return set_error(PB_ERR_ARG, "Chebyshev eigenvalue estimate: the Lanczos process broke down "
                                   "at its first step");
    emin = o.esteig[0] * lo + o.esteig[1] * hi;
    emax = o.esteig[2] * lo + o.esteig[3] * hi;
    if (check_cheb_pair(emin, emax, "estimate") != PB_OK)
      return set_error(PB_ERR_ARG,
                       "Chebyshev eigenvalue estimate: extremes %g, %g transform to emin %g, emax "
                       "%g, no valid bounds (a negative spectrum, as with -pc_type none, needs "
                       "-ksp_chebyshev_esteig weights that keep emax > emin, or explicit "
                       "-ksp_chebyshev_eigenvalues)", lo, hi, emin, emax);
    memcpy(k->ch.deltas, dl, sizeof(dl));
    k->ch.change[0] = k->A->change;
    k->ch.change[1] = k->P->change;
    k->ch.state = 2;
  } else {
    emin = k->ch.emin;
    emax = k->ch.emax;
  }
  k->ch.emin = emin;
  k->ch.emax = emax;
  // KSPSolve_Chebyshev's quantities
  k->ch.scale = 2.0 / (emax + emin);
  const double alpha = 1.0 - k->ch.scale * emin;
  k->ch.mu = 1.0 / alpha;
  k->ch.omegaprod = 2.0 / alpha;
  return PB_OK;
}

// KSPSolve_Richardson's setup: r_0 = b (read in place), x_0 = 0, or r_0 = b - A x_0 from a nonzero
// guess with CG's reference-norm rules; z_0, its norm, history[0] and the first test
int pb::rich_begin(pb_ksp* k, const pb_vec* b, pb_vec* x) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const size_t vb = (size_t)g->nlocal * sizeof(double);
  // b is read by every update (r = b - A x) while x is written
  PB_CHECK_ARG(b != x, k->cheb() ? "chebyshev needs distinct b and x"
                                   : "richardson needs distinct b and x");
  k->sr.on = false;
  k->pst = false;
  k->lazy0 = false;
  k->defer_x = 0;
  if (!k->ri.x2 && field_alloc(&k->ri.x2, vb) != hipSuccess)
    return set_error(PB_ERR_ALLOC, "Richardson solution buffer: out of device memory");
  if (k->cheb() && !k->ri.x3 && field_alloc(&k->ri.x3, vb) != hipSuccess)
    return set_error(PB_ERR_ALLOC, "Chebyshev solution buffer: out of device memory");
  if (!k->stored_z() && !k->r2 && field_alloc(&k->r2, vb) != hipSuccess)
    return set_error(PB_ERR_ALLOC, "Richardson residual buffer: out of device memory");
  if (!rich_engine(k) && !k->w && field_alloc(&k->w, vb) != hipSuccess)
    return set_error(PB_ERR_ALLOC, "Richardson work vector: out of device memory");
  // (the eigenvalue estimate, when it has to run, uses the work vectors: before anything of
  // this solve is in them; invalid bounds leave the KSP as it was)
  if (k->cheb()) PB_TRY(cheb_bounds(k));
  const double cmu = k->cheb() ? k->ch.mu : 0.0, cop = k->cheb() ? k->ch.omegaprod : 0.0;
  k->b = b;
  k->x = x;
  k->ri.guess = k->opts.initial_guess_nonzero != 0;
  const int width = k->stored_z() ? 4 : 2;
  int np = 0;
  RrParts rr;
  if (!k->ri.guess) {
    PB_HIP(hipMemsetAsync(x->d, 0, vb, ctx->stream));
    if (rich_rr(k)) {  // ||r_0|| = ||b||: a reduction pass of its own (setup only)
      int n2 = 0;
      PB_TRY(launch_rich_sums(g, b->d, k->d_st, &n2, rr_region(ctx)));
      rr = RrParts{rr_region(ctx), n2, 2};
    }
    if (k->stored_z()) PB_TRY(rich_pc(k, b->d, nullptr, &np));
    else PB_TRY(launch_rich_sums(g, b->d, k->d_st, &np));
    return rich_finalize(ctx, np, width, nullptr, 3, k->log(), -1, cmu, cop, rr);
  }
  PB_TRY(check_ref_norm_opts(&k->opts));
  const int ref = k->ref_norm();
  const double* bsums = nullptr;
  // the reference norm ||N(M^-1 b)||: the sums of M^-1 b kept aside (unpreconditioned, Jacobi / no
  // PC: ||b|| from the same sums of dinv b; none: no reference)
  if (ref != 1 && !k->norm_none()) {
    // (unpreconditioned with a stored-z PC: ||b|| from the plain sums of b, no PC application)
    const bool pc = k->stored_z() && !k->norm_unp();
    if (pc) PB_TRY(rich_pc(k, b->d, nullptr, &np));
    else PB_TRY(launch_rich_sums(g, b->d, k->d_st, &np));
    PB_TRY(rich_reduce(ctx, np, pc ? 4 : 2, k->guess_bsums()));
    bsums = k->guess_bsums();
  }
  PB_TRY(rich_residual(k, x->d, k->r, false, &np, &rr));
  if (k->stored_z()) PB_TRY(rich_pc(k, k->r, nullptr, &np));
  return rich_finalize(ctx, np, width, bsums, ref, k->log(), -1, cmu, cop, rr);
}

// one update: x_new = x + scale (M^-1 r - mean), r_new = b - A x_new, z_new and its sums, the
// norm and the test. On the 7-point operator (one rank) the first two are one engine pass
// (tuning rich_fused = 0: a vector kernel and the engine's residual pass, bit-identical)
int pb::enqueue_rich_iteration(pb_ksp* k) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const int64_t i = k->host_iter;
  const double* xin = k->xbuf(i);
  double* xout = k->xbuf(i + 1);
  const double* q = k->stored_z() ? k->z : k->rich_rbuf(i);
  double* r_out = k->stored_z() ? k->r : (((i + 1) & 1) ? k->r2 : k->r);
  // Chebyshev: update 0 is Richardson's with scale = 2 / (emax + emin); update i >= 1 reads
  // y_(i-1) too (host_iter is the device's update count while the state is not done, and every
  // launch of a done state exits at entry)
  const bool cheb = k->cheb();
  const double scale = cheb ? k->ch.scale : k->opts.richardson_scale;
  const double* xm1 = cheb && i >= 1 ? k->xbuf(i - 1) : nullptr;
  const bool fused = rich_engine(k) && (cheb ? tune("cheb_fused", 1) : tune("rich_fused", 1)) != 0;
  int np = 0;
  RrParts rr;
  if (fused) {
    const Star s = star_of(k->A);
    const StencilPlanes gp = wrap_planes();
    // (rich_rr: the sums variant of the same pass, its partials in the second region)
    const bool aside = rich_rr(k);
    const int off = aside ? rr_part_off(ctx, 2) : 0;
    int n2 = 0;
    if (xm1)
      PB_TRY(launch_cheb_update(g, s, xin, xm1, q, k->b->d, xout, r_out, gp, k->d_st, scale,
                                !k->stored_z() || aside, aside ? &n2 : &np, off));
    else
      PB_TRY(launch_rich_update(g, s, xin, q, k->b->d, xout, r_out, gp, k->d_st, scale,
                                !k->stored_z() || aside, true, aside ? &n2 : &np, off));
    if (aside) rr = RrParts{rr_region(ctx), n2, 2};
  } else {
    if (xm1) PB_TRY(launch_cheb_x(g, xin, xm1, q, xout, k->d_st, scale));
    else PB_TRY(launch_rich_x(g, xin, q, xout, k->d_st, scale));
    PB_TRY(rich_residual(k, xout, r_out, true, &np, &rr));
  }
  if (k->stored_z()) PB_TRY(rich_pc(k, r_out, &k->d_st->done, &np));
  return rich_finalize(ctx, np, k->stored_z() ? 4 : 2, nullptr, 0, k->log(), i,
                       cheb ? k->ch.mu : 0.0, cheb ? k->ch.omegaprod : 0.0, rr);
}

// KSPSolve_PREONLY: x = N(M^-1 b). No norm, no reduction but the mean's, no NaN check. The
// spectral PC zeroes mode 0 itself: its result keeps its rounding-level mean (poissbox_gpu.h)
int pb::solve_preonly(pb_ksp* k, const pb_vec* b, pb_vec* x, pb_ksp_result* res) {
  PB_CHECK_ARG(k && b && x, "bad solve args");
  pb_grid* g = k->A->grid;
  PB_CHECK_ARG(b->grid == g && x->grid == g, "vector/operator grid mismatch");
  PB_CHECK_ARG(b != x, "preonly needs distinct b and x");
  pb_ctx* ctx = g->ctx;
  int np = 0;
  if (k->fft) {
    PB_TRY(fftpc_apply(k->fft, b->d, x->d));
  } else {
    if (k->stored_z()) {  // mg, sor or the Jacobi PC of a variable P
      PB_TRY(pc_stored_apply(k, b->d, x->d));
      if (k->opts.nullspace) PB_TRY(launch_pre_scale_sum(g, x->d, nullptr, 1.0, &np));
    } else {
      const double dinv = k->opts.pc_type == PB_PC_JACOBI ? 1.0 / k->P->cc : 1.0;
      PB_TRY(launch_pre_scale_sum(g, b->d, x->d, dinv, &np));
    }
    if (k->opts.nullspace) {
      PB_TRY(rich_reduce(ctx, np, 2, nullptr));
      PB_TRY(launch_pre_shift(g, x->d, (double)(g->n[0] * g->n[1] * g->n[2])));
    }
  }
  PB_SYNC(ctx, "pb_ksp_solve (preonly)");
  if (res) {
    res->reason = PB_KSP_CONVERGED_ITS;
    res->its = 1;
    res->rnorm = 0.0;
    res->rnorm0 = 0.0;
    res->nhist = 0;
  }
  if (ctx->rank == 0 && k->opts.converged_reason) {
    printf("Linear solve converged due to CONVERGED_ITS iterations 1\n");
    fflush(stdout);
  }
  return PB_OK;
}

// Richardson after an odd number of updates, Chebyshev after one that is no multiple of 3: the
// result is in another buffer than the caller's
int pb::rich_copy_back(pb_ksp* k, int64_t its) {
  if (k->xbuf(its) == k->x->d) return PB_OK;
  pb_ctx* ctx = k->A->grid->ctx;
  PB_HIP(hipMemcpyAsync(k->x->d, k->xbuf(its), (size_t)k->A->grid->nlocal * sizeof(double),
                        hipMemcpyDeviceToDevice, ctx->stream));
  PB_SYNC(ctx, "pb_ksp_end");
  return PB_OK;
}

extern "C" {

int pb_ksp_chebyshev_set_opts(pb_ksp* k, const pb_ksp_chebyshev_opts* o) {
  PB_CHECK_ARG(k && o, "bad args");
  if (!k->cheb()) return set_error(PB_ERR_STATE, "KSP created without -ksp_type chebyshev");
  if (k->begun) return set_error(PB_ERR_STATE, "pb_ksp_chebyshev_set_opts inside a solve");
  PB_TRY(check_cheb_opts(o));
  k->ch.opts = *o;
  k->ch.state = 0;
  return PB_OK;
}

int pb_ksp_chebyshev_get_eigenvalues(pb_ksp* k, double* emin, double* emax, int* estimated) {
  PB_CHECK_ARG(k, "ksp is NULL");
  if (!k->cheb()) return set_error(PB_ERR_STATE, "KSP created without -ksp_type chebyshev");
  PB_TRY(cheb_bounds(k));
  PB_SYNC(k->A->grid->ctx, "pb_ksp_chebyshev_get_eigenvalues");
  if (emin) *emin = k->ch.emin;
  if (emax) *emax = k->ch.emax;
  if (estimated) *estimated = k->ch.state == 2 ? 1 : 0;
  return PB_OK;
}

// Bisection on the Sturm count (the number of eigenvalues below s = the number of negative pivots
// of T - s I), started from the Gershgorin interval; ends when the interval cannot be halved
int pb_tridiag_extreme_eigenvalues(int n, const double* diag, const double* off, double* lo,
                                   double* hi) {
  PB_CHECK_ARG(n >= 1 && n <= 64, "tridiagonal order outside 1..64");
  PB_CHECK_ARG(diag && lo && hi && (off || n == 1), "bad tridiagonal args");
  double gl = INFINITY, gu = -INFINITY;
  for (int i = 0; i < n; ++i) {
    const double a = i > 0 ? std::fabs(off[i - 1]) : 0.0, c = i + 1 < n ? std::fabs(off[i]) : 0.0;
    PB_CHECK_ARG(std::isfinite(diag[i]) && std::isfinite(a) && std::isfinite(c),
                 "tridiagonal entries must be finite");
    gl = std::min(gl, diag[i] - (a + c));
    gu = std::max(gu, diag[i] + (a + c));
  }
  PB_CHECK_ARG(std::isfinite(gl) && std::isfinite(gu), "tridiagonal entries too large");
  const double tiny = 1e-300 + 2.3e-16 * std::max(std::fabs(gl), std::fabs(gu));
  auto below = [&](double s) {
    int cnt = 0;
    double q = 1.0;
    for (int i = 0; i < n; ++i) {
      const double e = i > 0 ? off[i - 1] : 0.0;
      q = diag[i] - s - (i > 0 ? e * e / q : 0.0);
      if (std::fabs(q) < tiny) q = -tiny;
      if (q < 0.0) ++cnt;
    }
    return cnt;
  };
  // the index-th eigenvalue (ascending): the s where below(s) passes from <= index to > index
  auto kth = [&](int index) {
    double a = gl, b = gu;
    for (int it = 0; it < 2000; ++it) {
      const double m = a + 0.5 * (b - a);
      if (!(m > a && m < b)) break;
      if (below(m) > index) b = m;
      else a = m;
    }
    return a + 0.5 * (b - a);
  };
  *lo = kth(0);
  *hi = kth(n - 1);
  return PB_OK;
}

}  // extern "C"
