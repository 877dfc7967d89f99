// pb_solver.cpp -- KSP (KSPSolve_CG analogue) host logic: pb_ksp_create / begin / iterate / end /
// solve / destroy, the CG enqueue paths and pb_solve*. The operator is in pb_op.cpp, the options in
// pb_options.cpp, -ksp_type richardson | chebyshev | preonly in pb_ksp_stationary.cpp, fgmres in
// pb_ksp_fgmres.cpp, pipecg in pb_ksp_pipecg.cpp, the projected initial guess in pb_ksp_guess.cpp,
// -ksp_norm_type in pb_norm_type.cpp; struct pb_ksp and what they share in pb_ksp.hpp.
//
// The CG iteration runs as 2 fused stencil passes + 2 one-block finalize kernels per iteration
// (plus a plane-sized boundary kernel and, on several ranks, one halo exchange and two scalar
// allreduces). All CG scalars live on the device; the host never waits inside an iteration and
// polls a per-iteration "done" flag (host-mapped) every `check_every` iterations, lagged by one
// poll interval so that every rank stops after the same number of enqueued iterations.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pb_ksp.hpp"

using namespace pb;

static int sr_pass_s(pb_ksp* k, const double* r, const CgState* st, int* nparts, int64_t n);
static const double* sr_region(const pb_ctx* ctx, int64_t n);
static int cg_begin(pb_ksp* k, const pb_vec* b, pb_vec* x, CgState& st);

int pb::ensure_done_cap(pb_ksp* k, int64_t need) {
  if (need <= k->done_cap) return PB_OK;
  int64_t cap = need < 1024 ? 1024 : need * 2;
  int* h = nullptr;
  PB_HIP(hipHostMalloc(&h, (size_t)cap * sizeof(int), hipHostMallocMapped));
  memset(h, 0, (size_t)cap * sizeof(int));
  if (k->h_done) {
    PB_TRY(wait_stream(k->A->grid->ctx, k->A->grid->ctx->stream, "KSP flag buffer"));
    memcpy(h, k->h_done, (size_t)k->done_cap * sizeof(int));
    (void)hipHostFree(k->h_done);
  }
  k->h_done = h;
  PB_HIP(hipHostGetDevicePointer((void**)&k->h_done_dev, h, 0));
  k->done_cap = cap;
  return PB_OK;
}

// z = M^-1 r for the stored-z preconditioners; *np = residual-sum partial blocks written by the
// PC itself (MG's last sweep), 0 if the caller must take the sums
int pb::pc_apply_dev(pb_ksp* k, const double* r, double* z, const int* skip, int* np) {
  *np = 0;
  if (k->fft) return fftpc_apply(k->fft, r, z, skip, k->d_st, np);
  return mg_apply(k->mg, r, z, skip, k->d_st, np);
}

extern "C" {

// ---------------------------------------------------------------------------------------------
// KSP
// ---------------------------------------------------------------------------------------------
int pb_ksp_create(pb_op* A, pb_op* P, const pb_ksp_opts* opts, pb_ksp** out) {
  PB_CHECK_ARG(A && out, "bad ksp args");
  if (!P) P = A;
  PB_CHECK_ARG(A->grid == P->grid, "A and P on different grids");
  pb_ksp* k = new pb_ksp();
  k->A = A;
  k->P = P;
  // every failure below releases what was built so far (pb_ksp_destroy takes a partial KSP:
  // each field, the PC objects and the state are freed only if they exist)
  auto fail = [k](int rc) {
    const std::string msg = pb_last_error();
    pb_ksp_destroy(k);
    return set_error(rc, "%s", msg.c_str());
  };
  if (opts) k->opts = *opts;
  else pb_ksp_opts_default(&k->opts);
  if (k->opts.check_every < 1) k->opts.check_every = 8;
  if (check_ref_norm_opts(&k->opts) != PB_OK) return fail(PB_ERR_ARG);
  const int kt = k->opts.ksp_type;
  if (kt != PB_KSP_CG && kt != PB_KSP_PREONLY && kt != PB_KSP_RICHARDSON &&
      kt != PB_KSP_CHEBYSHEV && kt != PB_KSP_FGMRES && kt != PB_KSP_PIPECG)
    return fail(set_error(PB_ERR_UNSUPPORTED, "unknown ksp_type %d", kt));
  pb_ksp_chebyshev_opts_default(&k->ch.opts);
  pb_pc_mg_opts_default(&k->mgopts);
  if (const int rc = fgmres_create(k)) return fail(rc);
  if (const int rc = pipecg_create(k)) return fail(rc);
  if (check_richardson_scale(k->opts.richardson_scale) != PB_OK) return fail(PB_ERR_ARG);
  if (kt == PB_KSP_PREONLY &&
      (k->opts.initial_guess_nonzero || k->opts.guess_type != PB_GUESS_NONE))
    return fail(set_error(PB_ERR_ARG,
                          "preonly doesn't make sense with a nonzero initial guess; you probably "
                          "want richardson"));
  // SOR / MG / FFT iterations are expensive and few: poll the device flag more often -- every
  // iteration with the spectral PC (1-3 iterations per solve: an iteration enqueued ahead of the
  // poll costs its skipped launches, ~0.15 ms of a 512^3 config-5 solve, more than the idle
  // stream time of waiting for each iteration)
  // (only clamped down: a caller's explicit smaller interval stands -- ADVICE r03)
  if ((k->opts.pc_type == PB_PC_SOR || k->opts.pc_type == PB_PC_MG) && k->opts.check_every > 2)
    k->opts.check_every = 2;
  if (k->opts.pc_type == PB_PC_FFT)
    k->opts.check_every = 1;
  const int pc = k->opts.pc_type;
  if (pc != PB_PC_NONE && pc != PB_PC_JACOBI && pc != PB_PC_SOR && pc != PB_PC_MG &&
      pc != PB_PC_FFT)
    return fail(set_error(PB_ERR_UNSUPPORTED, "unknown pc_type %d", pc));
  pb_grid* g = A->grid;
  const size_t vb = (size_t)g->nlocal * sizeof(double);
  if (pc == PB_PC_SOR || pc == PB_PC_MG) {
    // the smoother / coarse operators are the 7-point P (src/coefficients.f90 star)
    if (P->kind == PB_OP_COMPACT)
      return fail(set_error(PB_ERR_UNSUPPORTED, "SOR / MG preconditioning needs a 7-point P"));
    const int rc = mg_create(g, P->deltas, pc, k->opts.mg_levels, k->opts.mg_coarse_its,
                             k->opts.sor_omega, &k->mg);
    if (rc != PB_OK) return fail(rc);
  }
  if (pc == PB_PC_FFT) {
    // the symbol of P: the compact operator (config 5: A = P = compact) or the 7-point star
    const int rc = fftpc_create(g, P->deltas, P->kind == PB_OP_COMPACT, &k->fft);
    if (rc != PB_OK) return fail(rc);
  }
  if (field_alloc(&k->r, vb) != hipSuccess || field_alloc(&k->pb[0], vb) != hipSuccess ||
      field_alloc(&k->pb[1], vb) != hipSuccess)
    return fail(set_error(PB_ERR_ALLOC, "KSP work vectors: out of device memory"));
  if (!fused_kind(A->kind) || k->stored_z()) {
    if (field_alloc(&k->w, vb) != hipSuccess || field_alloc(&k->z, vb) != hipSuccess)
      return fail(set_error(PB_ERR_ALLOC, "KSP work vectors: out of device memory"));
  }
  // [1]: the folded iteration's second slot; behind them four doubles: the sums of M^-1 b a
  // stored-z setup from a nonzero guess takes for its reference norm (guess_bsums: t, t^2 for
  // ||N(M^-1 b)||, and t.b, b for the natural norm's sqrt|b . N(M^-1 b)|)
  if (hipMalloc(&k->d_st, 2 * sizeof(CgState) + 4 * sizeof(double)) != hipSuccess)
    return fail(set_error(PB_ERR_ALLOC, "KSP state: out of device memory"));
  if (k->opts.guess_type != PB_GUESS_NONE) {
    if (k->opts.guess_type != PB_GUESS_FISCHER)
      return fail(set_error(PB_ERR_UNSUPPORTED, "unknown guess_type %d", k->opts.guess_type));
    const int rc = check_guess_opts(k->opts.guess_fischer_model, k->opts.guess_fischer_maxl);
    if (rc != PB_OK) return fail(rc);
    // 2 maxl + 1 fields: xt[maxl], bt[maxl] and the last formed guess
    pb_ksp::Fischer* f = k->fg = new pb_ksp::Fischer();
    f->maxl = k->opts.guess_fischer_maxl;
    f->xt.assign(f->maxl, nullptr);
    f->bt.assign(f->maxl, nullptr);
    bool ok = field_alloc(&f->guess, vb) == hipSuccess;
    for (int i = 0; ok && i < f->maxl; ++i)
      ok = field_alloc(&f->xt[i], vb) == hipSuccess && field_alloc(&f->bt[i], vb) == hipSuccess;
    if (!ok)
      return fail(set_error(PB_ERR_ALLOC, "projected guess: %d vectors: out of device memory",
                            2 * f->maxl + 1));
    if (hipMalloc(&f->d_coef, (kMaxVecs + 1) * sizeof(double)) != hipSuccess)
      return fail(set_error(PB_ERR_ALLOC, "projected guess state: out of device memory"));
    if (hipMemsetAsync(f->guess, 0, vb, g->ctx->stream) != hipSuccess)
      return fail(set_error(PB_ERR_HIP, "projected guess: clearing the stored guess failed"));
  }
  *out = k;
  return PB_OK;
}

// Setup from a nonzero initial guess (-ksp_initial_guess_nonzero): r = b - A x0, p = 0, z0 and
// stage 0 with KSPConvergedDefault's reference norm; x0 is read only
static int guess_setup(pb_ksp* k, const double* b, const double* x0, double dinv) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const int ref = k->opts.converged_use_initial_residual_norm
                      ? 1
                      : (k->opts.converged_use_min_initial_residual_norm ? 2 : 0);
  int np = 0;
  if (k->stored_z()) {
    const double* bsums = nullptr;
    // unpreconditioned: the reference is ||b||, taken beside ||r_0|| by the residual kernel -- the
    // PC application behind ||N(M^-1 b)|| disappears
    const bool unp = k->norm_unp();
    RrParts rr;
    if (ref != 1 && !k->norm_none() && !unp) {
      // the reference norm ||N(M^-1 b)|| (natural: sqrt|b . N(M^-1 b)|): one more PC application,
      // its sums kept aside; -ksp_norm_type none tests nothing and needs no reference
      PB_TRY(pc_apply_dev(k, b, k->z, nullptr, &np));
      if (np == 0) PB_TRY(launch_cg_pc_sums(g, k->z, b, k->d_st, &np));
      PB_TRY(cg_reduce_allreduce(ctx, ctx->d_partials, np, 4));
      PB_HIP(hipMemcpyAsync(k->guess_bsums(), ctx->d_scalars, 4 * sizeof(double),
                            hipMemcpyDeviceToDevice, ctx->stream));
      bsums = k->guess_bsums();
    }
    PB_TRY(op_apply_raw(k->A, x0, k->w));
    PB_TRY(launch_cg_guess_resid(g, b, k->w, k->r, k->pb[0], dinv, nullptr, unp ? &rr : nullptr));
    PB_TRY(pc_apply_dev(k, k->r, k->z, nullptr, &np));
    if (np == 0) PB_TRY(launch_cg_pc_sums(g, k->z, k->r, k->d_st, &np));
    return cg_finalize_guess(ctx, np, 4, bsums, ref, k->d_st, k->d_hist, k->h_done_dev, rr);
  }
  if (!fused_kind(k->A->kind)) {  // compact / assembled A with Jacobi / no PC
    PB_TRY(op_apply_raw(k->A, x0, k->w));
    PB_TRY(launch_cg_guess_resid(g, b, k->w, k->r, k->pb[0], dinv, &np));
    return cg_finalize_guess(ctx, np, 6, nullptr, ref, k->d_st, k->d_hist, k->h_done_dev);
  }
  // the fused pass; split grids exchange x0's boundary planes under the interior planes
  const Star s = star_of(k->A);
  StencilPlanes gp;
  const double* hi = x0 + (g->nzl - 1) * g->plane;
  if (!ctx->split) {
    gp.ghost_lo = hi;  // periodic wrap: no copy
    gp.ghost_hi = x0;
    PB_TRY(launch_cg_guess_init(g, s, x0, b, k->r, k->pb[0], gp, dinv, PLANES_ALL, 0, &np));
  } else {
    gp.ghost_lo = g->ghost_lo;
    gp.ghost_hi = g->ghost_hi;
    if (g->nzl < 3) {
      PB_TRY(halo_exchange(g, x0, hi));
      PB_TRY(launch_cg_guess_init(g, s, x0, b, k->r, k->pb[0], gp, dinv, PLANES_ALL, 0, &np));
    } else {
      int nb1 = 0, nb2 = 0;
      ScopedTimer tm(ctx, "cg_init_guess");
      PB_TRY(halo_begin(g, x0, hi));
      PB_TRY(launch_cg_guess_init(g, s, x0, b, k->r, k->pb[0], gp, dinv, PLANES_INTERIOR, 0,
                                  &nb1));
      PB_TRY(halo_end(g));
      PB_TRY(launch_cg_guess_init(g, s, x0, b, k->r, k->pb[0], gp, dinv, PLANES_BOUNDARY, nb1,
                                  &nb2));
      np = nb1 + nb2;
    }
  }
  PB_TRY(cg_finalize_guess(ctx, np, 6, nullptr, ref, k->d_st, k->d_hist, k->h_done_dev));
  if (k->sr.on) {
    // KSPSolve_CG_SingleReduction's setup as from a zero guess: pass S over r0
    PB_TRY(sr_pass_s(k, k->r, k->d_st, &np, 0));
    PB_TRY(cg_sr_finalize(ctx, sr_region(ctx, 0), np, k->d_st, k->d_hist, k->h_done_dev, -1,
                          true));
  }
  return PB_OK;
}

static int preonly_split_form(const pb_ksp* k) {
  if (k && k->opts.ksp_type == PB_KSP_PREONLY)
    return set_error(PB_ERR_UNSUPPORTED,
                     "-ksp_type preonly has no split form: use pb_ksp_solve or pb_solve");
  return PB_OK;
}

int pb_ksp_begin(pb_ksp* k, const pb_vec* b, pb_vec* x) {
  PB_CHECK_ARG(k && b && x, "bad begin args");
  PB_TRY(preonly_split_form(k));
  pb_grid* g = k->A->grid;
  PB_CHECK_ARG(b->grid == g && x->grid == g, "vector/operator grid mismatch");
  pb_ctx* ctx = g->ctx;
  // history buffer: max_it + 1 entries
  const int64_t nh = k->opts.max_it + 1;
  if (nh > k->nhist) {
    if (k->d_hist) (void)hipFree(k->d_hist);
    PB_HIP(hipMalloc(&k->d_hist, (size_t)nh * sizeof(double)));
    k->nhist = nh;
  }
  PB_TRY(ensure_done_cap(k, 1024));
  memset(k->h_done, 0, (size_t)k->done_cap * sizeof(int));
  CgState st;
  memset(&st, 0, sizeof(st));
  st.rtol = k->opts.rtol;
  st.atol = k->opts.atol;
  st.dtol = k->opts.dtol;
  st.max_it = k->opts.max_it;
  st.nhist = k->nhist;
  st.pc = k->opts.pc_type;
  st.nullspace = k->opts.nullspace;
  st.norm = k->norm();
  // PCJacobi stores the reciprocal of diag(P) (src/coefficients.f90:44-46 centre coefficient);
  // with SOR / MG the sums are taken over z = M^-1 r itself (dinv = 1)
  st.dinv = k->opts.pc_type == PB_PC_JACOBI ? 1.0 / k->P->cc : 1.0;
  st.ntot = (double)(g->n[0] * g->n[1] * g->n[2]);
  if (k->rich()) {
    PB_HIP(hipMemcpyAsync(k->d_st, &st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
    PB_TRY(rich_begin(k, b, x));
  } else if (k->fgmres()) {
    PB_HIP(hipMemcpyAsync(k->d_st, &st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
    PB_TRY(fgmres_begin(k, b, x));
  } else if (k->pipecg()) {
    PB_HIP(hipMemcpyAsync(k->d_st, &st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
    PB_TRY(pipecg_begin(k, b, x));
  } else {
    PB_TRY(cg_begin(k, b, x, st));
  }
  PB_SYNC(ctx, "pb_ksp_begin");
  k->b = b;
  k->x = x;
  k->host_iter = 0;
  k->stopped = k->h_done[0] != 0;
  k->begun = true;
  return PB_OK;
}

// KSPSolve_CG's setup: the buffers and the form of this solve's iteration, the state (st: the
// tolerances, filled in by pb_ksp_begin) to the device, r_0, z_0, history[0] and the first test
static int cg_begin(pb_ksp* k, const pb_vec* b, pb_vec* x, CgState& st) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  // depth 4 (default): 58 instead of 60 B/DoF per iteration, measured 3 % faster at 512^3
  // (profiles/r01/ab_defer_x.txt); the x update sums four alpha p terms instead of adding them
  // one per iteration (rounding-level difference in x only: the history is unaffected)
  const int dx = tune("cg_defer_x", 4);
  k->defer_x = dx == 0 ? 0 : (dx == 2 ? 2 : 4);
  if (!fused_kind(k->A->kind)) k->defer_x = 0;  // generic path: x every iteration
  st.defer_x = k->defer_x;
  // p stored by pass B (default): pass A read-only, 56 instead of 58 B/DoF per iteration and
  // the passes closer to their patterns' rates -- 1.29 vs 1.36 ms/iteration at 512^3 on one box
  // (profiles/r02/ab_pst_defer_512.jsonl); with a stored-z PC pass A stores p (the r01 split)
  k->pst = fused_kind(k->A->kind) && !k->stored_z();
  // single reduction: the fused operator with Jacobi / no PC (pass P forms p from r on load);
  // elsewhere the KSPSolve_CG iteration runs (equal in exact arithmetic; pb_ksp_opts)
  k->sr.on = k->opts.cg_single_reduction != 0 && fused_kind(k->A->kind) && !k->stored_z();
  st.sr = k->sr.on ? 1 : 0;
  if (k->sr.on) k->pst = true;  // r ping-pongs between r and r2 (pass P reads r_i, writes r_i+1)
  if (k->pst && !k->r2) {
    const size_t vb = (size_t)g->nlocal * sizeof(double);
    if (field_alloc(&k->r2, vb) != hipSuccess)
      return set_error(PB_ERR_ALLOC, "CG residual buffer: out of device memory");
  }
  if (k->defer_x == 4 && !k->pb[2]) {
    const size_t vb = (size_t)g->nlocal * sizeof(double);
    if (field_alloc(&k->pb[2], vb) != hipSuccess || field_alloc(&k->pb[3], vb) != hipSuccess)
      return set_error(PB_ERR_ALLOC, "CG direction buffers: out of device memory");
  }
  PB_HIP(hipMemcpyAsync(k->d_st, &st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
  // stored z with an operator without a stencil engine (compact A): r0 = b, x0 = 0 and p0 = 0 are
  // implicit -- the setup reads b in place of r, and the first iteration writes p = z, x = alpha p
  // and r = b - alpha w without reading them (three vector passes fewer)
  k->lazy0 = k->stored_z() && !fused_kind(k->A->kind) && tune("ksp_lazy0", 1) != 0;
  if (k->opts.initial_guess_nonzero) {
    // (read on every begin: a reused KSP warm-starts each solve of a time loop from its x)
    PB_CHECK_ARG(b != x, "a nonzero initial guess needs distinct b and x");
    PB_TRY(check_ref_norm_opts(&k->opts));
    k->lazy0 = false;  // x0 is not 0: every update accumulates onto it, none may overwrite
    PB_TRY(guess_setup(k, b->d, x->d, st.dinv));
  } else if (k->stored_z()) {
    // r = b, x = 0, p = 0; z = M^-1 r; sums of z (KSPSolve_CG setup, PC_LEFT)
    const size_t vb = (size_t)g->nlocal * sizeof(double);
    const double* r0 = k->lazy0 ? b->d : k->r;
    if (!k->lazy0) {
      PB_HIP(hipMemcpyAsync(k->r, b->d, vb, hipMemcpyDeviceToDevice, ctx->stream));
      PB_HIP(hipMemsetAsync(x->d, 0, vb, ctx->stream));
      PB_HIP(hipMemsetAsync(k->pb[0], 0, vb, ctx->stream));
    }
    int np = 0;
    RrParts rr;  // unpreconditioned: ||r_0|| = ||b|| by a reduction pass of its own (setup only)
    if (k->norm_unp()) PB_TRY(launch_cg_rr(g, r0, &rr));
    PB_TRY(pc_apply_dev(k, r0, k->z, nullptr, &np));
    if (np == 0) PB_TRY(launch_cg_pc_sums(g, k->z, r0, k->d_st, &np));
    PB_TRY(cg_finalize_init(ctx, np, k->d_st, k->d_hist, k->h_done_dev, rr));
  } else {
    PB_TRY(launch_cg_init(g, b->d, x->d, k->r, k->pb[0], k->d_st, st.dinv, k->d_hist,
                          k->h_done_dev));
    if (k->sr.on) {
      // KSPSolve_CG_SingleReduction's setup: S = A z, delta = z'S (pass S over r0 = b)
      int np = 0;
      PB_TRY(sr_pass_s(k, k->r, k->d_st, &np, 0));
      PB_TRY(cg_sr_finalize(ctx, sr_region(ctx, 0), np, k->d_st, k->d_hist, k->h_done_dev, -1,
                            true));
    }
  }
  return PB_OK;
}

// Unfused iteration for operators without a stencil engine (PB_OP_COMPACT): one vector pass
// for p, the operator, a dot pass, an x/r pass (same device scalar logic as the fused path).
static int enqueue_generic_iteration(pb_ksp* k) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  double* p = k->pb[0];
  int np = 0;
  PB_TRY(launch_cg_generic_p(g, k->r, p, k->d_st));
  {
    OpApplySkip guard(ctx, &k->d_st->done);
    PB_TRY(op_apply_raw(k->A, p, k->w));
  }
  PB_TRY(launch_cg_generic_dot(g, p, k->w, k->d_st, &np));
  PB_TRY(cg_finalize_pass_a(ctx, np, k->d_st));
  PB_TRY(launch_cg_generic_xr(g, p, k->w, k->x->d, k->r, k->d_st, &np));
  return cg_finalize_stage2(ctx, np, k->d_st, k->d_hist, k->h_done_dev, k->host_iter);
}

// Preconditioned iteration (SOR / MG): p = (z - mu) + b/b0 p, w = A p, p.w, x/r update,
// z = M^-1 r, sums of z -- PETSc KSPSolve_CG order with PC_LEFT and the null-space shift.
static int enqueue_pc_iteration(pb_ksp* k) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  double* p = k->pb[0];
  int np = 0;
  const int first = k->lazy0 && k->host_iter == 0;  // r0 = b, x0 = 0, p0 = 0 implicit
  if (k->A->kind == PB_OP_COMPACT && (compact_cg_fusable(g) || compact_cg_fusable_split(g))) {
    // the compact operator forms p in its Z pass (split grids: in the pack of the z -> y
    // transpose) and takes p . w in its X pass (CgFuse): two vector passes fewer (cg_gen_p,
    // cg_gen_dot), 16 B/DoF less per iteration
    CgFuse cf;
    cf.z = k->z;
    cf.p_old = p;
    cf.p_out = p;
    cf.st = k->d_st;
    cf.first = first;
    cf.dot_p = p;
    {
      OpApplySkip guard(ctx, &k->d_st->done);
      struct Set {
        pb_ctx* c;
        ~Set() { c->cg_fuse = nullptr; }
      } set{ctx};
      ctx->cg_fuse = &cf;
      PB_TRY(op_apply_raw(k->A, p, k->w));
    }
    np = cf.nparts;
    if (!cf.fused_z) {
      // a pass did not take the fusion (a launch shape the predicate cannot see): the operator
      // ran on p_old -- form p and apply again, unfused
      PB_TRY(launch_cg_generic_p(g, k->z, p, k->d_st, first));
      OpApplySkip guard(ctx, &k->d_st->done);
      PB_TRY(op_apply_raw(k->A, p, k->w));
    }
    if (!cf.fused_z || !cf.fused_dot) PB_TRY(launch_cg_generic_dot(g, p, k->w, k->d_st, &np));
  } else {
    PB_TRY(launch_cg_generic_p(g, k->z, p, k->d_st, first));  // dinv = 1: z - mu
    {
      OpApplySkip guard(ctx, &k->d_st->done);
      PB_TRY(op_apply_raw(k->A, p, k->w));
    }
    PB_TRY(launch_cg_generic_dot(g, p, k->w, k->d_st, &np));
  }
  PB_TRY(cg_finalize_pass_a(ctx, np, k->d_st));
  const double* r_in = first ? k->b->d : k->r;
  const int rupd = tune("fft_rupd", 1);
  // unpreconditioned norm: sum r^2 is taken where r is formed, in cg_pc_xr's registers -- the
  // spectral PC's fused r update has no sum of its own and gives way to the unfused pair
  RrParts rr;
  const bool unp = k->norm_unp();
  if (k->fft && rupd && fftpc_fuses_r_update(k->fft) && !unp) {
    // r = r_in - alpha w formed by the spectral PC's first pass as it loads r, x = x + alpha p
    // beside it (8 B/DoF and one vector pass fewer)
    const RUpdate ru{r_in, k->w, k->r, p, k->x->d, first, k->d_st};
    np = 0;
    PB_TRY(fftpc_apply(k->fft, k->r, k->z, &k->d_st->done, k->d_st, &np, &ru));
  } else {
    PB_TRY(launch_cg_pc_xr(g, p, k->w, k->x->d, r_in, k->r, k->d_st, first, unp ? &rr : nullptr));
    PB_TRY(pc_apply_dev(k, k->r, k->z, &k->d_st->done, &np));
  }
  if (np == 0) PB_TRY(launch_cg_pc_sums(g, k->z, k->r, k->d_st, &np));
  return cg_finalize_stage2(ctx, np, k->d_st, k->d_hist, k->h_done_dev, k->host_iter, rr);
}

// the single-reduction iteration's two partial-sum regions (5 wide): iteration n of a batch
// writes region n & 1 and its folded prologue reduces region (n - 1) & 1, so a launch never
// overwrites the partials its own blocks may still be reading (part_off in 5-wide blocks)
static int64_t sr_region_off(const pb_ctx* ctx, int64_t n) {
  return (n & 1) * (ctx->partials_cap / 10);
}
static const double* sr_region(const pb_ctx* ctx, int64_t n) {
  return ctx->d_partials + sr_region_off(ctx, n) * 5;
}

// pass S over r (t = dinv r - mu of state st): split grids exchange r's boundary planes (raw;
// the loader transforms ghosts too) under the interior planes. Every launch is bounded by the
// end of region n & 1 (a grid that does not fit is PB_ERR_UNSUPPORTED, not a spill into the
// region the next prologue reads)
static int sr_pass_s(pb_ksp* k, const double* r, const CgState* st, int* nparts, int64_t n) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const Star s = star_of(k->A);
  StencilPlanes gp;
  const int off = (int)sr_region_off(ctx, n);
  const int end = off + (int)(ctx->partials_cap / 10);
  if (!ctx->split) {
    gp = wrap_planes();
    return launch_cg_sr_pass_s(g, s, r, gp, st, PLANES_ALL, off, end, nparts);
  }
  gp.ghost_lo = g->ghost_lo;
  gp.ghost_hi = g->ghost_hi;
  const double* hi = r + (g->nzl - 1) * g->plane;
  if (g->nzl < 3) {
    PB_TRY(halo_exchange(g, r, hi));
    return launch_cg_sr_pass_s(g, s, r, gp, st, PLANES_ALL, off, end, nparts);
  }
  int nb1 = 0, nb2 = 0;
  ScopedTimer tm(ctx, "cg_sr_s");
  PB_TRY(halo_begin(g, r, hi));
  PB_TRY(launch_cg_sr_pass_s(g, s, r, gp, st, PLANES_INTERIOR, off, end, &nb1));
  PB_TRY(halo_end(g));
  PB_TRY(launch_cg_sr_pass_s(g, s, r, gp, st, PLANES_BOUNDARY, off + nb1, end, &nb2));
  *nparts = nb1 + nb2;
  return PB_OK;
}

// One single-reduction iteration (PETSc KSPSolve_CG_SingleReduction): pass P, pass S, and -- unless
// folded into the next pass P's prologue (one rank) -- the reduction + residual-sum stage.
// n = the iteration's index inside this pb_ksp_iterate batch (state slot parity).
static int enqueue_sr_iteration(pb_ksp* k, bool fold, int64_t n) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const Star s = star_of(k->A);
  const int64_t i = k->host_iter;
  const int ns = k->pslots();
  const double* p_prev[3] = {k->pb[i % ns], k->pb[(i + ns - 1) % ns], k->pb[(i + ns - 2) % ns]};
  double* p_new = k->pb[(i + 1) % ns];
  double* r = k->rbuf(i);
  double* r_out = k->rbuf(i + 1);
  // one rank: the state alternates between the slots by the batch index's parity; split grids:
  // slot 0 holds the state after the residual-sum stage (written by the boundary-plane kernel's
  // folded prologue, or copied there unfolded), slot 1 after the top of the iteration (pass P)
  CgState* st_in = ctx->split ? k->d_st : k->d_st + (n & 1);
  CgState* st_out = ctx->split ? k->d_st + 1 : k->d_st + ((n + 1) & 1);
  SrFold f;
  f.fold_sums = fold && n > 0 && !ctx->split;
  f.nparts_s = k->sr.nparts;
  f.parts = sr_region(ctx, n - 1);
  f.in = st_in;
  f.out = st_out;
  f.hist = k->d_hist;
  f.h_done = k->h_done_dev;
  StencilPlanes gp;
  // one pass per iteration where it applies: one rank, depth-4 x deferral; the iterations that
  // carry the x update run the two passes (pass P's x-update form streams at the copy rate)
  if (cg_sr1_supported(g) && k->defer_x == 4 && i % 4 != 3) {
    PB_TRY(launch_cg_sr1(g, s, r, p_prev[0], p_new, r_out, f, f.parts, const_cast<double*>(sr_region(ctx, n)), i,
                         &k->sr.nparts));
    if (!fold)
      PB_TRY(cg_sr_finalize(ctx, sr_region(ctx, n), k->sr.nparts, st_out, k->d_hist,
                            k->h_done_dev, i));
    return PB_OK;
  }
  if (!ctx->split) {
    gp = wrap_planes();
    PB_TRY(launch_cg_sr_pass_p(g, s, r, p_prev, p_new, k->x->d, r_out, gp, f, PLANES_ALL, i,
                               k->defer_x));
  } else {
    // p's boundary planes -> halo, under the interior planes. Folded: the boundary-plane kernel
    // first runs the previous iteration's residual-sum stage from pass S's allreduced sums (a
    // one-block partial, slot 1 -> slot 0); pass P then runs the top (slot 0 -> slot 1)
    Fold fb;
    if (fold && n > 0) {
      fb.stage = 2;
      fb.nparts = 1;
      fb.width = 5;
      fb.parts = ctx->d_scalars;
      fb.in = k->d_st + 1;
      fb.out = k->d_st;
      fb.hist = k->d_hist;
      fb.h_done = k->h_done_dev;
      fb.host_iter = i - 1;
    }
    gp.ghost_lo = g->ghost_lo;
    gp.ghost_hi = g->ghost_hi;
    PB_TRY(launch_cg_boundary(g, r, p_prev[0], st_in, fb));
    if (g->nzl < 3) {
      PB_TRY(halo_exchange(g, g->bnd_lo, g->bnd_hi));
      PB_TRY(launch_cg_sr_pass_p(g, s, r, p_prev, p_new, k->x->d, r_out, gp, f, PLANES_ALL, i,
                                 k->defer_x));
    } else {
      ScopedTimer tm(ctx, "cg_sr_p_split");
      PB_TRY(halo_begin(g, g->bnd_lo, g->bnd_hi));
      PB_TRY(launch_cg_sr_pass_p(g, s, r, p_prev, p_new, k->x->d, r_out, gp, f, PLANES_INTERIOR,
                                 i, k->defer_x));
      PB_TRY(halo_end(g));
      PB_TRY(launch_cg_sr_pass_p(g, s, r, p_prev, p_new, k->x->d, r_out, gp, f, PLANES_BOUNDARY,
                                 i, k->defer_x));
    }
  }
  PB_TRY(sr_pass_s(k, r_out, st_out, &k->sr.nparts, n));
  if (fold && ctx->split) return cg_reduce_allreduce(ctx, sr_region(ctx, n), k->sr.nparts, 5);
  if (!fold)
    PB_TRY(cg_sr_finalize(ctx, sr_region(ctx, n), k->sr.nparts, st_out, k->d_hist,
                          k->h_done_dev, i));
  if (!fold && ctx->split)  // the next boundary-plane kernel reads slot 0
    PB_HIP(hipMemcpyAsync(k->d_st, st_out, sizeof(CgState), hipMemcpyDeviceToDevice,
                          ctx->stream));
  return PB_OK;
}

// fold: the finalize steps run in the passes' prologues (one rank, Jacobi; fold_a = pass A also
// folds, i.e. this is not the first iteration of the batch)
static int enqueue_iteration(pb_ksp* k, bool fold, bool fold_a) {
  if (!fused_kind(k->A->kind))
    return k->stored_z() ? enqueue_pc_iteration(k) : enqueue_generic_iteration(k);
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const Star s = star_of(k->A);
  const int64_t i = k->host_iter;  // == device iteration index until convergence
  const int ns = k->pslots();
  double* p_old = k->pb[i % ns];
  double* p_new = k->pb[(i + 1) % ns];
  // p of iterations i-1, i-2, i-3 (depth-4 deferral reads all three at i % 4 == 3)
  const double* p_prev[3] = {p_old, k->pb[(i + ns - 1) % ns], k->pb[(i + ns - 2) % ns]};
  // Jacobi: pass A builds z = dinv*r - mu on the fly; SOR / MG: z is stored (dinv = 1)
  double* r = k->rbuf(i);
  const double* zsrc = k->stored_z() ? k->z : r;
  // Jacobi / none: pass A read-only, pass B stores p and the residual into the other buffer
  PStore ps;
  if (k->pst) {
    ps.zsrc = zsrc;
    ps.r_out = k->rbuf(i + 1);
  }
  const bool store_a = !k->pst;
  StencilPlanes gp;
  int nparts = 0;
  const bool fold_split = fold && ctx->split;
  if (fold && !ctx->split) {
    gp = wrap_planes();
    if (fold_a)
      PB_TRY(launch_cg_pass_a_folded(g, s, zsrc, p_old, p_new, gp, k->d_st, k->fold_nparts_b,
                                     k->d_hist, k->h_done_dev, i, &nparts, store_a));
    else
      PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_ALL, 0, &nparts,
                              store_a));
    return launch_cg_pass_b_folded(g, s, p_new, p_prev, k->x->d, r, gp, k->d_st, nparts, i,
                                   k->defer_x, &k->fold_nparts_b, ps);
  }
  if (fold_split) {
    // split grids, folded (r05): the previous iteration's stage 2 runs in the prologues of the
    // boundary-plane kernel and pass A (from pass B's allreduced sums, a one-block partial), stage
    // 1 in pass B's (from pass A's); only the reductions before each allreduce stay separate
    // launches (bit-identical to unfolded)
    Fold fb;
    if (fold_a) {
      fb.stage = 2;
      fb.nparts = 1;
      fb.width = 4;
      fb.parts = ctx->d_scalars;
      fb.in = k->d_st + 1;
      fb.out = k->d_st;
      fb.hist = k->d_hist;
      fb.h_done = k->h_done_dev;
      fb.host_iter = i - 1;
    }
    gp.ghost_lo = g->ghost_lo;
    gp.ghost_hi = g->ghost_hi;
    if (g->nzl >= 3) {
      // the boundary-plane kernel runs on the comm stream ahead of the exchange, beside pass A's
      // interior planes, from the stage-2 state in its registers; pass A's interior launch runs the
      // same stage 2 in its prologue and writes the state (the boundary launch reads it)
      Fold fbr = fb;
      fbr.out = nullptr;
      fbr.hist = nullptr;
      fbr.h_done = nullptr;
      int nb1 = 0, nb2 = 0;
      ScopedTimer tm(ctx, "cg_pass_a");
      PB_TRY(halo_begin_after(g, g->bnd_lo, g->bnd_hi, [&](hipStream_t sm) {
        return launch_cg_boundary(g, zsrc, p_old, k->d_st, fbr, sm);
      }));
      if (fold_a)
        PB_TRY(launch_cg_pass_a_fold(g, s, zsrc, p_old, p_new, gp, fb, PLANES_INTERIOR, 0, &nb1,
                                     store_a));
      else
        PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_INTERIOR, 0, &nb1,
                                store_a));
      if (ctx->comm) {
        // the two boundary planes on the comm stream right after the exchange (beside the
        // interior planes), from the stage-2 state in registers as well
        EngineOn eo(ctx, ctx->comm_stream);
        if (fold_a)
          PB_TRY(launch_cg_pass_a_fold(g, s, zsrc, p_old, p_new, gp, fbr, PLANES_BOUNDARY, nb1,
                                       &nb2, store_a));
        else
          PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_BOUNDARY, nb1,
                                  &nb2, store_a));
        PB_HIP(hipEventRecord(ctx->ev_done, ctx->comm_stream));
        PB_TRY(halo_end(g));
      } else {
        PB_TRY(halo_end(g));
        PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_BOUNDARY, nb1,
                                &nb2, store_a));
      }
      nparts = nb1 + nb2;
    } else {
      PB_TRY(launch_cg_boundary(g, zsrc, p_old, k->d_st, fb));
      PB_TRY(halo_exchange(g, g->bnd_lo, g->bnd_hi));
      PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_ALL, 0, &nparts,
                              store_a));
    }
    PB_TRY(cg_reduce_allreduce(ctx, nparts, 1, false));
    PB_TRY(launch_cg_pass_b_folded(g, s, p_new, p_prev, k->x->d, r, gp, k->d_st, 1, i,
                                   k->defer_x, &k->fold_nparts_b, ps, ctx->d_scalars));
    return cg_reduce_allreduce(ctx, k->fold_nparts_b, 4, true);
  }
  if (!ctx->split) {
    // periodic wrap read in place: pass A combines r, p_old of the wrap planes itself and pass B
    // reads p_new's wrap planes (no boundary-plane kernel on one rank)
    gp = wrap_planes();
    PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_ALL, 0, &nparts,
                            store_a));
  } else if (g->nzl < 3) {
    PB_TRY(launch_cg_boundary(g, zsrc, p_old, k->d_st));
    PB_TRY(halo_exchange(g, g->bnd_lo, g->bnd_hi));
    gp.ghost_lo = g->ghost_lo;
    gp.ghost_hi = g->ghost_hi;
    PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_ALL, 0, &nparts,
                            store_a));
  } else {
    // the p-plane halo exchange (RCCL, comm stream) overlaps pass A's interior planes
    PB_TRY(launch_cg_boundary(g, zsrc, p_old, k->d_st));
    gp.ghost_lo = g->ghost_lo;
    gp.ghost_hi = g->ghost_hi;
    int nb1 = 0, nb2 = 0;
    ScopedTimer tm(ctx, "cg_pass_a");  // the whole pass A (both launches and the wait)
    PB_TRY(halo_begin(g, g->bnd_lo, g->bnd_hi));
    PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_INTERIOR, 0, &nb1,
                            store_a));
    PB_TRY(halo_end(g));
    PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_BOUNDARY, nb1, &nb2,
                            store_a));
    nparts = nb1 + nb2;
  }
  PB_TRY(cg_finalize_pass_a(ctx, nparts, k->d_st));
  // (unpreconditioned norm with a stored-z PC: pass B's own four sums of t = r - mu, kept in the
  // second partial region, give sum r^2 to the stage below)
  RrParts rr;
  PB_TRY(launch_cg_pass_b(g, s, p_new, p_prev, k->x->d, r, gp, k->d_st, k->d_hist,
                          k->h_done_dev, i, k->defer_x, !k->stored_z(), ps,
                          k->stored_z() && k->norm_unp() ? &rr : nullptr));
  if (k->stored_z()) {  // z = M^-1 r, then the residual sums over z
    int np = 0;
    PB_TRY(pc_apply_dev(k, r, k->z, &k->d_st->done, &np));
    if (np == 0) PB_TRY(launch_cg_pc_sums(g, k->z, r, k->d_st, &np));
    PB_TRY(cg_finalize_stage2(ctx, np, k->d_st, k->d_hist, k->h_done_dev, i, rr));
  }
  return PB_OK;
}

int pb_ksp_iterate(pb_ksp* k, int64_t iters) {
  PB_CHECK_ARG(k, "ksp is NULL");
  PB_TRY(preonly_split_form(k));
  if (!k->begun) return set_error(PB_ERR_STATE, "pb_ksp_iterate before pb_ksp_begin");
  pb_ctx* ctx = k->A->grid->ctx;
  const int C = k->opts.check_every;
  const int R = 4 * C;
  if ((int)k->ring.size() < R) {
    for (int i = (int)k->ring.size(); i < R; ++i) {
      hipEvent_t e;
      PB_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      k->ring.push_back(e);
    }
  }
  PB_TRY(ensure_done_cap(k, k->host_iter + iters + 2));
  // one rank, Jacobi, fused operator: the finalize steps ride in the passes' prologues
  // (PB_CG_FOLD=0 keeps the separate finalize launches)
  const bool fold = C >= 2 && !k->rich() && !k->fgmres() && !k->pipecg() &&
                    fused_kind(k->A->kind) &&
                    !k->stored_z() && tune("cg_fold", 1) != 0;
  const bool none = k->norm_none();
  int64_t n = 0;
  for (; n < iters && !k->stopped; ++n) {
    if (k->rich()) PB_TRY(enqueue_rich_iteration(k));
    else if (k->fgmres()) PB_TRY(enqueue_fgmres_iteration(k));
    else if (k->pipecg()) PB_TRY(enqueue_pipecg_iteration(k));
    else if (k->sr.on) PB_TRY(enqueue_sr_iteration(k, fold, n));
    else PB_TRY(enqueue_iteration(k, fold, fold && n > 0));
    const int64_t hi = k->host_iter++;
    // only the iterations the poll below waits for get an event (j = 0 mod C; folded j + 1): an
    // event record between two kernels costs the stream ~6 us of idle time (measured 5.9 us per
    // iteration with one record per iteration; profiles/r02/cg_gaps_*.txt)
    if (none) continue;  // KSPConvergedSkip: no test to poll for; the caller's wait is the only one
    if (hi % C == (fold ? 1 : 0) % C)
      PB_HIP(hipEventRecord(k->ring[hi % R], ctx->stream));
    // lagged, rank-consistent poll: decide on the flag of iteration hi + 1 - C only (folded:
    // that flag is written by the next iteration's pass A, so wait for that iteration's event)
    if ((hi + 1) % C == 0 && hi + 1 >= C) {
      const int64_t j = hi + 1 - C;
      PB_TRY(wait_event(ctx, k->ring[(fold ? j + 1 : j) % R], "KSP convergence poll"));
      if (k->h_done[j + 1]) k->stopped = true;
    }
  }
  if (k->sr.on) {
    // the residual-sum stage of the batch's last iteration (folded runs), then the state back
    // into slot 0 for the next batch and the other entry points
    if (ctx->split) {  // (unfolded: the state is in slot 0 already)
      if (fold && n > 0) {
        PB_TRY(cg_stage2_from_sums(ctx, 5, k->d_st + 1, k->d_hist, k->h_done_dev,
                                   k->host_iter - 1));
        PB_HIP(hipMemcpyAsync(k->d_st, k->d_st + 1, sizeof(CgState), hipMemcpyDeviceToDevice,
                              ctx->stream));
      }
      return PB_OK;
    }
    if (fold && n > 0)
      PB_TRY(cg_sr_finalize(ctx, sr_region(ctx, n - 1), k->sr.nparts, k->d_st + (n & 1),
                            k->d_hist, k->h_done_dev, k->host_iter - 1));
    if (n & 1)
      PB_HIP(hipMemcpyAsync(k->d_st, k->d_st + 1, sizeof(CgState), hipMemcpyDeviceToDevice,
                            ctx->stream));
    return PB_OK;
  }
  if (fold && n > 0)
    PB_TRY(cg_fold_tail(ctx, k->fold_nparts_b, k->d_st, k->d_hist, k->h_done_dev,
                        k->host_iter - 1));
  return PB_OK;
}

static const char* reason_name(int r) {
  switch (r) {
    case PB_KSP_CONVERGED_RTOL: return "CONVERGED_RTOL";
    case PB_KSP_CONVERGED_ATOL: return "CONVERGED_ATOL";
    case PB_KSP_CONVERGED_ITS: return "CONVERGED_ITS";
    case PB_KSP_DIVERGED_ITS: return "DIVERGED_ITS";
    case PB_KSP_DIVERGED_DTOL: return "DIVERGED_DTOL";
    case PB_KSP_DIVERGED_NANORINF: return "DIVERGED_NANORINF";
    case PB_KSP_DIVERGED_INDEFINITE_MAT: return "DIVERGED_INDEFINITE_MAT";
    case PB_KSP_DIVERGED_INDEFINITE_PC: return "DIVERGED_INDEFINITE_PC";
    case PB_KSP_DIVERGED_BREAKDOWN: return "DIVERGED_BREAKDOWN";
    case PB_KSP_CONVERGED_HAPPY_BREAKDOWN: return "CONVERGED_HAPPY_BREAKDOWN";
    default: return "CONVERGED_ITERATING";
  }
}

int pb_ksp_end(pb_ksp* k, pb_ksp_result* res, double* history, int64_t cap) {
  PB_CHECK_ARG(k, "ksp is NULL");
  PB_TRY(preonly_split_form(k));
  if (!k->begun) return set_error(PB_ERR_STATE, "pb_ksp_end before pb_ksp_begin");
  pb_ctx* ctx = k->A->grid->ctx;
  PB_SYNC(ctx, "pb_ksp_end");
  if (k->lazy0 && k->host_iter == 0) {  // stopped at the setup: x = x0 = 0 was never written
    PB_HIP(hipMemsetAsync(k->x->d, 0, (size_t)k->A->grid->nlocal * sizeof(double), ctx->stream));
  }
  if (k->fgmres()) PB_TRY(fgmres_finish(k));  // x += the directions of the last cycle
  CgState st;
  PB_HIP(hipMemcpyAsync(&st, k->d_st, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
  PB_SYNC(ctx, "pb_ksp_end");
  if (k->rich()) PB_TRY(rich_copy_back(k, st.its));
  if (!k->rich() && st.pend_iter >= 0) {  // apply the still-deferred alpha_m p_m (p_m lives in pb[(m+1) % ns])
    const int ns = k->pslots();
    for (int64_t m = 0; m < st.pend_count; ++m)
      PB_TRY(launch_cg_flush(k->A->grid, k->x->d, k->pb[(st.pend_iter + m + 1) % ns], st.pa[m]));
    PB_SYNC(ctx, "pb_ksp_end");
  }
  if (res) {
    res->reason = st.reason;
    res->its = st.its;
    res->rnorm = st.dp;
    res->rnorm0 = st.rnorm0;
    res->nhist = std::min<int64_t>(st.nlog, k->nhist);
  }
  // only the norms the device logged (a breakdown exit leaves the last iteration without one)
  const int64_t nh = std::min<int64_t>(st.nlog, k->nhist);
  std::vector<double> hist((size_t)std::max<int64_t>(nh, 1));
  if (nh > 0) {
    PB_HIP(hipMemcpyAsync(hist.data(), k->d_hist, (size_t)nh * sizeof(double), hipMemcpyDeviceToHost,
                          ctx->stream));
    PB_SYNC(ctx, "pb_ksp_end");
  }
  if (history && cap > 0) memcpy(history, hist.data(), (size_t)std::min(nh, cap) * sizeof(double));
  if (ctx->rank == 0) {
    if (k->opts.monitor)
      for (int64_t i = 0; i < nh; ++i)
        printf("  %3lld KSP Residual norm %14.12e \n", (long long)i, hist[i]);
    if (k->opts.converged_reason) {
      if (st.reason > 0)
        printf("Linear solve converged due to %s iterations %lld\n", reason_name(st.reason),
               (long long)st.its);
      else
        printf("Linear solve did not converge due to %s iterations %lld\n",
               reason_name(st.reason), (long long)st.its);
    }
    fflush(stdout);
  }
  k->begun = false;
  return PB_OK;
}

int pb_ksp_solve(pb_ksp* k, const pb_vec* b, pb_vec* x, pb_ksp_result* res, double* history,
                 int64_t cap) {
  PB_CHECK_ARG(k, "ksp is NULL");
  ScopedTimer tm(k->A->grid->ctx, "KSPSolve");
  if (k->opts.ksp_type == PB_KSP_PREONLY) return solve_preonly(k, b, x, res);
  if (k->opts.guess_type != PB_GUESS_NONE) return solve_projected(k, b, x, res, history, cap);
  PB_TRY(pb_ksp_begin(k, b, x));
  PB_TRY(pb_ksp_iterate(k, k->solve_iters()));
  return pb_ksp_end(k, res, history, cap);
}

int pb_ksp_destroy(pb_ksp* k) {
  if (!k) return PB_OK;
  (void)wait_stream(k->A->grid->ctx, k->A->grid->ctx->stream, "pb_ksp_destroy");
  field_free(k->r);
  field_free(k->r2);
  for (double* p : k->pb) field_free(p);
  field_free(k->w);
  field_free(k->z);
  field_free(k->ri.x2);
  field_free(k->ri.x3);
  fgmres_destroy(k);
  pipecg_destroy(k);
  if (k->mg) mg_destroy(k->mg);
  fftpc_destroy(k->fft);
  if (k->fg) {
    for (double* p : k->fg->xt) field_free(p);
    for (double* p : k->fg->bt) field_free(p);
    field_free(k->fg->guess);
    if (k->fg->d_coef) (void)hipFree(k->fg->d_coef);
    delete k->fg;
  }
  if (k->d_st) (void)hipFree(k->d_st);
  if (k->d_hist) (void)hipFree(k->d_hist);
  if (k->h_done) (void)hipHostFree(k->h_done);
  for (hipEvent_t e : k->ring) (void)hipEventDestroy(e);
  delete k;
  return PB_OK;
}

int pb_ksp_pc_apply(pb_ksp* k, const pb_vec* r, pb_vec* z) {
  PB_CHECK_ARG(k && r && z && r != z, "bad pc apply args");
  pb_grid* g = k->A->grid;
  PB_CHECK_ARG(r->grid == g && z->grid == g, "vector/operator grid mismatch");
  pb_ctx* ctx = g->ctx;
  if (k->mg) {
    PB_TRY(mg_apply(k->mg, r->d, z->d));
  } else if (k->fft) {
    PB_TRY(fftpc_apply(k->fft, r->d, z->d));
  } else {
    PB_HIP(hipMemcpyAsync(z->d, r->d, (size_t)g->nlocal * sizeof(double),
                          hipMemcpyDeviceToDevice, ctx->stream));
    if (k->opts.pc_type == PB_PC_JACOBI)
      PB_TRY(vec_update(ctx, 2, z->d, nullptr, g->nlocal, 1.0 / k->P->cc));
  }
  PB_SYNC(ctx, "pb_ksp_pc_apply");
  return PB_OK;
}

int pb_ksp_pc_levels(const pb_ksp* k, int* levels) {
  PB_CHECK_ARG(k && levels, "bad args");
  *levels = k->mg ? mg_levels(k->mg) : 0;
  return PB_OK;
}

int pb_ksp_pc_mg_set_opts(pb_ksp* k, const pb_pc_mg_opts* o) {
  PB_CHECK_ARG(k && o, "bad args");
  if (k->opts.pc_type != PB_PC_MG || !k->mg)
    return set_error(PB_ERR_STATE, "KSP created without -pc_type mg");
  if (k->begun) return set_error(PB_ERR_STATE, "pb_ksp_pc_mg_set_opts inside a solve");
  PB_TRY(check_mg_opts(o));
  MgSmoother sm;
  sm.ksp = o->levels_ksp_type;
  sm.pc = o->levels_pc_type;
  sm.nu = o->levels_ksp_max_it;
  sm.rich_scale = o->levels_richardson_scale;
  mg_levels_bounds(o, &sm.emin, &sm.emax);
  PB_TRY(mg_set_smoother(k->mg, sm));
  k->mgopts = *o;
  k->ch.state = 0;  // an outer Chebyshev's estimate belongs to the old preconditioner
  return PB_OK;
}

int pb_ksp_pc_mg_get_opts(const pb_ksp* k, pb_pc_mg_opts* o) {
  PB_CHECK_ARG(k && o, "bad args");
  if (k->opts.pc_type != PB_PC_MG || !k->mg)
    return set_error(PB_ERR_STATE, "KSP created without -pc_type mg");
  *o = k->mgopts;
  return PB_OK;
}

int pb_solve(pb_op* A, pb_op* P, const pb_ksp_opts* opts, const pb_vec* b, pb_vec* x,
             pb_ksp_result* res, double* history, int64_t cap) {
  return pb_solve_chebyshev(A, P, opts, nullptr, b, x, res, history, cap);
}

static int solve_once(pb_op* A, pb_op* P, const pb_ksp_opts* opts,
                      const pb_ksp_chebyshev_opts* cheb, const pb_pc_mg_opts* mgo, const pb_vec* b,
                      pb_vec* x, pb_ksp_result* res, double* history, int64_t cap);

int pb_solve_chebyshev(pb_op* A, pb_op* P, const pb_ksp_opts* opts,
                       const pb_ksp_chebyshev_opts* cheb, const pb_vec* b, pb_vec* x,
                       pb_ksp_result* res, double* history, int64_t cap) {
  return solve_once(A, P, opts, cheb, nullptr, b, x, res, history, cap);
}

int pb_solve_mg(pb_op* A, pb_op* P, const pb_ksp_opts* opts, const pb_pc_mg_opts* mgo,
                const pb_vec* b, pb_vec* x, pb_ksp_result* res, double* history, int64_t cap) {
  return solve_once(A, P, opts, nullptr, mgo, b, x, res, history, cap);
}

static int solve_once(pb_op* A, pb_op* P, const pb_ksp_opts* opts,
                      const pb_ksp_chebyshev_opts* cheb, const pb_pc_mg_opts* mgo, const pb_vec* b,
                      pb_vec* x, pb_ksp_result* res, double* history, int64_t cap) {
  pb_ksp* k = nullptr;
  pb_ksp_opts one;
  if (opts && opts->guess_type == PB_GUESS_FISCHER) {
    // this KSP lives for one solve and keeps no direction: one pair of vectors is enough
    PB_TRY(check_guess_opts(opts->guess_fischer_model, opts->guess_fischer_maxl));
    one = *opts;
    one.guess_fischer_maxl = 1;
    opts = &one;
  }
  PB_TRY(pb_ksp_create(A, P, opts, &k));
  int rc = cheb && k->cheb() ? pb_ksp_chebyshev_set_opts(k, cheb) : PB_OK;
  if (rc == PB_OK && mgo && k->opts.pc_type == PB_PC_MG) rc = pb_ksp_pc_mg_set_opts(k, mgo);
  if (rc == PB_OK) rc = pb_ksp_solve(k, b, x, res, history, cap);
  const std::string msg = rc != PB_OK ? pb_last_error() : "";
  pb_ksp_destroy(k);
  return rc != PB_OK ? set_error(rc, "%s", msg.c_str()) : PB_OK;
}

}  // extern "C"
