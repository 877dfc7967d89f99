// pb_solver.cpp -- the KSP driver every solver shares: pb_ksp_create / begin / iterate / end /
// solve / destroy and pb_solve*. The solvers are in their own files: -ksp_type cg in pb_ksp_cg.cpp,
// richardson | chebyshev | preonly in pb_ksp_stationary.cpp, fgmres in pb_ksp_fgmres.cpp, pipecg in
// pb_ksp_pipecg.cpp; the operator is in pb_op.cpp, the options in pb_options.cpp, the projected
// initial guess in pb_ksp_guess.cpp, -ksp_norm_type in pb_norm_type.cpp; struct pb_ksp and what
// they share in pb_ksp.hpp.
//
// All of a solver's scalars live on the device; the host never waits inside an iteration and
// polls a per-iteration "done" flag (host-mapped) every `check_every` iterations, lagged by one
// poll interval so that every rank stops after the same number of enqueued iterations.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "pb_ksp.hpp"

using namespace pb;

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

// z = M^-1 r of a stored-z preconditioner, nothing else (no sums, no null-space shift)
int pb::pc_stored_apply(pb_ksp* k, const double* r, double* z, const int* skip) {
  if (k->fft) return fftpc_apply(k->fft, r, z, skip);
  if (k->mg) return mg_apply(k->mg, r, z, skip);
  // the Jacobi PC of a variable P: the reciprocal diagonal of P as it is now
  pb_grid* g = k->P->grid;
  if (!k->vj.dinv && field_alloc(&k->vj.dinv, (size_t)g->nlocal * sizeof(double)) != hipSuccess)
    return set_error(PB_ERR_ALLOC, "Jacobi diagonal: out of device memory");
  if (k->vj.seen != k->P->change) {
    PB_TRY(launch_varcoef_diag(g, varcoef_of(k->P), k->vj.dinv, true));
    k->vj.seen = k->P->change;
  }
  return launch_varcoef_jacobi(g, k->vj.dinv, r, z, skip);
}

// z = M^-1 r for the stored-z preconditioners; *np = residual-sum partial blocks written by the
// PC itself (MG's last sweep), 0 if the caller must take the sums
int pb::pc_apply_dev(pb_ksp* k, const double* r, double* z, const int* skip, int* np) {
  *np = 0;
  if (k->vj.on) return pc_stored_apply(k, r, z, skip);
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
  if (P->kind == PB_OP_VARCOEF && (pc == PB_PC_SOR || pc == PB_PC_MG || pc == PB_PC_FFT))
    return fail(set_error(PB_ERR_UNSUPPORTED,
                          "-pc_type sor / mg / fft cannot be built from a PB_OP_VARCOEF P: pass a "
                          "constant-coefficient P (PB_OP_STAR7 or PB_OP_ASSEMBLED27) for the "
                          "preconditioner, or use -pc_type jacobi / none"));
  k->vj.on = P->kind == PB_OP_VARCOEF && pc == PB_PC_JACOBI;
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

static int preonly_split_form(const pb_ksp* k) {
  if (k && k->opts.ksp_type == PB_KSP_PREONLY)
    return set_error(PB_ERR_UNSUPPORTED,
                     "-ksp_type preonly has no split form: use pb_ksp_solve or pb_solve");
  return PB_OK;
}

// A with the mass term on (pb_op_set_mass) is nonsingular: the constant null space must not be
// projected out of its solves. A alone is read: a mass in P or in the PC's coefficient operator
// only makes a nonsingular preconditioner of a singular A
static int mass_nullspace(const pb_ksp* k) {
  if (k->A->mass_on() && k->opts.nullspace != 0)
    return set_error(PB_ERR_STATE,
                     "A has a mass term (pb_op_set_mass, s != 0) and is nonsingular: create the "
                     "KSP with nullspace = 0");
  return PB_OK;
}

int pb_ksp_begin(pb_ksp* k, const pb_vec* b, pb_vec* x) {
  PB_CHECK_ARG(k && b && x, "bad begin args");
  PB_TRY(preonly_split_form(k));
  PB_TRY(mass_nullspace(k));
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
  st.pc = k->vj.on ? (int)PC_JACOBI_FIELD : k->opts.pc_type;
  st.nullspace = k->opts.nullspace;
  st.norm = k->norm();
  // PCJacobi stores the reciprocal of diag(P) (src/coefficients.f90:44-46 centre coefficient);
  // with SOR / MG the sums are taken over z = M^-1 r itself (dinv = 1)
  st.dinv = k->opts.pc_type == PB_PC_JACOBI && !k->vj.on ? 1.0 / k->P->cc : 1.0;
  st.ntot = (double)(g->n[0] * g->n[1] * g->n[2]);
  // (cg uploads the state itself, with the form of this solve's iteration in it)
  if (!k->cg())
    PB_HIP(hipMemcpyAsync(k->d_st, &st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
  if (k->rich()) PB_TRY(rich_begin(k, b, x));
  else if (k->fgmres()) PB_TRY(fgmres_begin(k, b, x));
  else if (k->pipecg()) PB_TRY(pipecg_begin(k, b, x));
  else PB_TRY(cg_begin(k, b, x, st));
  PB_SYNC(ctx, "pb_ksp_begin");
  k->b = b;
  k->x = x;
  k->host_iter = 0;
  k->stopped = k->h_done[0] != 0;
  if (!k->begun) {  // (pb_op_set_coefficient is PB_ERR_STATE until pb_ksp_end)
    ++k->A->in_solve;
    if (k->P != k->A) ++k->P->in_solve;
    if (pb_op* c = k->pc_coef()) ++c->in_solve;
  }
  k->begun = true;
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
  const bool fold = C >= 2 && k->cg() && fused_kind(k->A->kind) && !k->stored_z() &&
                    tune("cg_fold", 1) != 0;
  const bool none = k->norm_none();
  int64_t n = 0;
  for (; n < iters && !k->stopped; ++n) {
    if (k->rich()) PB_TRY(enqueue_rich_iteration(k));
    else if (k->fgmres()) PB_TRY(enqueue_fgmres_iteration(k));
    else if (k->pipecg()) PB_TRY(enqueue_pipecg_iteration(k));
    else PB_TRY(enqueue_cg_iteration(k, fold, n));
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
  return k->cg() ? cg_batch_end(k, fold, n) : PB_OK;
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
  if (k->fgmres()) PB_TRY(fgmres_finish(k));  // x += the directions of the last cycle
  CgState st;
  PB_HIP(hipMemcpyAsync(&st, k->d_st, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
  PB_SYNC(ctx, "pb_ksp_end");
  if (k->rich()) PB_TRY(rich_copy_back(k, st.its));
  if (k->cg()) PB_TRY(cg_finish(k, st));  // the deferred part of the x update
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
  --k->A->in_solve;
  if (k->P != k->A) --k->P->in_solve;
  if (pb_op* c = k->pc_coef()) --c->in_solve;
  k->begun = false;
  return PB_OK;
}

int pb_ksp_solve(pb_ksp* k, const pb_vec* b, pb_vec* x, pb_ksp_result* res, double* history,
                 int64_t cap) {
  PB_CHECK_ARG(k, "ksp is NULL");
  PB_TRY(mass_nullspace(k));
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
  if (k->begun) {  // destroyed inside a solve: the operators are free again
    --k->A->in_solve;
    if (k->P != k->A) --k->P->in_solve;
    if (pb_op* c = k->pc_coef()) --c->in_solve;
  }
  field_free(k->r);
  field_free(k->r2);
  for (double* p : k->pb) field_free(p);
  field_free(k->w);
  field_free(k->z);
  field_free(k->ri.x2);
  field_free(k->ri.x3);
  field_free(k->vj.dinv);
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
  if (k->stored_z()) {
    PB_TRY(pc_stored_apply(k, r->d, z->d));
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
  if (k->coef && o->levels_pc_type == PB_MG_LEVELS_JACOBI)
    return set_error(PB_ERR_UNSUPPORTED,
                     "a Jacobi-type level smoother with pb_ksp_pc_set_coefficient_from: the "
                     "variable-coefficient levels smooth with -mg_levels_pc_type sor");
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

int pb_ksp_pc_set_coefficient_from(pb_ksp* k, const pb_op* C) {
  PB_CHECK_ARG(k, "ksp is NULL");
  if (!k->mg)
    return set_error(PB_ERR_STATE,
                     "pb_ksp_pc_set_coefficient_from needs -pc_type sor or mg (the spectral PC "
                     "cannot diagonalise a variable operator; Jacobi takes a PB_OP_VARCOEF P)");
  if (k->begun) return set_error(PB_ERR_STATE, "pb_ksp_pc_set_coefficient_from inside a solve");
  if (C) {
    PB_CHECK_ARG(C->kind == PB_OP_VARCOEF, "the coefficient comes from a PB_OP_VARCOEF operator");
    PB_CHECK_ARG(C->grid == k->A->grid, "coefficient operator and KSP on different grids");
    if (k->mgopts.levels_pc_type == PB_MG_LEVELS_JACOBI)
      return set_error(PB_ERR_UNSUPPORTED,
                       "pb_ksp_pc_set_coefficient_from with a Jacobi-type level smoother: the "
                       "variable-coefficient levels smooth with -mg_levels_pc_type sor");
  }
  PB_TRY(mg_set_coefficient(k->mg, C));
  k->coef = C;
  k->ch.state = 0;  // an outer Chebyshev's estimate belongs to the old preconditioner
  return PB_OK;
}

int pb_ksp_pc_get_coefficient_from(const pb_ksp* k, const pb_op** C) {
  PB_CHECK_ARG(k && C, "bad args");
  *C = k->coef;
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
