// pb_mg.cpp -- the multigrid preconditioner's host path: the hierarchy (mg_create), the level plan
// and the V-cycle driver. One apply reads the tunings once (mg_tunings), plans every level once
// (level_plan) and runs down legs, the coarse solve or the one-launch tail, and up legs; a leg
// switches on its level's plan and calls launchers (pb_mg.hpp, pb_internal.hpp). No kernel is named
// here. The level smoothers (-mg_levels_*, Mg::custom()) run the same driver under a plan with
// every fusion, the tail and the agglomeration off (restated in tests/mg_smoothers_restatement.py);
// so do the variable-coefficient levels (mg_set_coefficient; their kernels: pb_mg_varcoef.hip,
// restated in tests/varcoef_mg_restatement.py).
#include <algorithm>
#include <cmath>

#include "pb_mg.hpp"

namespace pb {

int mg_plan_levels(const int64_t n[3], int nranks, int levels_req) {
  std::vector<int64_t> k0(nranks), nz(nranks);
  for (int r = 0; r < nranks; ++r) pb_slab_partition(n[2], nranks, r, &k0[r], &nz[r]);
  int64_t cur[3] = {n[0], n[1], n[2]};
  int L = 1;
  const int cap = levels_req > 0 ? levels_req : 64;
  while (L < cap) {
    bool ok = true;
    for (int d = 0; d < 3; ++d) ok = ok && cur[d] % 4 == 0;  // coarse extents stay even
    if (levels_req <= 0) ok = ok && std::min(cur[0], std::min(cur[1], cur[2])) > 4;
    for (int r = 0; r < nranks; ++r) ok = ok && k0[r] % 2 == 0 && nz[r] % 2 == 0;
    if (!ok) break;
    for (int d = 0; d < 3; ++d) cur[d] /= 2;
    for (int r = 0; r < nranks; ++r) {
      k0[r] /= 2;
      nz[r] /= 2;
    }
    ++L;
  }
  return L;
}

int mg_levels(const Mg* mg) { return (int)mg->lv.size(); }

void mg_destroy(Mg* mg) {
  if (!mg) return;
  (void)wait_stream(mg->ctx, mg->ctx->stream, "mg_destroy");
  for (auto& L : mg->lv)
    if (L.own) pb_grid_destroy(L.g);
  if (mg->mem) (void)hipFree(mg->mem);
  if (mg->agg) (void)hipFree(mg->agg);
  if (mg->pmem) (void)hipFree(mg->pmem);
  if (mg->vmem) (void)hipFree(mg->vmem);
  if (mg->qmem) (void)hipFree(mg->qmem);
  delete mg;
}

// The tunings in force: read at create and at the top of every apply, nowhere else.
// mg_engine_min_plane: levels whose planes hold at least this many points run the fused / engine
// passes: 256^2 on one rank (the 128^3 level's six per-level launches beat the fused passes there,
// 0.381 vs 0.409 ms); 128^2 on decomposed grids, where every per-level pass costs a halo exchange
// (force_comm 512^3 MG-PCG 48.1 -> 47.75 ms, profiles/r04/decomposed/mg_engine_128_ab.txt).
// mg_split_fused = 0 keeps the decomposed V-cycle on the per-pass kernels
static MgTune mg_tunings(const pb_ctx* ctx) {
  MgTune t;
  t.engine_min_plane = tune("mg_engine_min_plane", ctx->split ? 128 * 128 : 256 * 256);
  t.restrict_z_min_cols = tune("mg_restrict_z_min_cols", 4096);
  t.tail_max = tune("mg_tail_max", 8192);
  t.split_fused = tune("mg_split_fused", 1) != 0;
  t.poly_fused = tune("mg_poly_fused", 1) != 0;
  // the variable-coefficient levels (measured at 512^3): the one-pass zero-start
  // pre-smoothing 1.94 ms against 2.30 ms for its two launches (their spread 0.03); the in-place
  // half-sweep 1.51 ms forming dinv from its faces against 1.66 ms reading the stored field
  t.vc_pre_fused = tune("mg_varcoef_pre_fused", 1) != 0;
  t.vc_dinv_stored = tune("mg_varcoef_dinv_stored", 0) != 0;
  t.vc_kc = tune("mg_varcoef_kc", 0);
  return t;
}

// The passes of level l under the tunings mg->tn. have_xs: the level has an xs array (mg_create
// asks with true: which levels would use one), the precondition of PostSweep.
static LevelPlan level_plan(const Mg* mg, int l, bool have_xs) {
  const MgTune& tn = mg->tn;
  const pb_grid* g = mg->lv[l].g;
  const bool split = mg->ctx->split;
  LevelPlan p;
  p.engine = g->plane >= tn.engine_min_plane;
  if (l + 1 >= (int)mg->lv.size()) return p;  // the coarsest level: the coarse solve's half-sweeps
  const pb_grid* c = mg->lv[l + 1].g;
  p.march = c->n[0] * c->n[1] >= tn.restrict_z_min_cols;
  if (mg->custom()) return p;  // the level smoothers: one launch per pass
  // large level: the two-colour passes (zero-start half-sweeps + residual; both post half-sweeps)
  const bool sweep2 = p.engine && sor_sweep2_supported(g);
  // ... and the unrolled ones that take the transfer in too; N ranks: with deep ghost planes
  // (three of b, two of xs and of the coarse x), from an even slab origin (compile-time colours)
  const bool u4 = sweep2 && (!split || (tn.split_fused && g->k0 % 2 == 0));
  if (u4 && g->nzl % 2 == 0 && (!split || g->nzl >= 3)) p.pre = LevelPlan::FusedRestrict;
  else if (sweep2) p.pre = LevelPlan::FusedResidual;
  if (u4 && have_xs && p.march && (!split || (g->nzl >= 2 && c->nzl >= 2)))
    p.post = LevelPlan::PostSweep;
  else if (sweep2 && p.march)
    p.post = LevelPlan::ProlongThenSweep2;
  return p;
}

// The first level of the one-launch tail: it and every coarser level hold at most tail_max points
// of the whole grid (what one rank owns, and what the agglomerated levels of a decomposed grid
// are gathered to), at least level 1, at most kTailMax levels. L: no tail
static int tail_first(const Mg* mg) {
  const int L = (int)mg->lv.size();
  int Lt = L;
  for (int l = L - 1; l >= 1 && mg->lv[l].size() <= mg->tn.tail_max; --l) Lt = l;
  return L - Lt > kTailMax ? L : Lt;
}

// the agglomerated coarse levels of a decomposed grid (Mg::La): the levels of the one-launch tail
// (tail_first: <= mg_tail_max points, default PB_MG_TAIL_MAX as on one rank). Only with an
// all-to-all to gather them (RCCL, or a host transport with an alltoallv callback): the built-in
// shm transport keeps the halo-exchange levels
static int mg_agglomerate_setup(Mg* mg) {
  pb_ctx* ctx = mg->ctx;
  const int L = (int)mg->lv.size();
  mg->La = 0;
  if (!ctx->split || L < 2 || !tune("mg_agglomerate", 1)) return PB_OK;
  if (!ctx->comm && !ctx->h_alltoallv) return PB_OK;
  const int La = tail_first(mg);
  if (La >= L) return PB_OK;
  const int P = ctx->nranks;
  const MgLevel& A0 = mg->lv[La];
  int64_t total = 0;
  for (int l = La; l < L; ++l) total += 3 * ((mg->lv[l].size() + 1) & ~(int64_t)1);
  const int64_t slab = A0.g->nlocal;
  total += P * slab;
  if (hipMalloc(&mg->agg, (size_t)total * sizeof(double)) != hipSuccess)
    return set_error(PB_ERR_ALLOC, "multigrid coarse levels: out of device memory");
  double* q = mg->agg;
  for (int l = La; l < L; ++l) {
    const MgLevel& v = mg->lv[l];
    const int64_t n = v.size(), n2 = (n + 1) & ~(int64_t)1;
    mg->ageo.push_back(MgGeo{(int)v.n[0], (int)v.n[1], (int)v.n[2], v.n[0] * v.n[1], n, 0});
    mg->ax.push_back(q);
    mg->ab.push_back(q + n2);
    mg->ares.push_back(q + 2 * n2);
    q += 3 * n2;
  }
  mg->agg_send = q;
  mg->agg_sc.assign(P, slab);
  mg->agg_rc.resize(P);
  for (int r = 0; r < P; ++r) {
    int64_t k0 = 0, nz = 0;
    pb_slab_partition(mg->lv[0].g->n[2], P, r, &k0, &nz);
    mg->agg_rc[r] = (nz >> La) * A0.n[0] * A0.n[1];
  }
  mg->La = La;
  return PB_OK;
}

int mg_create(pb_grid* g, const double deltas[3], int pc_type, int levels_req, int coarse_its,
              double omega, Mg** out) {
  pb_ctx* ctx = g->ctx;
  for (int d = 0; d < 3; ++d)
    if (g->n[d] % 2)
      return set_error(PB_ERR_UNSUPPORTED,
                       "red-black SOR / multigrid needs even grid extents (got %lld x %lld x %lld)",
                       (long long)g->n[0], (long long)g->n[1], (long long)g->n[2]);
  if (g->nlocal >= ((int64_t)1 << 32))
    return set_error(PB_ERR_UNSUPPORTED, "multigrid: more than 2^32 points on one GPU");
  // PETSc PCSORSetOmega rejects omega outside (0, 2); PB_SOR_OMEGA_ANY=1 (diagnostics) accepts
  // it -- an indefinite SOR preconditioner, e.g. to exercise KSP_DIVERGED_INDEFINITE_PC
  if (!(omega > 0.0 && omega < 2.0) && !tune("sor_omega_any", 0))
    return set_error(PB_ERR_ARG, "SOR omega must be in (0, 2)");
  Mg* mg = new Mg();
  mg->ctx = ctx;
  mg->omega = omega;
  mg->tn = mg_tunings(ctx);
  const int L = pc_type == PB_PC_MG ? mg_plan_levels(g->n, ctx->nranks, levels_req) : 1;
  mg->coarse_its = pc_type == PB_PC_MG ? std::max(1, coarse_its) : 1;
  mg->lv.resize(L);
  for (int l = 0; l < L; ++l) {
    MgLevel& lv = mg->lv[l];
    for (int d = 0; d < 3; ++d) {
      lv.n[d] = g->n[d] >> l;
      lv.h[d] = deltas[d] * (double)(1 << l);
    }
    lv.s = star_coeffs(lv.h);
    if (l == 0) {
      lv.g = g;
      continue;
    }
    const int rc = grid_create_part(ctx, lv.n, g->L, g->k0 >> l, g->nzl >> l, &lv.g);
    if (rc != PB_OK) {
      mg_destroy(mg);
      return rc;
    }
    lv.own = true;
  }
  // the levels' arrays: x and b below level 0, a residual above the coarsest level, and an xs on
  // the levels whose plan takes the fused post-smoothing under the tunings of now
  std::vector<double**> arrays;
  std::vector<int64_t> sizes;
  int64_t total = 0;
  for (int l = 0; l < L; ++l) {
    MgLevel& lv = mg->lv[l];
    const bool xs = level_plan(mg, l, true).post == LevelPlan::PostSweep;
    for (double** a : {l > 0 ? &lv.x : nullptr, l > 0 ? &lv.b : nullptr,
                       l < L - 1 ? &lv.res : nullptr, xs ? &lv.xs : nullptr}) {
      if (!a) continue;
      arrays.push_back(a);
      sizes.push_back(lv.g->nlocal);
      total += lv.g->nlocal;
    }
  }
  if (total > 0 && hipMalloc(&mg->mem, (size_t)total * sizeof(double)) != hipSuccess) {
    mg_destroy(mg);
    return set_error(PB_ERR_ALLOC, "multigrid levels: out of device memory");
  }
  double* p = mg->mem;
  for (size_t i = 0; i < arrays.size(); ++i) {
    *arrays[i] = p;
    p += sizes[i];
  }
  if (const int rc = mg_agglomerate_setup(mg); rc != PB_OK) {
    mg_destroy(mg);
    return rc;
  }
  *out = mg;
  return PB_OK;
}

int mg_set_smoother(Mg* mg, const MgSmoother& sm) {
  const int L = (int)mg->lv.size();
  if (sm.pc == PB_MG_LEVELS_JACOBI && !mg->pmem && L > 1) {
    int64_t total = 0;
    for (int l = 0; l < L - 1; ++l) total += 3 * mg->lv[l].g->nlocal;
    if (hipMalloc(&mg->pmem, (size_t)total * sizeof(double)) != hipSuccess)
      return set_error(PB_ERR_ALLOC, "multigrid level smoother: out of device memory");
    double* p = mg->pmem;
    for (int l = 0; l < L - 1; ++l) {
      MgLevel& lv = mg->lv[l];
      lv.t1 = p;
      lv.t2 = p + lv.g->nlocal;
      lv.r2 = p + 2 * lv.g->nlocal;
      p += 3 * lv.g->nlocal;
    }
  }
  mg->sm = sm;
  return PB_OK;
}

// C: a PB_OP_VARCOEF operator on the hierarchy's grid (checked by the caller), nullptr: back to the
// constant-coefficient levels. The levels' beta (below level 0) and dinv are allocated on the
// first call, each with two ghost planes, and filled by the next apply (vmg_build)
int mg_set_coefficient(Mg* mg, const pb_op* C) {
  if (C && !mg->vmem) {
    const int L = (int)mg->lv.size();
    int64_t total = 0;
    for (int l = 0; l < L; ++l)
      total += (l > 0 ? 2 : 1) * (mg->lv[l].g->nlocal + 2 * mg->lv[l].g->plane);
    if (hipMalloc(&mg->vmem, (size_t)total * sizeof(double)) != hipSuccess)
      return set_error(PB_ERR_ALLOC, "multigrid level coefficients: out of device memory");
    double* p = mg->vmem;
    for (int l = 0; l < L; ++l) {
      MgLevel& lv = mg->lv[l];
      const int64_t len = lv.g->nlocal + 2 * lv.g->plane;
      lv.dinv = p + lv.g->plane;
      p += len;
      if (l == 0) continue;
      lv.beta_own = p + lv.g->plane;
      p += len;
    }
  }
  mg->coef = C;
  mg->coef_seen = -1;
  return PB_OK;
}

// coarsest level: `coarse_its` symmetric red-black sweeps from zero (red, black, red, black, ...)
static int coarse_solve(Mg* mg, MgLevel& L, MgSums sums) {
  PB_TRY(level_smooth(mg, L, 0, 1));  // red from zero + black
  const int its = mg->coarse_its;
  PB_TRY(level_smooth(mg, L, 0, 0, its == 1 ? sums : MgSums{}));
  for (int it = 1; it < its; ++it) {
    PB_TRY(level_smooth(mg, L, 1, 0));
    PB_TRY(level_smooth(mg, L, 0, 0, it == its - 1 ? sums : MgSums{}));
  }
  return PB_OK;
}

// nu steps of the Jacobi-type smoother on level F. pre: from zero, every step with its residual
// (the last one's is the V-cycle's); *ycur, *rcur = where the iterate and its residual ended up.
// post: from *ycur (its residual taken first), the last step stores no residual and writes F.x.
static int poly_smooth(Mg* mg, MgLevel& F, bool pre, double** ycur, double** rcur) {
  const MgSmoother& sm = mg->sm;
  const bool cheb = sm.ksp == PB_MG_LEVELS_CHEBYSHEV;
  double scale = sm.rich_scale, mu = 0.0, omegaprod = 0.0, rho = 0.0;
  if (cheb) {  // KSPSolve_Chebyshev's coefficients, restarted at every smoothing call
    scale = 2.0 / (sm.emax + sm.emin);
    const double alpha = 1.0 - scale * sm.emin;
    mu = 1.0 / alpha;
    omegaprod = 2.0 / alpha;
    rho = 1.0 / mu;
  }
  double* const ybuf[3] = {F.x, F.t1, F.t2};
  auto pick = [&](const double* a, const double* c) {
    for (double* q : ybuf)
      if (q != a && q != c) return q;
    return (double*)nullptr;
  };
  const double* y = nullptr;
  const double* yp = nullptr;
  const double* r = nullptr;
  if (!pre) {
    y = *ycur;
    PB_TRY(level_residual(mg, F, y, F.res));
    r = F.res;
  }
  for (int i = 0; i < sm.nu; ++i) {
    double omega = 1.0;
    if (cheb && i >= 1) {
      rho = 1.0 / (2.0 * mu - rho);
      omega = omegaprod * rho;
    }
    // y_prev enters from Chebyshev's second step on; after a zero start it is 0 in step 1
    const double* ypa = cheb && i >= 1 && !(pre && i == 1) ? yp : nullptr;
    const bool last = !pre && i == sm.nu - 1;
    double* yo = last ? F.x : pick(y, yp);
    double* ro = last ? nullptr : (r == F.res ? F.r2 : F.res);
    PB_TRY(poly_step(mg, F, y, ypa, r, scale, omega, yo, ro));
    yp = y;
    y = yo;
    r = ro;
  }
  *ycur = const_cast<double*>(y);
  *rcur = const_cast<double*>(r);
  return PB_OK;
}

// down: pre-smooth from zero (red, black), residual, restrict to C.b. F.cur = the pre-smoothed
// iterate: xs where the post-smoothing reads it apart from x
static int down_leg(Mg* mg, int l) {
  pb_ctx* ctx = mg->ctx;
  MgLevel& F = mg->lv[l];
  MgLevel& C = mg->lv[l + 1];
  const LevelPlan& p = F.plan;
  F.cur = p.post == LevelPlan::PostSweep ? F.xs : F.x;
  double* res = F.res;
  {
    ScopedTimer t1(ctx, l == 0 ? "mg_fine_smooth_first" : "mg_coarse_levels");
    if (p.pre == LevelPlan::FusedRestrict)
      return launch_presmooth_restrict(F.g, F.s, C.g, F.b, F.cur, C.b, mg->omega, mg->skip);
    if (p.pre == LevelPlan::FusedResidual) {
      PB_TRY(launch_presmooth_residual(F.g, F.s, F.b, F.cur, F.res, mg->omega, mg->skip));
    } else if (mg->poly()) {  // every step with its residual
      PB_TRY(poly_smooth(mg, F, true, &F.cur, &res));
    } else {  // nu x (red, black), the first pair from zero
      PB_TRY(level_smooth(mg, F, 0, 1));
      for (int i = 1; i < mg->sm.nu; ++i) {
        PB_TRY(level_smooth(mg, F, 0, 0));
        PB_TRY(level_smooth(mg, F, 1, 0));
      }
    }
  }
  ScopedTimer t2(ctx, l == 0 ? "mg_fine_resid_restrict" : "mg_coarse_levels");
  if (p.pre == LevelPlan::Sweeps && !mg->poly()) PB_TRY(level_residual(mg, F, F.x, res));
  return level_restrict(mg, F, res, C);
}

// gather the agglomerated level's right-hand side onto every rank (P copies out, P slabs in)
static int gather_coarse(Mg* mg) {
  pb_ctx* ctx = mg->ctx;
  ScopedTimer tg(ctx, "mg_coarse_levels");
  const MgLevel& A0 = mg->lv[mg->La];
  const size_t bytes = (size_t)A0.g->nlocal * sizeof(double);
  for (int r = 0; r < ctx->nranks; ++r)
    PB_HIP(hipMemcpyAsync(mg->agg_send + (int64_t)r * A0.g->nlocal, A0.b, bytes,
                          hipMemcpyDeviceToDevice, ctx->stream));
  return alltoallv_device(ctx, mg->agg_send, mg->agg_sc.data(), mg->ab[0], mg->agg_rc.data());
}

// up: prolongate + correct, post-smooth (black, red: the pre-smoothing mirrored) into F.x.
// from_agg: the coarse level is the agglomerated one -- this rank's planes of the full coarse
// correction, its wrap planes read in place. sums: level 0's
static int up_leg(Mg* mg, int l, bool from_agg, MgSums sums) {
  MgLevel& F = mg->lv[l];
  MgLevel& C = mg->lv[l + 1];
  ScopedTimer tm(mg->ctx, l == 0 ? "mg_fine_prolong_post" : "mg_coarse_levels");
  CoarsePlanes agg{C.x, nullptr, nullptr};
  if (from_agg) {
    const int64_t pc = C.g->plane, nzc = C.n[2], k0c = C.g->k0, nzl = C.g->nzl;
    const double* full = mg->ax[0];
    agg = {full + k0c * pc, full + ((k0c - 1 + nzc) % nzc) * pc, full + ((k0c + nzl) % nzc) * pc};
  }
  const CoarsePlanes* cp = from_agg ? &agg : nullptr;
  switch (F.plan.post) {
    case LevelPlan::PostSweep:  // prolongation + correction + both half-sweeps in one pass
      return launch_post_sweep(F.g, F.s, C.g, F.cur, agg.xc, F.b, F.x, mg->omega, mg->skip,
                               sums.st, sums.nparts, from_agg ? mg->ax[0] : nullptr);
    case LevelPlan::ProlongThenSweep2:  // into the residual scratch, then one pass back into F.x
      PB_TRY(level_prolong(mg, F, F.x, F.res, C, cp));
      return launch_sor_sweep2(F.g, F.s, F.res, F.b, F.x, mg->omega, 1, mg->skip, sums.st,
                               sums.nparts);
    case LevelPlan::ProlongThenHalves:
      break;
  }
  PB_TRY(level_prolong(mg, F, F.cur, F.cur, C, cp));
  if (mg->poly()) {
    double* res = nullptr;
    return poly_smooth(mg, F, false, &F.cur, &res);
  }
  for (int i = 0; i < mg->sm.nu; ++i) {
    PB_TRY(level_smooth(mg, F, 1, 0));
    PB_TRY(level_smooth(mg, F, 0, 0, i == mg->sm.nu - 1 ? sums : MgSums{}));
  }
  return PB_OK;
}

int mg_apply(Mg* mg, const double* r, double* z, const int* skip, const CgState* sums_st,
             int* nparts) {
  if (nparts) *nparts = 0;
  pb_ctx* ctx = mg->ctx;
  ScopedTimer tm(ctx, "mg_apply");
  const int L = (int)mg->lv.size();
  mg->skip = skip;
  mg->lv[0].b = const_cast<double*>(r);
  mg->lv[0].x = z;
  mg->tn = mg_tunings(ctx);
  if (mg->coef && mg->coef_seen != mg->coef->change) PB_TRY(vmg_build(mg));
  for (int l = 0; l < L; ++l) mg->lv[l].plan = level_plan(mg, l, mg->lv[l].xs != nullptr);
  // the level smoothers: no sums (the caller takes CG's), no tail, no agglomeration
  const bool custom = mg->custom();
  const MgSums sums = custom ? MgSums{} : MgSums{sums_st, nparts};
  // the coarse tail in one launch, levels Lt .. L-1: the agglomerated levels of a decomposed
  // grid, on one rank the levels of <= PB_MG_TAIL_MAX points
  const bool agg = mg->La > 0 && !custom;
  const int Lt = custom ? L : agg ? mg->La : ctx->split ? L : tail_first(mg);
  const int Lh = std::min(Lt, L - 1);  // the host legs: levels l < Lh
  for (int l = 0; l < Lh; ++l) PB_TRY(down_leg(mg, l));
  if (agg) PB_TRY(gather_coarse(mg));
  if (Lt < L) {
    ScopedTimer t3(ctx, "mg_coarse_levels");
    PB_TRY(launch_tail(mg, Lt, agg));
  } else {
    ScopedTimer t3(ctx, L > 1 ? "mg_coarse_levels" : "mg_fine_smooth_first");
    PB_TRY(coarse_solve(mg, mg->lv[L - 1], L == 1 ? sums : MgSums{}));
  }
  // (with a tail, the first host up-leg prolongates from level Lt)
  for (int l = Lh - 1; l >= 0; --l)
    PB_TRY(up_leg(mg, l, agg && l + 1 == mg->La, l == 0 ? sums : MgSums{}));
  return PB_OK;
}

}  // namespace pb
