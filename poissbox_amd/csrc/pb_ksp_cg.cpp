// pb_ksp_cg.cpp -- -ksp_type cg (KSPSolve_CG and KSPSolve_CG_SingleReduction analogues): the setup,
// the enqueue paths of one iteration and what pb_ksp_iterate / pb_ksp_end add for this solver. The
// driver is pb_solver.cpp; the passes and their launchers are in pb_cg_passes.hip, pb_cg_sr.hip and
// pb_cg_generic.hip.
//
// On the 7-point operator the iteration runs as 2 fused stencil passes + 2 one-block finalize
// kernels (plus a plane-sized boundary kernel and, on several ranks, one halo exchange and two
// scalar allreduces); folded, the finalize steps ride in the passes' prologues. Every pass that
// reads a neighbour plane goes through halo_overlap (pb_internal.hpp) but the folded pass A of a
// split grid, whose boundary-plane kernel and boundary launches run on the comm stream.
#include "pb_ksp.hpp"

using namespace pb;

// one rank: the periodic wrap read in place (no boundary-plane kernel); else the ghost planes
static StencilPlanes cg_planes(const pb_grid* g) {
  if (!g->ctx->split) return wrap_planes();
  StencilPlanes gp;
  gp.ghost_lo = g->ghost_lo;
  gp.ghost_hi = g->ghost_hi;
  return gp;
}

// the single-reduction iteration's two partial-sum regions (5 wide): iteration n of a batch
// writes region n & 1 and its folded prologue reduces region (n - 1) & 1, so a launch never
// overwrites the partials its own blocks may still be reading (part_off in 5-wide blocks)
static int64_t sr_region_off(const pb_ctx* ctx, int64_t n) {
  return (n & 1) * (ctx->partials_cap / 10);
}
static double* sr_region(const pb_ctx* ctx, int64_t n) {
  return ctx->d_partials + sr_region_off(ctx, n) * 5;
}

// pass S over r (t = dinv r - mu of state st): split grids exchange r's boundary planes (raw;
// the loader transforms ghosts too) under the interior planes. Every launch is bounded by the
// end of region n & 1 (a grid that does not fit is PB_ERR_UNSUPPORTED, not a spill into the
// region the next prologue reads)
static int sr_pass_s(pb_ksp* k, const double* r, const CgState* st, int* nparts, int64_t n) {
  pb_grid* g = k->A->grid;
  const Star s = star_of(k->A);
  const int off = (int)sr_region_off(g->ctx, n);
  const int end = off + (int)(g->ctx->partials_cap / 10);
  return halo_overlap(g, r, r + (g->nzl - 1) * g->plane, wrap_planes(), "cg_sr_s", off, nparts,
                      [&](int mode, const StencilPlanes& gp, int part_off, int* nb) {
                        return launch_cg_sr_pass_s(g, s, r, gp, st, mode, part_off, end, nb);
                      });
}

// KSPSolve_CG_SingleReduction's setup as from a zero guess: S = A z, delta = z'S (pass S over r0)
static int sr_setup(pb_ksp* k) {
  pb_ctx* ctx = k->A->grid->ctx;
  int np = 0;
  PB_TRY(sr_pass_s(k, k->r, k->d_st, &np, 0));
  return cg_sr_finalize(ctx, sr_region(ctx, 0), np, k->log(), -1, true);
}

// Setup from a nonzero initial guess (-ksp_initial_guess_nonzero): r = b - A x0, p = 0, z0 and
// stage 0 with KSPConvergedDefault's reference norm; x0 is read only
static int guess_setup(pb_ksp* k, const double* b, const double* x0, double dinv) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const int ref = k->ref_norm();
  const KspLog lg = k->log();
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
    return cg_finalize_guess(ctx, np, 4, bsums, ref, lg, rr);
  }
  if (!fused_kind(k->A->kind)) {  // compact / assembled A with Jacobi / no PC
    PB_TRY(op_apply_raw(k->A, x0, k->w));
    PB_TRY(launch_cg_guess_resid(g, b, k->w, k->r, k->pb[0], dinv, &np));
    return cg_finalize_guess(ctx, np, 6, nullptr, ref, lg);
  }
  // the fused pass; split grids exchange x0's boundary planes under the interior planes
  const Star s = star_of(k->A);
  const double* hi = x0 + (g->nzl - 1) * g->plane;
  StencilPlanes one;
  one.ghost_lo = hi;  // periodic wrap: no copy
  one.ghost_hi = x0;
  PB_TRY(halo_overlap(g, x0, hi, one, "cg_init_guess", 0, &np,
                      [&](int mode, const StencilPlanes& gp, int part_off, int* nb) {
                        return launch_cg_guess_init(g, s, x0, b, k->r, k->pb[0], gp, dinv, mode,
                                                    part_off, nb);
                      }));
  PB_TRY(cg_finalize_guess(ctx, np, 6, nullptr, ref, lg));
  return k->sr.on ? sr_setup(k) : PB_OK;
}

// KSPSolve_CG's setup: the buffers and the form of this solve's iteration, the state (st: the
// tolerances, filled in by pb_ksp_begin) to the device, r_0, z_0, history[0] and the first test
int pb::cg_begin(pb_ksp* k, const pb_vec* b, pb_vec* x, CgState& st) {
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
  const size_t vb = (size_t)g->nlocal * sizeof(double);
  if (k->pst && !k->r2) {
    if (field_alloc(&k->r2, vb) != hipSuccess)
      return set_error(PB_ERR_ALLOC, "CG residual buffer: out of device memory");
  }
  if (k->defer_x == 4 && !k->pb[2]) {
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
    return guess_setup(k, b->d, x->d, st.dinv);
  }
  if (k->stored_z()) {
    // r = b, x = 0, p = 0; z = M^-1 r; sums of z (KSPSolve_CG setup, PC_LEFT)
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
    return cg_finalize_init(ctx, np, k->log(), rr);
  }
  PB_TRY(launch_cg_init(g, b->d, x->d, k->r, k->pb[0], st.dinv, k->log()));
  return k->sr.on ? sr_setup(k) : PB_OK;
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
    // (the variable-coefficient operator may take p . w in its own pass: tuning varcoef_dot_fused)
    OpApplySkip guard(ctx, &k->d_st->done);
    PB_TRY(op_apply_dot(k->A, p, k->w, &np));
  }
  if (np == 0) PB_TRY(launch_cg_generic_dot(g, p, k->w, k->d_st, &np));
  PB_TRY(cg_finalize_pass_a(ctx, np, k->d_st));
  PB_TRY(launch_cg_generic_xr(g, p, k->w, k->x->d, k->r, k->d_st, &np));
  return cg_finalize_stage2(ctx, np, k->log(), k->host_iter);
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
      PB_TRY(op_apply_dot(k->A, p, k->w, &np));
    }
    if (np == 0) PB_TRY(launch_cg_generic_dot(g, p, k->w, k->d_st, &np));
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
  return cg_finalize_stage2(ctx, np, k->log(), k->host_iter, rr);
}

// One single-reduction iteration (PETSc KSPSolve_CG_SingleReduction): pass P, pass S, and -- unless
// folded into the next pass P's prologue (one rank) -- the reduction + residual-sum stage.
// n = the iteration's index inside this pb_ksp_iterate batch (state slot parity).
static int enqueue_sr_iteration(pb_ksp* k, bool fold, int64_t n) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const Star s = star_of(k->A);
  const int64_t i = k->host_iter;
  const pb_ksp::CgBufs v = k->cg_bufs();
  // one rank: the state alternates between the slots by the batch index's parity; split grids:
  // slot 0 holds the state after the residual-sum stage (written by the boundary-plane kernel's
  // folded prologue, or copied there unfolded), slot 1 after the top of the iteration (pass P)
  CgState* st_in = ctx->split ? k->d_st : k->d_st + (n & 1);
  const KspLog out = k->log(ctx->split ? 1 : (int)((n + 1) & 1));
  const Fold f = fold_sr_top(fold && n > 0 && !ctx->split, sr_region(ctx, n - 1), k->sr.nparts,
                             st_in, out.st, k->log(), i - 1);
  // one pass per iteration where it applies: one rank, depth-4 x deferral; the iterations that
  // carry the x update run the two passes (pass P's x-update form streams at the copy rate)
  if (cg_sr1_supported(g) && k->defer_x == 4 && i % 4 != 3) {
    PB_TRY(launch_cg_sr1(g, s, v.r, v.p_old, v.p_new, v.r_out, f, sr_region(ctx, n),
                         &k->sr.nparts));
    if (!fold) PB_TRY(cg_sr_finalize(ctx, sr_region(ctx, n), k->sr.nparts, out, i));
    return PB_OK;
  }
  // split grids: p's boundary planes -> halo, under the interior planes. Folded: the boundary-plane
  // kernel first runs the previous iteration's residual-sum stage from pass S's allreduced sums (a
  // one-block partial, slot 1 -> slot 0); pass P then runs the top (slot 0 -> slot 1)
  if (ctx->split)
    PB_TRY(launch_cg_boundary(g, v.r, v.p_old, st_in,
                              fold && n > 0 ? fold_stage2_allreduced(ctx, 5, k->log(), i - 1)
                                            : Fold{}));
  int none = 0;  // (pass P takes no sums)
  PB_TRY(halo_overlap(g, g->bnd_lo, g->bnd_hi, wrap_planes(), "cg_sr_p_split", 0, &none,
                      [&](int mode, const StencilPlanes& gp, int, int*) {
                        return launch_cg_sr_pass_p(g, s, v.r, v.p_prev, v.p_new, k->x->d, v.r_out,
                                                   gp, f, mode, i, k->defer_x);
                      }));
  PB_TRY(sr_pass_s(k, v.r_out, out.st, &k->sr.nparts, n));
  if (fold && ctx->split) return cg_reduce_allreduce(ctx, sr_region(ctx, n), k->sr.nparts, 5);
  if (!fold) PB_TRY(cg_sr_finalize(ctx, sr_region(ctx, n), k->sr.nparts, out, i));
  if (!fold && ctx->split)  // the next boundary-plane kernel reads slot 0
    PB_HIP(hipMemcpyAsync(k->d_st, out.st, sizeof(CgState), hipMemcpyDeviceToDevice,
                          ctx->stream));
  return PB_OK;
}

// fold: the finalize steps run in the passes' prologues (Jacobi / none; fold_a = pass A also
// folds, i.e. this is not the first iteration of the batch)
static int enqueue_iteration(pb_ksp* k, bool fold, bool fold_a) {
  if (!fused_kind(k->A->kind))
    return k->stored_z() ? enqueue_pc_iteration(k) : enqueue_generic_iteration(k);
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const Star s = star_of(k->A);
  const int64_t i = k->host_iter;  // == device iteration index until convergence
  const pb_ksp::CgBufs v = k->cg_bufs();
  const KspLog lg = k->log();
  int nparts = 0;
  // Jacobi: pass A builds z = dinv*r - mu on the fly; SOR / MG: z is stored (dinv = 1)
  CgPassA a;
  a.r = k->stored_z() ? k->z : v.r;
  a.p_old = v.p_old;
  a.p_new = v.p_new;
  a.gp = cg_planes(g);
  a.nblocks = &nparts;
  a.store = !k->pst;
  a.st = k->d_st;
  CgPassB b;
  b.p = v.p_new;
  b.p_prev = v.p_prev;
  b.x = k->x->d;
  b.r = v.r;
  b.gp = a.gp;
  b.host_iter = i;
  b.defer = k->defer_x;
  // Jacobi / none: pass A read-only, pass B stores p and the residual into the other buffer
  if (k->pst) b.ps = PStore{a.r, v.r_out};
  b.nparts = &k->fold_nparts_b;
  if (fold && !ctx->split) {
    if (fold_a) a.fold = fold_stage2_pass_b(ctx, k->fold_nparts_b, lg, i - 1);
    PB_TRY(launch_cg_pass_a(g, s, a));
    b.fold = fold_stage1_pass_a(ctx, nparts, false, k->d_st);
    return launch_cg_pass_b(g, s, b);
  }
  if (fold) {
    // split grids, folded (r05): the previous iteration's stage 2 runs in the prologues of the
    // boundary-plane kernel and pass A (from pass B's allreduced sums, a one-block partial), stage
    // 1 in pass B's (from pass A's); only the reductions before each allreduce stay separate
    // launches (bit-identical to unfolded)
    const Fold fb = fold_a ? fold_stage2_allreduced(ctx, 4, lg, i - 1) : Fold{};
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
      PB_TRY(halo_begin(g, g->bnd_lo, g->bnd_hi, [&](hipStream_t sm) {
        return launch_cg_boundary(g, a.r, a.p_old, k->d_st, fbr, sm);
      }));
      a.mode = PLANES_INTERIOR;
      a.nblocks = &nb1;
      a.fold = fb;
      PB_TRY(launch_cg_pass_a(g, s, a));
      a.mode = PLANES_BOUNDARY;
      a.part_off = nb1;
      a.nblocks = &nb2;
      if (ctx->comm) {
        // the two boundary planes on the comm stream right after the exchange (beside the
        // interior planes), from the stage-2 state in registers as well
        EngineOn eo(ctx, ctx->comm_stream);
        a.fold = fbr;
        PB_TRY(launch_cg_pass_a(g, s, a));
        PB_HIP(hipEventRecord(ctx->ev_done, ctx->comm_stream));
        PB_TRY(halo_end(g));
      } else {
        PB_TRY(halo_end(g));
        a.fold = Fold{};  // (the interior launch's prologue wrote the state)
        PB_TRY(launch_cg_pass_a(g, s, a));
      }
      nparts = nb1 + nb2;
    } else {
      PB_TRY(launch_cg_boundary(g, a.r, a.p_old, k->d_st, fb));
      PB_TRY(halo_exchange(g, g->bnd_lo, g->bnd_hi));
      PB_TRY(launch_cg_pass_a(g, s, a));
    }
    PB_TRY(cg_reduce_allreduce(ctx, nparts, 1, false));
    b.fold = fold_stage1_pass_a(ctx, 1, true, k->d_st);
    PB_TRY(launch_cg_pass_b(g, s, b));
    return cg_reduce_allreduce(ctx, k->fold_nparts_b, 4, true);
  }
  // one rank: pass A combines r, p_old of the wrap planes itself and pass B reads p_new's wrap
  // planes; split grids: the p-plane halo exchange overlaps pass A's interior planes
  if (ctx->split) PB_TRY(launch_cg_boundary(g, a.r, a.p_old, k->d_st));
  PB_TRY(halo_overlap(g, g->bnd_lo, g->bnd_hi, a.gp, "cg_pass_a", 0, &nparts,
                      [&](int mode, const StencilPlanes& gp, int part_off, int* nb) {
                        a.mode = mode;
                        a.gp = gp;
                        a.part_off = part_off;
                        a.nblocks = nb;
                        return launch_cg_pass_a(g, s, a);
                      }));
  PB_TRY(cg_finalize_pass_a(ctx, nparts, k->d_st));
  // (unpreconditioned norm with a stored-z PC: pass B's own four sums of t = r - mu, kept in the
  // second partial region, give sum r^2 to the stage below)
  RrParts rr;
  b.st = k->d_st;
  b.nparts = &nparts;
  if (k->stored_z() && k->norm_unp()) b.rr = &rr;
  PB_TRY(launch_cg_pass_b(g, s, b));
  if (k->stored_z()) {  // z = M^-1 r, then the residual sums over z
    nparts = 0;
    PB_TRY(pc_apply_dev(k, v.r, k->z, &k->d_st->done, &nparts));
    if (nparts == 0) PB_TRY(launch_cg_pc_sums(g, k->z, v.r, k->d_st, &nparts));
  }
  return cg_finalize_stage2(ctx, nparts, lg, i, rr);
}

int pb::enqueue_cg_iteration(pb_ksp* k, bool fold, int64_t n) {
  return k->sr.on ? enqueue_sr_iteration(k, fold, n) : enqueue_iteration(k, fold, fold && n > 0);
}

// after the n iterations of a pb_ksp_iterate batch: the residual-sum stage of the last one
// (folded runs), then the state back into slot 0 for the next batch and the other entry points
int pb::cg_batch_end(pb_ksp* k, bool fold, int64_t n) {
  pb_ctx* ctx = k->A->grid->ctx;
  const int64_t last = k->host_iter - 1;
  if (!k->sr.on) return fold && n > 0 ? cg_fold_tail(ctx, k->fold_nparts_b, k->log(), last) : PB_OK;
  // the slot the complete state is in (split grids, unfolded: in slot 0 already)
  const int from = ctx->split ? (fold && n > 0 ? 1 : 0) : (int)(n & 1);
  if (fold && n > 0) {
    if (ctx->split) PB_TRY(cg_stage2_from_sums(ctx, 5, k->log(from), last));
    else PB_TRY(cg_sr_finalize(ctx, sr_region(ctx, n - 1), k->sr.nparts, k->log(from), last));
  }
  if (from)
    PB_HIP(hipMemcpyAsync(k->d_st, k->d_st + 1, sizeof(CgState), hipMemcpyDeviceToDevice,
                          ctx->stream));
  return PB_OK;
}

// pb_ksp_end's share, from the final state: x = 0 after a lazy start that stopped at the setup
// (x = x0 = 0 was never written), then the still-deferred alpha_m p_m (p_m lives in
// pb[(m + 1) % ns])
int pb::cg_finish(pb_ksp* k, const CgState& st) {
  pb_grid* g = k->A->grid;
  const bool unwritten = k->lazy0 && k->host_iter == 0;
  if (unwritten)
    PB_HIP(hipMemsetAsync(k->x->d, 0, (size_t)g->nlocal * sizeof(double), g->ctx->stream));
  if (st.pend_iter >= 0) {
    const int ns = k->pslots();
    for (int64_t m = 0; m < st.pend_count; ++m)
      PB_TRY(launch_cg_flush(g, k->x->d, k->pb[(st.pend_iter + m + 1) % ns], st.pa[m]));
  }
  if (unwritten || st.pend_iter >= 0) PB_SYNC(g->ctx, "pb_ksp_end");
  return PB_OK;
}
