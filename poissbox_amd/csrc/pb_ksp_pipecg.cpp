// pb_ksp_pipecg.cpp -- the host part of -ksp_type pipecg: pipelined CG, PETSc
// KSPSolve_PIPECG with PC_LEFT, kept on the device. pb_ksp_create's share, pb_ksp_begin's setup
// and one iteration of pb_ksp_iterate. The kernels and the update pass are in
// pb_ksp_pipecg.hip; the done flags, history and polling are CG's (pb_solver.cpp).
//
//   r = b (x = 0) or b - A x0;  u = N(M^-1 r);  w = A u;  the five sums;  the finalize (i = 0)
//   iteration i:  m = N(M^-1 w);  n = A m;  the eight updates with alpha_i, beta_i and the five
//                 sums of the new vectors;  the finalize: ONE reduction, the norm of i + 1 logged
//                 and tested, beta and alpha of i + 1
//
// With Jacobi / no PC the mean of m follows from sum w, which rides in the reduction: one
// allreduce per iteration on N ranks. With a PC that stores its result (sor, mg, fft) the mean of
// M^-1 w is a second, one-double allreduce, as in fgmres. The allreduce runs on the compute stream:
// nothing of m and n depends on it but the shift of Jacobi's m, yet moving it to the
// communication stream is not done here.
#include "pb_ksp.hpp"
#include "pb_cg_device.hpp"  // REF_*

using namespace pb;

// the 7-point operator on one rank with Jacobi / no PC: an iteration is the engine pass and the
// finalize (tuning pipecg_fused = 0: the sequence it replaces, bit-identical)
static bool pcg_engine(const pb_ksp* k) {
  return fused_kind(k->A->kind) && !k->A->grid->ctx->split && !k->stored_z();
}

static int pcg_alloc(pb_ksp* k, double** p) {
  if (*p) return PB_OK;
  if (field_alloc(p, (size_t)k->A->grid->nlocal * sizeof(double)) != hipSuccess)
    return set_error(PB_ERR_ALLOC, "pipecg work vectors: out of device memory");
  return PB_OK;
}

int pb::pipecg_create(pb_ksp* k) {
  if (!k->pipecg()) return PB_OK;
  if (k->opts.guess_type != PB_GUESS_NONE)
    return set_error(PB_ERR_UNSUPPORTED, "-ksp_guess_type fischer with -ksp_type pipecg");
  if (hipMalloc(&k->pcg.d, sizeof(PcgState)) != hipSuccess)
    return set_error(PB_ERR_ALLOC, "pipecg state: out of device memory");
  PB_HIP(hipMemsetAsync(k->pcg.d, 0, sizeof(PcgState), k->A->grid->ctx->stream));
  PB_TRY(pcg_alloc(k, &k->pcg.z));
  PB_TRY(pcg_alloc(k, &k->pcg.q));
  PB_TRY(pcg_alloc(k, &k->pcg.s));
  return pcg_alloc(k, &k->pcg.p);
}

void pb::pipecg_destroy(pb_ksp* k) {
  field_free(k->pcg.z);
  field_free(k->pcg.q);
  field_free(k->pcg.s);
  field_free(k->pcg.p);
  field_free(k->pcg.w2);
  if (k->pcg.d) (void)hipFree(k->pcg.d);
}

// dst = N(M^-1 src). sum: where the sum of src already is (an iteration with Jacobi / no PC: the
// reduction's sum w), nullptr: taken here. skip: an iteration's launches (exit once done)
static int pcg_pc(pb_ksp* k, const double* src, double* dst, const double* sum, bool skip) {
  pb_ctx* ctx = k->A->grid->ctx;
  const int64_t n = k->A->grid->nlocal;
  const CgState* st = k->d_st;
  const bool ns = k->opts.nullspace != 0;
  PcgState* ps = k->pcg.d;
  if (k->stored_z()) {
    const int* sk = skip ? &st->done : nullptr;
    PB_TRY(pc_stored_apply(k, src, dst, sk));
    if (!ns) return PB_OK;
    // (dinv = 1 with these PCs: dst = dst + (-(sum dst / ntot)), MatNullSpaceRemove's VecShift)
    PB_TRY(launch_pcg_sum(ctx, dst, &ps->zsum, st, skip, n));
    return launch_pcg_pcshift(ctx, dst, dst, &ps->zsum, st, skip, n, true);
  }
  if (ns && !sum) {
    PB_TRY(launch_pcg_sum(ctx, src, &ps->zsum, st, skip, n));
    sum = &ps->zsum;
  }
  return launch_pcg_pcshift(ctx, src, dst, sum, st, skip, n, ns);
}

// KSPSolve_PIPECG's setup: r_0, u_0 = N(M^-1 r_0), w_0 = A u_0, the first sums, with a nonzero
// guess the reference norm's sums (CG's rules: of N(M^-1 b), or of b under unpreconditioned),
// history[0] and the first test. Runs once per solve: the unfused kernels
int pb::pipecg_begin(pb_ksp* k, const pb_vec* b, pb_vec* x) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const int64_t n = g->nlocal;
  const size_t vb = (size_t)n * sizeof(double);
  PB_CHECK_ARG(b != x, "pipecg needs distinct b and x");
  k->sr.on = false;
  k->pst = false;
  k->lazy0 = false;
  k->defer_x = 0;
  k->b = b;
  k->x = x;
  k->pcg.cur = 0;
  k->pcg.fused = pcg_engine(k) && tune("pipecg_fused", 1) != 0;
  if (k->pcg.fused) {
    PB_TRY(pcg_alloc(k, &k->pcg.w2));
  } else {
    PB_TRY(pcg_alloc(k, &k->w));  // m
    PB_TRY(pcg_alloc(k, &k->z));  // n
  }
  PcgState* ps = k->pcg.d;
  double* r = k->r;
  double* u = k->pb[0];
  double* w = k->pb[1];
  int ref = REF_ZERO_GUESS;
  if (!k->opts.initial_guess_nonzero) {
    PB_HIP(hipMemsetAsync(x->d, 0, vb, ctx->stream));
    PB_HIP(hipMemcpyAsync(r, b->d, vb, hipMemcpyDeviceToDevice, ctx->stream));
  } else {
    PB_TRY(check_ref_norm_opts(&k->opts));
    ref = k->ref_norm();
    if (ref != REF_INITIAL && !k->norm_none()) {
      if (k->norm_unp()) {
        PB_TRY(launch_pcg_sums(ctx, b->d, b->d, b->d, ps->bsums, n));
      } else {
        PB_TRY(pcg_pc(k, b->d, u, nullptr, false));
        PB_TRY(launch_pcg_sums(ctx, b->d, u, u, ps->bsums, n));
      }
    }
    PB_TRY(op_apply_raw(k->A, x->d, w));
    PB_TRY(launch_guess_diff(ctx, b->d, w, r, n));
  }
  PB_TRY(pcg_pc(k, r, u, nullptr, false));
  PB_TRY(op_apply_raw(k->A, u, w));
  PB_TRY(launch_pcg_sums(ctx, r, u, w, ps->sums, n));
  return launch_pcg_finalize(ctx, k->log(), ps, nullptr, 0, true, ref, -1);
}

// One iteration at the host's count (the device's while the state is not done; every kernel that
// writes a vector or the state exits at entry once it is)
int pb::enqueue_pipecg_iteration(pb_ksp* k) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  PcgState* ps = k->pcg.d;
  CgState* st = k->d_st;
  PcgVecs v{k->pcg.z, k->pcg.q, k->pcg.s, k->pcg.p, k->x->d, k->r, k->pb[0], k->pb[1], k->pb[1]};
  const bool ns = k->opts.nullspace != 0;
  int np = 0;
  if (k->pcg.fused) {
    v.w = k->pcg_wbuf(k->pcg.cur);
    v.w_out = k->pcg_wbuf(k->pcg.cur ^ 1);
    k->pcg.cur ^= 1;
    PB_TRY(launch_pcg_fused(g, star_of(k->A), v, ps, st, ns, &np));
  } else {
    double* m = k->w;
    double* nn = k->z;
    PB_TRY(pcg_pc(k, v.w, m, k->stored_z() ? nullptr : &ps->sums[4], true));
    {
      OpApplySkip guard(ctx, &st->done);
      PB_TRY(op_apply_raw(k->A, m, nn));
    }
    PB_TRY(launch_pcg_update(g, m, nn, v, ps, st, &np));
  }
  if (ctx->split) {
    PB_TRY(reduce_partials(ctx, ctx->d_partials, np, kPcgSums, ps->sums));
    PB_TRY(allreduce_device(ctx, ps->sums, kPcgSums));
    np = 0;
  }
  return launch_pcg_finalize(ctx, k->log(), ps, ctx->d_partials, np, false, 0, k->host_iter);
}
