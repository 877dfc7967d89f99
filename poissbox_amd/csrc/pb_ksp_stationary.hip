// pb_ksp_stationary.hip -- the vector kernels and the one-block finalize of the stationary solves:
// -ksp_type richardson (PETSc KSPSolve_Richardson: x += scale N(M^-1 (b - A x)), PC_LEFT, the
// preconditioned norm, KSPConvergedDefault) and -ksp_type preonly (KSPSolve_PREONLY: x = N(M^-1 b)).
// -ksp_type chebyshev (KSPSolve_Chebyshev) shares all of Richardson's but the update's expression
// from its second update on and the omega recurrence in the finalize.
// The hot step of Richardson on the 7-point operator is one stencil-engine pass (RichLoad /
// RichEpi, at the end of this file; Chebyshev: ChebLoad / RichEpi); the other kernels are its
// unfused form, the steps around operators without an engine (compact, assembled, split grids) and the scalar
// logic; their host drivers are in pb_ksp_stationary.cpp. The device-resident state, done flag,
// history and polling are CG's (CgState, pb_solver.cpp).
#include "pb_cg_device.hpp"
#include "pb_star7.hpp"

namespace pb {

// ---------------------------------------------------------------------------------------------
// Scalar logic: iteration i has z_i = N(M^-1 r_i) behind the sums S = (sum t, sum t^2) of
// t = M^-1 r_i - mean_old (shifted by the previous mean, as CG's stage 2: the sums stay accurate
// when the residual is almost constant). setup: i = 0 and the stopping reference; else i = it + 1
// (the update before this norm happened: every kernel of it ran, the state was not done).
//   ||z_i|| -> NaN / Inf: DIVERGED_NANORINF, its = i; history[i]; the default test with its = i;
//   no reason and i = max_it: DIVERGED_ITS; else the mean for the next update.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void rich_stage(CgState& st, const double* S, bool setup, int ref,
                                           double bnorm, double* hist, int* h_done,
                                           int64_t host_iter, double cheb_mu,
                                           double cheb_omegaprod, const double* Q = nullptr) {
  if (setup) {
    st.it = 0;
    st.its = 0;
    st.reason = 0;
    st.done = 0;
    st.mu = 0.0;
    st.nlog = 0;
    st.pend_iter = -1;
    st.pend_count = 0;
  }
  if (!st.done) {
    const int64_t i = setup ? 0 : st.it + 1;
    const double N = st.ntot;
    double delta = 0.0, zz = S[1];
    if (st.nullspace) {
      delta = S[0] / N;
      zz = S[1] - N * delta * delta;
    }
    // -ksp_norm_type: unpreconditioned is ||r_i|| = ||b - A x_i||, the plain
    // 2-norm, from the same two sums (Jacobi / no PC: t = dinv r - mean_old, so
    // sum r^2 = (sum t^2 + 2 mean_old sum t + N mean_old^2) / dinv^2; a stored-z PC: the residual
    // pass took the same two sums of t = r - mean_old aside, Q, dinv = 1); none: no norm, no test
    const bool skip = st.norm == PB_KSP_NORM_NONE;
    double dp = 0.0;
    if (st.norm == PB_KSP_NORM_PRECONDITIONED) {
      dp = norm_from_sq(zz);
    } else if (st.norm == PB_KSP_NORM_UNPRECONDITIONED) {
      const double* T = Q ? Q : S;
      dp = norm_from_sq((T[1] + st.mu * (2.0 * T[0] + N * st.mu)) / (st.dinv * st.dinv));
    }
    st.it = i;
    st.its = i;
    st.dp = dp;
    if (setup) {
      double rn0 = dp;  // REF_ZERO_GUESS, REF_INITIAL
      if (ref == REF_RHS) rn0 = bnorm == 0.0 ? dp : bnorm;
      else if (ref == REF_MIN) rn0 = fmin(bnorm, dp);
      st.rnorm0 = rn0;
      st.ttol = fmax(st.rtol * rn0, st.atol);
    }
    if (i < st.nhist) {
      hist[i] = dp;
      st.nlog = i + 1;
    }
    if (!finite(dp)) {
      st.reason = PB_KSP_DIVERGED_NANORINF;
      st.done = 1;
    } else if (!skip && dp <= st.ttol) {
      st.reason = dp < st.atol ? PB_KSP_CONVERGED_ATOL : PB_KSP_CONVERGED_RTOL;
      st.done = 1;
    } else if (!skip && !(setup && ref == REF_ZERO_GUESS) && dp >= st.dtol * st.rnorm0) {
      // (from a zero guess ||z_0|| is the reference itself: no test at i = 0, as CG's stage 0)
      st.reason = PB_KSP_DIVERGED_DTOL;
      st.done = 1;
    } else if (i >= st.max_it) {
      st.reason = skip ? PB_KSP_CONVERGED_ITS : PB_KSP_DIVERGED_ITS;  // (KSPConvergedSkip)
      st.done = 1;
    } else {
      st.mu = st.mu + delta;
      if (cheb_mu != 0.0) {
        // -ksp_type chebyshev: update i follows; rho_i = c_i / c_(i+1) of PETSc's c_(k+1) =
        // 2 mu c_k - c_(k-1) (which overflows in long runs), omega_i = omegaprod rho_i. Every
        // setup restarts it (i = 0; update 0 is Richardson's and reads no omega)
        const double rho = i == 0 ? 1.0 / cheb_mu : 1.0 / (2.0 * cheb_mu - st.beta);
        st.beta = rho;
        st.alpha = cheb_omegaprod * rho;
      }
    }
  }
  h_done[setup ? 0 : host_iter + 1] = st.done;
}

// mode bit 1: reduce nparts x width partials into sums[0..1] in a fixed order (only the first two
// sums of a block are read: CG's 4-wide PC sums carry t, t^2 first); bit 2: rich_stage from
// sums[] (split around the allreduce on several ranks). bsums / ref: cg_guess_finalize_kernel's.
__global__ __launch_bounds__(256) void rich_finalize_kernel(const double* __restrict__ parts,
                                                            int nparts, int width, double* sums,
                                                            int mode, const double* bsums, int ref,
                                                            CgState* st, double* hist, int* h_done,
                                                            int64_t host_iter, double cheb_mu,
                                                            double cheb_omegaprod, RrParts rr) {
  if ((mode & 1) && rr.parts) {  // the second region's two sums -> sums[2..3], same fixed order
    __shared__ double red2[256][2];
    for (int s = 0; s < 2; ++s) {
      double v = 0.0;
      for (int b = threadIdx.x; b < rr.nparts; b += 256) v += rr.parts[(int64_t)b * 2 + s];
      red2[threadIdx.x][s] = v;
    }
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
      if ((int)threadIdx.x < off)
        for (int s = 0; s < 2; ++s) red2[threadIdx.x][s] += red2[threadIdx.x + off][s];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      sums[2] = red2[0][0];
      sums[3] = red2[0][1];
    }
  }
  if (mode & 1) {
    __shared__ double red[256][2];
    for (int s = 0; s < 2; ++s) {
      double v = 0.0;
      for (int b = threadIdx.x; b < nparts; b += 256) v += parts[(int64_t)b * width + s];
      red[threadIdx.x][s] = v;
    }
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
      if ((int)threadIdx.x < off)
        for (int s = 0; s < 2; ++s) red[threadIdx.x][s] += red[threadIdx.x + off][s];
      __syncthreads();
    }
    if (threadIdx.x == 0) {
      sums[0] = red[0][0];
      sums[1] = red[0][1];
    }
  }
  if (!(mode & 2) || threadIdx.x != 0) return;
  const double S[2] = {sums[0], sums[1]};
  const bool setup = host_iter < 0;
  double bnorm = 0.0;
  if (setup && (ref == REF_RHS || ref == REF_MIN) && st->norm != PB_KSP_NORM_NONE) {
    double zz = bsums[1];
    if (st->norm == PB_KSP_NORM_UNPRECONDITIONED) {
      zz = bsums[1] / (st->dinv * st->dinv);  // ||b||^2 from the sums of dinv b: no PC application
    } else if (st->nullspace) {
      const double delta = bsums[0] / st->ntot;
      zz = bsums[1] - st->ntot * delta * delta;
    }
    bnorm = norm_from_sq(zz);
  }
  const double Q[2] = {sums[2], sums[3]};
  rich_stage(*st, S, setup, ref, bnorm, hist, h_done, host_iter, cheb_mu, cheb_omegaprod,
             rr.parts ? Q : nullptr);
}

// ---------------------------------------------------------------------------------------------
// Vector kernels. Those of an iteration exit at entry once the state is done (enqueued ahead of
// the host's poll): x and r then stay as the last update left them.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void rich_x_kernel(const double* __restrict__ x,
                                                     const double* __restrict__ q,
                                                     double* __restrict__ x_out, int64_t n,
                                                     const CgState* st, double scale) {
  if (st->done) return;
  const double dinv = st->dinv, shift = -st->mu;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    x_out[i] = rich_step<true>(x[i], q[i], dinv, shift, scale);
  }
}

// Chebyshev's update i >= 1 (cheb_step, pb_device.hpp: ChebLoad below calls the same)
__global__ __launch_bounds__(256) void cheb_x_kernel(const double* __restrict__ y,
                                                     const double* __restrict__ ym1,
                                                     const double* __restrict__ q,
                                                     double* __restrict__ y_out, int64_t n,
                                                     const CgState* st, double scale) {
  if (st->done) return;
  const double dinv = st->dinv, shift = -st->mu, omega = st->alpha;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double qi = q[i], ykm1 = ym1[i];  // (read in the order the step uses them)
    y_out[i] = cheb_step<true>(y[i], ykm1, qi, dinv, shift, scale, omega);
  }
}

template <bool SUMS>
__global__ __launch_bounds__(256) void rich_resid_kernel(const double* __restrict__ b,
                                                         const double* __restrict__ w,
                                                         double* __restrict__ r, int64_t n,
                                                         double* parts, const CgState* st,
                                                         int skip) {
  if (skip && st->done) return;
  const double dinv = st->dinv, mu = st->mu;
  double acc[2] = {0, 0};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double rv = b[i] - w[i];
    r[i] = rv;
    if constexpr (SUMS) {
      const double t = dinv * rv - mu;
      acc[0] += t;
      acc[1] += t * t;
    }
  }
  if constexpr (SUMS) block_partials<2>(acc, parts);
}

__global__ __launch_bounds__(256) void rich_sums_kernel(const double* __restrict__ q, int64_t n,
                                                        double* parts, const CgState* st) {
  const double dinv = st->dinv, mu = st->mu;
  double acc[2] = {0, 0};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const double t = dinv * q[i] - mu;
    acc[0] += t;
    acc[1] += t * t;
  }
  block_partials<2>(acc, parts);
}

// preonly: dst = dinv src (PCApply_Jacobi / PCApply_None) and the sum of it, or the sum alone
__global__ __launch_bounds__(256) void pre_scale_sum_kernel(const double* __restrict__ src,
                                                            double* __restrict__ dst, int64_t n,
                                                            double dinv, double* parts) {
  double acc[2] = {0, 0};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    double v = src[i];
    if (dst) {
      v = dinv * v;
      dst[i] = v;
    }
    acc[0] += v;
  }
  block_partials<2>(acc, parts);
}

// MatNullSpaceRemove of the constant: x -= sum / ntot
__global__ __launch_bounds__(256) void pre_shift_kernel(double* __restrict__ x, int64_t n,
                                                        const double* sums, double ntot) {
  const double mean = sums[0] / ntot;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    x[i] = x[i] - mean;
}

static int vec_blocks(pb_ctx* ctx, int64_t n) {
  const int64_t b = (n + 255) / 256, cap = (int64_t)ctx->num_cus * 8;
  return (int)(b > cap ? cap : (b < 1 ? 1 : b));
}

int launch_rich_x(pb_grid* g, const double* x, const double* q, double* x_out, const CgState* st,
                  double scale) {
  ScopedTimer tm(g->ctx, "rich_axpy");
  hipLaunchKernelGGL(rich_x_kernel, dim3(vec_blocks(g->ctx, g->nlocal)), dim3(256), 0,
                     g->ctx->stream, x, q, x_out, g->nlocal, st, scale);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int launch_cheb_x(pb_grid* g, const double* y, const double* ym1, const double* q, double* y_out,
                  const CgState* st, double scale) {
  ScopedTimer tm(g->ctx, "cheb_axpy");
  hipLaunchKernelGGL(cheb_x_kernel, dim3(vec_blocks(g->ctx, g->nlocal)), dim3(256), 0,
                     g->ctx->stream, y, ym1, q, y_out, g->nlocal, st, scale);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int launch_rich_resid(pb_grid* g, const double* b, const double* w, double* r, const CgState* st,
                      bool skip, int* nparts, double* parts) {
  ScopedTimer tm(g->ctx, "rich_resid_vec");
  const int nb = vec_blocks(g->ctx, g->nlocal);  // (<= 8 blocks per CU x 2 sums: fits either region)
  if (nparts) {
    hipLaunchKernelGGL(rich_resid_kernel<true>, dim3(nb), dim3(256), 0, g->ctx->stream, b, w, r,
                       g->nlocal, parts ? parts : g->ctx->d_partials, st, skip ? 1 : 0);
    *nparts = nb;
  } else {
    hipLaunchKernelGGL(rich_resid_kernel<false>, dim3(nb), dim3(256), 0, g->ctx->stream, b, w, r,
                       g->nlocal, g->ctx->d_partials, st, skip ? 1 : 0);
  }
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int launch_rich_sums(pb_grid* g, const double* q, const CgState* st, int* nparts, double* parts) {
  ScopedTimer tm(g->ctx, "rich_sums");
  const int nb = vec_blocks(g->ctx, g->nlocal);
  hipLaunchKernelGGL(rich_sums_kernel, dim3(nb), dim3(256), 0, g->ctx->stream, q, g->nlocal,
                     parts ? parts : g->ctx->d_partials, st);
  PB_HIP(hipGetLastError());
  *nparts = nb;
  return PB_OK;
}

int rich_reduce(pb_ctx* ctx, int nparts, int width, double* dst, const RrParts& rr) {
  hipLaunchKernelGGL(rich_finalize_kernel, dim3(1), dim3(256), 0, ctx->stream,
                     (const double*)ctx->d_partials, nparts, width, ctx->d_scalars, 1,
                     (const double*)nullptr, 0, (CgState*)nullptr, (double*)nullptr,
                     (int*)nullptr, (int64_t)0, 0.0, 0.0, rr);
  PB_HIP(hipGetLastError());
  if (ctx->split) PB_TRY(allreduce_device(ctx, ctx->d_scalars, rr.parts ? 4 : 2));
  if (dst)
    PB_HIP(hipMemcpyAsync(dst, ctx->d_scalars, 2 * sizeof(double), hipMemcpyDeviceToDevice,
                          ctx->stream));
  return PB_OK;
}

int rich_finalize(pb_ctx* ctx, int nparts, int width, const double* bsums, int ref,
                  const KspLog& lg, int64_t host_iter, double cheb_mu, double cheb_omegaprod,
                  const RrParts& rr) {
  ScopedTimer tm(ctx, "rich_finalize");  // (with its allreduce on several ranks)
  const double* parts = ctx->d_partials;
  // (the PC's own partials must have stayed below the second region)
  if (rr.parts && ((int64_t)nparts * width > ctx->partials_cap / 2 || rr.width != 2))
    return set_error(PB_ERR_UNSUPPORTED, "unpreconditioned norm: partial sums do not fit");
  if (!ctx->split) {
    hipLaunchKernelGGL(rich_finalize_kernel, dim3(1), dim3(256), 0, ctx->stream, parts, nparts,
                       width, ctx->d_scalars, 3, bsums, ref, lg.st, lg.hist, lg.h_done, host_iter, cheb_mu,
                       cheb_omegaprod, rr);
    PB_HIP(hipGetLastError());
    return PB_OK;
  }
  PB_TRY(rich_reduce(ctx, nparts, width, nullptr, rr));
  hipLaunchKernelGGL(rich_finalize_kernel, dim3(1), dim3(256), 0, ctx->stream, parts, nparts,
                     width, ctx->d_scalars, 2, bsums, ref, lg.st, lg.hist, lg.h_done, host_iter, cheb_mu,
                     cheb_omegaprod, rr);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int launch_pre_scale_sum(pb_grid* g, const double* src, double* dst, double dinv, int* nparts) {
  ScopedTimer tm(g->ctx, "preonly_sum");
  const int nb = vec_blocks(g->ctx, g->nlocal);
  hipLaunchKernelGGL(pre_scale_sum_kernel, dim3(nb), dim3(256), 0, g->ctx->stream, src, dst,
                     g->nlocal, dinv, g->ctx->d_partials);
  PB_HIP(hipGetLastError());
  *nparts = nb;
  return PB_OK;
}

int launch_pre_shift(pb_grid* g, double* x, double ntot) {
  ScopedTimer tm(g->ctx, "preonly_shift");
  hipLaunchKernelGGL(pre_shift_kernel, dim3(vec_blocks(g->ctx, g->nlocal)), dim3(256), 0,
                     g->ctx->stream, x, g->nlocal, (const double*)g->ctx->d_scalars, ntot);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

// ---------------------------------------------------------------------------------------------
// The fused update passes on the stencil engine (pb_star7.hpp)
// ---------------------------------------------------------------------------------------------
// Richardson (-ksp_type richardson, PETSc KSPSolve_Richardson) on the 7-point operator: the update
// and the residual in one pass. The field is x_new = x + scale (dinv q + shift), formed on load
// from two raw arrays (q = r with Jacobi / no PC, the stored z = M^-1 r otherwise; shift = -mean,
// the null-space removal), every product and sum rounded (no FMA contraction: the build's
// -ffp-contract=off; rich_step in pb_device.hpp is the one definition), so rich_x_kernel
// (pb_ksp_stationary.hip) gives the same bits. The epilogue stores the centre value x_new and
// r_new = b - A x_new (reference summation order) and, with SUMS (Jacobi / no PC), takes the sums
// of t = dinv r_new - mean_old (t, t^2) behind the next iteration's norm and mean. x and (SUMS) r
// go to other buffers than they are read from: neighbouring waves and blocks still read x_old and
// q at this point's neighbours while this block stores. Reads x, q, b and writes x, r: 40 B/DoF,
// pass B's pattern (two streams written, non-temporal), whose launch shape it takes.
// STOREX = false with PlainLoad: the unfused form's second step, r = b - A x of a stored x, with
// the same tiles, chunks and partial sums (tuning rich_fused = 0; bit-identical).
struct RichLoad {
  static constexpr int NR = 2;
  static constexpr bool GHOST_RAW = false;
  const double* __restrict__ x;
  const double* __restrict__ q;
  const CgState* st;
  double scale;
  double dinv = 1.0, shift = 0.0;
  __device__ __forceinline__ void prepare() {
    dinv = st->dinv;
    shift = -st->mu;
  }
  __device__ __forceinline__ const double* src(int a) const { return a == 0 ? x : q; }
  __device__ __forceinline__ double value(const double* raw) const {
    return rich_step<true>(raw[0], raw[1], dinv, shift, scale);
  }
};
// Chebyshev (-ksp_type chebyshev, PETSc KSPSolve_Chebyshev), update i >= 1: the field is
// y_new = omega ((y - ym1) + scale (dinv q + shift)) + ym1, formed on load from three raw arrays
// (omega = the state's alpha, advanced by the finalize before this pass), every operation rounded
// in cheb_step's order (pb_device.hpp), as in cheb_x_kernel (pb_ksp_stationary.hip). RichEpi
// stores y_new and r_new = b - A y_new: reads y, ym1, q, b and writes y, r, 48 B/DoF. y_new goes
// to a third buffer: neighbouring waves and blocks still read y and ym1 around this point.
struct ChebLoad {
  static constexpr int NR = 3;
  static constexpr bool GHOST_RAW = false;
  const double* __restrict__ y;
  const double* __restrict__ ym1;
  const double* __restrict__ q;
  const CgState* st;
  double scale;
  double dinv = 1.0, shift = 0.0, omega = 0.0;
  __device__ __forceinline__ void prepare() {
    dinv = st->dinv;
    shift = -st->mu;
    omega = st->alpha;
  }
  __device__ __forceinline__ const double* src(int a) const {
    return a == 0 ? y : (a == 1 ? ym1 : q);
  }
  __device__ __forceinline__ double value(const double* raw) const {
    return cheb_step<true>(raw[0], raw[1], raw[2], dinv, shift, scale, omega);
  }
};
template <bool STOREX, bool SUMS>
struct RichEpi {
  static constexpr int NS = SUMS ? 2 : 0, NE = 1;
  static constexpr bool RAW = false;
  static constexpr int WGCU = 1;
  static constexpr bool CAP = true, WIDE8 = true;
  static constexpr bool PREFETCH = true;
  double* __restrict__ x_out;
  double* __restrict__ r_out;
  const double* __restrict__ b;
  const CgState* st;
  double dinv = 1.0, mu = 0.0;
  __device__ __forceinline__ void prepare() {
    if constexpr (SUMS) {
      dinv = st->dinv;
      mu = st->mu;
    }
  }
  __device__ __forceinline__ const double* src(int) const { return b; }
  template <int V>
  __device__ __forceinline__ void put(RowIx idx, const double (&c)[V], const double (&w)[V],
                                      double (&op)[1][V], double* acc, int nt) const {
    double rv[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      rv[e] = op[0][e] - w[e];
      if constexpr (SUMS) {
        const double s = dinv * rv[e];
        const double t = s - mu;
        acc[0] += t;
        acc[1] += t * t;
      }
    }
    (void)acc;
    store_row<V>(r_out, idx, rv, nt);
    if constexpr (STOREX) store_row<V>(x_out, idx, c, nt);
  }
};

// Richardson's update + residual pass (RichLoad / RichEpi), whole grid, wrap planes or ghosts of
// x as gp says. q != nullptr: fused, x_out = x + scale (dinv q - mean), r_out = b - A x_out;
// q == nullptr: r_out = b - A x of the stored x (the unfused form and the nonzero-guess setup).
// sums: the two sums of dinv r_out - mean per block into ctx->d_partials (*nparts blocks).
// skip = false: the setup's launch (the state's done flag is not valid yet)
int launch_rich_update(pb_grid* g, const Star& s, const double* x, const double* q,
                       const double* b, double* x_out, double* r_out, const StencilPlanes& gp,
                       const CgState* st, double scale, bool sums, bool skip, int* nparts,
                       int part_off) {
  ScopedTimer tm(g->ctx, q ? "rich_update" : "rich_resid");
  const int* sk = skip ? &st->done : nullptr;
  *nparts = 0;
  if (q) {
    const RichLoad ld{x, q, st, scale};
    if (sums)
      return launch_any(g, s, ld, gp, RichEpi<true, true>{x_out, r_out, b, st},
                        Launch{sk}.sums(part_off, nparts));
    return launch_any(g, s, ld, gp, RichEpi<true, false>{x_out, r_out, b, st}, Launch{sk});
  }
  if (sums)
    return launch_any(g, s, PlainLoad{x}, gp, RichEpi<false, true>{nullptr, r_out, b, st},
                      Launch{sk}.sums(part_off, nparts));
  return launch_any(g, s, PlainLoad{x}, gp, RichEpi<false, false>{nullptr, r_out, b, st},
                    Launch{sk});
}

// Chebyshev's update + residual pass for updates i >= 1 (ChebLoad / RichEpi), whole grid, wrap
// planes; always an iteration's launch (exits at entry once the state is done)
int launch_cheb_update(pb_grid* g, const Star& s, const double* y, const double* ym1,
                       const double* q, const double* b, double* y_out, double* r_out,
                       const StencilPlanes& gp, const CgState* st, double scale, bool sums,
                       int* nparts, int part_off) {
  ScopedTimer tm(g->ctx, "cheb_update");
  *nparts = 0;
  const ChebLoad ld{y, ym1, q, st, scale};
  if (sums)
    return launch_any(g, s, ld, gp, RichEpi<true, true>{y_out, r_out, b, st},
                      Launch{&st->done}.sums(part_off, nparts));
  return launch_any(g, s, ld, gp, RichEpi<true, false>{y_out, r_out, b, st}, Launch{&st->done});
}

}  // namespace pb
