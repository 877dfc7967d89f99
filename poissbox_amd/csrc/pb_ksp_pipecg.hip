// pb_ksp_pipecg.hip -- the device side of -ksp_type pipecg: pipelined CG, PETSc
// KSPSolve_PIPECG (Ghysels & Vanroose) with PC_LEFT, KSPConvergedDefault and the constant null
// space. The small state (PcgState, pb_ksp.hpp) with its finalize kernel -- the one reduction of
// an iteration, the norm logged and tested, beta and alpha -- and the field passes of the setup
// and of the unfused iteration: the sum of a field, the Jacobi / identity preconditioner with its
// null-space shift (the 7-point operator on one rank forms it on load instead: PcgLoad,
// below), the setup's five sums. The update pass itself runs in the stencil engine's tiles
// (pb_star7.hpp: PcgEpi with the engine's Laplacian, or with a stored n), so that the fused and
// the unfused iteration sum their partials in one order and give the same bits.
//
// Breakdown: like PETSc's pipecg this has no indefinite-PC or indefinite-matrix test. A zero or
// non-finite denominator (delta at i = 0, delta - (beta / alpha_old) gamma later, gamma_old) makes
// alpha or beta non-finite, the next vectors with it, and the solve ends DIVERGED_NANORINF at the
// next test (under -ksp_norm_type none, which tests nothing, at max_it).
//
// The host enqueues iterations ahead of its convergence poll, so every kernel here that writes a
// vector or the state exits at entry once the state is done. Field passes as pb_ksp_fgmres.hip's:
// 16-byte accesses, grid-stride, a scalar tail; every product and sum rounded (no contraction).
#include "pb_ksp.hpp"
#include "pb_device.hpp"
#include "pb_cg_device.hpp"
#include "pb_star7.hpp"

namespace pb {

static int pcg_grid(pb_ctx* ctx, int64_t n2) {
  int64_t b = (n2 + 511) / 512;
  const int64_t cap = (int64_t)ctx->num_cus * 8;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

// parts[block] = this block's share of sum v
__global__ __launch_bounds__(256) void pcg_sum_kernel(const double* __restrict__ v,
                                                      const CgState* __restrict__ st, int skip,
                                                      int64_t n, double* parts) {
  if (skip && st->done) return;  // (uniform: the partials of a done state are never used)
  const int64_t n2 = n >> 1;
  dv2 acc = dv2{0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256)
    acc += reinterpret_cast<const dv2*>(v)[i];
  double s[1] = {acc.x + acc.y};
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) s[0] += v[n - 1];
  block_partials<1>(s, parts);
}

template <bool SHIFT>
__global__ __launch_bounds__(256) void pcg_pcshift_kernel(const double* src, double* dst,
                                                          const double* __restrict__ sum,
                                                          const CgState* __restrict__ st,
                                                          int skip, int64_t n) {
  if (skip && st->done) return;
  const double dinv = st->dinv;
  const double shift = SHIFT ? pcg_shift(dinv, *sum, st->ntot) : 0.0;
  const int64_t n2 = n >> 1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2;
       i += (int64_t)gridDim.x * 256) {
    const dv2 v = reinterpret_cast<const dv2*>(src)[i];
    dv2 m;
    m.x = fg_z<SHIFT>(v.x, dinv, shift);
    m.y = fg_z<SHIFT>(v.y, dinv, shift);
    reinterpret_cast<dv2*>(dst)[i] = m;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    dst[n - 1] = fg_z<SHIFT>(src[n - 1], dinv, shift);
}

// the five sums of pcg_update, of vectors as they are
__global__ __launch_bounds__(256) void pcg_sums_kernel(const double* __restrict__ r,
                                                       const double* __restrict__ u,
                                                       const double* __restrict__ w, int64_t n,
                                                       double* parts) {
  double acc[kPcgSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double rv = r[i], uv = u[i], wv = w[i];
    acc[0] += rv * uv;
    acc[1] += wv * uv;
    acc[2] += uv * uv;
    acc[3] += rv * rv;
    acc[4] += wv;
  }
  block_partials<kPcgSums>(acc, parts);
}

// the number -ksp_norm_type logs and tests, from the sums (gamma, delta, sum u^2, sum r^2, sum w)
__device__ __forceinline__ double pcg_dp(int norm, const double* S) {
  if (norm == PB_KSP_NORM_PRECONDITIONED) return norm_from_sq(S[2]);
  if (norm == PB_KSP_NORM_UNPRECONDITIONED) return norm_from_sq(S[3]);
  if (norm == PB_KSP_NORM_NATURAL) return sqrt(fabs(S[0]));
  return 0.0;
}

__global__ __launch_bounds__(256) void pcg_finalize_kernel(CgState* st_g, PcgState* ps,
                                                           const double* __restrict__ parts,
                                                           int nparts, double* hist, int* h_done,
                                                           int setup, int ref, int64_t host_iter) {
  if (!setup && st_g->done) {  // (uniform)
    if (threadIdx.x == 0 && h_done) h_done[host_iter + 1] = 1;
    return;
  }
  if (nparts > 0) {
    double acc[kPcgSums] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int b = threadIdx.x; b < nparts; b += 256)
#pragma unroll
      for (int s = 0; s < kPcgSums; ++s) acc[s] += parts[(int64_t)b * kPcgSums + s];
    block_partials<kPcgSums>(acc, ps->sums);  // (one block: its "partials" are the sums)
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  CgState& st = *st_g;
  const double* S = ps->sums;
  const double gamma = S[0], delta = S[1];
  const double dp = pcg_dp(st.norm, S);
  if (setup) {
    double rn0 = dp;
    const double bn = pcg_dp(st.norm, ps->bsums);
    if (ref == REF_RHS) rn0 = bn == 0.0 ? dp : bn;
    else if (ref == REF_MIN) rn0 = fmin(bn, dp);
    st.rnorm0 = rn0;
    st.ttol = fmax(st.rtol * rn0, st.atol);
    st.it = 0;
    st.mu = 0.0;
    st.pend_iter = -1;
    st.pend_count = 0;
    st.reason = 0;
  } else {
    st.it = st.it + 1;
  }
  st.its = st.it;
  st.dp = dp;
  if (st.its < st.nhist) {
    if (hist) hist[st.its] = dp;
    st.nlog = st.its + 1;
  }
  ksp_default_test(st, dp, !setup || ref != REF_ZERO_GUESS);
  if (!st.reason && st.its >= st.max_it) st.reason = PB_KSP_DIVERGED_ITS;
  if (!st.reason) {
    // the update that follows: i = 0 from the device's count (the host enqueues ahead)
    if (st.it == 0) {
      ps->beta = 0.0;
      ps->alpha = gamma / delta;
    } else {
      const double beta = gamma / ps->gamma_old;
      ps->beta = beta;
      ps->alpha = gamma / (delta - (beta / ps->alpha) * gamma);
    }
    ps->gamma_old = gamma;
  }
  st.done = st.reason != 0;
  ablate_keep_going(st);
  if (h_done) h_done[setup ? 0 : host_iter + 1] = st.done;
}

static int pcg_reduce(pb_ctx* ctx, int nb, int width, double* dst) {
  PB_TRY(reduce_partials(ctx, ctx->d_partials, nb, width, dst));
  return ctx->split ? allreduce_device(ctx, dst, width) : PB_OK;
}

int launch_pcg_sum(pb_ctx* ctx, const double* v, double* dst, const CgState* st, bool skip,
                   int64_t n) {
  const int nb = pcg_grid(ctx, n >> 1);
  if (nb > ctx->partials_cap)
    return set_error(PB_ERR_UNSUPPORTED, "pipecg: partial sums do not fit");
  hipLaunchKernelGGL(pcg_sum_kernel, dim3(nb), dim3(256), 0, ctx->stream, v, st, skip ? 1 : 0, n,
                     ctx->d_partials);
  PB_HIP(hipGetLastError());
  return pcg_reduce(ctx, nb, 1, dst);
}

int launch_pcg_pcshift(pb_ctx* ctx, const double* src, double* dst, const double* sum,
                       const CgState* st, bool skip, int64_t n, bool nullspace) {
  ScopedTimer tm(ctx, "pipecg_pc");
  const int nb = pcg_grid(ctx, n >> 1);
  if (nullspace)
    hipLaunchKernelGGL(pcg_pcshift_kernel<true>, dim3(nb), dim3(256), 0, ctx->stream, src, dst,
                       sum, st, skip ? 1 : 0, n);
  else
    hipLaunchKernelGGL(pcg_pcshift_kernel<false>, dim3(nb), dim3(256), 0, ctx->stream, src, dst,
                       sum, st, skip ? 1 : 0, n);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int launch_pcg_sums(pb_ctx* ctx, const double* r, const double* u, const double* w, double* dst,
                    int64_t n) {
  const int nb = pcg_grid(ctx, n);
  if ((int64_t)nb * kPcgSums > ctx->partials_cap)
    return set_error(PB_ERR_UNSUPPORTED, "pipecg: partial sums do not fit");
  hipLaunchKernelGGL(pcg_sums_kernel, dim3(nb), dim3(256), 0, ctx->stream, r, u, w, n,
                     ctx->d_partials);
  PB_HIP(hipGetLastError());
  return pcg_reduce(ctx, nb, kPcgSums, dst);
}

int launch_pcg_finalize(pb_ctx* ctx, const KspLog& lg, PcgState* ps, const double* parts,
                        int nparts, bool setup, int ref, int64_t host_iter) {
  ScopedTimer tm(ctx, "pipecg_finalize");
  hipLaunchKernelGGL(pcg_finalize_kernel, dim3(1), dim3(256), 0, ctx->stream, lg.st, ps, parts,
                     nparts, lg.hist, lg.h_done, setup ? 1 : 0, ref, host_iter);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

// ---------------------------------------------------------------------------------------------
// The iteration pass on the stencil engine (pb_star7.hpp)
// ---------------------------------------------------------------------------------------------
// Pipelined CG (-ksp_type pipecg) on the 7-point operator with Jacobi / no PC:
// the whole iteration in one pass. The field is the preconditioned vector m = dinv w + shift,
// formed on load from w (the shift follows from sum w, one of the five sums of the iteration's one
// reduction: pcg_shift / fg_z in pb_device.hpp are the one definition, so pcg_pcshift_kernel and
// the standalone operator give the same bits); the engine's Laplacian is n = A m (reference
// summation order). The epilogue reads z, q, s, p, x, r, u and w at the point, takes m from the
// z-queue's centre, performs the eight updates (pcg_update) with the state's alpha and beta and
// accumulates the five sums of the new values. z, q, s, p, x, r, u are updated in place: a point
// is read and written by one lane. w_new goes to the other w buffer: neighbouring waves and
// blocks still read w around this point. 64 B read, 64 B written per DoF.
// Eight operand rows of a 4-row tile are 64 doubles: prefetching them one plane ahead (as PassB
// does with up to 5) would double that and leave the registers of the file; they are loaded in
// the plane's own step, ahead of the z-queue's loads, and no 8-row tiles (WIDE8) are used.
template <bool SHIFT>
struct PcgLoad {
  static constexpr int NR = 1;
  static constexpr bool GHOST_RAW = false;
  const double* __restrict__ w;
  const PcgState* ps;
  const CgState* st;
  double dinv = 1.0, shift = 0.0;
  __device__ __forceinline__ void prepare() {
    dinv = st->dinv;
    if constexpr (SHIFT) shift = pcg_shift(dinv, ps->sums[4], st->ntot);
  }
  __device__ __forceinline__ const double* src(int) const { return w; }
  __device__ __forceinline__ double value(const double* raw) const {
    return fg_z<SHIFT>(raw[0], dinv, shift);
  }
};
struct PcgEpi {
  static constexpr int NS = kPcgSums, NE = 8;
  static constexpr bool RAW = false;
  static constexpr int WGCU = 1;
  static constexpr bool CAP = true;
  static constexpr bool PREFETCH = false;
  PcgVecs v;
  const PcgState* ps;
  const CgState* st;
  double alpha = 0.0, beta = 0.0;
  bool first = false;
  __device__ __forceinline__ void prepare() {
    alpha = ps->alpha;
    beta = ps->beta;
    first = st->it == 0;
  }
  __device__ __forceinline__ const double* src(int a) const {
    return a == 0 ? v.z
                  : (a == 1 ? v.q
                            : (a == 2 ? v.s
                                      : (a == 3 ? v.p
                                                : (a == 4 ? v.x
                                                          : (a == 5 ? v.r : (a == 6 ? v.u : v.w))))));
  }
  // c = m, w = n at the point
  template <int V>
  __device__ __forceinline__ void put(RowIx idx, const double (&c)[V], const double (&w)[V],
                                      double (&op)[NE][V], double* acc, int nt) const {
#pragma unroll
    for (int e = 0; e < V; ++e)
      pcg_update(first, alpha, beta, c[e], w[e], op[0][e], op[1][e], op[2][e], op[3][e], op[4][e],
                 op[5][e], op[6][e], op[7][e], acc);
    store_row<V>(v.z, idx, op[0], nt);
    store_row<V>(v.q, idx, op[1], nt);
    store_row<V>(v.s, idx, op[2], nt);
    store_row<V>(v.p, idx, op[3], nt);
    store_row<V>(v.x, idx, op[4], nt);
    store_row<V>(v.r, idx, op[5], nt);
    store_row<V>(v.u, idx, op[6], nt);
    store_row<V>(v.w_out, idx, op[7], nt);
  }
};

// Pipelined CG's iteration pass (PcgLoad / PcgEpi), whole grid, wrap planes, and the same
// epilogue from stored m and n; always an iteration's launch (exits at entry once the state is
// done). The five sums per block go to ctx->d_partials (*nparts blocks)
int launch_pcg_fused(pb_grid* g, const Star& s, const PcgVecs& v, const PcgState* ps,
                     const CgState* st, bool nullspace, int* nparts) {
  ScopedTimer tm(g->ctx, "pipecg_pass");
  const StencilPlanes gp = wrap_planes();
  const PcgEpi ep{v, ps, st};
  const Launch lc = Launch{&st->done}.sums(0, nparts);
  if (nullspace)
    return launch_any(g, s, PcgLoad<true>{v.w, ps, st}, gp, ep, lc);
  return launch_any(g, s, PcgLoad<false>{v.w, ps, st}, gp, ep, lc);
}

int launch_pcg_update(pb_grid* g, const double* m, const double* n, const PcgVecs& v,
                      const PcgState* ps, const CgState* st, int* nparts) {
  ScopedTimer tm(g->ctx, "pipecg_update");
  return launch_tiled(g, m, n, PcgEpi{v, ps, st}, &st->done, nparts);
}

}  // namespace pb
