// pb_cg_passes.hip -- the fused CG passes on the stencil engine (pb_star7.hpp) and the kernels
// around them: PETSc KSPSolve_CG + PCJacobi + MatNullSpace with a
// device-resident state. Loaders and epilogues of pass A and pass B (with the p store in either,
// the deferred x update, the finalize stages folded into their prologues), of the
// single-reduction iteration's passes P and S and of the setup from a nonzero guess; the init,
// boundary-plane, finalize and flush kernels; and every launch_cg_* / cg_finalize_* / fold_* the
// solver's host code (pb_ksp_cg.cpp) calls. The scalar logic itself is pb_cg_device.hpp's.
#include "pb_star7.hpp"

namespace pb {

// p_new = (dinv*r + shift) + bb*p_old  -- PCApply_Jacobi + MatNullSpaceRemove + VecAYPX fused
struct CombineLoad {
  static constexpr int NR = 2;
  static constexpr bool GHOST_RAW = false;
  const double* __restrict__ r;
  const double* __restrict__ p;
  const CgState* st;
  double dinv, shift, bb;
  // 1: the state is past stage 1 (betaold already overwritten): take pass A's beta/betaold from
  // bbp, which stage 1 computed with the same operands (pass B re-forming p, PB_CG_PSTORE_B)
  int after1 = 0;
  __device__ __forceinline__ void prepare() { prepare_from(*st); }
  template <class S>
  __device__ __forceinline__ void prepare_from(const S& s) {
    dinv = s.dinv;
    shift = -s.mu;
    bb = after1 ? s.bbp : (s.it == 0 ? 0.0 : s.beta / s.betaold);
  }
  __device__ __forceinline__ const double* src(int a) const { return a == 0 ? r : p; }
  __device__ __forceinline__ double f(double rv, double pv) const {
    double z = dinv * rv;
    z = z + shift;
    return z + bb * pv;
  }
  __device__ __forceinline__ double value(const double* raw) const { return f(raw[0], raw[1]); }
  __device__ __forceinline__ double one(int64_t idx) const { return f(r[idx], p[idx]); }
};

// CG pass A: store p_new, accumulate p.w (VecXDot(P, W)). STORE = false: the
// p store moves to pass B, which re-forms p from r and p_old on load (PB_CG_PSTORE_B): pass A
// becomes read-only (16 B/DoF) and pass B reads 2 / writes 2 arrays (32 B/DoF), same 48 B/DoF.
// Read-only (STORE = false): 4-row tiles, one workgroup per CU (z-chunks of half the slab at
// 512^3), measured 0.378 vs 0.391 ms for 8-row tiles (profiles/r02/ab_pst_defer_512.jsonl).
#ifndef PB_PASSA_TALL
#define PB_PASSA_TALL 0
#endif
template <bool STORE>
struct PassAT {
  static constexpr int NS = 1, NE = 0;
  static constexpr bool RAW = false, TALL = STORE || PB_PASSA_TALL;  // put() takes the Laplacian; 8-row tiles
  static constexpr int WGCU = STORE ? 3 : 1;        // (4-row tiles; 1 with 8 rows)
  static constexpr bool CAP = !STORE, WIDE8 = !STORE;
  static constexpr bool PREFETCH = true;
  // (p stores non-temporal like every engine output: cached stores, which pass B could re-read
  // from the Infinity Cache, measured within noise, profiles/r01/ab_passa_nt.txt)
  double* __restrict__ p_new;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ const double* src(int) const { return nullptr; }
  template <int V>
  __device__ __forceinline__ void put(RowIx idx, const double (&c)[V], const double (&w)[V],
                                      double (&)[1][V], double* acc, int nt) const {
    if constexpr (STORE) store_row<V>(p_new, idx, c, nt);
#pragma unroll
    for (int e = 0; e < V; ++e) acc[0] += w[e] * c[e];
  }
};
using PassA = PassAT<true>;

// CG pass B: r += (-a) w with w = A p recomputed; then the PC/null-space sums of the new
// residual: s = dinv*r, t = s - mu_old:  sum t, sum t^2, sum t*r, sum r.
// The solution update is deferred over D iterations (x is not part of the recurrence; D = 4 by
// default, 2 or 0 by PB_CG_DEFER_X), the directions kept in a ring of D p buffers:
//   XU = 0 (i % D < D-1):      no x traffic, alpha_i p_i stays pending;
//   XU = 3 (D = 4, i % 4 = 3): x += a_{i-3} p_{i-3} + a_{i-2} p_{i-2} + a_{i-1} p_{i-1} + a_i p_i
//   XU = 1 (D = 2, odd i):     x += (alpha_{i-1} p_{i-1} + alpha_i p_i);
//   XU = 2 (no deferral):      x += alpha_i p_i every iteration.
// Operands are prefetched one plane ahead (XU = 1: 3 operand rows, 238 VGPRs -- one workgroup
// per CU is all the grid uses; measured 2 % faster than loading them in the plane's own step).
#ifndef PB_PSTB_WGCU
#define PB_PSTB_WGCU 1
#endif
#ifndef PB_PSTB_TALL
#define PB_PSTB_TALL 0
#endif
// PST (PB_CG_PSTORE_B): the field is p re-formed from (r, p_old) by CombineLoad, stored to p_out;
// r is read from op[0] (= r) and written to r_out (another buffer: neighbouring waves still read
// r through the z-queue, an in-place update would race with them).
// SUMS = false: the single-reduction iteration's pass P (the residual sums move to pass S)
template <int XU, bool PST = false, bool SUMS = true>
struct PassB {
  static constexpr int NS = SUMS ? 4 : 0, NE = XU == 1 ? 3 : (XU == 2 ? 2 : (XU == 3 ? 5 : 1));
  static constexpr bool RAW = false;  // put() takes the Laplacian, not the 7 values
  // one workgroup per CU (z-chunks of half the slab at 512^3): 8-10 % faster than 3 per CU
  static constexpr int WGCU = PST ? PB_PSTB_WGCU : 1;
  static constexpr bool TALL = PST && XU == 0 && PB_PSTB_TALL;  // (A/B builds)
  static constexpr bool CAP = true, WIDE8 = PST && XU == 0;
  static constexpr bool PREFETCH = true;
  double* __restrict__ x;
  double* __restrict__ r;
  const double* __restrict__ p_prev;  // p of iteration i-1
  const double* __restrict__ p_m2;    // XU = 3: p of iterations i-2, i-3
  const double* __restrict__ p_m3;
  const CgState* st;
  double alpha, alpha_prev, dinv, mu, a2, a3;
  double* __restrict__ r_out = nullptr;  // PST only
  double* __restrict__ p_out = nullptr;
  // PST: operands r (op 0) and p_{i-1} = p_old (op 2) are the centre plane's raw z-queue values
  // (CombineLoad arrays 0 and 1) -- taken from the queue instead of loaded again
  static constexpr int qop(int a) { return !PST ? -1 : (a == 0 ? 0 : (a == 2 ? 1 : -1)); }
  __device__ __forceinline__ void prepare() { prepare_from(*st); }
  template <class S>
  __device__ __forceinline__ void prepare_from(const S& s) {
    alpha = s.alpha;
    alpha_prev = s.alpha_prev;
    dinv = s.dinv;
    mu = s.mu;
    if constexpr (XU == 3) {  // pending alphas of iterations i-3, i-2, i-1
      a3 = s.pa[0];
      a2 = s.pa[1];
      alpha_prev = s.pa[2];
    }
  }
  __device__ __forceinline__ const double* src(int a) const {
    return a == 0 ? r : (a == 1 ? x : (a == 2 ? p_prev : (a == 3 ? p_m2 : p_m3)));
  }
  template <int V>
  __device__ __forceinline__ void put(RowIx idx, const double (&c)[V], const double (&w)[V],
                                      double (&op)[NE][V], double* acc, int nt) const {
    double rv[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      rv[e] = op[0][e] + (-alpha) * w[e];
      if constexpr (SUMS) {
        const double s = dinv * rv[e];
        const double t = s - mu;
        acc[0] += t;
        acc[1] += t * t;
        acc[2] += t * rv[e];
        acc[3] += rv[e];
      }
    }
    (void)acc;
    if constexpr (PST) {
      store_row<V>(r_out, idx, rv, nt);
      store_row<V>(p_out, idx, c, nt);
    } else {
      store_row<V>(r, idx, rv, nt);
    }
    if constexpr (XU == 1) {
      double xv[V];
#pragma unroll
      for (int e = 0; e < V; ++e) xv[e] = op[1][e] + (alpha_prev * op[2][e] + alpha * c[e]);
      store_row<V>(x, idx, xv, nt);
    } else if constexpr (XU == 2) {
      double xv[V];
#pragma unroll
      for (int e = 0; e < V; ++e) xv[e] = op[1][e] + alpha * c[e];
      store_row<V>(x, idx, xv, nt);
    } else if constexpr (XU == 3) {  // x += a3 p_{i-3} + a2 p_{i-2} + alpha_prev p_{i-1} + alpha p_i
      double xv[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        double u = a3 * op[4][e];
        u = u + a2 * op[3][e];
        u = u + alpha_prev * op[2][e];
        u = u + alpha * c[e];
        xv[e] = op[1][e] + u;
      }
      store_row<V>(x, idx, xv, nt);
    }
  }
};

// Single-reduction CG pass S (PETSc KSPSolve_CG_SingleReduction: z = B r, S = A z, then z'z,
// z'r and z'S in one reduction): the field is t = dinv r' - mu_old, formed on load (ghost planes
// of a split grid hold raw r' and are transformed too); the engine's Laplacian is s = A t. Sums
// t, t^2, t.r', r' (norm, beta and the mean as pass B's) and t.s (delta = z'A z: z = t - const
// and A annihilates constants, so t'A t is z'A z up to rounding). Read-only: 8 B/DoF.
struct ZLoad {
  static constexpr int NR = 1;
  static constexpr bool GHOST_RAW = true;
  const double* __restrict__ r;
  const CgState* st;
  double dinv = 1.0, shift = 0.0;
  __device__ __forceinline__ void prepare() { prepare_from(*st); }
  template <class S>
  __device__ __forceinline__ void prepare_from(const S& s) {
    dinv = s.dinv;
    shift = -s.mu;
  }
  __device__ __forceinline__ const double* src(int) const { return r; }
  __device__ __forceinline__ double value(const double* raw) const {
    double z = dinv * raw[0];
    return z + shift;
  }
};
struct SrSums {
  static constexpr int NS = 5, NE = 1;
  static constexpr bool RAW = false;
  static constexpr int WGCU = 1;
  static constexpr bool CAP = true, WIDE8 = true;
  static constexpr bool PREFETCH = true;
  // operand 0 (r') is the centre plane's raw queue value
  static constexpr int qop(int a) { return a == 0 ? 0 : -1; }
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ const double* src(int) const { return nullptr; }
  template <int V>
  __device__ __forceinline__ void put(RowIx, const double (&c)[V], const double (&w)[V],
                                      double (&op)[1][V], double* acc, int) const {
#pragma unroll
    for (int e = 0; e < V; ++e) {
      const double t = c[e], rv = op[0][e];
      acc[0] += t;
      acc[1] += t * t;
      acc[2] += t * rv;
      acc[3] += rv;
      acc[4] += t * w[e];
    }
  }
};

// CG setup from a nonzero initial guess (-ksp_initial_guess_nonzero) with Jacobi / no PC: the field
// is x0, the engine's Laplacian y = A x0 (reference order); r = b - y and p = 0 are stored, x0 is
// left alone. Sums: the setup's four of s = dinv r (s, s^2, s.r, r: cg_init_kernel's) and, from b
// already in registers, dinv b and (dinv b)^2 -- the stopping reference ||N(M^-1 b)|| of
// KSPConvergedDefault without a pass of its own. Reads x0, b and writes r, p: 32 B/DoF, pass B's
// pattern (PST, no x update), whose launch shape it takes.
struct GuessInit {
  static constexpr int NS = 6, NE = 1;
  static constexpr bool RAW = false;
  static constexpr int WGCU = 1;
  static constexpr bool CAP = true, WIDE8 = true;
  static constexpr bool PREFETCH = true;
  double* __restrict__ r;
  double* __restrict__ p;
  const double* __restrict__ b;
  double dinv;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ const double* src(int) const { return b; }
  template <int V>
  __device__ __forceinline__ void put(RowIx idx, const double (&c)[V], const double (&w)[V],
                                      double (&op)[1][V], double* acc, int nt) const {
    double rv[V], zero[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      rv[e] = op[0][e] - w[e];
      zero[e] = 0.0;
      const double s = dinv * rv[e];
      acc[0] += s;
      acc[1] += s * s;
      acc[2] += s * rv[e];
      acc[3] += rv[e];
      const double sb = dinv * op[0][e];
      acc[4] += sb;
      acc[5] += sb * sb;
    }
    store_row<V>(r, idx, rv, nt);
    store_row<V>(p, idx, zero, nt);
    (void)c;
  }
};

// ---------------------------------------------------------------------------------------------
// CG (PETSc KSPSolve_CG + PCJacobi + MatNullSpace), device-resident state
// ---------------------------------------------------------------------------------------------
// r = b, x = 0, p = 0 and the sums of s = dinv*r (t = s - 0)
__global__ __launch_bounds__(256) void cg_init_kernel(const double* __restrict__ b,
                                                      double* __restrict__ x,
                                                      double* __restrict__ r,
                                                      double* __restrict__ p, int64_t n,
                                                      double dinv, double* parts) {
  double acc[4] = {0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    double rv = b[i];
    r[i] = rv;
    x[i] = 0.0;
    p[i] = 0.0;
    double s = dinv * rv;
    acc[0] += s;
    acc[1] += s * s;
    acc[2] += s * rv;
    acc[3] += rv;
  }
  block_partials<4>(acc, parts);
}

// boundary planes of p_new (for the halo exchange / periodic self-wrap)
// fold.stage = 2 (split grids): every wave first runs the previous iteration's stage 2 from the
// allreduced sums (a one-block partial) and the lead lane stores the state (fold.out)
__global__ __launch_bounds__(256) void cg_boundary_kernel(const double* __restrict__ r,
                                                          const double* __restrict__ p,
                                                          int64_t plane, int64_t last_off,
                                                          double* __restrict__ lo,
                                                          double* __restrict__ hi,
                                                          const CgState* st, Fold fold) {
  // the first PER points of both planes are loaded before the state (prologue) is ready: the
  // loads do not depend on it, so their latency hides the prologue's (r05: 23.7 -> 13.3 us with
  // one block per CU alone, at 512^2)
  constexpr int PER = 4;
  const int64_t gs = (int64_t)gridDim.x * blockDim.x;
  const int64_t i0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  double vr[2][PER], vp[2][PER];
  auto fetch = [&](int64_t base) {
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int64_t i = min(base + q * gs, plane - 1);  // (clamped: valid address, unused)
      vr[0][q] = r[i];
      vp[0][q] = p[i];
      vr[1][q] = r[last_off + i];
      vp[1][q] = p[last_off + i];
    }
  };
  fetch(i0);
  CgState sst;
  if (fold.stage) {
    fold_prologue(fold, sst);
    st = &sst;
  }
  if (st->done) return;
  CombineLoad c{r, p, nullptr, 0.0, 0.0, 0.0};
  c.prepare_from(*st);
  for (int64_t base = i0; base < plane; base += PER * gs) {
    if (base != i0) fetch(base);
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      const int64_t i = base + q * gs;
      if (i < plane) {
        lo[i] = c.f(vr[0][q], vp[0][q]);
        hi[i] = c.f(vr[1][q], vp[1][q]);
      }
    }
  }
}

// Finalize: deterministic fixed-order reduction of the per-block partials, then the PETSc CG
// scalar logic (KSPSolve_CG + KSPConvergedDefault) on the device. mode bit 1 = reduce partials
// into sums[], bit 2 = update the state from sums[] (split around the RCCL allreduce).
// stage 0 = after init, 1 = after pass A (p.w), 2 = after pass B (residual sums), 3 = delta only.
// the second partial region of -ksp_norm_type unpreconditioned with a stored-z PC (RrParts):
// columns c0, c1 (c1 < 0: none) of nparts x width partials summed by the block's 256 threads in a
// fixed order into out[0..1]
__device__ __forceinline__ void rr_reduce(const RrParts& rr, int c0, int c1, double* out) {
  __shared__ double red2[256][2];
  double v0 = 0.0, v1 = 0.0;
  for (int b = threadIdx.x; b < rr.nparts; b += 256) {
    v0 += rr.parts[(int64_t)b * rr.width + c0];
    if (c1 >= 0) v1 += rr.parts[(int64_t)b * rr.width + c1];
  }
  red2[threadIdx.x][0] = v0;
  red2[threadIdx.x][1] = v1;
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) {
      red2[threadIdx.x][0] += red2[threadIdx.x + off][0];
      red2[threadIdx.x][1] += red2[threadIdx.x + off][1];
    }
    __syncthreads();
  }
  out[0] = red2[0][0];
  out[1] = red2[0][1];
}

// rr.parts != nullptr (stages 0 and 2, width 4): this rank's sum r^2 joins the four as sums[4]
// (mode bit 1) and travels in the same allreduce
__global__ __launch_bounds__(256) void cg_finalize_kernel(const double* __restrict__ parts,
                                                          int nparts, int width, double* sums,
                                                          int mode, int stage, CgState* st,
                                                          double* hist, int* h_done,
                                                          int64_t host_iter, RrParts rr) {
  double S[kMaxSums];
  if ((mode & 1) && rr.parts) {
    double q[2];
    rr_reduce(rr, rr.width == 4 ? 2 : 0, rr.width == 4 ? 3 : -1, q);
    // (pass B's sums: t = r - mu with the mean the state still holds, so t.r + mu r = r^2)
    if (threadIdx.x == 0) sums[4] = rr.width == 4 ? q[0] + st->mu * q[1] : q[0];
  }
  if ((mode & 1) && nparts > kFoldMaxParts) {
    // many partials (elementwise / multigrid kernels): 256-thread fixed-order tree
    __shared__ double red[256][kMaxSums];
    for (int s = 0; s < width; ++s) {
      double v = 0.0;
      for (int b = threadIdx.x; b < nparts; b += 256) v += parts[(int64_t)b * width + s];
      red[threadIdx.x][s] = v;
    }
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
      if ((int)threadIdx.x < off)
        for (int s = 0; s < width; ++s) red[threadIdx.x][s] += red[threadIdx.x + off][s];
      __syncthreads();
    }
    if (threadIdx.x == 0)
      for (int s = 0; s < width; ++s) sums[s] = red[0][s];
  } else if (mode & 1) {
    // up to kFoldMaxParts: one wave, the folded prologues' order (folded == unfolded bits)
    if (threadIdx.x >= 64) return;
    wave_reduce_parts(parts, nparts, width, S);
    if (threadIdx.x == 0)
      for (int s = 0; s < width; ++s) sums[s] = S[s];
  }
  if (!(mode & 2) || threadIdx.x != 0) return;
  const int ws = rr.parts ? 5 : width;
  for (int s = 0; s < kMaxSums; ++s) S[s] = s < ws ? sums[s] : 0.0;
  if (stage == 0) cg_stage0(*st, S, hist, h_done);
  else if (stage == 1) cg_stage1(*st, S[0]);
  else if (stage == 2) cg_stage2(*st, S, hist, h_done, host_iter);
  else st->delta = S[4];  // 3: the single-reduction setup's delta = z0'A z0
}

static int cg_reduce_update(pb_ctx* ctx, int stage, int nparts, int width, const KspLog& lg,
                            int64_t host_iter, const double* parts = nullptr,
                            const RrParts& rr = RrParts{}) {
  CgState* st = lg.st;
  double* hist = lg.hist;
  int* h_done = lg.h_done;
  double* sums = ctx->d_scalars;
  if (!parts) parts = ctx->d_partials;
  ScopedTimer tm(ctx, "cg_finalize");  // (with its allreduce on several ranks)
  // (the PC's own partials must have stayed below the second region)
  if (rr.parts && ((int64_t)nparts * width > ctx->partials_cap / 2 || width != 4))
    return set_error(PB_ERR_UNSUPPORTED, "unpreconditioned norm: partial sums do not fit");
  if (!ctx->split) {
    hipLaunchKernelGGL(cg_finalize_kernel, dim3(1), dim3(256), 0, ctx->stream, parts,
                       nparts, width, sums, 3, stage, st, hist, h_done, host_iter, rr);
    PB_HIP(hipGetLastError());
    return PB_OK;
  }
  hipLaunchKernelGGL(cg_finalize_kernel, dim3(1), dim3(256), 0, ctx->stream, parts,
                     nparts, width, sums, 1, stage, st, hist, h_done, host_iter, rr);
  PB_HIP(hipGetLastError());
  PB_TRY(allreduce_device(ctx, sums, rr.parts ? 5 : width));
  hipLaunchKernelGGL(cg_finalize_kernel, dim3(1), dim3(256), 0, ctx->stream, parts,
                     nparts, width, sums, 2, stage, st, hist, h_done, host_iter, rr);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

static int elementwise_blocks(pb_ctx* ctx, int64_t n) {
  int64_t b = (n + 255) / 256;
  int64_t cap = (int64_t)ctx->num_cus * 8;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

int launch_cg_init(pb_grid* g, const double* b, double* x, double* r, double* p, double dinv,
                   const KspLog& lg) {
  pb_ctx* ctx = g->ctx;
  ScopedTimer tm(ctx, "cg_init");
  const int nb = elementwise_blocks(ctx, g->nlocal);
  hipLaunchKernelGGL(cg_init_kernel, dim3(nb), dim3(256), 0, ctx->stream, b, x, r, p, g->nlocal,
                     dinv, ctx->d_partials);
  PB_HIP(hipGetLastError());
  return cg_reduce_update(ctx, 0, nb, 4, lg, -1);
}

// Setup from a nonzero initial guess: the fused pass (GuessInit) over the planes of `mode`; its
// six sums per block go to ctx->d_partials + part_off * 6
int launch_cg_guess_init(pb_grid* g, const Star& s, const double* x0, const double* b, double* r,
                         double* p, const StencilPlanes& gp, double dinv, int mode, int part_off,
                         int* nblocks) {
  ScopedTimer tm(g->ctx, timer_name(mode, "cg_init_guess", "cg_init_guess_interior",
                                    "cg_init_guess_boundary"));
  return launch_any(g, s, PlainLoad{x0}, gp, GuessInit{r, p, b, dinv},
                    Launch{nullptr, mode}.sums(part_off, nblocks));
}

// cg_finalize_kernel's stage 0 for a setup from a nonzero guess: reduces `width` (4 or 6) sums per
// block in a fixed order (mode bit 1), then runs stage 0 with the stopping reference `ref`
// (REF_*; mode bit 2). The sums of dinv b and (dinv b)^2 behind ||N(M^-1 b)|| are sums[4..5]
// (width 6: the fused pass took them) or bsums[0..1] (taken earlier from M^-1 b)
__global__ __launch_bounds__(256) void cg_guess_finalize_kernel(const double* __restrict__ parts,
                                                                int nparts, int width,
                                                                double* sums, int mode,
                                                                const double* bsums, int ref,
                                                                CgState* st, double* hist,
                                                                int* h_done, RrParts rr) {
  constexpr int W = 6;
  // rr (unpreconditioned norm, stored-z PC; width 4): sum r^2 and sum b^2 of the residual kernel
  // join the four as sums[4..5] -- ||r_0|| and the reference ||b||, no PC application behind it
  if ((mode & 1) && rr.parts) {
    double q[2];
    rr_reduce(rr, 0, 1, q);
    if (threadIdx.x == 0) sums[4] = q[0], sums[5] = q[1];
  }
  if (mode & 1) {
    __shared__ double red[256][W];
    for (int s = 0; s < width; ++s) {
      double v = 0.0;
      for (int b = threadIdx.x; b < nparts; b += 256) v += parts[(int64_t)b * width + s];
      red[threadIdx.x][s] = v;
    }
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
      if ((int)threadIdx.x < off)
        for (int s = 0; s < width; ++s) red[threadIdx.x][s] += red[threadIdx.x + off][s];
      __syncthreads();
    }
    if (threadIdx.x == 0)
      for (int s = 0; s < width; ++s) sums[s] = red[0][s];
  }
  if (!(mode & 2) || threadIdx.x != 0) return;
  double S[kMaxSums];
  for (int s = 0; s < kMaxSums; ++s) S[s] = s < (rr.parts ? 5 : 4) ? sums[s] : 0.0;
  double bnorm = 0.0;
  if (ref != REF_INITIAL && st->norm != PB_KSP_NORM_NONE) {
    const double* bs = bsums ? bsums : sums + 4;
    const double delta = st->nullspace ? bs[0] / st->ntot : 0.0;
    if (st->norm == PB_KSP_NORM_PRECONDITIONED) {
      double zz = bs[1];
      if (st->nullspace) zz = bs[1] - st->ntot * delta * delta;
      bnorm = norm_from_sq(zz);
    } else if (st->norm == PB_KSP_NORM_NATURAL) {
      // sqrt|b . N(M^-1 b)|. bsums: the four sums of t = M^-1 b (t, t^2, t.b, b); the fused
      // setup's pair: sb = dinv b, so b . sb = sum sb^2 / dinv and sum b = sum sb / dinv
      const double bz = bsums ? bs[2] - delta * bs[3] : (bs[1] - delta * bs[0]) / st->dinv;
      bnorm = sqrt(fabs(bz));
    } else {
      // ||b||_2, no PC application: sum b^2 = sum sb^2 / dinv^2 (Jacobi / no PC), or taken beside
      // sum r^2 (rr)
      bnorm = norm_from_sq(rr.parts ? sums[5] : bs[1] / (st->dinv * st->dinv));
    }
  }
  cg_stage0(*st, S, hist, h_done, ref, bnorm);
}

int cg_finalize_guess(pb_ctx* ctx, int nparts, int width, const double* bsums, int ref,
                      const KspLog& lg, const RrParts& rr) {
  CgState* st = lg.st;
  double* hist = lg.hist;
  int* h_done = lg.h_done;
  double* sums = ctx->d_scalars;
  if (rr.parts && ((int64_t)nparts * width > ctx->partials_cap / 2 || width != 4))
    return set_error(PB_ERR_UNSUPPORTED, "unpreconditioned norm: partial sums do not fit");
  if (!ctx->split) {
    hipLaunchKernelGGL(cg_guess_finalize_kernel, dim3(1), dim3(256), 0, ctx->stream,
                       (const double*)ctx->d_partials, nparts, width, sums, 3, bsums, ref, st, hist,
                       h_done, rr);
    PB_HIP(hipGetLastError());
    return PB_OK;
  }
  hipLaunchKernelGGL(cg_guess_finalize_kernel, dim3(1), dim3(256), 0, ctx->stream,
                     (const double*)ctx->d_partials, nparts, width, sums, 1, bsums, ref, st, hist,
                     h_done, rr);
  PB_HIP(hipGetLastError());
  PB_TRY(allreduce_device(ctx, sums, rr.parts ? 6 : width));
  hipLaunchKernelGGL(cg_guess_finalize_kernel, dim3(1), dim3(256), 0, ctx->stream,
                     (const double*)ctx->d_partials, nparts, width, sums, 2, bsums, ref, st, hist,
                     h_done, rr);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int launch_cg_boundary(pb_grid* g, const double* r, const double* p_old, CgState* st,
                       const Fold& fold, hipStream_t stream) {
  pb_ctx* ctx = g->ctx;
  hipStream_t sm = stream ? stream : ctx->stream;
  hipEvent_t tev = nullptr;
  const bool timed = ctx->timing && timer_wanted(ctx, "cg_boundary");
  if (timed) timer_begin(ctx, "cg_boundary", &tev, sm);
  // one block per CU at most, four points of each plane per thread (every wave of the folded
  // form runs the stage-2 prologue first)
  const int nb = (int)std::max<int64_t>(
      1, std::min<int64_t>(ctx->num_cus, (g->plane + 256 * 4 - 1) / (256 * 4)));
  hipLaunchKernelGGL(cg_boundary_kernel, dim3(nb), dim3(256), 0, sm, r, p_old, g->plane,
                     (g->nzl - 1) * g->plane, g->bnd_lo, g->bnd_hi, (const CgState*)st, fold);
  PB_HIP(hipGetLastError());
  if (timed) timer_end(ctx, "cg_boundary", tev, sm);
  return PB_OK;
}

int launch_cg_boundary(pb_grid* g, const double* r, const double* p_old, CgState* st) {
  return launch_cg_boundary(g, r, p_old, st, Fold{});
}

int launch_cg_pass_a(pb_grid* g, const Star& s, const CgPassA& a) {
  ScopedTimer tm(g->ctx,
                 timer_name(a.mode, "cg_pass_a", "cg_pass_a_interior", "cg_pass_a_boundary"));
  // with a fold the prologue leaves the state (and the done flag) in registers
  CgState* st = a.fold.stage ? nullptr : a.st;
  const CombineLoad ld{a.r, a.p_old, st, 0.0, 0.0, 0.0};
  Launch lc = Launch{st ? &st->done : nullptr, a.mode}.sums(a.part_off, a.nblocks);
  lc.fold = a.fold;
  if (!a.store) return launch_any(g, s, ld, a.gp, PassAT<false>{a.p_new}, lc);
  return launch_any(g, s, ld, a.gp, PassA{a.p_new}, lc);
}

// Folded iteration: partial sums of pass A at block 0, of pass B at fold_parts_b_off(); state
// slots st2[0] (read by pass B, written by pass A) and st2[1].
static int64_t fold_parts_b_off(const pb_ctx* ctx) { return ctx->partials_cap / 8; }

static Fold fold_of(int stage, const double* parts, int nparts, int width, const CgState* in,
                    CgState* out, const KspLog& lg, int64_t host_iter) {
  Fold f;
  f.stage = stage;
  f.nparts = nparts;
  f.width = width;
  f.parts = parts;
  f.in = in;
  f.out = out;
  f.hist = lg.hist;
  f.h_done = lg.h_done;
  f.host_iter = host_iter;
  return f;
}
Fold fold_stage2_allreduced(const pb_ctx* ctx, int width, const KspLog& lg, int64_t host_iter) {
  return fold_of(2, ctx->d_scalars, 1, width, lg.st + 1, lg.st, lg, host_iter);
}
Fold fold_stage2_pass_b(const pb_ctx* ctx, int nparts_b, const KspLog& lg, int64_t host_iter) {
  return fold_of(2, ctx->d_partials + fold_parts_b_off(ctx) * 4, nparts_b, 4, lg.st + 1, lg.st, lg,
                 host_iter);
}
Fold fold_stage1_pass_a(const pb_ctx* ctx, int nparts_a, bool allreduced, CgState* st2) {
  return fold_of(1, allreduced ? ctx->d_scalars : ctx->d_partials, nparts_a, 1, st2, st2 + 1,
                 KspLog{nullptr, nullptr, nullptr}, 0);
}
Fold fold_sr_top(bool sums, const double* parts, int nparts_s, const CgState* in, CgState* out,
                 const KspLog& lg, int64_t host_iter) {
  return fold_of(sums ? 3 : 4, parts, nparts_s, 5, in, out, lg, host_iter);
}

// split grids, folded iteration: reduce a pass's partials and allreduce them into d_scalars, where
// the next kernel's prologue reads them as a one-block partial (pass A's -> pass B; pass B's ->
// the next boundary-plane kernel); b_region: pass B's partials (fold_parts_b_off)
int cg_reduce_allreduce(pb_ctx* ctx, int nparts, int width, bool b_region) {
  return cg_reduce_allreduce(ctx, ctx->d_partials + (b_region ? fold_parts_b_off(ctx) * 4 : 0),
                             nparts, width);
}

int cg_reduce_allreduce(pb_ctx* ctx, const double* parts, int nparts, int width) {
  hipLaunchKernelGGL(cg_finalize_kernel, dim3(1), dim3(256), 0, ctx->stream, parts, nparts, width,
                     ctx->d_scalars, 1, 0, (CgState*)nullptr, (double*)nullptr, (int*)nullptr,
                     (int64_t)0, RrParts{});
  PB_HIP(hipGetLastError());
  return allreduce_device(ctx, ctx->d_scalars, width);
}

// the residual-sum stage (2) on st in place from sums already allreduced into d_scalars
int cg_stage2_from_sums(pb_ctx* ctx, int width, const KspLog& lg, int64_t host_iter) {
  hipLaunchKernelGGL(cg_finalize_kernel, dim3(1), dim3(256), 0, ctx->stream,
                     (const double*)nullptr, 0, width, ctx->d_scalars, 2, 2, lg.st, lg.hist,
                     lg.h_done, host_iter, RrParts{});
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int cg_finalize_init(pb_ctx* ctx, int nparts, const KspLog& lg, const RrParts& rr) {
  return cg_reduce_update(ctx, 0, nparts, 4, lg, -1, nullptr, rr);
}

int cg_finalize_pass_a(pb_ctx* ctx, int nparts, CgState* st) {
  return cg_reduce_update(ctx, 1, nparts, 1, KspLog{st, nullptr, nullptr}, 0);
}

int cg_finalize_stage2(pb_ctx* ctx, int nparts, const KspLog& lg, int64_t host_iter,
                       const RrParts& rr) {
  return cg_reduce_update(ctx, 2, nparts, 4, lg, host_iter, nullptr, rr);
}

// pass B variants by the x-update position; fold.stage = 1: stage 1 in the prologue (partials
// of pass A at block 0, state st2[0] -> st2[1]) and the partials written at fold_parts_b_off().
// ps.r_out != nullptr (PB_CG_PSTORE_B): pass B re-forms p = CombineLoad(ps.zsrc, p_old) on load,
// stores it to p, reads r and writes the new residual to ps.r_out.
template <int XU, bool PST>
static int pass_b_one(pb_grid* g, const Star& s, const CgPassB& b, const char* timer) {
  ScopedTimer tm(g->ctx, timer);
  CgState* st = b.fold.stage ? nullptr : b.st;
  // rr: the sums go to the second region, where the PC's sums do not overwrite them
  const int off = b.fold.stage ? (int)fold_parts_b_off(g->ctx)
                               : (b.rr ? rr_part_off(g->ctx, 4) : 0);
  Launch lc = Launch{st ? &st->done : nullptr}.sums(off, b.nparts);
  lc.rev = 1;  // (pass A marched upwards)
  lc.fold = b.fold;
  PassB<XU, PST> ep{b.x, b.r, b.p_prev[0], XU == 3 ? b.p_prev[1] : nullptr,
                    XU == 3 ? b.p_prev[2] : nullptr, st, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if constexpr (PST) {
    ep.r_out = b.ps.r_out;
    ep.p_out = const_cast<double*>(b.p);
    CombineLoad ld{b.ps.zsrc, b.p_prev[0], st, 0.0, 0.0, 0.0};
    ld.after1 = 1;
    return launch_any(g, s, ld, b.gp, ep, lc);
  } else {
    return launch_any(g, s, PlainLoad{b.p}, b.gp, ep, lc);
  }
}

template <bool PST>
static int pass_b_pick(pb_grid* g, const Star& s, const CgPassB& b) {
  if (b.defer == 0) return pass_b_one<2, PST>(g, s, b, "cg_pass_b");
  if (b.host_iter % b.defer != b.defer - 1) return pass_b_one<0, PST>(g, s, b, "cg_pass_b_even");
  if (b.defer == 2) return pass_b_one<1, PST>(g, s, b, "cg_pass_b_odd");
  return pass_b_one<3, PST>(g, s, b, "cg_pass_b_x4");
}

int launch_cg_pass_b(pb_grid* g, const Star& s, const CgPassB& b) {
  PB_TRY(b.ps.r_out ? pass_b_pick<true>(g, s, b) : pass_b_pick<false>(g, s, b));
  if (b.rr) *b.rr = RrParts{rr_region(g->ctx), *b.nparts, 4};
  return PB_OK;
}

// after the last folded iteration of a pb_ksp_iterate call: its stage 2 (in place on st2[1]),
// then st2[0] = st2[1], so the unfolded entry points find the complete state in slot 0
int cg_fold_tail(pb_ctx* ctx, int nparts_b, const KspLog& lg, int64_t host_iter) {
  CgState* st2 = lg.st;
  // split grids: pass B's sums are already reduced and allreduced into d_scalars (mode 2 only)
  hipLaunchKernelGGL(cg_finalize_kernel, dim3(1), dim3(256), 0, ctx->stream,
                     ctx->d_partials + fold_parts_b_off(ctx) * 4, nparts_b, 4, ctx->d_scalars,
                     ctx->split ? 2 : 3, 2, st2 + 1, lg.hist, lg.h_done, host_iter, RrParts{});
  PB_HIP(hipGetLastError());
  PB_HIP(hipMemcpyAsync(st2, st2 + 1, sizeof(CgState), hipMemcpyDeviceToDevice, ctx->stream));
  return PB_OK;
}

// ---------------------------------------------------------------------------------------------
// Single-reduction CG (-ksp_cg_single_reduction): pass P (p, r' and the deferred x update; no
// sums) and pass S (t = dinv r' - mu, s = A t, five sums). 32 + 8 B/DoF per iteration (+ the x
// update's 32 every fourth), one reduction -- against 16 + 32 and two for the KSPSolve_CG passes.
// ---------------------------------------------------------------------------------------------
template <int XU>
static int sr_pass_p_one(pb_grid* g, const Star& s, const double* r, const double* const* p_prev,
                         double* p_new, double* x, double* r_out, const StencilPlanes& gp,
                         const Fold& f, int mode) {
  PassB<XU, true, false> ep{x, nullptr, p_prev[0], XU == 3 ? p_prev[1] : nullptr,
                            XU == 3 ? p_prev[2] : nullptr, nullptr, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  ep.r_out = r_out;
  ep.p_out = p_new;
  CombineLoad ld{r, p_prev[0], nullptr, 0.0, 0.0, 0.0};
  ld.after1 = 1;  // b = beta / betaold as the prologue's top found it (bbp)
  Launch lc{nullptr, mode};
  lc.rev = 1;
  lc.fold = f;
  return launch_any(g, s, ld, gp, ep, lc);
}

int launch_cg_sr_pass_p(pb_grid* g, const Star& s, const double* r, const double* const* p_prev,
                        double* p_new, double* x, double* r_out, const StencilPlanes& gp,
                        const Fold& f, int mode, int64_t host_iter, int defer) {
  if (defer == 4 && host_iter % 4 == 3) {
    ScopedTimer tm(g->ctx, timer_name(mode, "cg_sr_p_x4", "cg_sr_p_x4_interior", "cg_sr_p_x4_boundary"));
    return sr_pass_p_one<3>(g, s, r, p_prev, p_new, x, r_out, gp, f, mode);
  }
  if (defer == 4) {
    ScopedTimer tm(g->ctx, timer_name(mode, "cg_sr_p", "cg_sr_p_interior", "cg_sr_p_boundary"));
    return sr_pass_p_one<0>(g, s, r, p_prev, p_new, x, r_out, gp, f, mode);
  }
  if (defer == 2 && host_iter % 2 == 1) {
    ScopedTimer tm(g->ctx, timer_name(mode, "cg_sr_p_x2", "cg_sr_p_x2_interior", "cg_sr_p_x2_boundary"));
    return sr_pass_p_one<1>(g, s, r, p_prev, p_new, x, r_out, gp, f, mode);
  }
  if (defer == 2) {
    ScopedTimer tm(g->ctx, timer_name(mode, "cg_sr_p", "cg_sr_p_interior", "cg_sr_p_boundary"));
    return sr_pass_p_one<0>(g, s, r, p_prev, p_new, x, r_out, gp, f, mode);
  }
  ScopedTimer tm(g->ctx, timer_name(mode, "cg_sr_p_x1", "cg_sr_p_x1_interior", "cg_sr_p_x1_boundary"));
  return sr_pass_p_one<2>(g, s, r, p_prev, p_new, x, r_out, gp, f, mode);
}

int launch_cg_sr_pass_s(pb_grid* g, const Star& s, const double* r, const StencilPlanes& gp,
                        const CgState* st, int mode, int part_off, int part_end, int* nblocks) {
  ScopedTimer tm(g->ctx, timer_name(mode, "cg_sr_s", "cg_sr_s_interior", "cg_sr_s_boundary"));
  // (marches upwards after pass P marched downwards: it starts on the planes P wrote last)
  // 4-row tiles, two workgroups per CU (a single read-only stream: 0.218-0.221 ms at 512^3 against
  // 0.247 with one per CU, 0.223-0.228 with three, 0.224 with 8-row tiles)
  Launch lc = Launch{&st->done, mode}.sums(part_off, nblocks, part_end);
  lc.wgcu = 2;
  return launch_any(g, s, ZLoad{r, st}, gp, SrSums{}, lc);
}

int cg_sr_finalize(pb_ctx* ctx, const double* parts, int nparts, const KspLog& lg,
                   int64_t host_iter, bool stage_delta0) {
  return cg_reduce_update(ctx, stage_delta0 ? 3 : 2, nparts, 5, lg, host_iter, parts);
}

// x += alpha * p (the pending half of the deferred solution update)
__global__ __launch_bounds__(256) void cg_flush_kernel(double* __restrict__ x,
                                                       const double* __restrict__ p, int64_t n,
                                                       double alpha) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    x[i] = x[i] + alpha * p[i];
}

int launch_cg_flush(pb_grid* g, double* x, const double* p, double alpha) {
  const int nb = elementwise_blocks(g->ctx, g->nlocal);
  hipLaunchKernelGGL(cg_flush_kernel, dim3(nb), dim3(256), 0, g->ctx->stream, x, p, g->nlocal, alpha);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

}  // namespace pb
