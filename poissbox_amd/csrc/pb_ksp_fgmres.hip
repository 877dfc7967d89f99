// pb_ksp_fgmres.hip -- the device side of -ksp_type fgmres: the small state of
// a cycle (FgState, pb_ksp.hpp) with its one-thread kernels -- the cycle start, the Arnoldi step's
// scalar part, the triangular solve -- and the field passes around them: the basis vector's
// scaling, the Jacobi / identity preconditioner with its null-space shift (the 7-point operator
// on one rank runs these two and the operator as one engine pass instead: FgLoad below),
// the sum and shift behind a stored-z preconditioner, and the solution build over the live
// directions. The orthogonalisation itself is the multi-dot / multi-axpy pair of pb_guess.hip, the
// operator and the stored-z preconditioners are the KSP's.
//
// The host enqueues steps ahead of its convergence poll, so every kernel here that writes a basis
// vector, a preconditioned direction, x or the state exits at entry once the state is done: what
// the solve formed stays as it was for pb_ksp_end's build, which reads the live count from the
// device. Field passes: 16-byte accesses, grid-stride with the block cap of the other vector
// kernels, an odd length ends in a scalar tail; every product and sum rounded (no contraction).
#include "pb_ksp.hpp"
#include "pb_device.hpp"
#include "pb_cg_device.hpp"
#include "pb_star7.hpp"

namespace pb {

static int fg_grid(pb_ctx* ctx, int64_t n2) {
  int64_t b = (n2 + 511) / 512;
  const int64_t cap = (int64_t)ctx->num_cus * 8;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

__global__ __launch_bounds__(256) void fg_scale_kernel(const double* __restrict__ w,
                                                       double* __restrict__ v,
                                                       const FgState* __restrict__ fs,
                                                       const CgState* __restrict__ st, int64_t n) {
  if (st->done) return;
  const double s = fs->scale;
  const int64_t n2 = n >> 1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256)
    reinterpret_cast<dv2*>(v)[i] = s * reinterpret_cast<const dv2*>(w)[i];
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) v[n - 1] = s * w[n - 1];
}

// parts[block] = this block's share of sum z (z as a stored-z PC wrote it)
__global__ __launch_bounds__(256) void fg_zsum_kernel(const double* __restrict__ z,
                                                      const CgState* __restrict__ st, int64_t n,
                                                      double* parts) {
  if (st->done) return;  // (uniform over the grid: the partials of a done state are never read)
  const int64_t n2 = n >> 1;
  dv2 acc = dv2{0.0, 0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256)
    acc += reinterpret_cast<const dv2*>(z)[i];
  double s[1] = {acc.x + acc.y};
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) s[0] += z[n - 1];
  block_partials<1>(s, parts);
}

// z = dinv v + shift (fg_z: PCJacobi's stored reciprocal, dinv = 1 without a PC; the shift is the
// state's, from the sum the multi-axpy left)
template <bool SHIFT>
__global__ __launch_bounds__(256) void fg_pcshift_kernel(const double* __restrict__ v,
                                                         double* __restrict__ z,
                                                         const FgState* __restrict__ fs,
                                                         const CgState* __restrict__ st,
                                                         int64_t n) {
  if (st->done) return;
  const double dinv = st->dinv, shift = fs->shift;
  const int64_t n2 = n >> 1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2;
       i += (int64_t)gridDim.x * 256) {
    const dv2 vv = reinterpret_cast<const dv2*>(v)[i];
    dv2 zv;
    zv.x = fg_z<SHIFT>(vv.x, dinv, shift);
    zv.y = fg_z<SHIFT>(vv.y, dinv, shift);
    reinterpret_cast<dv2*>(z)[i] = zv;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0)
    z[n - 1] = fg_z<SHIFT>(v[n - 1], dinv, shift);
}

__global__ __launch_bounds__(256) void fg_shift_kernel(double* __restrict__ z,
                                                       const FgState* __restrict__ fs,
                                                       const CgState* __restrict__ st, int64_t n) {
  if (st->done) return;
  const double shift = -(fs->zsum / st->ntot);
  const int64_t n2 = n >> 1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256)
    reinterpret_cast<dv2*>(z)[i] = reinterpret_cast<const dv2*>(z)[i] + shift;
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) z[n - 1] = z[n - 1] + shift;
}

// Jacobi / no PC: the next direction is z = dinv (scale w) + shift, and its mean follows from the
// sum of w the multi-axpy took: shift = -(dinv (scale sum w)) / ntot
__device__ __forceinline__ void fg_next_shift(const CgState& st, FgState* fs) {
  fs->shift = st.nullspace ? -((st.dinv * (fs->scale * fs->wsum)) / st.ntot) : 0.0;
}

__global__ void fg_start_kernel(CgState* st_g, FgState* fs, double* hist, int* h_done, int mode,
                                int ref, int restart, double haptol, int64_t host_iter) {
  if (threadIdx.x != 0) return;
  CgState& st = *st_g;
  if (mode == 1 && st.done) return;
  const double rn = norm_from_sq(fs->nrm2);
  fs->loc = 0;
  fs->g[0] = rn;
  fs->scale = 1.0 / rn;
  fg_next_shift(st, fs);
  st.dp = rn;
  if (mode == 0) {
    fs->restart = restart;
    fs->haptol = haptol;
    double rn0 = rn;
    const double bn = norm_from_sq(fs->bsq);
    if (ref == REF_RHS) rn0 = bn == 0.0 ? rn : bn;
    else if (ref == REF_MIN) rn0 = fmin(bn, rn);
    st.rnorm0 = rn0;
    st.it = 0;
    st.its = 0;
    st.mu = 0.0;
    st.pend_iter = -1;
    st.pend_count = 0;
    st.reason = 0;
    st.done = 0;
    if (st.nhist > 0 && hist) hist[0] = rn;
    st.nlog = st.nhist > 0 ? 1 : 0;
    st.ttol = fmax(st.rtol * rn0, st.atol);
    ksp_default_test(st, rn, ref != REF_ZERO_GUESS);
    // (KSPSolve_FGMRES leaves its loop without a step at max_it = 0)
    if (!st.reason && st.max_it <= 0) st.reason = PB_KSP_DIVERGED_ITS;
    st.done = st.reason != 0;
    if (h_done) h_done[0] = st.done;
  } else {
    // a restart: the recomputed ||b - A x|| at the iteration count the cycle ended with
    ksp_default_test(st, rn, true);
    st.done = st.reason != 0;
    if (h_done) h_done[host_iter + 1] = st.done;
  }
}

// KSPFGMRESCycle's scalar part after the orthogonalisation of step k = fs->loc, then
// KSPFGMRESUpdateHessenberg: the stored rotations on the new column, the new rotation, the
// estimate |g_(k+1)|
__global__ void fg_step_kernel(CgState* st_g, FgState* fs, double* hist, int* h_done, int passes,
                               int64_t host_iter) {
  if (threadIdx.x != 0) return;
  CgState& st = *st_g;
  if (st.done) {
    if (h_done) h_done[host_iter + 1] = 1;
    return;
  }
  const int k = fs->loc;
  double* col = fs->hh + (int64_t)k * kFgLd;
  bool bad = false;  // KSPCheckDot
  for (int j = 0; j <= k; ++j) {
    const double h = passes == 2 ? fs->dots[j] + fs->dots2[j] : fs->dots[j];
    bad = bad || !finite(h);
    col[j] = h;
  }
  const double tt = norm_from_sq(fs->nrm2);
  if (bad || !finite(tt)) {
    st.reason = PB_KSP_DIVERGED_NANORINF;
    st.done = 1;
    if (h_done) h_done[host_iter + 1] = 1;
    return;
  }
  // the happy breakdown: the new direction is (next to) nothing -- the solution lies in the
  // space already built, and 1 / tt would be no scale
  double hapbnd = fabs(tt / fs->g[k]);
  if (hapbnd > fs->haptol) hapbnd = fs->haptol;
  const bool hapend = !(tt > hapbnd);
  if (!hapend) {
    fs->scale = 1.0 / tt;
    fg_next_shift(st, fs);
  }
  col[k + 1] = tt;
  for (int j = 0; j < k; ++j) {
    const double t = col[j], c = fs->cs[j], s = fs->sn[j];
    col[j] = c * t + s * col[j + 1];
    col[j + 1] = c * col[j + 1] - s * t;
  }
  double res = 0.0;
  bool breakdown = false;
  if (!hapend) {
    const double d = sqrt(col[k] * col[k] + col[k + 1] * col[k + 1]);
    if (d == 0.0) {
      breakdown = true;
    } else {
      const double c = col[k] / d, s = col[k + 1] / d;
      fs->cs[k] = c;
      fs->sn[k] = s;
      fs->g[k + 1] = -(s * fs->g[k]);
      fs->g[k] = c * fs->g[k];
      col[k] = c * col[k] + s * col[k + 1];
      res = fabs(fs->g[k + 1]);
    }
  }
  if (breakdown) {
    st.reason = PB_KSP_DIVERGED_BREAKDOWN;
  } else {
    fs->loc = k + 1;
    st.it = st.it + 1;
    st.its = st.it;
    st.dp = res;
    if (st.its < st.nhist) {
      if (hist) hist[st.its] = res;
      st.nlog = st.its + 1;
    }
    ksp_default_test(st, res, true);
    if (!st.reason && hapend)
      st.reason = st.norm == PB_KSP_NORM_NONE ? PB_KSP_CONVERGED_HAPPY_BREAKDOWN
                                              : PB_KSP_DIVERGED_BREAKDOWN;
    if (!st.reason && st.its >= st.max_it) st.reason = PB_KSP_DIVERGED_ITS;
  }
  st.done = st.reason != 0;
  if (h_done) h_done[host_iter + 1] = st.done;
}

// KSPFGMRESBuildSoln's back substitution over the m = fs->loc live columns (a zero pivot -- the
// unrotated column of a happy breakdown can have one -- leaves that direction out)
__global__ void fg_trisolve_kernel(const CgState* st, FgState* fs, int force) {
  if (threadIdx.x != 0) return;
  if (!force && st->done) return;
  const int m = fs->loc;
  for (int k = m - 1; k >= 0; --k) {
    double t = fs->g[k];
    for (int j = k + 1; j < m; ++j) t = t - fs->hh[(int64_t)j * kFgLd + k] * fs->y[j];
    const double piv = fs->hh[(int64_t)k * kFgLd + k];
    fs->y[k] = piv != 0.0 ? t / piv : 0.0;
  }
}

// x = x + (((0 + y_0 z_0) + y_1 z_1) + ...) over j < fs->loc: VecMAXPY into a zeroed work vector,
// then VecAXPY. Directions past the live count are never read: they may hold anything
__global__ __launch_bounds__(256) void fg_build_kernel(double* __restrict__ x, FgTable zt,
                                                       const FgState* __restrict__ fs,
                                                       const CgState* __restrict__ st, int force,
                                                       int64_t n) {
  if (!force && st->done) return;
  const int m = fs->loc;
  if (m <= 0) return;
  const int64_t n2 = n >> 1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2;
       i += (int64_t)gridDim.x * 256) {
    dv2 t = dv2{0.0, 0.0};
    for (int j = 0; j < m; ++j) t = t + fs->y[j] * reinterpret_cast<const dv2*>(zt.p[j])[i];
    reinterpret_cast<dv2*>(x)[i] = reinterpret_cast<const dv2*>(x)[i] + t;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    double t = 0.0;
    for (int j = 0; j < m; ++j) t = t + fs->y[j] * zt.p[j][n - 1];
    x[n - 1] = x[n - 1] + t;
  }
}

int launch_fg_scale(pb_ctx* ctx, const double* w, double* v, const FgState* fs, const CgState* st,
                    int64_t n) {
  ScopedTimer tm(ctx, "fgmres_scale");
  hipLaunchKernelGGL(fg_scale_kernel, dim3(fg_grid(ctx, n >> 1)), dim3(256), 0, ctx->stream, w, v,
                     fs, st, n);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int launch_fg_zsum(pb_ctx* ctx, const double* z, FgState* fs, const CgState* st, int64_t n) {
  const int nb = fg_grid(ctx, n >> 1);
  if (nb > ctx->partials_cap)
    return set_error(PB_ERR_UNSUPPORTED, "fgmres: partial sums do not fit");
  hipLaunchKernelGGL(fg_zsum_kernel, dim3(nb), dim3(256), 0, ctx->stream, z, st, n,
                     ctx->d_partials);
  PB_HIP(hipGetLastError());
  PB_TRY(reduce_partials(ctx, ctx->d_partials, nb, 1, &fs->zsum));
  return allreduce_device(ctx, &fs->zsum, 1);
}

int launch_fg_pcshift(pb_ctx* ctx, const double* v, double* z, const FgState* fs,
                      const CgState* st, int64_t n, bool nullspace) {
  ScopedTimer tm(ctx, "fgmres_pc");
  const int nb = fg_grid(ctx, n >> 1);
  if (nullspace)
    hipLaunchKernelGGL(fg_pcshift_kernel<true>, dim3(nb), dim3(256), 0, ctx->stream, v, z, fs, st,
                       n);
  else
    hipLaunchKernelGGL(fg_pcshift_kernel<false>, dim3(nb), dim3(256), 0, ctx->stream, v, z, fs, st,
                       n);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int launch_fg_shift(pb_ctx* ctx, double* z, const FgState* fs, const CgState* st, int64_t n) {
  hipLaunchKernelGGL(fg_shift_kernel, dim3(fg_grid(ctx, n >> 1)), dim3(256), 0, ctx->stream, z, fs,
                     st, n);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int launch_fg_start(pb_ctx* ctx, const KspLog& lg, FgState* fs, int mode, int ref, int restart,
                    double haptol, int64_t host_iter) {
  hipLaunchKernelGGL(fg_start_kernel, dim3(1), dim3(64), 0, ctx->stream, lg.st, fs, lg.hist,
                     lg.h_done, mode, ref, restart, haptol, host_iter);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int launch_fg_step(pb_ctx* ctx, const KspLog& lg, FgState* fs, int passes, int64_t host_iter) {
  hipLaunchKernelGGL(fg_step_kernel, dim3(1), dim3(64), 0, ctx->stream, lg.st, fs, lg.hist,
                     lg.h_done, passes, host_iter);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int launch_fg_trisolve(pb_ctx* ctx, const CgState* st, FgState* fs, bool force) {
  hipLaunchKernelGGL(fg_trisolve_kernel, dim3(1), dim3(64), 0, ctx->stream, st, fs,
                     force ? 1 : 0);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int launch_fg_build(pb_ctx* ctx, double* x, const FgTable& z, const FgState* fs, const CgState* st,
                    bool force, int64_t n) {
  hipLaunchKernelGGL(fg_build_kernel, dim3(fg_grid(ctx, n >> 1)), dim3(256), 0, ctx->stream, x, z,
                     fs, st, force ? 1 : 0, n);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

// ---------------------------------------------------------------------------------------------
// The step-start pass on the stencil engine (pb_star7.hpp)
// ---------------------------------------------------------------------------------------------
// Flexible GMRES (-ksp_type fgmres) on the 7-point operator with Jacobi / no PC:
// the start of an Arnoldi step in one pass. The field is the preconditioned direction
// z = dinv (s wt) + shift, formed on load from the unnormalised direction wt the orthogonalisation
// left (s = 1 / ||wt|| and the null-space shift are the state's: fg_step_kernel / fg_start_kernel
// set them from the multi-axpy's sums), every product and sum rounded (fg_z in pb_device.hpp is
// the one definition), so fg_scale_kernel + fg_pcshift_kernel (pb_ksp_fgmres.hip) and the
// standalone operator give the same bits. The epilogue stores the basis vector v = s wt (wt read
// again at the point: the z-queue holds z, not wt), the centre value z and w = A z (reference
// summation order). Reads wt, writes v, z, w: 8 + 24 B/DoF against 48 for the three passes
// (scale 16, preconditioner 16, operator 16). w goes to another buffer than wt: neighbouring
// waves and blocks still read wt around this point. RichEpi's launch shape (two and more streams
// written, non-temporal).
template <bool SHIFT>
struct FgLoad {
  static constexpr int NR = 1;
  static constexpr bool GHOST_RAW = false;
  const double* __restrict__ wt;
  const FgState* fs;
  const CgState* st;
  double scale = 0.0, dinv = 1.0, shift = 0.0;
  __device__ __forceinline__ void prepare() {
    scale = fs->scale;
    dinv = st->dinv;
    shift = fs->shift;
  }
  __device__ __forceinline__ const double* src(int) const { return wt; }
  __device__ __forceinline__ double value(const double* raw) const {
    const double v = scale * raw[0];
    return fg_z<SHIFT>(v, dinv, shift);
  }
};
struct FgEpi {
  static constexpr int NS = 0, NE = 1;
  static constexpr bool RAW = false;
  static constexpr int WGCU = 1;
  static constexpr bool CAP = true, WIDE8 = true;
  static constexpr bool PREFETCH = true;
  double* __restrict__ v_out;
  double* __restrict__ z_out;
  double* __restrict__ w_out;
  const double* __restrict__ wt;
  const FgState* fs;
  double scale = 0.0;
  __device__ __forceinline__ void prepare() { scale = fs->scale; }
  __device__ __forceinline__ const double* src(int) const { return wt; }
  template <int V>
  __device__ __forceinline__ void put(RowIx idx, const double (&c)[V], const double (&w)[V],
                                      double (&op)[1][V], double* acc, int nt) const {
    double vv[V];
#pragma unroll
    for (int e = 0; e < V; ++e) vv[e] = scale * op[0][e];
    (void)acc;
    store_row<V>(w_out, idx, w, nt);
    store_row<V>(z_out, idx, c, nt);
    store_row<V>(v_out, idx, vv, nt);
  }
};

// FGMRES's step-start pass (FgLoad / FgEpi), whole grid, wrap planes; always an iteration's launch
// (exits at entry once the state is done)
int launch_fg_fused(pb_grid* g, const Star& s, const double* wt, double* v, double* z,
                    double* w_out, const FgState* fs, const CgState* st, bool nullspace) {
  ScopedTimer tm(g->ctx, "fgmres_fused");
  const StencilPlanes gp = wrap_planes();
  const FgEpi ep{v, z, w_out, wt, fs};
  if (nullspace) return launch_any(g, s, FgLoad<true>{wt, fs, st}, gp, ep, Launch{&st->done});
  return launch_any(g, s, FgLoad<false>{wt, fs, st}, gp, ep, Launch{&st->done});
}

}  // namespace pb
