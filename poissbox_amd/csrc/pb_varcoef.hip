// pb_varcoef.hip -- PB_OP_VARCOEF: the variable-coefficient 7-point operator y = div(beta grad x)
// in flux form, its diagonal, the check of a coefficient field and the Jacobi PC
// of a variable P (z = dinv o r from the stored reciprocal diagonal).
//
// The apply is a register-queue z-march of its own: the engine (pb_star7.hpp) carries ONE combined
// value per point through its queue, this pass carries two, x and beta, and forms the six face
// coefficients of a point from beta on the fly -- 8 B (x) + 8 B (beta) read and 8 B (y) written per
// DoF, no face value ever stored. It shares the engine's tiles and chunks (Geo, make_geo: a wave
// owns 64 V points of TY rows and marches in z over a chunk of planes), its row loads / stores,
// DPP lane shifts, block reduction and block order (pb_device.hpp).
//
// Per point, with c_d = 1 / h_d^2 and every product, sum and quotient rounded (-ffp-contract=off):
//   face(a, b) = 0.5 (a + b)  |  (2 (a b)) / (a + b)          arithmetic | harmonic
//   g_n = c_d face(beta_n, beta_c),  t_n = g_n (x_n - x_c)
//   y_c = ((((t_z- + t_y-) + t_x-) + t_x+) + t_y+) + t_z+
// Both means are commutative in IEEE arithmetic, so a face has the same bits seen from either
// side: the kernel forms each face once per wave where both sides are in its registers (the z face
// above a plane is carried to the next plane, the y faces between a wave's rows and the x faces
// between a lane's points are shared) -- 3.75 instead of 6 faces per point on 4-row, 2-point tiles,
// which matters for the harmonic mean's fp64 division.
#include "pb_star7.hpp"

namespace pb {

// The rows j0 .. j0 + TY - 1 of plane kk in [-1, nzl] of x and beta. The pointers come by value: a
// select between references to the kernel's arguments would keep the arguments in scratch
template <int V, int TY>
__device__ __forceinline__ void vc_issue_rows(int kk, int nzl, int wrap, int64_t plane, int nx,
                                              int j0, unsigned boff, const double* x,
                                              const double* bt, const double* ghost_lo,
                                              const double* ghost_hi, double (&dx)[TY][V],
                                              double (&db)[TY][V]) {
  const int64_t bbase = (int64_t)kk * plane;  // the operator's own ghost planes: no select
  int kx = kk;
  if (wrap) kx = kk < 0 ? kk + nzl : (kk >= nzl ? kk - nzl : kk);
  const bool ghost = kx < 0 || kx >= nzl;
  const double* gp = kx < 0 ? ghost_lo : ghost_hi;
  const double* src = ghost ? gp : x;
  const int64_t xbase = ghost ? 0 : (int64_t)kx * plane;
#pragma unroll
  for (int t = 0; t < TY; ++t) {
    load_row<V>(src, RowIx{xbase + (int64_t)(j0 + t) * nx, boff}, dx[t]);
    load_row<V>(bt, RowIx{bbase + (int64_t)(j0 + t) * nx, boff}, db[t]);
  }
}

// bt: the operator's beta at local plane 0; planes -1 and nzl are its own ghost planes (filled by
// pb_op_set_coefficient: the neighbouring ranks' planes, on one rank the periodic wrap), so beta
// needs no plane select. x's planes -1 / nzl: the wrap planes of x in place (g.wrap, one rank) or
// the grid's ghost planes. parts != nullptr: the per-block partial sum of x . y (CG's p . Ap).
// RES (the variable multigrid's residual pass, pb_mg_varcoef.hip): y = rb - A x instead of A x.
// MASS (pb_op_set_mass): A x = S6 - q x with q = ms (1: the bytes of MASS = 0) or ms * mf at the
// point (2: one more non-temporal row load, as rb's -- q is point-local, it does not go through
// the z-queue and nothing of it is shared between points); 0: no term, the code without it.
template <int V, int TY, int HARM, int RES, int MASS>
__global__ __launch_bounds__(kThreads) void varcoef_kernel(Geo g, double cx, double cy, double cz,
                                                           const double* __restrict__ x,
                                                           const double* __restrict__ bt,
                                                           const double* __restrict__ ghost_lo,
                                                           const double* __restrict__ ghost_hi,
                                                           const double* __restrict__ rb,
                                                           const double* __restrict__ mf, double ms,
                                                           double* __restrict__ y, double* parts,
                                                           const int* __restrict__ skip) {
  if (skip && *skip) return;  // device-side convergence flag (uniform)
  double acc[1] = {0.0};
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int b = xcd_block(g.remap);
  const int seg = b % g.nsegx;
  b /= g.nsegx;
  const int tile = b % g.ntile;
  const int chunk = b / g.ntile;
  const int j0 = (tile * kWaves + wid) * TY;
  const int kb = g.k_lo + chunk * g.kstride;
  const int ke = min(kb + g.kc, g.k_hi);
  const int nx = g.nx;
  const int i0 = seg * 64 * V + lane * V;
  const bool active = i0 < nx;
  const bool wave_on = j0 < g.ny && kb < g.k_hi;
  const int ic = active ? i0 : 0;  // idle lanes load (and never store) point 0 of their rows
  // segment ends (the engine's scheme): one masked load per plane and array fetches the left edge
  // of row t in lane t and the right edge in lane 32 + t; every lane loads a valid address
  const int seg0 = seg * 64 * V;
  const int seg_end = min(seg0 + 64 * V, nx);
  const bool needL = lane == 0;
  const bool needR = active && (lane == 63 || i0 + V >= nx);
  const int edge_row = lane < 32 ? lane : lane - 32;
  const bool edge_lane = edge_row < TY;
  const int edge_i = lane < 32 ? (seg0 == 0 ? nx - 1 : seg0 - 1) : (seg_end >= nx ? 0 : seg_end);
  const int64_t edge_off = (int64_t)(j0 + (edge_lane ? edge_row : 0)) * nx + edge_i;
  const unsigned boff = (unsigned)ic * 8u;
  const int64_t row_dn = (int64_t)(j0 == 0 ? g.ny - 1 : j0 - 1) * nx;
  const int64_t row_up = (int64_t)((j0 + TY >= g.ny) ? 0 : j0 + TY) * nx;
  auto rix = [&](int64_t row) { return RowIx{row, boff}; };

  if (wave_on) {
    // planes k-1, k, k+1 of x and beta, the prefetch of plane k+2, the z faces below plane k
    double x0[TY][V], x1[TY][V], x2[TY][V], b0[TY][V], b1[TY][V], b2[TY][V];
    double zx[TY][V], zb[TY][V], fzm[TY][V];
    // plane k's halo rows and segment ends, and their plane-(k+1) prefetch
    double xdn[V], xup[V], bdn[V], bup[V], xe = 0.0, be = 0.0;
    double xdn_r[V], xup_r[V], bdn_r[V], bup_r[V], xe_r = 0.0, be_r = 0.0;

    // every load is issued unconditionally (x's ghost planes by a uniform pointer select, the
    // chunk's last step re-loading valid planes): no load under a branch
    auto issue_rows = [&](int kk, double (&dx)[TY][V], double (&db)[TY][V]) {
      vc_issue_rows<V, TY>(kk, g.nzl, g.wrap, g.plane, nx, j0, boff, x, bt, ghost_lo, ghost_hi, dx,
                           db);
    };
    auto issue_plane_ops = [&](int kk) {  // halo rows and segment ends of the owned plane kk
      const int64_t base = (int64_t)kk * g.plane;
      load_row<V>(x, rix(base + row_dn), xdn_r);
      load_row<V>(x, rix(base + row_up), xup_r);
      load_row<V>(bt, rix(base + row_dn), bdn_r);
      load_row<V>(bt, rix(base + row_up), bup_r);
      xe_r = x[base + edge_off];
      be_r = bt[base + edge_off];
    };
    auto copy_rows = [](const double (&s)[TY][V], double (&d)[TY][V]) {
#pragma unroll
      for (int t = 0; t < TY; ++t)
#pragma unroll
        for (int e = 0; e < V; ++e) d[t][e] = s[t][e];
    };

    const int nk = ke - kb;
    issue_rows(kb - 1, x0, b0);
    issue_rows(kb, x1, b1);
    issue_plane_ops(kb);
    issue_rows(kb + 1, zx, zb);
#pragma unroll
    for (int t = 0; t < TY; ++t)
#pragma unroll
      for (int e = 0; e < V; ++e) fzm[t][e] = cz * vc_face<HARM>(b0[t][e], b1[t][e]);

    for (int m = 0; m < nk; ++m) {
      const int k = kb + m;
      copy_rows(zx, x2);  // plane k+1 (in flight since the previous step)
      copy_rows(zb, b2);
#pragma unroll
      for (int e = 0; e < V; ++e) {
        xdn[e] = xdn_r[e];
        xup[e] = xup_r[e];
        bdn[e] = bdn_r[e];
        bup[e] = bup_r[e];
      }
      xe = xe_r;
      be = be_r;
      issue_rows(m + 2 <= nk ? k + 2 : k + 1, zx, zb);  // (last step: a valid plane, unused)
      issue_plane_ops(m + 1 < nk ? k + 1 : k);
      const int64_t base = (int64_t)k * g.plane;
      // the y faces of the wave's TY rows: TY + 1 per column
      double fy[TY + 1][V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        fy[0][e] = cy * vc_face<HARM>(bdn[e], b1[0][e]);
#pragma unroll
        for (int t = 1; t < TY; ++t) fy[t][e] = cy * vc_face<HARM>(b1[t - 1][e], b1[t][e]);
        fy[TY][e] = cy * vc_face<HARM>(bup[e], b1[TY - 1][e]);
      }
#pragma unroll
      for (int t = 0; t < TY; ++t) {
        const double xeL = readlane_d(xe, t), xeR = readlane_d(xe, 32 + t);
        const double beL = readlane_d(be, t), beR = readlane_d(be, 32 + t);
        const double xfromL = dpp_from_lower(x1[t][V - 1]), xfromR = dpp_from_upper(x1[t][0]);
        const double bfromL = dpp_from_lower(b1[t][V - 1]), bfromR = dpp_from_upper(b1[t][0]);
        const double xl = needL ? xeL : xfromL, xr = needR ? xeR : xfromR;
        const double bl = needL ? beL : bfromL, br = needR ? beR : bfromR;
        // the x faces of the lane's V points: V + 1
        double fx[V + 1];
        fx[0] = cx * vc_face<HARM>(bl, b1[t][0]);
#pragma unroll
        for (int e = 1; e < V; ++e) fx[e] = cx * vc_face<HARM>(b1[t][e - 1], b1[t][e]);
        fx[V] = cx * vc_face<HARM>(br, b1[t][V - 1]);
        double w[V], rbv[V], mv[V];
        if constexpr (RES) load_row_nt<V>(rb, rix(base + (int64_t)(j0 + t) * nx), rbv);
        if constexpr (MASS == 2) load_row_nt<V>(mf, rix(base + (int64_t)(j0 + t) * nx), mv);
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const double xc = x1[t][e];
          const double xm = e == 0 ? xl : x1[t][e - 1];
          const double xp = e == V - 1 ? xr : x1[t][e + 1];
          const double ym = t == 0 ? xdn[e] : x1[t - 1][e];
          const double yp = t == TY - 1 ? xup[e] : x1[t + 1][e];
          const double fzp = cz * vc_face<HARM>(b2[t][e], b1[t][e]);
          double s = fzm[t][e] * (x0[t][e] - xc);
          s = s + fy[t][e] * (ym - xc);
          s = s + fx[e] * (xm - xc);
          s = s + fx[e + 1] * (xp - xc);
          s = s + fy[t + 1][e] * (yp - xc);
          s = s + fzp * (x2[t][e] - xc);
          if constexpr (MASS == 2) s = s - (ms * mv[e]) * xc;
          else if constexpr (MASS == 1) s = s - ms * xc;
          if constexpr (RES) w[e] = rbv[e] - s;
          else w[e] = s;
          fzm[t][e] = fzp;  // the face above plane k is the face below plane k + 1
          if (active) acc[0] += s * xc;
        }
        if (active) store_row<V>(y, rix(base + (int64_t)(j0 + t) * nx), w, g.nt);
      }
      copy_rows(x1, x0);
      copy_rows(x2, x1);
      copy_rows(b2, b1);
    }
  }
  if (parts) block_partials<1>(acc, parts);
}

// rb != nullptr: y = rb - A x (no sums), exiting at entry on `skip` instead of ctx->op_skip
template <int V, int TY, int HARM, int MASS>
static int launch_varcoef_t(pb_grid* g, const VarCoef& c, const double* x, double* y,
                            const StencilPlanes& gp, int mode, bool dot, int part_off,
                            int* nblocks, const double* rb, const int* skip) {
  // workgroups per CU the z-chunks are sized for (two are resident at most: the registers).
  // Measured at 512^3 over 1, 2, 3, 4, 6: the arithmetic mean is fastest with 1 (four 128-plane
  // chunks), the harmonic mean, with its divisions to hide, with 3; 256^3 does not tell them apart
  // 
  int wgcu = tune("varcoef_wgcu", 0);
  if (wgcu <= 0) wgcu = HARM ? 3 : 1;
  Geo geo = make_geo(g, V, TY, mode, 0, wgcu, 0);
  geo.wrap = gp.wrap && !g->ctx->split ? 1 : 0;
  const int64_t nb = (int64_t)geo.nsegx * geo.ntile * geo.nchunk;
  if (dot && part_off + nb > g->ctx->partials_cap)
    return set_error(PB_ERR_UNSUPPORTED, "varcoef grid of %lld blocks exceeds partials capacity",
                     (long long)nb);
  if (rb)
    hipLaunchKernelGGL((varcoef_kernel<V, TY, HARM, 1, MASS>), dim3((unsigned)nb), dim3(kThreads),
                       0, g->ctx->stream, geo, c.cx, c.cy, c.cz, x, c.beta, gp.ghost_lo,
                       gp.ghost_hi, rb, c.mass, c.ms, y, nullptr, skip);
  else
    hipLaunchKernelGGL((varcoef_kernel<V, TY, HARM, 0, MASS>), dim3((unsigned)nb), dim3(kThreads),
                       0, g->ctx->stream, geo, c.cx, c.cy, c.cz, x, c.beta, gp.ghost_lo,
                       gp.ghost_hi, rb, c.mass, c.ms, y,
                       dot ? g->ctx->d_partials + part_off : nullptr, g->ctx->op_skip);
  PB_HIP(hipGetLastError());
  if (nblocks) *nblocks = dot ? (int)nb : 0;
  return PB_OK;
}

template <int HARM, int MASS>
static int launch_varcoef_k(pb_grid* g, const VarCoef& c, const double* x, double* y,
                            const StencilPlanes& gp, int mode, bool dot, int part_off,
                            int* nblocks, const double* rb, const int* skip) {
  const int ty = pick_ty((int)g->n[1]);
#define PB_VC(V_, TY_)                                                                         \
  return launch_varcoef_t<V_, TY_, HARM, MASS>(g, c, x, y, gp, mode, dot, part_off, nblocks, rb, \
                                               skip)
  if (g->n[0] % 2 == 0) {
    if (ty == 4) PB_VC(2, 4);
    if (ty == 2) PB_VC(2, 2);
    PB_VC(2, 1);
  }
  if (ty == 4) PB_VC(1, 4);
  if (ty == 2) PB_VC(1, 2);
  PB_VC(1, 1);
#undef PB_VC
}

// the mass off: MASS = 0, the instantiations without the term
template <int HARM>
static int launch_varcoef_m(pb_grid* g, const VarCoef& c, const double* x, double* y,
                            const StencilPlanes& gp, int mode, bool dot, int part_off,
                            int* nblocks, const double* rb = nullptr, const int* skip = nullptr) {
  switch (c.mass_kind()) {
    case 0: return launch_varcoef_k<HARM, 0>(g, c, x, y, gp, mode, dot, part_off, nblocks, rb, skip);
    case 1: return launch_varcoef_k<HARM, 1>(g, c, x, y, gp, mode, dot, part_off, nblocks, rb, skip);
    default: return launch_varcoef_k<HARM, 2>(g, c, x, y, gp, mode, dot, part_off, nblocks, rb, skip);
  }
}

int launch_varcoef_apply(pb_grid* g, const VarCoef& c, const double* x, double* y,
                         const StencilPlanes& gp, int mode, bool dot, int part_off, int* nblocks) {
  ScopedTimer tm(g->ctx, timer_name(mode, "varcoef", "varcoef_interior", "varcoef_boundary"));
  if (c.mean == PB_COEF_HARMONIC)
    return launch_varcoef_m<1>(g, c, x, y, gp, mode, dot, part_off, nblocks);
  return launch_varcoef_m<0>(g, c, x, y, gp, mode, dot, part_off, nblocks);
}

int launch_varcoef_residual(pb_grid* g, const VarCoef& c, const double* x, const double* b,
                            double* res, const StencilPlanes& gp, const int* skip) {
  if (c.mean == PB_COEF_HARMONIC)
    return launch_varcoef_m<1>(g, c, x, res, gp, PLANES_ALL, false, 0, nullptr, b, skip);
  return launch_varcoef_m<0>(g, c, x, res, gp, PLANES_ALL, false, 0, nullptr, b, skip);
}

// ---------------------------------------------------------------------------------------------
// The diagonal -(((((g_z- + g_y-) + g_x-) + g_x+) + g_y+) + g_z+) - q, q the mass term by MASS
// (recip: 1.0 / it, PCJacobi's), the check of a field and z = dinv o r. Grid-stride passes.
// ---------------------------------------------------------------------------------------------
static int vc_blocks(const pb_ctx* ctx, int64_t n) {
  const int64_t want = (n + 255) / 256, cap = (int64_t)ctx->num_cus * 8;
  return (int)std::max<int64_t>(1, std::min(want, cap));
}

template <int HARM, int MASS>
__global__ __launch_bounds__(256) void varcoef_diag_kernel(int nx, int ny, int64_t plane,
                                                           int64_t n, double cx, double cy,
                                                           double cz, const double* __restrict__ bt,
                                                           const double* __restrict__ mf, double ms,
                                                           double* out, int recip) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < n;
       idx += (int64_t)gridDim.x * 256) {
    const int64_t in = idx % plane;
    const int i = (int)(in % nx), j = (int)(in / nx);
    const double bc = bt[idx];
    const double gzm = cz * vc_face<HARM>(bt[idx - plane], bc);
    const double gym =
        cy * vc_face<HARM>(bt[idx + (j == 0 ? (int64_t)(ny - 1) * nx : -(int64_t)nx)], bc);
    const double gxm = cx * vc_face<HARM>(bt[idx + (i == 0 ? nx - 1 : -1)], bc);
    const double gxp = cx * vc_face<HARM>(bt[idx + (i == nx - 1 ? -(nx - 1) : 1)], bc);
    const double gyp =
        cy * vc_face<HARM>(bt[idx + (j == ny - 1 ? -(int64_t)(ny - 1) * nx : (int64_t)nx)], bc);
    const double gzp = cz * vc_face<HARM>(bt[idx + plane], bc);
    double s = gzm + gym;
    s = s + gxm;
    s = s + gxp;
    s = s + gyp;
    s = s + gzp;
    double d = -s;
    if constexpr (MASS == 2) d = d - ms * mf[idx];
    else if constexpr (MASS == 1) d = d - ms;
    out[idx] = recip ? 1.0 / d : d;
  }
}

template <int HARM, int MASS>
static void launch_varcoef_diag_t(pb_grid* g, const VarCoef& c, double* out, bool recip) {
  pb_ctx* ctx = g->ctx;
  hipLaunchKernelGGL((varcoef_diag_kernel<HARM, MASS>), dim3(vc_blocks(ctx, g->nlocal)), dim3(256),
                     0, ctx->stream, (int)g->n[0], (int)g->n[1], g->plane, g->nlocal, c.cx, c.cy,
                     c.cz, c.beta, c.mass, c.ms, out, recip ? 1 : 0);
}

int launch_varcoef_diag(pb_grid* g, const VarCoef& c, double* out, bool recip) {
  const int mk = c.mass_kind();
  if (c.mean == PB_COEF_HARMONIC) {
    if (mk == 0) launch_varcoef_diag_t<1, 0>(g, c, out, recip);
    else if (mk == 1) launch_varcoef_diag_t<1, 1>(g, c, out, recip);
    else launch_varcoef_diag_t<1, 2>(g, c, out, recip);
  } else {
    if (mk == 0) launch_varcoef_diag_t<0, 0>(g, c, out, recip);
    else if (mk == 1) launch_varcoef_diag_t<0, 1>(g, c, out, recip);
    else launch_varcoef_diag_t<0, 2>(g, c, out, recip);
  }
  PB_HIP(hipGetLastError());
  return PB_OK;
}

// the number of values that are not finite and > 0 (zero_ok: >= 0, a mass field), per block
__global__ __launch_bounds__(256) void varcoef_check_kernel(const double* __restrict__ v, int64_t n,
                                                            int zero_ok, double* parts) {
  double acc[1] = {0.0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const double a = v[i];
    if (!((zero_ok ? a >= 0.0 : a > 0.0) && a < INFINITY)) acc[0] += 1.0;
  }
  block_partials<1>(acc, parts);
}

int varcoef_count_bad(pb_grid* g, const double* v, bool zero_ok, double* count) {
  pb_ctx* ctx = g->ctx;
  const int nb = vc_blocks(ctx, g->nlocal);
  hipLaunchKernelGGL(varcoef_check_kernel, dim3(nb), dim3(256), 0, ctx->stream, v, g->nlocal,
                     zero_ok ? 1 : 0, ctx->d_partials);
  PB_HIP(hipGetLastError());
  double* dsum = ctx->d_scalars + 8;
  PB_TRY(reduce_partials(ctx, ctx->d_partials, nb, 1, dsum));
  PB_TRY(allreduce_device(ctx, dsum, 1));
  PB_HIP(hipMemcpyAsync(ctx->h_scalars, dsum, sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  PB_SYNC(ctx, "coefficient check");
  *count = ctx->h_scalars[0];
  return PB_OK;
}

__global__ __launch_bounds__(256) void varcoef_jacobi_kernel(const double* __restrict__ dinv,
                                                             const double* __restrict__ r,
                                                             double* __restrict__ z, int64_t n,
                                                             const int* __restrict__ skip) {
  if (skip && *skip) return;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    z[i] = dinv[i] * r[i];
}

int launch_varcoef_jacobi(pb_grid* g, const double* dinv, const double* r, double* z,
                          const int* skip) {
  pb_ctx* ctx = g->ctx;
  ScopedTimer tm(ctx, "varcoef_jacobi");
  hipLaunchKernelGGL(varcoef_jacobi_kernel, dim3(vc_blocks(ctx, g->nlocal)), dim3(256), 0,
                     ctx->stream, dinv, r, z, g->nlocal, skip);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

}  // namespace pb
