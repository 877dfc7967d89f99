// pb_mac.hip -- the MAC-grid (staggered) gradient, projection and divergence of the 7-point
// operators PB_OP_VARCOEF and PB_OP_STAR7 ("Projection"): the two thirds of a
// projection step around the solve. A face field is three cell-indexed arrays, u_d(c) on the face
// between cell c and cell c + e_d. With r_d = 1.0 / h_d and every product, sum and quotient
// rounded (-ffp-contract=off):
//   G_d(c) = (r_d face(beta_(c+e_d), beta_c)) (p_(c+e_d) - p_c)     (PB_OP_STAR7: r_d (p_+ - p_c))
//   u_d(c) <- u_d(c) - (s G_d(c))                                   the projection, in place
//   D(c)   = s ((((ux(c) - ux(c-ex)) r_x) + ((uy(c) - uy(c-ey)) r_y)) + ((uz(c) - uz(c-ez)) r_z))
// face() is the operator's own mean (vc_face), beta the operator's own field and ghost planes, so
// D G = A to rounding and the projected field is discretely divergence-free.
//
// Both kernels are z-marches on the engine's tiles and chunks (Geo, make_geo: a wave owns 64 V
// points of TY rows and marches in z over a chunk of planes), with its row loads / stores, DPP lane
// shifts, one-masked-load segment ends and block order (pb_star7.hpp, pb_device.hpp). Neither takes
// a sum: no partials, no device flag.
#include "pb_star7.hpp"

namespace pb {

// BETA: 0 none (PB_OP_STAR7: the face coefficient is r_d), 1 arithmetic, 2 harmonic
template <int BETA>
__device__ __forceinline__ double mac_coef(double r, double bn, double bc) {
  if constexpr (BETA == 0) return r;
  else return r * vc_face<BETA == 2>(bn, bc);
}

// G of p on the plus faces: only plus neighbours, so the march holds planes k and k + 1 of p and
// beta (plane k + 1's values become plane k's: one load of each per point). x+ from the upper lane
// or the right segment end, y+ from the wave's next row or the row above the tile, z+ the plane in
// flight. bt: the operator's beta at local plane 0, plane nzl its own ghost plane (no select);
// p's plane nzl: the wrap plane in place (g.wrap, one rank) or ghost_hi after a halo exchange.
// PROJECT = 0: ux, uy, uz = G (three stores); 1: u_d = u_d - (s G_d), rows loaded non-temporally
// (read once) and stored in place.
template <int V, int TY, int BETA, int PROJECT>
__global__ __launch_bounds__(kThreads) void mac_grad_kernel(Geo g, double rx, double ry, double rz,
                                                            double s, const double* __restrict__ p,
                                                            const double* __restrict__ bt,
                                                            const double* __restrict__ ghost_hi,
                                                            double* __restrict__ ux,
                                                            double* __restrict__ uy,
                                                            double* __restrict__ uz) {
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
  // segment ends (the engine's scheme): one masked load per plane and array, lane 32 + t the right
  // edge of row t (lanes below 32 fetch the left edge, unused here); every lane loads a valid address
  const int seg0 = seg * 64 * V;
  const int seg_end = min(seg0 + 64 * V, nx);
  const bool needR = active && (lane == 63 || i0 + V >= nx);
  const int edge_row = lane < 32 ? lane : lane - 32;
  const bool edge_lane = edge_row < TY;
  const int edge_i = lane < 32 ? (seg0 == 0 ? nx - 1 : seg0 - 1) : (seg_end >= nx ? 0 : seg_end);
  const int64_t edge_off = (int64_t)(j0 + (edge_lane ? edge_row : 0)) * nx + edge_i;
  const unsigned boff = (unsigned)ic * 8u;
  const int64_t row_up = (int64_t)((j0 + TY >= g.ny) ? 0 : j0 + TY) * nx;
  auto rix = [&](int64_t row) { return RowIx{row, boff}; };
  if (!wave_on) return;

  // planes k and k + 1 of p and beta, the prefetch of plane k + 2; plane k's row above the tile and
  // segment ends, and their plane-(k + 1) prefetch
  double p1[TY][V], p2[TY][V], zp[TY][V], b1[TY][V], b2[TY][V], zb[TY][V];
  double pup[V], bup[V], pe = 0.0, be = 0.0;
  double pup_r[V], bup_r[V], pe_r = 0.0, be_r = 0.0;

  // every load is issued unconditionally (p's ghost plane by a uniform pointer select, the chunk's
  // last step re-loading a valid plane): no load under a branch
  auto issue_rows = [&](int kk, double (&dp)[TY][V], double (&db)[TY][V]) {  // kk in [0, nzl]
    int kx = kk;
    if (g.wrap) kx = kk >= g.nzl ? kk - g.nzl : kk;
    const bool ghost = kx >= g.nzl;
    const double* src = ghost ? ghost_hi : p;
    const int64_t pbase = ghost ? 0 : (int64_t)kx * g.plane;
    const int64_t bbase = (int64_t)kk * g.plane;
#pragma unroll
    for (int t = 0; t < TY; ++t) {
      load_row<V>(src, rix(pbase + (int64_t)(j0 + t) * nx), dp[t]);
      if constexpr (BETA != 0) load_row<V>(bt, rix(bbase + (int64_t)(j0 + t) * nx), db[t]);
    }
  };
  auto issue_plane_ops = [&](int kk) {  // the row above the tile and the segment ends, owned plane
    const int64_t base = (int64_t)kk * g.plane;
    load_row<V>(p, rix(base + row_up), pup_r);
    pe_r = p[base + edge_off];
    if constexpr (BETA != 0) {
      load_row<V>(bt, rix(base + row_up), bup_r);
      be_r = bt[base + edge_off];
    }
  };
  auto copy_rows = [](const double (&src)[TY][V], double (&dst)[TY][V]) {
#pragma unroll
    for (int t = 0; t < TY; ++t)
#pragma unroll
      for (int e = 0; e < V; ++e) dst[t][e] = src[t][e];
  };

  const int nk = ke - kb;
  issue_rows(kb, p1, b1);
  issue_plane_ops(kb);
  issue_rows(kb + 1, zp, zb);
  for (int m = 0; m < nk; ++m) {
    const int k = kb + m;
    copy_rows(zp, p2);  // plane k + 1 (in flight since the previous step)
    if constexpr (BETA != 0) copy_rows(zb, b2);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      pup[e] = pup_r[e];
      if constexpr (BETA != 0) bup[e] = bup_r[e];
    }
    pe = pe_r;
    if constexpr (BETA != 0) be = be_r;
    issue_rows(m + 1 < nk ? k + 2 : k + 1, zp, zb);  // (last step: a valid plane, unused)
    issue_plane_ops(m + 1 < nk ? k + 1 : k);
    const int64_t base = (int64_t)k * g.plane;
    double uo[PROJECT ? TY : 1][3][V];
    if constexpr (PROJECT) {
#pragma unroll
      for (int t = 0; t < TY; ++t) {
        const RowIx ix = rix(base + (int64_t)(j0 + t) * nx);
        load_row_nt<V>(ux, ix, uo[t][0]);
        load_row_nt<V>(uy, ix, uo[t][1]);
        load_row_nt<V>(uz, ix, uo[t][2]);
      }
    }
#pragma unroll
    for (int t = 0; t < TY; ++t) {
      const double peR = readlane_d(pe, 32 + t);
      const double pfromR = dpp_from_upper(p1[t][0]);
      const double pr = needR ? peR : pfromR;
      double br = 0.0;
      if constexpr (BETA != 0) {
        const double beR = readlane_d(be, 32 + t);
        const double bfromR = dpp_from_upper(b1[t][0]);
        br = needR ? beR : bfromR;
      }
      double wx[V], wy[V], wz[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const double pc = p1[t][e];
        const double bc = BETA != 0 ? b1[t][e] : 0.0;
        const double pxp = e == V - 1 ? pr : p1[t][e + 1];
        const double pyp = t == TY - 1 ? pup[e] : p1[t + 1][e];
        double bxp = 0.0, byp = 0.0, bzp = 0.0;
        if constexpr (BETA != 0) {
          bxp = e == V - 1 ? br : b1[t][e + 1];
          byp = t == TY - 1 ? bup[e] : b1[t + 1][e];
          bzp = b2[t][e];
        }
        const double gx = mac_coef<BETA>(rx, bxp, bc) * (pxp - pc);
        const double gy = mac_coef<BETA>(ry, byp, bc) * (pyp - pc);
        const double gz = mac_coef<BETA>(rz, bzp, bc) * (p2[t][e] - pc);
        if constexpr (PROJECT) {
          wx[e] = uo[t][0][e] - s * gx;
          wy[e] = uo[t][1][e] - s * gy;
          wz[e] = uo[t][2][e] - s * gz;
        } else {
          wx[e] = gx;
          wy[e] = gy;
          wz[e] = gz;
        }
      }
      if (active) {
        const RowIx ix = rix(base + (int64_t)(j0 + t) * nx);
        store_row<V>(ux, ix, wx, g.nt);
        store_row<V>(uy, ix, wy, g.nt);
        store_row<V>(uz, ix, wz, g.nt);
      }
    }
    copy_rows(p2, p1);
    if constexpr (BETA != 0) copy_rows(b2, b1);
  }
}

// out = s D(u): only minus neighbours. x- from the lower lane or the left segment end, y- from the
// wave's previous row or the row below the tile, z- plane k - 1 of uz carried in registers from
// the previous step. uz's plane -1: the wrap plane in place (g.wrap) or ghost_lo after a halo
// exchange of uz. Plane k + 1's rows are in flight while plane k is computed.
template <int V, int TY>
__global__ __launch_bounds__(kThreads) void mac_div_kernel(Geo g, double rx, double ry, double rz,
                                                           double s, const double* __restrict__ ux,
                                                           const double* __restrict__ uy,
                                                           const double* __restrict__ uz,
                                                           const double* __restrict__ ghost_lo,
                                                           double* __restrict__ out) {
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
  const int ic = active ? i0 : 0;
  // segment ends: lane t the left edge of row t (lanes from 32 on fetch the right edge, unused)
  const int seg0 = seg * 64 * V;
  const int seg_end = min(seg0 + 64 * V, nx);
  const bool needL = lane == 0;
  const int edge_row = lane < 32 ? lane : lane - 32;
  const bool edge_lane = edge_row < TY;
  const int edge_i = lane < 32 ? (seg0 == 0 ? nx - 1 : seg0 - 1) : (seg_end >= nx ? 0 : seg_end);
  const int64_t edge_off = (int64_t)(j0 + (edge_lane ? edge_row : 0)) * nx + edge_i;
  const unsigned boff = (unsigned)ic * 8u;
  const int64_t row_dn = (int64_t)(j0 == 0 ? g.ny - 1 : j0 - 1) * nx;
  auto rix = [&](int64_t row) { return RowIx{row, boff}; };
  if (!wave_on) return;

  // plane k of the three components, plane k - 1 of uz, uy's row below the tile and ux's left
  // segment ends; the plane-(k + 1) prefetch of all but the carried plane
  double x1[TY][V], y1[TY][V], z1[TY][V], z0[TY][V], ydn[V], xe = 0.0;
  double x_r[TY][V], y_r[TY][V], z_r[TY][V], ydn_r[V], xe_r = 0.0;

  auto issue_plane = [&](int kk) {  // owned plane kk
    const int64_t base = (int64_t)kk * g.plane;
#pragma unroll
    for (int t = 0; t < TY; ++t) {
      const RowIx ix = rix(base + (int64_t)(j0 + t) * nx);
      load_row<V>(ux, ix, x_r[t]);
      load_row<V>(uy, ix, y_r[t]);
      load_row<V>(uz, ix, z_r[t]);
    }
    load_row<V>(uy, rix(base + row_dn), ydn_r);
    xe_r = ux[base + edge_off];
  };

  const int nk = ke - kb;
  {  // plane kb - 1 of uz (uniform pointer select, as the engine's ghost planes)
    int kx = kb - 1;
    if (g.wrap) kx = kx < 0 ? kx + g.nzl : kx;
    const bool ghost = kx < 0;
    const double* src = ghost ? ghost_lo : uz;
    const int64_t zbase = ghost ? 0 : (int64_t)kx * g.plane;
#pragma unroll
    for (int t = 0; t < TY; ++t) load_row<V>(src, rix(zbase + (int64_t)(j0 + t) * nx), z0[t]);
  }
  issue_plane(kb);
  for (int m = 0; m < nk; ++m) {
    const int k = kb + m;
#pragma unroll
    for (int t = 0; t < TY; ++t)
#pragma unroll
      for (int e = 0; e < V; ++e) {
        x1[t][e] = x_r[t][e];
        y1[t][e] = y_r[t][e];
        z1[t][e] = z_r[t][e];
      }
#pragma unroll
    for (int e = 0; e < V; ++e) ydn[e] = ydn_r[e];
    xe = xe_r;
    issue_plane(m + 1 < nk ? k + 1 : k);  // (last step: a valid plane, unused)
    const int64_t base = (int64_t)k * g.plane;
#pragma unroll
    for (int t = 0; t < TY; ++t) {
      const double xeL = readlane_d(xe, t);
      const double xfromL = dpp_from_lower(x1[t][V - 1]);
      const double xl = needL ? xeL : xfromL;
      double w[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const double xm = e == 0 ? xl : x1[t][e - 1];
        const double ym = t == 0 ? ydn[e] : y1[t - 1][e];
        double d = (x1[t][e] - xm) * rx;
        d = d + (y1[t][e] - ym) * ry;
        d = d + (z1[t][e] - z0[t][e]) * rz;
        w[e] = s * d;
        z0[t][e] = z1[t][e];  // plane k of uz is plane k + 1's z- neighbour
      }
      if (active) store_row<V>(out, rix(base + (int64_t)(j0 + t) * nx), w, g.nt);
    }
  }
}

// workgroups per CU the z-chunks are sized for (tuning mac_wgcu)
static int mac_wgcu() {
  const int w = tune("mac_wgcu", 0);
  return w > 0 ? w : 2;
}

template <int V, int TY, int BETA>
static int launch_mac_grad_t(pb_grid* g, const MacCoef& c, const double* p, double s,
                             double* const u[3], bool project, const StencilPlanes& gp, int mode) {
  Geo geo = make_geo(g, V, TY, mode, 0, mac_wgcu(), 0);
  geo.wrap = gp.wrap && !g->ctx->split ? 1 : 0;
  const int64_t nb = (int64_t)geo.nsegx * geo.ntile * geo.nchunk;
  if (project)
    hipLaunchKernelGGL((mac_grad_kernel<V, TY, BETA, 1>), dim3((unsigned)nb), dim3(kThreads), 0,
                       g->ctx->stream, geo, c.rx, c.ry, c.rz, s, p, c.beta, gp.ghost_hi, u[0], u[1],
                       u[2]);
  else
    hipLaunchKernelGGL((mac_grad_kernel<V, TY, BETA, 0>), dim3((unsigned)nb), dim3(kThreads), 0,
                       g->ctx->stream, geo, c.rx, c.ry, c.rz, s, p, c.beta, gp.ghost_hi, u[0], u[1],
                       u[2]);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

template <int BETA>
static int launch_mac_grad_k(pb_grid* g, const MacCoef& c, const double* p, double s,
                             double* const u[3], bool project, const StencilPlanes& gp, int mode) {
  const int ty = pick_ty((int)g->n[1]);
#define PB_MAC(V_, TY_) return launch_mac_grad_t<V_, TY_, BETA>(g, c, p, s, u, project, gp, mode)
  if (g->n[0] % 2 == 0) {
    if (ty == 4) PB_MAC(2, 4);
    if (ty == 2) PB_MAC(2, 2);
    PB_MAC(2, 1);
  }
  if (ty == 4) PB_MAC(1, 4);
  if (ty == 2) PB_MAC(1, 2);
  PB_MAC(1, 1);
#undef PB_MAC
}

int launch_mac_grad(pb_grid* g, const MacCoef& c, const double* p, double s, double* const u[3],
                    bool project, const StencilPlanes& gp, int mode) {
  ScopedTimer tm(g->ctx, project ? timer_name(mode, "mac_project", "mac_project_interior",
                                              "mac_project_boundary")
                                 : timer_name(mode, "mac_grad", "mac_grad_interior",
                                              "mac_grad_boundary"));
  if (!c.beta) return launch_mac_grad_k<0>(g, c, p, s, u, project, gp, mode);
  if (c.mean == PB_COEF_HARMONIC) return launch_mac_grad_k<2>(g, c, p, s, u, project, gp, mode);
  return launch_mac_grad_k<1>(g, c, p, s, u, project, gp, mode);
}

template <int V, int TY>
static int launch_mac_div_t(pb_grid* g, const MacCoef& c, double s, const double* const u[3],
                            double* out, const StencilPlanes& gp, int mode) {
  Geo geo = make_geo(g, V, TY, mode, 0, mac_wgcu(), 0);
  geo.wrap = gp.wrap && !g->ctx->split ? 1 : 0;
  const int64_t nb = (int64_t)geo.nsegx * geo.ntile * geo.nchunk;
  hipLaunchKernelGGL((mac_div_kernel<V, TY>), dim3((unsigned)nb), dim3(kThreads), 0, g->ctx->stream,
                     geo, c.rx, c.ry, c.rz, s, u[0], u[1], u[2], gp.ghost_lo, out);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int launch_mac_div(pb_grid* g, const MacCoef& c, double s, const double* const u[3], double* out,
                   const StencilPlanes& gp, int mode) {
  ScopedTimer tm(g->ctx, timer_name(mode, "mac_div", "mac_div_interior", "mac_div_boundary"));
  const int ty = pick_ty((int)g->n[1]);
#define PB_MAC(V_, TY_) return launch_mac_div_t<V_, TY_>(g, c, s, u, out, gp, mode)
  if (g->n[0] % 2 == 0) {
    if (ty == 4) PB_MAC(2, 4);
    if (ty == 2) PB_MAC(2, 2);
    PB_MAC(2, 1);
  }
  if (ty == 4) PB_MAC(1, 4);
  if (ty == 2) PB_MAC(1, 2);
  PB_MAC(1, 1);
#undef PB_MAC
}

}  // namespace pb
