// pb_mg.hip -- geometric multigrid V-cycle with red-black SOR smoothing, and symmetric red-black
// SOR alone, as CG preconditioners (the reference README.md:40-45 recommends
// GAMG + SOR through PETSc, which is absent here: this is the geometric, GPU-native analogue).
//
// Levels: the periodic 7-point operator rediscretised with h_l = 2^l h (star_coeffs, the
// reference's coefficients, src/coefficients.f90:22-48), cell-centred coarsening by 2 in every
// direction, trilinear prolongation P (weights 3/4, 1/4 per direction) and restriction
// R = P^T / 8 (weights 1/8, 3/8, 3/8, 1/8 per direction). V(1,1): pre-smoothing red then black,
// post-smoothing black then red, coarsest level `coarse_its` symmetric sweeps (red, black, red,
// [black, red]...), all from a zero initial guess -- the V-cycle is a symmetric operator, as CG
// needs. SOR update (PETSc PCSOR form): x = (1 - w) x + w (b - sum_nb c x_nb) / c_centre.
// Red = (i + j + k_global) even; every smoothed level has even extents, so a colour's
// neighbours all carry the other colour across the periodic wrap too.
//
// Slab decomposition: level l owns planes [k0 / 2^l, (k0 + nzl) / 2^l); coarsening stops before
// any rank's slab would become odd (mg_plan_levels is a function of the global grid and the rank
// count only, so every rank builds the same hierarchy). Halo planes are exchanged before every
// half-sweep, residual, restriction and prolongation on N > 1 ranks; one rank reads the periodic
// wrap planes in place.
//
// The arithmetic order of every kernel is restated in oracle/pb_oracle.c (pbo_mg_apply), which
// the tests compare bit for bit.
//
// Selectable level smoothers (pb_pc_mg_opts, -mg_levels_*): nu sweeps per leg, and damped Jacobi or
// Chebyshev over Jacobi instead of SOR (mg_poly_kernel, mg_poly_x_kernel; restated in
// tests/mg_smoothers_restatement.py).
//
// This file: the per-pair, per-cell, polynomial and tail kernels and, at its end, the launchers
// that name them, one per pass (pb_mg.hpp). The host path -- hierarchy, level plan, driver and
// legs -- is pb_mg.cpp; the fused sweeps are pb_mg_sweep.hip, the engine passes pb_mg_engine.hip,
// the variable-coefficient levels' half-sweeps and residual (level_smooth's and level_residual's
// branch under Mg::coef) pb_mg_varcoef.hip.
#include <algorithm>
#include <type_traits>

#include "pb_device.hpp"
#include "pb_mg.hpp"

namespace pb {

// ---------------------------------------------------------------------------------------------
// kernels. Every level has an even x extent, so one thread owns an (i even, i + 1) pair: 16-byte
// loads and full-line 16-byte stores; the pair holds one red and one black point.
// ---------------------------------------------------------------------------------------------
typedef double dv2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int wrapm(int v, int n) { return v < 0 ? v + n : (v >= n ? v - n : v); }

struct PairPos {
  int i0, j, k;       // pair origin (i0 even), row j, local plane k
  int64_t idx;        // linear index of (i0, j, k)
};

// 32-bit index arithmetic (a level never holds 2^32 pairs on one GPU)
__device__ __forceinline__ PairPos pair_pos(const MgGeo& G, int64_t q64) {
  const uint32_t q = (uint32_t)q64, hx = (uint32_t)G.nx >> 1;
  const uint32_t row = q / hx;
  PairPos p;
  p.i0 = (int)(q - row * hx) * 2;
  p.k = (int)(row / (uint32_t)G.ny);
  p.j = (int)(row - (uint32_t)p.k * (uint32_t)G.ny);
  p.idx = (int64_t)row * G.nx + p.i0;
  return p;
}

// value of v at (i, j +- 1) and (i, j, k +- 1) for the point at linear index id (plane offset
// pid = id - k*plane); lo / hi are the planes below / above the slab
struct Nb4 {
  double zm, ym, yp, zp;
};
__device__ __forceinline__ Nb4 nb4(const MgGeo& G, const double* v, const double* lo,
                                   const double* hi, int64_t id, int j, int k) {
  const int64_t pid = id - (int64_t)k * G.plane;
  Nb4 r;
  r.zm = k > 0 ? v[id - G.plane] : lo[pid];
  r.zp = k < G.nzl - 1 ? v[id + G.plane] : hi[pid];
  r.ym = v[id + (int64_t)(wrapm(j - 1, G.ny) - j) * G.nx];
  r.yp = v[id + (int64_t)(wrapm(j + 1, G.ny) - j) * G.nx];
  return r;
}

// red value after the zero-initialised first half-sweep: (1 - w) * 0 + w * ((b - 0) * (1 / c))
__device__ __forceinline__ double red0(double b, const Star& s, double omega) {
  const double t = (b - 0.0) * (1.0 / s.cc);
  return (1.0 - omega) * 0.0 + omega * t;
}

// mode 0: one red-black SOR half-sweep over `color` (x holds the current iterate).
// mode 1: the first two half-sweeps from x = 0 fused: red = w D^-1 b, then black from those red
//         values, computed from b directly (lo / hi are then b's ghost planes).
__device__ __forceinline__ void mg_smooth_body(MgGeo G, double* x, const double* __restrict__ b,
                                               const double* lo, const double* hi, Star s,
                                               double omega, int color, int mode, int64_t t0,
                                               int64_t ts) {
  const int64_t npairs = G.nlocal >> 1;
  for (int64_t q = t0; q < npairs; q += ts) {
    const PairPos P = pair_pos(G, q);
    const int64_t row = P.idx - P.i0;
    if (mode == 1) {
      const dv2 bp = *(const dv2*)(b + P.idx);
      const int dr = (int)((P.j + G.k0 + P.k) & 1);  // red offset in the pair
      const int ib = P.i0 + (dr ^ 1);
      const int64_t idb = row + ib;
      const double bb = dr ? bp.x : bp.y;               // black point's b
      const double br = dr ? bp.y : bp.x;
      const Nb4 n4 = nb4(G, b, lo, hi, idb, P.j, P.k);
      const double bxm = ib == P.i0 + 1 ? bp.x : b[row + wrapm(ib - 1, G.nx)];
      const double bxp = ib == P.i0 ? bp.y : b[row + wrapm(ib + 1, G.nx)];
      double nb = s.cz * red0(n4.zm, s, omega);
      nb = nb + s.cy * red0(n4.ym, s, omega);
      nb = nb + s.cx * red0(bxm, s, omega);
      nb = nb + s.cx * red0(bxp, s, omega);
      nb = nb + s.cy * red0(n4.yp, s, omega);
      nb = nb + s.cz * red0(n4.zp, s, omega);
      const double t = (bb - nb) * (1.0 / s.cc);
      const double xb = (1.0 - omega) * 0.0 + omega * t;
      const double xr = red0(br, s, omega);
      dv2 o;
      o.x = dr ? xb : xr;
      o.y = dr ? xr : xb;
      *(dv2*)(x + P.idx) = o;
      continue;
    }
    const dv2 xp = *(const dv2*)(x + P.idx);
    const int d = (int)((color + P.j + G.k0 + P.k) & 1);  // offset of the updated point
    const int ic = P.i0 + d;
    const int64_t id = row + ic;
    const Nb4 n4 = nb4(G, x, lo, hi, id, P.j, P.k);
    const double xm = d ? xp.x : x[row + wrapm(P.i0 - 1, G.nx)];
    const double xq = d ? x[row + wrapm(P.i0 + 2, G.nx)] : xp.y;
    double nb = s.cz * n4.zm;
    nb = nb + s.cy * n4.ym;
    nb = nb + s.cx * xm;
    nb = nb + s.cx * xq;
    nb = nb + s.cy * n4.yp;
    nb = nb + s.cz * n4.zp;
    const double xo = d ? xp.y : xp.x;
    const double t = (b[id] - nb) * (1.0 / s.cc);
    const double xn = (1.0 - omega) * xo + omega * t;
    dv2 o = xp;
    if (d) o.y = xn;
    else o.x = xn;
    *(dv2*)(x + P.idx) = o;
  }
}
__global__ __launch_bounds__(256) void mg_smooth_kernel(MgGeo G, double* x,
                                                        const double* __restrict__ b,
                                                        const double* lo, const double* hi, Star s,
                                                        double omega, int color, int mode,
                                                        const int* skip) {
  if (skip && *skip) return;
  mg_smooth_body(G, x, b, lo, hi, s, omega, color, mode,
                 (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
}

// b - A x at both points of a pair (the reference operator's summation order): xc the pair, zm,
// zp, ym, yp its neighbour pairs, xl / xr the points left and right of it
__device__ __forceinline__ dv2 residual_pair(const Star& s, dv2 bc, dv2 xc, dv2 zm, dv2 zp, dv2 ym,
                                             dv2 yp, double xl, double xr) {
  double a0 = s.cz * zm.x;
  a0 = a0 + s.cy * ym.x;
  a0 = a0 + s.cx * xl;
  a0 = a0 + s.cc * xc.x;
  a0 = a0 + s.cx * xc.y;
  a0 = a0 + s.cy * yp.x;
  a0 = a0 + s.cz * zp.x;
  double a1 = s.cz * zm.y;
  a1 = a1 + s.cy * ym.y;
  a1 = a1 + s.cx * xc.x;
  a1 = a1 + s.cc * xc.y;
  a1 = a1 + s.cx * xr;
  a1 = a1 + s.cy * yp.y;
  a1 = a1 + s.cz * zp.y;
  dv2 o;
  o.x = bc.x - a0;
  o.y = bc.y - a1;
  return o;
}

// res = b - A x for both points of the pair
__device__ __forceinline__ void mg_residual_body(MgGeo G, const double* __restrict__ x,
                                                 const double* __restrict__ b,
                                                 const double* __restrict__ lo,
                                                 const double* __restrict__ hi, Star s,
                                                 double* __restrict__ res, int64_t t0,
                                                 int64_t ts) {
  const int64_t npairs = G.nlocal >> 1;
  for (int64_t q = t0; q < npairs; q += ts) {
    const PairPos P = pair_pos(G, q);
    const int64_t row = P.idx - P.i0;
    const dv2 xc = *(const dv2*)(x + P.idx);
    const dv2 bc = *(const dv2*)(b + P.idx);
    const int64_t pid = P.idx - (int64_t)P.k * G.plane;
    const dv2 zm = P.k > 0 ? *(const dv2*)(x + P.idx - G.plane) : *(const dv2*)(lo + pid);
    const dv2 zp = P.k < G.nzl - 1 ? *(const dv2*)(x + P.idx + G.plane) : *(const dv2*)(hi + pid);
    const dv2 ym = *(const dv2*)(x + P.idx + (int64_t)(wrapm(P.j - 1, G.ny) - P.j) * G.nx);
    const dv2 yp = *(const dv2*)(x + P.idx + (int64_t)(wrapm(P.j + 1, G.ny) - P.j) * G.nx);
    const double xl = x[row + wrapm(P.i0 - 1, G.nx)];
    const double xr = x[row + wrapm(P.i0 + 2, G.nx)];
    *(dv2*)(res + P.idx) = residual_pair(s, bc, xc, zm, zp, ym, yp, xl, xr);
  }
}
__global__ __launch_bounds__(256) void mg_residual_kernel(MgGeo G, const double* __restrict__ x,
                                                          const double* __restrict__ b,
                                                          const double* __restrict__ lo,
                                                          const double* __restrict__ hi, Star s,
                                                          double* __restrict__ res, const int* skip) {
  if (skip && *skip) return;
  mg_residual_body(G, x, b, lo, hi, s, res, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                   (int64_t)gridDim.x * blockDim.x);
}

__device__ __forceinline__ void mg_ijk(const MgGeo& G, int64_t idx, int& i, int& j, int& k) {
  const uint32_t u = (uint32_t)idx, nx = (uint32_t)G.nx;
  const uint32_t row = u / nx;
  i = (int)(u - row * nx);
  k = (int)(row / (uint32_t)G.ny);
  j = (int)(row - (uint32_t)k * (uint32_t)G.ny);
}

// b_c = R res_f, R = P^T / 8: 4 x 4 x 4 fine cells (2I-1 .. 2I+2 per direction). (The x-y sum is
// restrict_xy's below, written out: calling it here changes this kernel's and the tail's code)
__device__ __forceinline__ void mg_restrict_body(MgGeo F, const double* __restrict__ rf,
                                                 const double* __restrict__ lo,
                                                 const double* __restrict__ hi, MgGeo Cg,
                                                 double* __restrict__ bc, int64_t t0,
                                                 int64_t ts) {
  const double w[4] = {0.125, 0.375, 0.375, 0.125};
  for (int64_t idx = t0; idx < Cg.nlocal; idx += ts) {
    int I, J, K;
    mg_ijk(Cg, idx, I, J, K);
    const int xl = wrapm(2 * I - 1, F.nx), xr = wrapm(2 * I + 2, F.nx);
    double sz = 0.0;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int kf = 2 * K - 1 + c;
      const double* pl = kf < 0 ? lo : (kf >= F.nzl ? hi : rf + (int64_t)kf * F.plane);
      double sy = 0.0;
#pragma unroll
      for (int bb = 0; bb < 4; ++bb) {
        const double* row = pl + (int64_t)wrapm(2 * J - 1 + bb, F.ny) * F.nx;
        const dv2 mid = *(const dv2*)(row + 2 * I);
        double sx = w[0] * row[xl];
        sx = sx + w[1] * mid.x;
        sx = sx + w[2] * mid.y;
        sx = sx + w[3] * row[xr];
        sy = sy + w[bb] * sx;
      }
      sz = sz + w[c] * sy;
    }
    bc[idx] = sz;
  }
}
__global__ __launch_bounds__(256) void mg_restrict_kernel(MgGeo F, const double* __restrict__ rf,
                                                          const double* __restrict__ lo,
                                                          const double* __restrict__ hi, MgGeo Cg,
                                                          double* __restrict__ bc, const int* skip) {
  if (skip && *skip) return;
  mg_restrict_body(F, rf, lo, hi, Cg, bc, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                   (int64_t)gridDim.x * blockDim.x);
}

// The same restriction, one thread per coarse (I, J) column marching over a chunk of coarse
// planes: the x-y weighted sum sy of each fine plane is formed once and kept in a 4-plane
// window (the per-cell kernel forms it twice); the z sum is the per-cell kernel's, same order.
__device__ __forceinline__ double restrict_xy(const MgGeo& F, const double* pl, int I, int J,
                                              int xl, int xr) {
  const double w[4] = {0.125, 0.375, 0.375, 0.125};
  double sy = 0.0;
#pragma unroll
  for (int bb = 0; bb < 4; ++bb) {
    const double* row = pl + (int64_t)wrapm(2 * J - 1 + bb, F.ny) * F.nx;
    const dv2 mid = *(const dv2*)(row + 2 * I);
    double sx = w[0] * row[xl];
    sx = sx + w[1] * mid.x;
    sx = sx + w[2] * mid.y;
    sx = sx + w[3] * row[xr];
    sy = sy + w[bb] * sx;
  }
  return sy;
}

__global__ __launch_bounds__(256) void mg_restrict_z_kernel(MgGeo F, const double* __restrict__ rf,
                                                            const double* __restrict__ lo,
                                                            const double* __restrict__ hi,
                                                            MgGeo Cg, int kc,
                                                            double* __restrict__ bc,
                                                            const int* skip) {
  if (skip && *skip) return;
  const int64_t cols = (int64_t)Cg.nx * Cg.ny;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t col = t % cols;
  const int K0 = (int)(t / cols) * kc;
  if (K0 >= Cg.nzl) return;
  const int K1 = min(K0 + kc, Cg.nzl);
  const int I = (int)(col % Cg.nx), J = (int)(col / Cg.nx);
  const int xl = wrapm(2 * I - 1, F.nx), xr = wrapm(2 * I + 2, F.nx);
  auto plane = [&](int kf) {
    return kf < 0 ? lo : (kf >= F.nzl ? hi : rf + (int64_t)kf * F.plane);
  };
  double s0 = restrict_xy(F, plane(2 * K0 - 1), I, J, xl, xr);
  double s1 = restrict_xy(F, plane(2 * K0), I, J, xl, xr);
  for (int K = K0; K < K1; ++K) {
    const double s2 = restrict_xy(F, plane(2 * K + 1), I, J, xl, xr);
    const double s3 = restrict_xy(F, plane(2 * K + 2), I, J, xl, xr);
    double sz = 0.0;
    sz = sz + 0.125 * s0;
    sz = sz + 0.375 * s1;
    sz = sz + 0.375 * s2;
    sz = sz + 0.125 * s3;
    bc[(int64_t)K * Cg.plane + col] = sz;
    s0 = s2;
    s1 = s3;
  }
}

// x_f += P x_c (trilinear, cell-centred: near parent 3/4, far 1/4), one thread per coarse cell:
// its 2 x 2 x 2 fine children from the 3 x 3 x 3 coarse neighbourhood (each child by the formula
// above, same operation order), so a fine row pair is read and written with 16-byte accesses and
// each coarse value is fetched ~27/8 times per fine point instead of 6.
__device__ __forceinline__ void mg_prolong_cell_body(MgGeo F, double* __restrict__ xf, MgGeo Cg,
                                                     const double* __restrict__ xc,
                                                     const double* __restrict__ lo,
                                                     const double* __restrict__ hi, int64_t t0,
                                                     int64_t ts) {
  for (int64_t idx = t0; idx < Cg.nlocal; idx += ts) {
    int I, J, K;
    mg_ijk(Cg, idx, I, J, K);
    const int Im = wrapm(I - 1, Cg.nx), Ip = wrapm(I + 1, Cg.nx);
    const int Jm = wrapm(J - 1, Cg.ny), Jp = wrapm(J + 1, Cg.ny);
    const double* pn = xc + (int64_t)K * Cg.plane;
    const int64_t rn = (int64_t)J * Cg.nx;
#pragma unroll
    for (int dk = 0; dk < 2; ++dk) {
      const int fK = dk ? K + 1 : K - 1;
      const double* pf = fK < 0 ? lo : (fK >= Cg.nzl ? hi : xc + (int64_t)fK * Cg.plane);
#pragma unroll
      for (int dj = 0; dj < 2; ++dj) {
        const int64_t rf = (int64_t)(dj ? Jp : Jm) * Cg.nx;
        const double vn0 = 0.75 * (0.75 * pn[rn + I] + 0.25 * pn[rn + Im]) +
                           0.25 * (0.75 * pn[rf + I] + 0.25 * pn[rf + Im]);
        const double vf0 = 0.75 * (0.75 * pf[rn + I] + 0.25 * pf[rn + Im]) +
                           0.25 * (0.75 * pf[rf + I] + 0.25 * pf[rf + Im]);
        const double vn1 = 0.75 * (0.75 * pn[rn + I] + 0.25 * pn[rn + Ip]) +
                           0.25 * (0.75 * pn[rf + I] + 0.25 * pn[rf + Ip]);
        const double vf1 = 0.75 * (0.75 * pf[rn + I] + 0.25 * pf[rn + Ip]) +
                           0.25 * (0.75 * pf[rf + I] + 0.25 * pf[rf + Ip]);
        dv2* q = (dv2*)(xf + (int64_t)(2 * K + dk) * F.plane + (int64_t)(2 * J + dj) * F.nx + 2 * I);
        dv2 o = *q;
        o.x = o.x + (0.75 * vn0 + 0.25 * vf0);
        o.y = o.y + (0.75 * vn1 + 0.25 * vf1);
        *q = o;
      }
    }
  }
}
__global__ __launch_bounds__(256) void mg_prolong_cell_kernel(MgGeo F, double* __restrict__ xf,
                                                              MgGeo Cg,
                                                              const double* __restrict__ xc,
                                                              const double* __restrict__ lo,
                                                              const double* __restrict__ hi,
                                                              const int* skip) {
  if (skip && *skip) return;
  mg_prolong_cell_body(F, xf, Cg, xc, lo, hi, (int64_t)blockIdx.x * blockDim.x + threadIdx.x,
                       (int64_t)gridDim.x * blockDim.x);
}

// The same prolongation, one thread per coarse (I, J) column marching over a chunk of coarse
// planes: the 3 x 3 coarse values of planes K-1, K, K+1 stay in registers (each coarse value is
// loaded ~3 times per coarse cell instead of 27), children by the formula above.
// xout = xf + P xc (xout may be xf: in place).
struct Coarse9 {
  double v[3][3];  // [row Jm, J, Jp][col Im, I, Ip]
};
__device__ __forceinline__ void load9(const double* pl, int64_t rm, int64_t r0, int64_t rp, int Im,
                                      int I, int Ip, Coarse9& c) {
  const int64_t rows[3] = {rm, r0, rp};
  const int cols[3] = {Im, I, Ip};
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) c.v[a][b] = pl[rows[a] + cols[b]];
}

__global__ __launch_bounds__(256) void mg_prolong_z_kernel(MgGeo F, const double* xf,
                                                           double* xout, MgGeo Cg,
                                                           int kc, const double* __restrict__ xc,
                                                           const double* __restrict__ lo,
                                                           const double* __restrict__ hi,
                                                           const int* skip) {
  if (skip && *skip) return;
  const int64_t cols = (int64_t)Cg.nx * Cg.ny;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t col = t % cols;
  const int K0 = (int)(t / cols) * kc;
  if (K0 >= Cg.nzl) return;
  const int K1 = min(K0 + kc, Cg.nzl);
  const int I = (int)(col % Cg.nx), J = (int)(col / Cg.nx);
  const int Im = wrapm(I - 1, Cg.nx), Ip = wrapm(I + 1, Cg.nx);
  const int64_t rm = (int64_t)wrapm(J - 1, Cg.ny) * Cg.nx, r0 = (int64_t)J * Cg.nx,
                rp = (int64_t)wrapm(J + 1, Cg.ny) * Cg.nx;
  auto plane = [&](int K) {
    return K < 0 ? lo : (K >= Cg.nzl ? hi : xc + (int64_t)K * Cg.plane);
  };
  Coarse9 cm, c0, cp;
  load9(plane(K0 - 1), rm, r0, rp, Im, I, Ip, cm);
  load9(plane(K0), rm, r0, rp, Im, I, Ip, c0);
  for (int K = K0; K < K1; ++K) {
    load9(plane(K + 1), rm, r0, rp, Im, I, Ip, cp);
    // all four fine pairs are loaded before any is stored (the stores would otherwise order
    // each later load behind them)
    int64_t q[2][2];
    dv2 ov[2][2];
#pragma unroll
    for (int dk = 0; dk < 2; ++dk)
#pragma unroll
      for (int dj = 0; dj < 2; ++dj) {
        q[dk][dj] = (int64_t)(2 * K + dk) * F.plane + (int64_t)(2 * J + dj) * F.nx + 2 * I;
        ov[dk][dj] = *(const dv2*)(xf + q[dk][dj]);
      }
#pragma unroll
    for (int dk = 0; dk < 2; ++dk) {
      const Coarse9& pf = dk ? cp : cm;  // far plane: K+1 for odd fine k, K-1 for even
#pragma unroll
      for (int dj = 0; dj < 2; ++dj) {
        const int f = dj ? 2 : 0;  // far row: J+1 for odd fine j, J-1 for even
        const double vn0 = 0.75 * (0.75 * c0.v[1][1] + 0.25 * c0.v[1][0]) +
                           0.25 * (0.75 * c0.v[f][1] + 0.25 * c0.v[f][0]);
        const double vf0 = 0.75 * (0.75 * pf.v[1][1] + 0.25 * pf.v[1][0]) +
                           0.25 * (0.75 * pf.v[f][1] + 0.25 * pf.v[f][0]);
        const double vn1 = 0.75 * (0.75 * c0.v[1][1] + 0.25 * c0.v[1][2]) +
                           0.25 * (0.75 * c0.v[f][1] + 0.25 * c0.v[f][2]);
        const double vf1 = 0.75 * (0.75 * pf.v[1][1] + 0.25 * pf.v[1][2]) +
                           0.25 * (0.75 * pf.v[f][1] + 0.25 * pf.v[f][2]);
        dv2 o = ov[dk][dj];
        o.x = o.x + (0.75 * vn0 + 0.25 * vf0);
        o.y = o.y + (0.75 * vn1 + 0.25 * vf1);
        ov[dk][dj] = o;
      }
    }
#pragma unroll
    for (int dk = 0; dk < 2; ++dk)
#pragma unroll
      for (int dj = 0; dj < 2; ++dj) *(dv2*)(xout + q[dk][dj]) = ov[dk][dj];
    cm = c0;
    c0 = cp;
  }
}

// ---------------------------------------------------------------------------------------------
// Jacobi-type level smoothers (-mg_levels_pc_type jacobi under richardson or chebyshev). One step:
//   y_new = omega ((y - yp) + scale (dinv r)) + yp,  dinv = 1 / cc,
// every operation rounded in the order of its one definition (cheb_step, poly_second_step,
// poly_start_step in pb_device.hpp, which PolyLoad in pb_mg_engine.hip calls too), so the engine
// pass, the pair kernel and the vector kernel give the same bits. N = 3: y, yp, r; N = 2: y, r
// (yp = 0 or Richardson); N = 1: the zero start, from b alone.
// ---------------------------------------------------------------------------------------------
struct PolyArgs {
  const double* a0;  // N = 1: b; else y
  const double* a1;  // N = 2: r; N = 3: yp
  const double* a2;  // N = 3: r
  double scale, omega, dinv;
};
template <int N>
__device__ __forceinline__ double poly_value(const PolyArgs& A, double v0, double v1, double v2) {
  if constexpr (N == 1) return poly_start_step(v0, A.dinv, A.scale, A.omega);
  else if constexpr (N == 2) return poly_second_step(v0, v1, A.dinv, A.scale, A.omega);
  else return cheb_step<false>(v0, v1, v2, A.dinv, 0.0, A.scale, A.omega);
}
template <int N>
__device__ __forceinline__ double poly_at(const PolyArgs& A, int64_t id) {
  return poly_value<N>(A, A.a0[id], N >= 2 ? A.a1[id] : 0.0, N >= 3 ? A.a2[id] : 0.0);
}
template <int N>
__device__ __forceinline__ dv2 poly_pair(const PolyArgs& A, int64_t id) {
  const dv2 v0 = *(const dv2*)(A.a0 + id);
  dv2 v1 = v0, v2 = v0;
  if constexpr (N >= 2) v1 = *(const dv2*)(A.a1 + id);
  if constexpr (N >= 3) v2 = *(const dv2*)(A.a2 + id);
  dv2 o;
  o.x = poly_value<N>(A, v0.x, v1.x, v2.x);
  o.y = poly_value<N>(A, v0.y, v1.y, v2.y);
  return o;
}

// the vector kernel: y_out = the step's y_new (the unfused form, and a post-smoothing's last
// step, whose residual nobody reads). Elementwise: y_out may be one of the inputs.
template <int N>
__global__ __launch_bounds__(256) void mg_poly_x_kernel(int64_t npairs, PolyArgs A, double* y_out,
                                                        const int* skip) {
  if (skip && *skip) return;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npairs;
       q += (int64_t)gridDim.x * blockDim.x) {
    const dv2 o = poly_pair<N>(A, 2 * q);
    *(dv2*)(y_out + 2 * q) = o;
  }
}

// the pair kernel (one rank, small levels): y_new formed at the pair and its neighbours, stored
// with r_new = b - A y_new (mg_residual_body's sums). y_out, r_out: buffers the step does not read.
template <int N>
__global__ __launch_bounds__(256) void mg_poly_kernel(MgGeo G, PolyArgs A,
                                                      const double* __restrict__ b, Star s,
                                                      double* __restrict__ y_out,
                                                      double* __restrict__ r_out, const int* skip) {
  if (skip && *skip) return;
  const int64_t npairs = G.nlocal >> 1;
  for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < npairs;
       q += (int64_t)gridDim.x * blockDim.x) {
    const PairPos P = pair_pos(G, q);
    const int64_t row = P.idx - P.i0;
    const dv2 xc = poly_pair<N>(A, P.idx);
    const dv2 bc = *(const dv2*)(b + P.idx);
    const dv2 zm = poly_pair<N>(A, P.idx + (int64_t)(wrapm(P.k - 1, G.nzl) - P.k) * G.plane);
    const dv2 zp = poly_pair<N>(A, P.idx + (int64_t)(wrapm(P.k + 1, G.nzl) - P.k) * G.plane);
    const dv2 ym = poly_pair<N>(A, P.idx + (int64_t)(wrapm(P.j - 1, G.ny) - P.j) * G.nx);
    const dv2 yp = poly_pair<N>(A, P.idx + (int64_t)(wrapm(P.j + 1, G.ny) - P.j) * G.nx);
    const double xl = poly_at<N>(A, row + wrapm(P.i0 - 1, G.nx));
    const double xr = poly_at<N>(A, row + wrapm(P.i0 + 2, G.nx));
    *(dv2*)(r_out + P.idx) = residual_pair(s, bc, xc, zm, zp, ym, yp, xl, xr);
    *(dv2*)(y_out + P.idx) = xc;
  }
}

// ---------------------------------------------------------------------------------------------
// The coarse tail of the V-cycle in ONE launch (one rank): every level of at most
// PB_MG_TAIL_MAX points (16^3 at 512^3: the 16^3, 8^3 and 4^3 levels) -- down-legs, the coarsest
// level's sweeps and the up-legs -- run by one workgroup, step after step with a barrier between
// them, through the same per-point bodies as the per-level kernels (same operations, bit for bit).
// Replaces ~28 launches of a few microseconds each per V-cycle.
// ---------------------------------------------------------------------------------------------
struct TailLevel {
  MgGeo G;
  double* x;
  double* b;
  double* res;
  Star s;
  int64_t ox, ob, ores;  // LDS offsets (doubles) of x, b, res when the tail runs in LDS
};
static constexpr size_t kTailLdsMax = 144 * 1024;  // LDS the tail may take (of 160 KB per CU)
struct TailArgs {
  TailLevel lv[kTailMax];
  int nl;           // levels in the tail; lv[nl-1] is the coarsest
  int coarse_its;
  double omega;
  int lds;          // 1: every tail array lives in LDS (lv[0].b copied in, lv[0].x copied out)
};

__device__ __forceinline__ const double* wrap_lo(const MgGeo& G, const double* v) {
  return v + (int64_t)(G.nzl - 1) * G.plane;  // one rank: plane -1 is the last plane
}

// With A.lds the tail's arrays live in the workgroup's LDS (the 16^3, 8^3, 4^3 levels of a 512^3
// hierarchy: 109 KB): lv[0].b is copied in, lv[0].x copied out at the end, and every step in
// between reads and writes LDS through the same bodies (generic pointers) -- same operations on
// the same values, so the same bits; LDS instead of L2 latency on each of the ~35 dependent steps.
__global__ __launch_bounds__(512) void mg_tail_kernel(TailArgs A, const int* skip) {
  if (skip && *skip) return;
  extern __shared__ __attribute__((aligned(16))) double tl[];
  const int64_t t0 = threadIdx.x, ts = blockDim.x;
  const double w = A.omega;
  // level t's arrays (LDS or global); computed per use, so no array of pointers goes to scratch
  auto X = [&](int t) { return A.lds ? tl + A.lv[t].ox : A.lv[t].x; };
  auto Bv = [&](int t) { return A.lds ? tl + A.lv[t].ob : A.lv[t].b; };
  auto RES = [&](int t) { return A.lds ? tl + A.lv[t].ores : A.lv[t].res; };
  if (A.lds) {
    const double* src = A.lv[0].b;
    double* dst = Bv(0);
    for (int64_t i = t0; i < A.lv[0].G.nlocal; i += ts) dst[i] = src[i];
    __syncthreads();
  }
  auto smooth = [&](int t, int color, int mode) {
    const TailLevel& L = A.lv[t];
    double* x = X(t);
    const double* b = Bv(t);
    const double* v = mode == 1 ? b : x;
    mg_smooth_body(L.G, x, b, wrap_lo(L.G, v), v, L.s, w, color, mode, t0, ts);
    __syncthreads();
  };
  for (int t = 0; t + 1 < A.nl; ++t) {  // down: pre-smooth, residual, restrict
    const TailLevel& F = A.lv[t];
    smooth(t, 0, 1);
    double* x = X(t);
    double* res = RES(t);
    mg_residual_body(F.G, x, Bv(t), wrap_lo(F.G, x), x, F.s, res, t0, ts);
    __syncthreads();
    mg_restrict_body(F.G, res, wrap_lo(F.G, res), res, A.lv[t + 1].G, Bv(t + 1), t0, ts);
    __syncthreads();
  }
  {  // coarsest: `coarse_its` symmetric red-black sweeps from zero (coarse_solve's order)
    const int c = A.nl - 1;
    smooth(c, 0, 1);
    smooth(c, 0, 0);
    for (int it = 1; it < A.coarse_its; ++it) {
      smooth(c, 1, 0);
      smooth(c, 0, 0);
    }
  }
  for (int t = A.nl - 2; t >= 0; --t) {  // up: prolongate + correct, post-smooth
    const TailLevel& F = A.lv[t];
    const TailLevel& Cl = A.lv[t + 1];
    double* xf = X(t);
    const double* xc = X(t + 1);
    mg_prolong_cell_body(F.G, xf, Cl.G, xc, wrap_lo(Cl.G, xc), xc, t0, ts);
    __syncthreads();
    smooth(t, 1, 0);
    smooth(t, 0, 0);
  }
  if (A.lds) {
    const double* src = X(0);
    double* dst = A.lv[0].x;
    for (int64_t i = t0; i < A.lv[0].G.nlocal; i += ts) dst[i] = src[i];
  }
}

// chunks of coarse planes for the z-marching transfer kernels: ~16 resident waves per CU, at
// least 4 coarse planes per chunk
static int transfer_chunk(pb_ctx* ctx, int64_t cols, int64_t nzl, int64_t* nchunk_out) {
  const int64_t tpc = 1024;  // threads per CU
  const int64_t minz = 4;    // coarse planes per chunk, at least
  int64_t nchunk = ((int64_t)ctx->num_cus * tpc + cols - 1) / cols;
  nchunk = std::max<int64_t>(1, std::min<int64_t>(nchunk, nzl / minz));
  const int kc = (int)((nzl + nchunk - 1) / nchunk);
  *nchunk_out = (nzl + kc - 1) / kc;
  return kc;
}

// ---- the launchers (pb_mg.hpp): each kernel above is named here once; engine or pair kernel,
// marching or per-cell transfer is the level's LevelPlan's to say (pb_mg.cpp) ----
// one thread per item (no grid-stride loop unless the grid would exceed 2^30 blocks)
static int mg_blocks(int64_t n) {
  int64_t b = (n + 255) / 256;
  return (int)std::max<int64_t>(1, std::min<int64_t>(b, (int64_t)1 << 30));
}

int level_ghosts(MgLevel& L, const double* v, const double** lo, const double** hi) {
  pb_grid* g = L.g;
  if (!g->ctx->split) {
    *lo = v + (g->nzl - 1) * g->plane;
    *hi = v;
    return PB_OK;
  }
  PB_TRY(halo_exchange(g, v, v + (g->nzl - 1) * g->plane));
  *lo = g->ghost_lo;
  *hi = g->ghost_hi;
  return PB_OK;
}

int level_smooth(Mg* mg, MgLevel& L, int color, int mode, MgSums sums) {
  if (mg->coef) return vmg_smooth(mg, L, color, mode);
  const double *lo = nullptr, *hi = nullptr;
  PB_TRY(level_ghosts(L, mode == 1 ? L.b : L.x, &lo, &hi));
  if (L.plan.engine) {
    const StencilPlanes gp{lo, hi};
    return launch_mg_sor(L.g, L.s, L.x, L.b, gp, mg->omega, color, mode == 1, mg->skip,
                         mode == 0 ? sums.st : nullptr, mode == 0 ? sums.nparts : nullptr);
  }
  const MgGeo G = L.geo();
  hipLaunchKernelGGL(mg_smooth_kernel, dim3(mg_blocks(G.nlocal / 2)), dim3(256), 0,
                     mg->ctx->stream, G, L.x, (const double*)L.b, lo, hi, L.s, mg->omega, color,
                     mode, mg->skip);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int level_residual(Mg* mg, MgLevel& F, const double* x, double* res) {
  if (mg->coef) return vmg_residual(mg, F, x, res);
  const double *lo, *hi;
  PB_TRY(level_ghosts(F, x, &lo, &hi));
  if (F.plan.engine)
    return launch_mg_residual(F.g, F.s, x, F.b, StencilPlanes{lo, hi}, res, mg->skip);
  const MgGeo G = F.geo();
  hipLaunchKernelGGL(mg_residual_kernel, dim3(mg_blocks(G.nlocal / 2)), dim3(256), 0,
                     mg->ctx->stream, G, x, (const double*)F.b, lo, hi, F.s, res, mg->skip);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int level_restrict(Mg* mg, MgLevel& F, const double* res, MgLevel& C) {
  const double *lo, *hi;
  PB_TRY(level_ghosts(F, res, &lo, &hi));
  const MgGeo G = F.geo(), CG = C.geo();
  if (F.plan.march) {
    const int64_t cols = (int64_t)CG.nx * CG.ny;
    int64_t nchunk = 1;
    const int kc = transfer_chunk(mg->ctx, cols, CG.nzl, &nchunk);
    hipLaunchKernelGGL(mg_restrict_z_kernel, dim3(mg_blocks(cols * nchunk)), dim3(256), 0,
                       mg->ctx->stream, G, res, lo, hi, CG, kc, C.b, mg->skip);
  } else {
    hipLaunchKernelGGL(mg_restrict_kernel, dim3(mg_blocks(CG.nlocal)), dim3(256), 0,
                       mg->ctx->stream, G, res, lo, hi, CG, C.b, mg->skip);
  }
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int level_prolong(Mg* mg, MgLevel& F, const double* xf, double* xout, MgLevel& C,
                  const CoarsePlanes* cp) {
  CoarsePlanes p{C.x, nullptr, nullptr};
  if (cp) p = *cp;
  else PB_TRY(level_ghosts(C, C.x, &p.lo, &p.hi));
  const MgGeo G = F.geo(), CG = C.geo();
  if (F.plan.march) {
    const int64_t cols = (int64_t)CG.nx * CG.ny;
    int64_t nchunk = 1;
    const int kc = transfer_chunk(mg->ctx, cols, CG.nzl, &nchunk);
    hipLaunchKernelGGL(mg_prolong_z_kernel, dim3(mg_blocks(cols * nchunk)), dim3(256), 0,
                       mg->ctx->stream, G, xf, xout, CG, kc, p.xc, p.lo, p.hi, mg->skip);
  } else {
    if (xout != xf) return set_error(PB_ERR_ARG, "the per-cell prolongation runs in place");
    hipLaunchKernelGGL(mg_prolong_cell_kernel, dim3(mg_blocks(CG.nlocal)), dim3(256), 0,
                       mg->ctx->stream, G, xout, CG, p.xc, p.lo, p.hi, mg->skip);
  }
  PB_HIP(hipGetLastError());
  return PB_OK;
}

// f(N) with N = std::integral_constant<int, n>, n = 1 | 2 | 3: a polynomial kernel's inputs
template <class Fn>
static void with_poly_inputs(int n, Fn&& f) {
  if (n == 1) f(std::integral_constant<int, 1>{});
  else if (n == 2) f(std::integral_constant<int, 2>{});
  else f(std::integral_constant<int, 3>{});
}

// Fused (one rank, tuning mg_poly_fused = 1): the engine pass on large levels, the pair kernel
// below; else the vector kernel, a ghost exchange of y_out and the residual pass -- the same
// expressions, so the same bits, and what a decomposed grid runs.
int poly_step(Mg* mg, MgLevel& F, const double* y, const double* yp, const double* r, double scale,
              double omega, double* y_out, double* r_out) {
  pb_ctx* ctx = mg->ctx;
  const MgGeo G = F.geo();
  const int n = !y ? 1 : (!yp ? 2 : 3);
  const double dinv = 1.0 / F.s.cc;
  const PolyArgs A = n == 1 ? PolyArgs{F.b, nullptr, nullptr, scale, omega, dinv}
                   : n == 2 ? PolyArgs{y, r, nullptr, scale, omega, dinv}
                            : PolyArgs{y, yp, r, scale, omega, dinv};
  const dim3 grid(mg_blocks(G.nlocal / 2)), block(256);
  const bool fused = r_out && !ctx->split && mg->tn.poly_fused;
  if (fused && F.plan.engine)
    return launch_mg_poly(F.g, F.s, y, yp, r, F.b, scale, omega, y_out, r_out, mg->skip);
  if (fused) {
    const double* b = F.b;
    with_poly_inputs(n, [&](auto N) {
      hipLaunchKernelGGL(mg_poly_kernel<decltype(N)::value>, grid, block, 0, ctx->stream, G, A, b,
                         F.s, y_out, r_out, mg->skip);
    });
    PB_HIP(hipGetLastError());
    return PB_OK;
  }
  const int64_t npairs = G.nlocal / 2;
  with_poly_inputs(n, [&](auto N) {
    hipLaunchKernelGGL(mg_poly_x_kernel<decltype(N)::value>, grid, block, 0, ctx->stream, npairs,
                       A, y_out, mg->skip);
  });
  PB_HIP(hipGetLastError());
  return r_out ? level_residual(mg, F, y_out, r_out) : PB_OK;
}

int launch_tail(Mg* mg, int Lt, bool agg) {
  pb_ctx* ctx = mg->ctx;
  TailArgs A{};
  A.nl = (int)mg->lv.size() - Lt;
  A.coarse_its = mg->coarse_its;
  A.omega = mg->omega;
  int64_t off = 0;
  for (int t = 0; t < A.nl; ++t) {
    const MgLevel& lv = mg->lv[Lt + t];
    A.lv[t] = agg ? TailLevel{mg->ageo[t], mg->ax[t], mg->ab[t], mg->ares[t], lv.s, 0, 0, 0}
                  : TailLevel{lv.geo(), lv.x, lv.b, lv.res, lv.s, 0, 0, 0};
    const int64_t n = (A.lv[t].G.nlocal + 1) & ~(int64_t)1;  // 16-byte aligned arrays
    A.lv[t].ox = off;
    A.lv[t].ob = off + n;
    A.lv[t].ores = off + 2 * n;
    off += (t + 1 < A.nl ? 3 : 2) * n;
  }
  // the tail in LDS when it fits (512^3: 109 KB of the 160 KB per CU)
  const size_t lds = (size_t)off * sizeof(double);
  A.lds = lds <= kTailLdsMax;
  if (A.lds && !mg->tail_attr) {
    PB_HIP(hipFuncSetAttribute((const void*)mg_tail_kernel,
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)kTailLdsMax));
    mg->tail_attr = true;
  }
  hipLaunchKernelGGL(mg_tail_kernel, dim3(1), dim3(512), A.lds ? lds : 0, ctx->stream, A,
                     mg->skip);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

}  // namespace pb
