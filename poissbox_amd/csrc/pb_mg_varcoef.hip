// pb_mg_varcoef.hip -- the variable-coefficient levels of -pc_type sor | mg
// (pb_ksp_pc_set_coefficient_from; DESIGN.md §3.5, restated in tests/varcoef_mg_restatement.py):
// every level's smoother, residual and operator are div(beta_l grad) with the face mean of the
// PB_OP_VARCOEF operator the coefficient comes from.
//
//   levels      beta_0 = the operator's beta; a coarse cell is the arithmetic mean of its 8 children,
//               0.125 (((b000 + b100) + (b010 + b110)) + ((b001 + b101) + (b011 + b111))), b_abc the
//               fine cell (2I + a, 2J + b, 2K + c); c_d = 1 / (2^l h_d)^2 of the operator's deltas
//   faces       g_n = c_d face(beta_n, beta_c) (vc_face, pb_device.hpp: the operator's own)
//   mass        the operator's q = s m (pb_op_set_mass): q_0 = s * m, q_(l+1) the 8-child mean of
//               q_l as beta's; a scalar-only mass is s on every level; point-local, no ghost planes
//   dinv        1.0 / diag_c, diag_c = -(((((g_z- + g_y-) + g_x-) + g_x+) + g_y+) + g_z+) - q_c
//               (varcoef_diag_kernel), stored per level with its ghost planes
//   half-sweep  nb = ((((g_z- x_z- + g_y- x_y-) + g_x- x_x-) + g_x+ x_x+) + g_y+ x_y+) + g_z+ x_z+,
//               t = (b - nb) dinv, x = (1 - omega) x + omega t on the colour, red = (i + j + k) even;
//               the zero-initialised first half-sweep has nb = 0.0 and x = 0.0 in the same formula
//   residual    b - A x by the operator's own kernel (varcoef_kernel's RES form, pb_varcoef.hip),
//               A x = S6 - q x
//
// The half-sweeps: one thread owns an (i even, i + 1) pair of a row and marches over a chunk of
// planes with the pairs of x and beta of planes k - 1, k, k + 1 in registers (each loaded once per
// chunk); it updates the point of the colour and stores that point alone. No two points of a colour
// are neighbours, so a half-sweep has no face in common between the points it updates.
// The zero-start red + black pass (tuning mg_varcoef_pre_fused): black needs the red values at its
// six neighbours, each omega ((b - 0.0) dinv) of b and dinv there -- the pairs of b, dinv and beta
// march in registers, x is written once, never read.
#include <algorithm>

#include "pb_device.hpp"
#include "pb_mg.hpp"

namespace pb {

struct VcLevel {
  double cx, cy, cz;
  const double* beta;  // local plane 0; planes -1 and nzl in place
  const double* dinv;  // likewise
  const double* q;     // the level's mass field (MASS = 2), qs the scalar mass (MASS = 1)
  double qs;
};

__device__ __forceinline__ int vwrap(int v, int n) { return v < 0 ? v + n : (v >= n ? v - n : v); }

// the column of pairs a thread owns and its chunk of planes [K0, K1)
struct VcCol {
  int i0, j, im, ip, K0, K1;
  int64_t rj, rjm, rjp;  // row offsets of j, j - 1, j + 1 in a plane
};
__device__ __forceinline__ bool vc_col(const MgGeo& G, int kc, VcCol& q) {
  const uint32_t hx = (uint32_t)G.nx >> 1;
  const int64_t cols = (int64_t)hx * G.ny;
  const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t col = (uint32_t)(t % cols);
  q.K0 = (int)(t / cols) * kc;
  if (q.K0 >= G.nzl) return false;
  q.K1 = min(q.K0 + kc, G.nzl);
  q.j = (int)(col / hx);
  q.i0 = (int)(col - (uint32_t)q.j * hx) * 2;
  q.im = vwrap(q.i0 - 1, G.nx);
  q.ip = vwrap(q.i0 + 2, G.nx);
  q.rj = (int64_t)q.j * G.nx;
  q.rjm = (int64_t)vwrap(q.j - 1, G.ny) * G.nx;
  q.rjp = (int64_t)vwrap(q.j + 1, G.ny) * G.nx;
  return true;
}

// the six face coefficients of the point (i0 + d, j, k), z-, y-, x-, x+, y+, z+: bm, bc, bp the
// beta pairs of planes k - 1, k, k + 1, bk the plane k of beta
struct Faces {
  double zm, ym, xm, xp, yp, zp;
};
template <int HARM>
__device__ __forceinline__ Faces vc_faces(const VcLevel& c, const VcCol& q, int d, dv2 bm, dv2 bc,
                                          dv2 bp, const double* __restrict__ bk) {
  const int ic = q.i0 + d;
  const double b0 = d ? bc.y : bc.x;
  Faces f;
  f.zm = c.cz * vc_face<HARM>(d ? bm.y : bm.x, b0);
  f.ym = c.cy * vc_face<HARM>(bk[q.rjm + ic], b0);
  f.xm = c.cx * vc_face<HARM>(d ? bc.x : bk[q.rj + q.im], b0);
  f.xp = c.cx * vc_face<HARM>(d ? bk[q.rj + q.ip] : bc.y, b0);
  f.yp = c.cy * vc_face<HARM>(bk[q.rjp + ic], b0);
  f.zp = c.cz * vc_face<HARM>(d ? bp.y : bp.x, b0);
  return f;
}
// q: the mass term at the point (MASS != 0)
template <int MASS>
__device__ __forceinline__ double faces_dinv(const Faces& f, double q) {
  double s = f.zm + f.ym;
  s = s + f.xm;
  s = s + f.xp;
  s = s + f.yp;
  s = s + f.zp;
  if constexpr (MASS != 0) return 1.0 / (-s - q);
  else return 1.0 / -s;
}

// One half-sweep of `color` in place. lo / hi: x's planes -1 and nzl. ZERO: the zero-initialised
// first half-sweep -- x is not read, the colour gets omega ((b - 0.0) dinv) and the other colour
// 0.0 (a pair store). DST: dinv from the level's stored field, else from the six faces and the
// mass term at the point (MASS: 0 none, 1 the scalar c.qs, 2 the field c.q; DST: 0, the stored
// field holds it).
template <int HARM, int ZERO, int DST, int MASS>
__global__ __launch_bounds__(256) void vmg_half_kernel(MgGeo G, VcLevel c, double* x,
                                                       const double* __restrict__ b,
                                                       const double* lo, const double* hi,
                                                       double omega, int color, int kc,
                                                       const int* __restrict__ skip) {
  if (skip && *skip) return;
  VcCol q;
  if (!vc_col(G, kc, q)) return;
  constexpr bool kFaces = !(ZERO && DST);
  auto xpl = [&](int k) {
    return k < 0 ? lo : (k >= G.nzl ? hi : (const double*)x + (int64_t)k * G.plane);
  };
  const int64_t pc = q.rj + q.i0;
  dv2 bm = {0.0, 0.0}, bc = {0.0, 0.0}, xm = {0.0, 0.0}, xc = {0.0, 0.0};
  if constexpr (kFaces) {
    bm = *(const dv2*)(c.beta + (int64_t)(q.K0 - 1) * G.plane + pc);
    bc = *(const dv2*)(c.beta + (int64_t)q.K0 * G.plane + pc);
  }
  if constexpr (!ZERO) {
    xm = *(const dv2*)(xpl(q.K0 - 1) + pc);
    xc = *(const dv2*)(xpl(q.K0) + pc);
  }
  for (int k = q.K0; k < q.K1; ++k) {
    const int64_t base = (int64_t)k * G.plane;
    dv2 bp = {0.0, 0.0}, xp = {0.0, 0.0};
    if constexpr (kFaces) bp = *(const dv2*)(c.beta + base + G.plane + pc);
    if constexpr (!ZERO) xp = *(const dv2*)(xpl(k + 1) + pc);
    const int d = (int)((color + q.j + G.k0 + k) & 1);  // offset of the updated point in the pair
    const int ic = q.i0 + d;
    const int64_t id = base + q.rj + ic;
    Faces f = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if constexpr (kFaces) f = vc_faces<HARM>(c, q, d, bm, bc, bp, c.beta + base);
    double dinv;
    if constexpr (DST) dinv = c.dinv[id];
    else if constexpr (MASS == 2) dinv = faces_dinv<2>(f, c.q[id]);
    else dinv = faces_dinv<MASS>(f, c.qs);
    double nb = 0.0, xo = 0.0;
    if constexpr (!ZERO) {
      const double* xk = x + base;
      nb = f.zm * (d ? xm.y : xm.x) + f.ym * xk[q.rjm + ic];
      nb = nb + f.xm * (d ? xc.x : xk[q.rj + q.im]);
      nb = nb + f.xp * (d ? xk[q.rj + q.ip] : xc.y);
      nb = nb + f.yp * xk[q.rjp + ic];
      nb = nb + f.zp * (d ? xp.y : xp.x);
      xo = d ? xc.y : xc.x;
    }
    const double t = (b[id] - nb) * dinv;
    const double xn = (1.0 - omega) * xo + omega * t;
    if constexpr (ZERO) {
      dv2 o;
      o.x = d ? 0.0 : xn;
      o.y = d ? xn : 0.0;
      *(dv2*)(x + base + pc) = o;
    } else {
      x[id] = xn;
    }
    bm = bc;
    bc = bp;
    xm = xc;
    xc = xp;
  }
}

// The zero-initialised red and black half-sweeps in one pass: x from b, dinv and beta.
// lo / hi: b's planes -1 and nzl.
template <int HARM>
__global__ __launch_bounds__(256) void vmg_pre_kernel(MgGeo G, VcLevel c, double* __restrict__ x,
                                                      const double* __restrict__ b,
                                                      const double* __restrict__ lo,
                                                      const double* __restrict__ hi, double omega,
                                                      int kc, const int* __restrict__ skip) {
  if (skip && *skip) return;
  VcCol q;
  if (!vc_col(G, kc, q)) return;
  auto bpl = [&](int k) { return k < 0 ? lo : (k >= G.nzl ? hi : b + (int64_t)k * G.plane); };
  // a red value after the first half-sweep, from b and dinv there
  auto red0 = [&](double bv, double dv) {
    const double t = (bv - 0.0) * dv;
    return (1.0 - omega) * 0.0 + omega * t;
  };
  const int64_t pc = q.rj + q.i0;
  const int64_t b0 = (int64_t)q.K0 * G.plane;
  dv2 tm = *(const dv2*)(c.beta + b0 - G.plane + pc), tc = *(const dv2*)(c.beta + b0 + pc);
  dv2 dm = *(const dv2*)(c.dinv + b0 - G.plane + pc), dc = *(const dv2*)(c.dinv + b0 + pc);
  dv2 rm = *(const dv2*)(bpl(q.K0 - 1) + pc), rc = *(const dv2*)(bpl(q.K0) + pc);
  for (int k = q.K0; k < q.K1; ++k) {
    const int64_t base = (int64_t)k * G.plane;
    const dv2 tp = *(const dv2*)(c.beta + base + G.plane + pc);
    const dv2 dp = *(const dv2*)(c.dinv + base + G.plane + pc);
    const dv2 rp = *(const dv2*)(bpl(k + 1) + pc);
    const int d = (int)((1 + q.j + G.k0 + k) & 1);  // offset of the black point in the pair
    const int ic = q.i0 + d;
    const double* bk = b + base;
    const double* dk = c.dinv + base;
    const Faces f = vc_faces<HARM>(c, q, d, tm, tc, tp, c.beta + base);
    const double xr = d ? red0(rc.x, dc.x) : red0(rc.y, dc.y);  // the pair's red point
    double nb = f.zm * (d ? red0(rm.y, dm.y) : red0(rm.x, dm.x)) +
                f.ym * red0(bk[q.rjm + ic], dk[q.rjm + ic]);
    nb = nb + f.xm * (d ? xr : red0(bk[q.rj + q.im], dk[q.rj + q.im]));
    nb = nb + f.xp * (d ? red0(bk[q.rj + q.ip], dk[q.rj + q.ip]) : xr);
    nb = nb + f.yp * red0(bk[q.rjp + ic], dk[q.rjp + ic]);
    nb = nb + f.zp * (d ? red0(rp.y, dp.y) : red0(rp.x, dp.x));
    const double t = ((d ? rc.y : rc.x) - nb) * (d ? dc.y : dc.x);
    const double xb = (1.0 - omega) * 0.0 + omega * t;
    dv2 o;
    o.x = d ? xr : xb;
    o.y = d ? xb : xr;
    *(dv2*)(x + base + pc) = o;
    tm = tc;
    tc = tp;
    dm = dc;
    dc = dp;
    rm = rc;
    rc = rp;
  }
}

// beta_c = the arithmetic mean of the 8 children (owned coarse cells: the children are local)
__global__ __launch_bounds__(256) void vmg_coarsen_kernel(MgGeo F, const double* __restrict__ bf,
                                                          MgGeo C, double* __restrict__ bc) {
  for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x; idx < C.nlocal;
       idx += (int64_t)gridDim.x * 256) {
    const uint32_t u = (uint32_t)idx, nx = (uint32_t)C.nx;
    const uint32_t row = u / nx;
    const int I = (int)(u - row * nx);
    const int K = (int)(row / (uint32_t)C.ny);
    const int J = (int)(row - (uint32_t)K * (uint32_t)C.ny);
    const double* p0 = bf + (int64_t)(2 * K) * F.plane + (int64_t)(2 * J) * F.nx + 2 * I;
    const double* p1 = p0 + F.plane;
    const dv2 a00 = *(const dv2*)p0, a10 = *(const dv2*)(p0 + F.nx);
    const dv2 a01 = *(const dv2*)p1, a11 = *(const dv2*)(p1 + F.nx);
    const double s0 = (a00.x + a00.y) + (a10.x + a10.y);
    const double s1 = (a01.x + a01.y) + (a11.x + a11.y);
    bc[idx] = 0.125 * (s0 + s1);
  }
}

// ---- the launchers ----
static int vmg_blocks(int64_t n) {
  return (int)std::max<int64_t>(1, std::min<int64_t>((n + 255) / 256, (int64_t)1 << 30));
}

// chunks of planes for the marching half-sweeps: ~16 resident waves per CU where the level has
// the planes for it
static int vmg_chunk(const Mg* mg, int64_t cols, int64_t nzl, int64_t* nchunk_out) {
  int64_t nchunk = ((int64_t)mg->ctx->num_cus * 1024 + cols - 1) / cols;
  nchunk = std::max<int64_t>(1, std::min<int64_t>(nchunk, nzl));
  int kc = (int)((nzl + nchunk - 1) / nchunk);
  if (mg->tn.vc_kc > 0) kc = (int)std::min<int64_t>(mg->tn.vc_kc, nzl);
  *nchunk_out = (nzl + kc - 1) / kc;
  return kc;
}

static VcLevel vc_level(const MgLevel& L) {
  return VcLevel{L.vs.cx, L.vs.cy, L.vs.cz, L.beta, L.dinv, L.q, L.qs};
}

template <int HARM, int ZERO>
static void launch_half(Mg* mg, MgLevel& L, const double* lo, const double* hi, int color) {
  const MgGeo G = L.geo();
  const int64_t cols = (int64_t)(G.nx / 2) * G.ny;
  int64_t nchunk = 1;
  const int kc = vmg_chunk(mg, cols, G.nzl, &nchunk);
  const dim3 grid(vmg_blocks(cols * nchunk)), block(256);
#define PB_VMG_HALF(DST_, MASS_)                                                                \
  hipLaunchKernelGGL((vmg_half_kernel<HARM, ZERO, DST_, MASS_>), grid, block, 0, mg->ctx->stream, \
                     G, vc_level(L), L.x, (const double*)L.b, lo, hi, mg->omega, color, kc,       \
                     mg->skip)
  if (mg->tn.vc_dinv_stored) PB_VMG_HALF(1, 0);
  else if (L.q) PB_VMG_HALF(0, 2);
  else if (L.qs != 0.0) PB_VMG_HALF(0, 1);
  else PB_VMG_HALF(0, 0);
#undef PB_VMG_HALF
}

int vmg_smooth(Mg* mg, MgLevel& L, int color, int mode) {
  const bool harm = mg->mean == PB_COEF_HARMONIC;
  const double *lo = nullptr, *hi = nullptr;
  // (timers: vmg_pre | vmg_pre_red + vmg_pre_black | vmg_half, vmg_residual: scripts/bench_varcoef_mg.py)
  if (mode == 1 && mg->tn.vc_pre_fused) {
    PB_TRY(level_ghosts(L, L.b, &lo, &hi));
    ScopedTimer tm(mg->ctx, "vmg_pre");
    const MgGeo G = L.geo();
    const int64_t cols = (int64_t)(G.nx / 2) * G.ny;
    int64_t nchunk = 1;
    const int kc = vmg_chunk(mg, cols, G.nzl, &nchunk);
    const dim3 grid(vmg_blocks(cols * nchunk)), block(256);
    if (harm)
      hipLaunchKernelGGL(vmg_pre_kernel<1>, grid, block, 0, mg->ctx->stream, G, vc_level(L), L.x,
                         (const double*)L.b, lo, hi, mg->omega, kc, mg->skip);
    else
      hipLaunchKernelGGL(vmg_pre_kernel<0>, grid, block, 0, mg->ctx->stream, G, vc_level(L), L.x,
                         (const double*)L.b, lo, hi, mg->omega, kc, mg->skip);
    PB_HIP(hipGetLastError());
    return PB_OK;
  }
  const bool pre = mode == 1;
  if (pre) {  // red from zero (no plane of x is read), then black as any half-sweep
    ScopedTimer tm(mg->ctx, "vmg_pre_red");
    if (harm) launch_half<1, 1>(mg, L, nullptr, nullptr, 0);
    else launch_half<0, 1>(mg, L, nullptr, nullptr, 0);
    PB_HIP(hipGetLastError());
    color = 1;
  }
  PB_TRY(level_ghosts(L, L.x, &lo, &hi));
  ScopedTimer tm(mg->ctx, pre ? "vmg_pre_black" : "vmg_half");
  if (harm) launch_half<1, 0>(mg, L, lo, hi, color);
  else launch_half<0, 0>(mg, L, lo, hi, color);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

// what the operator's kernels read of a level: its q as the field with s = 1.0 (1.0 * q is exact)
// or the scalar
static VarCoef level_coef(const Mg* mg, const MgLevel& L) {
  return VarCoef{L.vs.cx, L.vs.cy, L.vs.cz, L.beta, mg->mean, L.q, L.q ? 1.0 : L.qs};
}

int vmg_residual(Mg* mg, MgLevel& F, const double* x, double* res) {
  StencilPlanes gp = wrap_planes();  // one rank: x's wrap planes in place
  if (mg->ctx->split) {
    PB_TRY(level_ghosts(F, x, &gp.ghost_lo, &gp.ghost_hi));
    gp.wrap = false;
  }
  const VarCoef c = level_coef(mg, F);
  ScopedTimer tm(mg->ctx, "vmg_residual");
  return launch_varcoef_residual(F.g, c, x, F.b, res, gp, mg->skip);
}

// q_0 = s * m
__global__ __launch_bounds__(256) void vmg_mass_kernel(const double* __restrict__ m, double s,
                                                       double* __restrict__ q, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
    q[i] = s * m[i];
}

int vmg_build(Mg* mg) {
  const pb_op* C = mg->coef;
  mg->mean = C->mean;
  const bool qfield = C->mass_on() && C->mass;
  if (qfield && !mg->qmem) {
    int64_t total = 0;
    for (const MgLevel& lv : mg->lv) total += lv.g->nlocal;
    if (hipMalloc(&mg->qmem, (size_t)total * sizeof(double)) != hipSuccess)
      return set_error(PB_ERR_ALLOC, "multigrid level mass fields: out of device memory");
  }
  double* qp = mg->qmem;
  for (size_t l = 0; l < mg->lv.size(); ++l) {
    MgLevel& lv = mg->lv[l];
    pb_grid* g = lv.g;
    double h[3];
    for (int d = 0; d < 3; ++d) h[d] = C->deltas[d] * (double)(1 << l);
    lv.vs = star_coeffs(h);
    if (l == 0) {
      lv.beta = C->beta;
    } else {
      const MgLevel& F = mg->lv[l - 1];
      hipLaunchKernelGGL(vmg_coarsen_kernel, dim3(vmg_blocks(g->nlocal)), dim3(256), 0,
                         mg->ctx->stream, F.geo(), F.beta, lv.geo(), lv.beta_own);
      PB_HIP(hipGetLastError());
      PB_TRY(halo_exchange_n(g, lv.beta_own, lv.beta_own + (g->nzl - 1) * g->plane, 1,
                             lv.beta_own - g->plane, lv.beta_own + g->nlocal));
      lv.beta = lv.beta_own;
    }
    lv.q = nullptr;
    lv.qs = qfield ? 0.0 : C->mass_s;
    if (qfield) {
      lv.q = qp;
      qp += g->nlocal;
      if (l == 0)
        hipLaunchKernelGGL(vmg_mass_kernel, dim3(vmg_blocks(g->nlocal)), dim3(256), 0,
                           mg->ctx->stream, C->mass, C->mass_s, lv.q, g->nlocal);
      else
        hipLaunchKernelGGL(vmg_coarsen_kernel, dim3(vmg_blocks(g->nlocal)), dim3(256), 0,
                           mg->ctx->stream, mg->lv[l - 1].geo(), (const double*)mg->lv[l - 1].q,
                           lv.geo(), lv.q);
      PB_HIP(hipGetLastError());
    }
    const VarCoef c = level_coef(mg, lv);
    PB_TRY(launch_varcoef_diag(g, c, lv.dinv, true));
    PB_TRY(halo_exchange_n(g, lv.dinv, lv.dinv + (g->nzl - 1) * g->plane, 1, lv.dinv - g->plane,
                           lv.dinv + g->nlocal));
  }
  mg->coef_seen = C->change;
  return PB_OK;
}

}  // namespace pb
