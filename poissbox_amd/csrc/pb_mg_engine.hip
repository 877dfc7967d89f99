// pb_mg_engine.hip -- the multigrid's passes on the stencil engine (pb_star7.hpp): the red-black
// SOR half-sweeps, the level residual and the Jacobi-type level smoothers with their residual, as
// pb_mg.hip launches them on levels with large planes (mg_engine_min_plane). The fused sweeps of
// the V-cycle's legs are pb_mg_sweep.hip's.
#include "pb_star7.hpp"

namespace pb {

// ---------------------------------------------------------------------------------------------
// Red-black SOR smoothing and the multigrid residual on the engine (pb_mg.hip; oracle
// pbo_mg_apply). PETSc PCSOR update form x = (1 - w) x + w (b - sum_nb c x_nb) / c_centre,
// neighbour sum in the order z-, y-, x-, x+, y+, z+. A half-sweep updates the points with
// (i + j + k_global) % 2 == color in place: their neighbours all carry the other colour, which
// the half-sweep does not modify, so halo rows read from other waves are the same whether or not
// those waves have stored their plane yet (the stored other-colour values are bit-identical).
// ---------------------------------------------------------------------------------------------
// the red values of the first half-sweep from x = 0: (1 - w) * 0 + w * ((b - 0) * (1 / c))
struct Red0Load {
  static constexpr int NR = 1;
  static constexpr bool GHOST_RAW = true;  // ghost planes are b's: transform them too
  const double* __restrict__ b;
  double icc, omega;  // icc = 1 / c (the SOR update multiplies by the inverted diagonal)
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ const double* src(int) const { return b; }
  __device__ __forceinline__ double value(const double* raw) const {
    const double t = (raw[0] - 0.0) * icc;
    return (1.0 - omega) * 0.0 + omega * t;
  }
};

// SUMS: the last half-sweep of a preconditioner apply inside CG also takes the residual sums of
// its output z against r = b (t = z - mu_old: sum t, t^2, t.r, r -- cg_pc_sums_kernel's)
template <bool SUMS>
struct SorHalfT {
  static constexpr int NS = SUMS ? 4 : 0, NE = 1;
  static constexpr bool PREFETCH = true, RAW = true;
  static constexpr int WGCU = 1;  // (the zero-start sweep overrides: 3)
  double* x;
  const double* __restrict__ b;
  double cx, cy, cz, icc, omega;  // icc = 1 / c
  int color;  // points with (i + j + k_global) % 2 == color are updated
  int first;  // 1: black half-sweep after the zero-start red one (x_old = 0, field = Red0Load)
  const CgState* st;
  double mu;
  __device__ __forceinline__ void prepare() {
    if constexpr (SUMS) mu = st->mu;
  }
  __device__ __forceinline__ const double* src(int) const { return b; }
  template <int V>
  __device__ __forceinline__ void put_raw(RowIx idx, int par, const double (&zm)[V],
                                          const double (&ym)[V], const double (&xm)[V],
                                          const double (&c)[V], const double (&xp)[V],
                                          const double (&yp)[V], const double (&zp)[V],
                                          const double (&op)[1][V], double* acc, int nt) const {
    double o[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
      double nb = cz * zm[e];
      nb = nb + cy * ym[e];
      nb = nb + cx * xm[e];
      nb = nb + cx * xp[e];
      nb = nb + cy * yp[e];
      nb = nb + cz * zp[e];
      const double t = (op[0][e] - nb) * icc;
      const double xo = first ? 0.0 : c[e];
      const double xn = (1.0 - omega) * xo + omega * t;
      o[e] = ((par + e) & 1) == color ? xn : c[e];
      if constexpr (SUMS) {
        const double rv = op[0][e];
        const double t2 = o[e] - mu;
        acc[0] += t2;
        acc[1] += t2 * t2;
        acc[2] += t2 * rv;
        acc[3] += rv;
      }
    }
    store_row<V>(x, idx, o, nt);
    (void)acc;
  }
};
typedef SorHalfT<false> SorHalf;

// res = b - A x (the reference operator's summation order)
struct ResidEpi {
  static constexpr int NS = 0, NE = 1;
  static constexpr bool PREFETCH = true, RAW = false;
  static constexpr int WGCU = 1;
  double* __restrict__ res;
  const double* __restrict__ b;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ const double* src(int) const { return b; }
  template <int V>
  __device__ __forceinline__ void put(RowIx idx, const double (&c)[V], const double (&w)[V],
                                      double (&op)[1][V], double*, int nt) const {
    double o[V];
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = op[0][e] - w[e];
    store_row<V>(res, idx, o, nt);
    (void)c;
  }
};

// The Jacobi-type level smoothers of the multigrid (-mg_levels_pc_type jacobi under richardson or
// chebyshev, pb_mg.hip): one smoothing step and its residual in one pass. The field is
//   y_new = omega ((y - yp) + scale (dinv r)) + yp,
// formed on load from up to three raw arrays, every operation rounded in the order of cheb_step,
// poly_second_step and poly_start_step (pb_device.hpp; poly_value in pb_mg.hip calls the same).
// scale, omega and dinv = 1 / cc are host-known constants passed by value: no state prologue, no
// mean shift, no sums.
//   PolyLoad<3>: y, yp, r  (Chebyshev step i >= 2; 48 B/DoF with b and the two stores)
//   PolyLoad<2>: y, r      (yp = 0 or Richardson: y - 0 and + 0 are exact, so the same bits)
//   PolyLoad<1>: b         (the zero start, y = yp = 0 and r = b: neither is read; PolyEpi<true>
//                           takes b for the residual from the z-queue, 24 B/DoF)
// PolyEpi stores the centre value y_new and r_new = b - A y_new (reference summation order) to
// other buffers than the loaders read: neighbouring waves still read y, yp, r around this point.
template <int N>
struct PolyLoad {
  static constexpr int NR = N;
  static constexpr bool GHOST_RAW = true;
  const double* __restrict__ a0;  // N = 1: b; else y
  const double* __restrict__ a1;  // N = 2: r; N = 3: yp
  const double* __restrict__ a2;  // N = 3: r
  double scale, omega, dinv;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ const double* src(int a) const {
    return a == 0 ? a0 : (a == 1 ? a1 : a2);
  }
  __device__ __forceinline__ double value(const double* raw) const {
    if constexpr (N == 1) return poly_start_step(raw[0], dinv, scale, omega);
    else if constexpr (N == 2) return poly_second_step(raw[0], raw[1], dinv, scale, omega);
    else return cheb_step<false>(raw[0], raw[1], raw[2], dinv, 0.0, scale, omega);
  }
};
template <bool QB>
struct PolyEpi {
  static constexpr int NS = 0, NE = 1;
  static constexpr bool RAW = false;
  static constexpr int WGCU = 1;
  static constexpr bool CAP = true, WIDE8 = true;
  static constexpr bool PREFETCH = true;
  // QB (PolyLoad<1>): operand b is the centre plane's raw queue value
  static constexpr int qop(int) { return QB ? 0 : -1; }
  double* __restrict__ y_out;
  double* __restrict__ r_out;
  const double* __restrict__ b;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ const double* src(int) const { return b; }
  template <int V>
  __device__ __forceinline__ void put(RowIx idx, const double (&c)[V], const double (&w)[V],
                                      double (&op)[1][V], double*, int nt) const {
    double rv[V];
#pragma unroll
    for (int e = 0; e < V; ++e) rv[e] = op[0][e] - w[e];
    store_row<V>(r_out, idx, rv, nt);
    store_row<V>(y_out, idx, c, nt);
  }
};

int launch_mg_sor(pb_grid* g, const Star& s, double* x, const double* b, const StencilPlanes& gp,
                  double omega, int color, int first, const int* skip, const CgState* sums_st,
                  int* nparts) {
  ScopedTimer tm(g->ctx, "mg_sor");
  if (sums_st) {  // partial sums -> ctx->d_partials[0 .. nparts*4)
    SorHalfT<true> ep{x, b, s.cx, s.cy, s.cz, 1.0 / s.cc, omega, color, 0, sums_st, 0.0};
    return launch_any(g, s, PlainLoad{x}, gp, ep, Launch{skip}.sums(0, nparts));
  }
  SorHalf ep{x, b, s.cx, s.cy, s.cz, 1.0 / s.cc, omega, first ? 1 : color, first, nullptr, 0.0};
  Launch lc{skip};
  if (first) {  // measured: the zero-start sweep prefers 3 workgroups per CU, the others 1
    lc.wgcu = 3;
    return launch_any(g, s, Red0Load{b, 1.0 / s.cc, omega}, gp, ep, lc);
  }
  return launch_any(g, s, PlainLoad{x}, gp, ep, lc);
}

int launch_mg_residual(pb_grid* g, const Star& s, const double* x, const double* b,
                       const StencilPlanes& gp, double* res, const int* skip) {
  ScopedTimer tm(g->ctx, "mg_residual");
  return launch_any(g, s, PlainLoad{x}, gp, ResidEpi{res, b}, Launch{skip});
}

int launch_mg_poly(pb_grid* g, const Star& s, const double* y, const double* yp, const double* r,
                   const double* b, double scale, double omega, double* y_out, double* r_out,
                   const int* skip) {
  ScopedTimer tm(g->ctx, "mg_poly");
  if (g->ctx->split)  // the update-on-load form reads y, yp and r on the wrap planes in place
    return set_error(PB_ERR_STATE, "launch_mg_poly on a decomposed grid");
  const StencilPlanes gp{nullptr, nullptr, true};
  const double dinv = 1.0 / s.cc;
  if (!y)
    return launch_any(g, s, PolyLoad<1>{b, nullptr, nullptr, scale, omega, dinv}, gp,
                      PolyEpi<true>{y_out, r_out, b}, Launch{skip});
  if (!yp)
    return launch_any(g, s, PolyLoad<2>{y, r, nullptr, scale, omega, dinv}, gp,
                      PolyEpi<false>{y_out, r_out, b}, Launch{skip});
  return launch_any(g, s, PolyLoad<3>{y, yp, r, scale, omega, dinv}, gp,
                    PolyEpi<false>{y_out, r_out, b}, Launch{skip});
}

}  // namespace pb
