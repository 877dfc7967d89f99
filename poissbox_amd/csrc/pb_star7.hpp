// pb_star7.hpp -- the 7-point periodic Laplacian engine for gfx950 (MI355X): the register-queue
// z-march every 7-point pass of the library runs on (star7_kernel), its launch geometry and launch
// path (make_geo, Launch, for_tile_shape, launch_any), and the same tiles run from stored fields
// (tiled_epi_kernel, launch_tiled). A pass is a (Load, Epi) pair: the loader forms the field on
// load, the epilogue consumes the centre value and the Laplacian. The pairs live with their
// solvers (pb_stencil.hip: the operator apply; pb_cg_passes.hip, pb_ksp_stationary.hip,
// pb_ksp_fgmres.hip, pb_ksp_pipecg.hip, pb_mg_engine.hip); the engine reaches a solver's state
// only through them. DESIGN.md §3.1 says what a new pass has to provide.
//
// Replaces the reference hot loop src/poissbox.f90:112-119 (compute_lapl_pointwise ->
// evaluate_laplacian_pointwise, :128-148) and the PETSc KSPSolve_CG vector kernels around it
// (SURVEY.md Appendix A).
//
// Work decomposition (HBM-bound, AI ~ 0.8 flop/B, MFMA unused):
//   * a wave owns an x-segment of 64*V points (V = 2 -> one 16-B load per lane, 1 KiB per
//     wave-instruction) of TY consecutive y-rows and marches in z over a chunk of planes, keeping
//     planes k-1, k, k+1 of its rows in registers (each plane is read from HBM once per chunk);
//   * software pipeline: while plane k is computed, plane k+2 of the z-queue and the halo rows,
//     segment edges and epilogue operands (r, x, p_prev in CG pass B; non-temporal loads, they
//     are read once) of plane k+1 are in flight -- the grid is one resident round of 1-3
//     workgroups per CU (Epi::WGCU), so registers, not occupancy, buy the latency hiding;
//   * each chunk is marched upwards or downwards (Geo::rev): consecutive kernels start on the
//     planes their predecessor touched last, still in the Infinity Cache;
//   * x-neighbours come from the neighbouring lane (DPP wave shift); the two segment-end values
//     of all TY rows come from ONE masked load, broadcast with readlane; y-neighbours come from
//     the wave's own rows, the tile's top/bottom rows from the neighbouring tile (L2 hit: tiles
//     are remapped so neighbours share an XCD);
//   * z ghosts (periodic wrap or the neighbouring rank's plane) are read through plane pointers
//     chosen per plane, or (Geo::wrap, one rank) as the wrap planes of the raw input arrays, so no
//     ghost copy is made on one rank.
// Summation order per point matches the reference dot product with its zero terms dropped:
// z-, y-, x-, centre, x+, y+, z+ (built with -ffp-contract=off => bit-identical to the oracle).
#pragma once

#include <algorithm>
#include <type_traits>

#include "pb_cg_device.hpp"

namespace pb {

struct Geo {
  int nx, ny, nzl;
  int64_t plane;
  int nsegx, ntile, nchunk, kc, ty;
  int k_lo, k_hi, kstride;  // chunk c covers planes [k_lo + c*kstride, min(+kc, k_hi))
  int remap;  // XCD-aware block remap on/off (PB_XCD_REMAP, default on)
  int nt;     // non-temporal output stores (PB_STENCIL_NT, default on)
  int rev;    // march each chunk downwards (k from the top plane to the bottom one)
  int k0;     // global index of local plane 0 (red-black colouring)
  int wrap;   // planes -1 / nzl are the periodic wrap of the raw arrays (StencilPlanes::wrap)
};

// ---------------------------------------------------------------------------------------------
// Loaders: NR raw arrays per point, combined into the field value by value().
// ---------------------------------------------------------------------------------------------
struct PlainLoad {
  static constexpr int NR = 1;
  static constexpr bool GHOST_RAW = false;  // ghost planes hold raw values to transform
  const double* __restrict__ x;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ const double* src(int) const { return x; }
  __device__ __forceinline__ double value(const double* raw) const { return raw[0]; }
};

// ---------------------------------------------------------------------------------------------
// Epilogues: NE operand arrays prefetched one plane ahead; put() consumes centre value c,
// Laplacian w and the operands at owned index idx.
// ---------------------------------------------------------------------------------------------
// Optional member of an epilogue: Op<E> names it as a std::bool_constant; where E has no such
// member the trait is false
template <template <class> class Op, class E, class = void>
struct OptTrait {
  static constexpr bool v = false;
};
template <template <class> class Op, class E>
struct OptTrait<Op, E, std::void_t<Op<E>>> {
  static constexpr bool v = Op<E>::value;
};
// Epi::CAP: keep at most WGCU workgroups resident per CU (launch_t)
template <class E>
using cap_member = std::bool_constant<E::CAP>;
template <class E>
using CapOf = OptTrait<cap_member, E>;
// Epi::TALL: on planes of >= 512^2 points the epilogue runs 8 rows per wave with one workgroup per
// CU (at 512^3: matvec 0.402 -> 0.386 ms, pass A 0.616 -> 0.586 ms; the pass B variants are slower
// that way and keep 4 rows, profiles/r01/tune_ty8.txt)
template <class E>
using tall_member = std::bool_constant<E::TALL>;
template <class E>
using TallOf = OptTrait<tall_member, E>;
// Epi::WIDE8: 8 rows per wave when 4-row tiles would leave more columns than WGCU workgroups per
// CU (planes 1024 or more points wide): the CG passes then run one column per CU as at 512^3.
// 1024x1024x128: pass A 0.412 -> 0.389 ms, pass B 0.759 -> 0.720 ms, iteration 1.39 -> 1.33 ms,
// the 512^3 rate; at 512^3 itself 4-row tiles stay faster (profiles/r04/shapes_r4b.txt)
template <class E>
using wide8_member = std::bool_constant<E::WIDE8>;
template <class E>
using Wide8Of = OptTrait<wide8_member, E>;
// Epi::qop(a): operand a is raw z-queue array qop(a) of the centre plane (-1: loaded)
template <class E>
using qop_member = std::bool_constant<sizeof(E::qop(0)) != 0>;
template <class E>
using HasQop = OptTrait<qop_member, E>;
template <class E>
__device__ __forceinline__ constexpr int qop_of(int a) {
  if constexpr (HasQop<E>::v) return E::qop(a);
  else return -1;
}

// Load / Epi structs that read CG scalars have prepare_from(state): fed the register copy
template <class T>
__device__ __forceinline__ auto prepare_state(T& t, const CgState& s, int)
    -> decltype(t.prepare_from(s), void()) {
  t.prepare_from(s);
}
template <class T>
__device__ __forceinline__ void prepare_state(T& t, const CgState&, long) {
  t.prepare();
}

// ---------------------------------------------------------------------------------------------
// The stencil engine
// ---------------------------------------------------------------------------------------------
template <int V, int TY, class Load, class Epi>
__global__ __launch_bounds__(kThreads) void star7_kernel(Geo g, double cx, double cy, double cz,
                                                         double cc, Load ld0,
                                                         const double* __restrict__ ghost_lo,
                                                         const double* __restrict__ ghost_hi,
                                                         Epi ep0, double* parts,
                                                         const int* __restrict__ skip, Fold fold) {
  Load ld = ld0;
  Epi ep = ep0;
  if (!fold.stage) {
    if (skip && *skip) return;  // device-side convergence flag (uniform)
    ld.prepare();
    ep.prepare();
  }
  // folded finalize: run after the first planes' loads are issued (they need no CG scalar), so
  // the partial-sum loads and the plane loads are in flight together
  auto do_fold = [&]() -> bool {
    CgState sst;  // register copy
    fold_prologue(fold, sst);
    if (sst.done) return false;  // uniform: every wave computed the same state
    prepare_state(ld, sst, 0);
    prepare_state(ep, sst, 0);
    return true;
  };
  constexpr int NS = Epi::NS, NR = Load::NR;
  constexpr int NE = Epi::NE > 0 ? Epi::NE : 1;
  double acc[NS > 0 ? NS : 1];
#pragma unroll
  for (int s = 0; s < (NS > 0 ? NS : 1); ++s) acc[s] = 0.0;

  // wave index as a scalar: row addresses are wave-uniform (SGPR base + one lane offset, RowIx)
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // XCD-aware remap (speed only): the dispatcher deals blocks round-robin over the 8 XCDs, so
  // give each XCD a contiguous range of logical tiles -- y/x-neighbouring tiles then share the
  // XCD's L2 and their halo rows hit there. Bijective for any grid size.
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
  const int ic = active ? i0 : 0;  // clamp addresses of idle lanes
  // x-edges: lane 0 needs x[seg0-1]; the last active lane needs x[seg_end] (periodic wrap).
  // One masked load per plane and array fetches them for all TY rows: lane t < TY the left edge
  // of row t, lane 32 + t the right edge; they are broadcast with readlane.
  const int seg0 = seg * 64 * V;
  const int seg_end = min(seg0 + 64 * V, nx);
  const bool needL = lane == 0;
  const bool needR = active && (lane == 63 || i0 + V >= nx);
  const int edge_row = lane < 32 ? lane : lane - 32;
  const bool edge_lane = edge_row < TY;
  const int edge_i = lane < 32 ? (seg0 == 0 ? nx - 1 : seg0 - 1) : (seg_end >= nx ? 0 : seg_end);
  const int64_t edge_off = (int64_t)(j0 + (edge_lane ? edge_row : 0)) * nx + edge_i;
  const unsigned boff = (unsigned)ic * 8u;  // lane byte offset inside a row
  const int64_t row_dn = (int64_t)(j0 == 0 ? g.ny - 1 : j0 - 1) * nx;
  const int64_t row_up = (int64_t)((j0 + TY >= g.ny) ? 0 : j0 + TY) * nx;
  auto rix = [&](int64_t row) { return RowIx{row, boff}; };
  if (fold.stage && !wave_on && !do_fold()) return;

  if (wave_on) {
    // combined z-queue (planes k-1, k, k+1) and raw prefetch of plane k+2
    double q0[TY][V], q1[TY][V], q2[TY][V];
    double zr[NR][TY][V];
    bool zr_ghost = false;
    // plane-k operands (combined) and their plane-(k+1) prefetch (raw)
    double hdn[V], hup[V], edge = 0.0;
    double hdn_r[NR][V], hup_r[NR][V], edge_r[NR];
    double opc[TY][NE][V], opn[Epi::PREFETCH ? TY : 1][NE][V];

    // Every load below is issued unconditionally (ghost planes by a uniform pointer select, the
    // chunk's last step re-loading valid planes): no branch around a load, so the compiler keeps
    // the prefetch registers stable instead of copying them at control-flow joins -- such copies
    // must wait for the loads and serialised the software pipeline (pass A ran ~10 % slower).
    // raw rows of plane kk in [-1, nzl] -> dst (ghost: the plane is a ghost buffer)
    auto issue_rows = [&](int kk, double (&dst)[NR][TY][V], bool& ghost) {
      if (g.wrap) kk = kk < 0 ? kk + g.nzl : (kk >= g.nzl ? kk - g.nzl : kk);
      ghost = kk < 0 || kk >= g.nzl;
      const double* gp = kk < 0 ? ghost_lo : ghost_hi;
      const int64_t base = ghost ? 0 : (int64_t)kk * g.plane;
#pragma unroll
      for (int a = 0; a < NR; ++a) {
        const double* src = ghost ? gp : ld.src(a);
#pragma unroll
        for (int t = 0; t < TY; ++t) load_row<V>(src, rix(base + (int64_t)(j0 + t) * nx), dst[a][t]);
      }
    };
    auto take_rows = [&](const double (&src)[NR][TY][V], bool ghost, double (&q)[TY][V]) {
#pragma unroll
      for (int t = 0; t < TY; ++t)
#pragma unroll
        for (int e = 0; e < V; ++e) {
          double raw[NR];
#pragma unroll
          for (int a = 0; a < NR; ++a) raw[a] = src[a][t][e];
          q[t][e] = (ghost && !Load::GHOST_RAW) ? src[0][t][e] : ld.value(raw);
        }
    };
    auto issue_zrow = [&](int kk) { issue_rows(kk, zr, zr_ghost); };
    auto take_zrow = [&](double (&q)[TY][V]) { take_rows(zr, zr_ghost, q); };
    auto issue_plane_ops = [&](int kk) {  // halo rows, edges, epilogue operands of own plane kk
      const int64_t base = (int64_t)kk * g.plane;
#pragma unroll
      for (int a = 0; a < NR; ++a) {
#ifdef PB_ABLATE_HALO  // timing experiments only (wrong results): y-halo rows from own rows
        load_row<V>(ld.src(a), rix(base + (int64_t)j0 * nx), hdn_r[a]);
        load_row<V>(ld.src(a), rix(base + (int64_t)(j0 + TY - 1) * nx), hup_r[a]);
#else
        load_row<V>(ld.src(a), rix(base + row_dn), hdn_r[a]);
        load_row<V>(ld.src(a), rix(base + row_up), hup_r[a]);
#endif
        edge_r[a] = 0.0;
#ifndef PB_ABLATE_EDGES  // timing experiments only (wrong results): no segment-edge loads
        edge_r[a] = ld.src(a)[base + edge_off];  // (all lanes: valid address, only edge lanes read)
#endif
      }
      if constexpr (Epi::NE > 0 && Epi::PREFETCH) {
#pragma unroll
        for (int t = 0; t < TY; ++t)
#pragma unroll
          for (int a = 0; a < Epi::NE; ++a)
            if (qop_of<Epi>(a) < 0)
              load_row_nt<V>(ep.src(a), rix(base + (int64_t)(j0 + t) * nx), opn[t][a]);
      }
    };
    // operands that are raw queue values of a plane (Epi::qop): copied, not loaded
    auto take_queue_ops = [&](const double (&raw)[NR][TY][V]) {
      if constexpr (Epi::NE > 0 && Epi::PREFETCH && HasQop<Epi>::v) {
#pragma unroll
        for (int t = 0; t < TY; ++t)
#pragma unroll
          for (int a = 0; a < Epi::NE; ++a)
            if (qop_of<Epi>(a) >= 0)
#pragma unroll
              for (int e = 0; e < V; ++e) opn[t][a][e] = raw[qop_of<Epi>(a)][t][e];
      }
    };
    auto issue_ops_now = [&](int kk) {  // operands without prefetch: plane kk straight to opc
      if constexpr (Epi::NE > 0 && !Epi::PREFETCH) {
        const int64_t base = (int64_t)kk * g.plane;
#pragma unroll
        for (int t = 0; t < TY; ++t)
#pragma unroll
          for (int a = 0; a < Epi::NE; ++a)
            load_row_nt<V>(ep.src(a), rix(base + (int64_t)(j0 + t) * nx), opc[t][a]);
      }
    };
    auto take_plane_ops = [&]() {
#pragma unroll
      for (int e = 0; e < V; ++e) {
        double rd[NR], ru[NR];
#pragma unroll
        for (int a = 0; a < NR; ++a) {
          rd[a] = hdn_r[a][e];
          ru[a] = hup_r[a][e];
        }
        hdn[e] = ld.value(rd);
        hup[e] = ld.value(ru);
      }
      edge = ld.value(edge_r);
      if constexpr (Epi::NE > 0 && Epi::PREFETCH) {
#pragma unroll
        for (int t = 0; t < TY; ++t)
#pragma unroll
          for (int a = 0; a < Epi::NE; ++a)
#pragma unroll
            for (int e = 0; e < V; ++e) opc[t][a][e] = opn[t][a][e];
      }
    };

    // prologue: planes kf-dir, kf combined; raw plane kf+dir and plane kf's operands in flight.
    // Marching downwards (g.rev) lets a kernel start on the planes its predecessor touched last
    // (still in the 256 MiB Infinity Cache); per-point arithmetic is unchanged (zm/zp swap).
    const int dir = g.rev ? -1 : 1;
    const int kf = g.rev ? ke - 1 : kb;
    const int nk = ke - kb;
    // The first planes' loads go out together (one wait instead of one per plane; the
    // prologue is ~10 % of a 32-plane chunk): one array through the queue -- planes kf-dir, kf,
    // kf+dir and plane kf's operands all in flight; two -- kf-dir and kf, then the rest.
    {
      double r0[NR][TY][V], r1[NR][TY][V];
      bool g0 = false, g1 = false;
      issue_rows(kf - dir, r0, g0);
      issue_rows(kf, r1, g1);
      if constexpr (NR == 1) {
        issue_plane_ops(kf);
        issue_zrow(kf + dir);
      }
      if (fold.stage && !do_fold()) return;
      take_rows(r0, g0, q0);
      take_rows(r1, g1, q1);
      take_queue_ops(r1);  // plane kf (owned, never a ghost)
      if constexpr (NR != 1) {
        issue_plane_ops(kf);
        issue_zrow(kf + dir);
      }
    }
    for (int m = 0; m < nk; ++m) {
      const int k = kf + m * dir;
      take_zrow(q2);                    // plane k+dir (in flight since the previous step)
      take_plane_ops();                 // halo/edges/operands of plane k
      take_queue_ops(zr);               // queue-sourced operands of plane k+dir
      issue_ops_now(k);
      issue_zrow(m + 2 <= nk ? k + 2 * dir : k + dir);  // (last step: a valid plane, unused)
      issue_plane_ops(m + 1 < nk ? k + dir : k);
      const int64_t base = (int64_t)k * g.plane;
#pragma unroll
      for (int t = 0; t < TY; ++t) {
        const double eL = readlane_d(edge, t);
        const double eR = readlane_d(edge, 32 + t);
        const double fromL = dpp_from_lower(q1[t][V - 1]);
        const double fromR = dpp_from_upper(q1[t][0]);
        const double xl0 = needL ? eL : fromL;
        const double xrl = needR ? eR : fromR;
        if constexpr (Epi::RAW) {  // the epilogue combines the 7 values itself
          double nzm[V], nym[V], nxm[V], nxp[V], nyp[V], nzp[V];
#pragma unroll
          for (int e = 0; e < V; ++e) {
            nxm[e] = e == 0 ? xl0 : q1[t][e - 1];
            nxp[e] = e == V - 1 ? xrl : q1[t][e + 1];
            nym[e] = t == 0 ? hdn[e] : q1[t - 1][e];
            nyp[e] = t == TY - 1 ? hup[e] : q1[t + 1][e];
            nzm[e] = g.rev ? q2[t][e] : q0[t][e];
            nzp[e] = g.rev ? q0[t][e] : q2[t][e];
          }
          if (active)
            ep.template put_raw<V>(rix(base + (int64_t)(j0 + t) * nx), i0 + j0 + t + g.k0 + k,
                                   nzm, nym, nxm, q1[t], nxp, nyp, nzp, opc[t], acc, g.nt);
        } else {
          double w[V];
#pragma unroll
          for (int e = 0; e < V; ++e) {
            const double xm = e == 0 ? xl0 : q1[t][e - 1];
            const double xp = e == V - 1 ? xrl : q1[t][e + 1];
            const double ym = t == 0 ? hdn[e] : q1[t - 1][e];
            const double yp = t == TY - 1 ? hup[e] : q1[t + 1][e];
            const double zm = g.rev ? q2[t][e] : q0[t][e];
            const double zp = g.rev ? q0[t][e] : q2[t][e];
            double s = cz * zm;
            s = s + cy * ym;
            s = s + cx * xm;
            s = s + cc * q1[t][e];
            s = s + cx * xp;
            s = s + cy * yp;
            s = s + cz * zp;
            w[e] = s;
          }
          if (active)
            ep.template put<V>(rix(base + (int64_t)(j0 + t) * nx), q1[t], w, opc[t], acc, g.nt);
        }
      }
#pragma unroll
      for (int t = 0; t < TY; ++t)
#pragma unroll
        for (int e = 0; e < V; ++e) {
          q0[t][e] = q1[t][e];
          q1[t][e] = q2[t][e];
        }
    }
  }
  block_partials<NS>(acc, parts);
}

// ---------------------------------------------------------------------------------------------
// Launch configuration
// ---------------------------------------------------------------------------------------------
// Plane sets: PLANES_ALL = [0, nzl); PLANES_INTERIOR = [1, nzl-1) (no ghost plane is read);
// PLANES_BOUNDARY = {0, nzl-1} (the two planes that read ghosts) -- the split lets the halo
// exchange of a multi-rank step overlap the interior.
static Geo make_geo(pb_grid* g, int V, int TY, int mode, int rev, int wgcu, int skew) {
  Geo geo;
  geo.rev = rev;
  geo.k0 = (int)g->k0;
  geo.wrap = 0;
  geo.nx = (int)g->n[0];
  geo.ny = (int)g->n[1];
  geo.nzl = (int)g->nzl;
  geo.plane = g->plane;
  geo.ty = TY;
  geo.remap = 1;  // XCD-aware block remap
  geo.nt = 1;     // non-temporal output stores
  geo.nsegx = (geo.nx + 64 * V - 1) / (64 * V);
  geo.ntile = (geo.ny + kWaves * TY - 1) / (kWaves * TY);
  if (mode == PLANES_BOUNDARY) {
    geo.k_lo = 0;
    geo.k_hi = geo.nzl;
    geo.kc = 1;
    geo.kstride = geo.nzl - 1;
    geo.nchunk = 2;
    return geo;
  }
  geo.k_lo = mode == PLANES_INTERIOR ? 1 : 0;
  geo.k_hi = mode == PLANES_INTERIOR ? geo.nzl - 1 : geo.nzl;
  const int nk = geo.k_hi - geo.k_lo;
  const int columns = geo.nsegx * geo.ntile;
  // wgcu (the epilogue's WGCU) workgroups per CU: long z-chunks, few chunk-boundary re-reads.
  // Measured at 512^3: 3 per CU for the matvec and pass A (768 blocks beat 512 even where the
  // registers allow only 2 resident), 1 per CU for pass B
  int target = wgcu * g->ctx->num_cus;
  int nchunk = (target + columns - 1) / columns;
  // z-chunks shorter than 64 planes re-read too many boundary planes (2 per
  // chunk): use fewer, longer chunks, but keep at least one workgroup per CU (256^3: 8 chunks of
  // 32 planes instead of 24 of 11, measured 8-15 % faster)
  const int kcmin = 64;
  if (nk / nchunk < kcmin) {
    const int floor_cu = (g->ctx->num_cus + columns - 1) / columns;
    nchunk = std::max(nk / kcmin, floor_cu);
  }
  if (nchunk > nk) nchunk = nk;
  if (nchunk < 1) nchunk = 1;
  geo.kc = (nk + nchunk - 1) / nchunk;
  // chunk skew (in 64ths of a chunk): longer chunks and a shorter last one, so that the planes
  // the chunks march through together are not a power-of-two number of planes apart. The
  // standalone matvec's four 128-plane chunks at 512^3 ran 0.37-0.42 ms depending on where its x
  // and y sat (pairs of buffers: one slow, one fast group); chunks of 136 planes ran 0.36-0.38
  // over the same pairs (profiles/r06/placement/). The CG passes' two 256-plane chunks gained
  // nothing from it (skew 2: within noise, 4 / 8: slower) and keep 0. Only for chunks at least
  // 128 MiB of planes apart: 256^3's matvec (eight 32-plane chunks, 16 MiB apart) ran 0.0439
  // against 0.0414 ms with the skew (profiles/r06/placement/cgcfg256.jsonl)
  if (nchunk > 1 && skew > 0 && (int64_t)geo.kc * g->plane * 8 >= ((int64_t)128 << 20)) {
    const int kc = geo.kc + std::max(1, geo.kc * skew / 64);
    if ((int64_t)kc * (nchunk - 1) < nk) geo.kc = kc;
  }
  geo.kstride = geo.kc;
  geo.nchunk = (nk + geo.kc - 1) / geo.kc;
  return geo;
}

static int pick_ty(int ny) {
  if (ny % 4 == 0) return 4;
  if (ny % 2 == 0) return 2;
  return 1;
}

// What a launch sets beside the pass itself; a caller names only what differs from the default
struct Launch {
  const int* skip = nullptr;  // device-side convergence flag: the kernel exits at entry when set
  int mode = PLANES_ALL;
  int part_off = 0;        // first block of the partial sums in ctx->d_partials (blocks of Epi::NS)
  int* nb_out = nullptr;   // the number of blocks launched (= partial sums written)
  int rev = 0;             // march each chunk downwards
  int wgcu = 0;            // workgroups per CU the grid is sized for (0: Epi::WGCU)
  Fold fold = {};          // a finalize stage run in the kernel's prologue
  int64_t part_end = 0;    // the end of the caller's partial-sum region in blocks (0: the buffer's)
  Launch& sums(int off, int* nb, int64_t end = 0) {
    part_off = off;
    nb_out = nb;
    part_end = end;
    return *this;
  }
};

// The tile shape of a launch, chosen once for the engine and for launch_tiled: V points per lane
// by nx's parity, TY rows per wave by ny's divisibility, 8-row tiles for the epilogues with the
// WIDE8 / TALL traits (above). f(Tile<V, TY>{}, wgcu) launches; wgcu as given, or the TALL
// promotion's one workgroup per CU.
template <int V_, int TY_>
struct Tile {
  static constexpr int V = V_, TY = TY_;
};
template <class Epi, class F>
static int for_tile_shape(const pb_grid* g, int wgcu, F f) {
  const bool vec2 = (g->n[0] % 2) == 0;
  const int ty = pick_ty((int)g->n[1]);
  if constexpr (Wide8Of<Epi>::v) {
    const int64_t cols4 = ((g->n[0] + 127) / 128) * ((g->n[1] + kWaves * 4 - 1) / (kWaves * 4));
    const int w = wgcu > 0 ? wgcu : Epi::WGCU;
    if (vec2 && ty == 4 && g->n[1] % 8 == 0 && cols4 > (int64_t)w * g->ctx->num_cus)
      return f(Tile<2, 8>{}, wgcu);
  }
  if constexpr (TallOf<Epi>::v) {
    if (vec2 && ty == 4 && g->n[1] % 8 == 0 && g->plane >= 512 * 512 &&
        tune("stencil_tall", 1) != 0)
      return f(Tile<2, 8>{}, wgcu > 0 ? wgcu : 1);
  }
  if (vec2) {
    switch (ty) {
      case 4: return f(Tile<2, 4>{}, wgcu);
      case 2: return f(Tile<2, 2>{}, wgcu);
      default: return f(Tile<2, 1>{}, wgcu);
    }
  }
  switch (ty) {
    case 4: return f(Tile<1, 4>{}, wgcu);
    case 2: return f(Tile<1, 2>{}, wgcu);
    default: return f(Tile<1, 1>{}, wgcu);
  }
}

constexpr size_t kLdsPerCu = 160 * 1024;
struct StoreY;  // the operator apply's epilogue (pb_stencil.hip): its A/B tunings are read below

template <int V, int TY, class Load, class Epi>
static int launch_t(pb_grid* g, const Star& s, const Load& ld, const StencilPlanes& gp,
                    const Epi& ep, const Launch& lc, int wgcu) {
  Geo geo = make_geo(g, V, TY, lc.mode, lc.rev, wgcu > 0 ? wgcu : Epi::WGCU,
                     std::is_same_v<Epi, StoreY> ? tune("stencil_kc_skew", 4)
                                                 : tune("engine_kc_skew", 0));
  geo.wrap = gp.wrap && !g->ctx->split ? 1 : 0;
  if constexpr (std::is_same_v<Epi, StoreY>) {  // (A/B runs)
    geo.nt = tune("stencil_nt", 1);
    const int kc = tune("stencil_kc", 0);
    if (kc > 0 && lc.mode != PLANES_BOUNDARY) {
      const int nk = geo.k_hi - geo.k_lo;
      geo.kc = std::min(kc, nk);
      geo.kstride = geo.kc;
      geo.nchunk = (nk + geo.kc - 1) / geo.kc;
    }
  }
  const int64_t nblocks = (int64_t)geo.nsegx * geo.ntile * geo.nchunk;
  constexpr int NS = Epi::NS > 0 ? Epi::NS : 1;
  const int64_t end = lc.part_end > 0 ? lc.part_end * NS : g->ctx->partials_cap;
  if ((lc.part_off + nblocks) * NS > std::min(end, g->ctx->partials_cap))
    return set_error(PB_ERR_UNSUPPORTED, "stencil grid of %lld blocks exceeds partials capacity",
                     (long long)nblocks);
  // Residency cap (Epi::CAP, the CG passes): a grid with more columns than the epilogue's WGCU
  // workgroups per CU (planes of 1024^2 points: 512 columns of 4-row tiles, twice the 1-per-CU
  // count) would run two workgroups per CU side by side; an LDS request no kernel uses keeps it at
  // WGCU resident per CU, the rest following as slots free. 1024x1024x128 (config 4's per-GPU
  // slab): pass B 0.847 -> 0.772 ms, iteration 1.47 -> 1.40 ms (profiles/r04/shapes_r4.txt).
  size_t lds = 0;
  if constexpr (CapOf<Epi>::v) {
    const int w = wgcu > 0 ? wgcu : Epi::WGCU;
    if (nblocks > (int64_t)w * g->ctx->num_cus) lds = kLdsPerCu / (size_t)(w + 1) + 4096;
  }
  hipLaunchKernelGGL((star7_kernel<V, TY, Load, Epi>), dim3((unsigned)nblocks), dim3(kThreads),
                     lds, g->ctx->engine_stream ? g->ctx->engine_stream : g->ctx->stream, geo, s.cx,
                     s.cy, s.cz, s.cc, ld, gp.ghost_lo, gp.ghost_hi, ep,
                     g->ctx->d_partials + (int64_t)lc.part_off * NS, lc.skip, lc.fold);
  PB_HIP(hipGetLastError());
  if (lc.nb_out) *lc.nb_out = (int)nblocks;
  return PB_OK;
}

template <class Load, class Epi>
static int launch_any(pb_grid* g, const Star& s, const Load& ld, const StencilPlanes& gp,
                      const Epi& ep, const Launch& lc) {
  return for_tile_shape<Epi>(g, lc.wgcu, [&](auto tile, int wgcu) {
    return launch_t<decltype(tile)::V, decltype(tile)::TY>(g, s, ld, gp, ep, lc, wgcu);
  });
}

// ---------------------------------------------------------------------------------------------
// An engine epilogue run from stored fields: the centre value c and the Laplacian w come from two
// arrays instead of the z-queue, in the engine's tiles, z-chunks and per-lane order of
// accumulation (launch_any's choice of V and TY, make_geo's chunks, block_partials), so the
// partial sums -- and with them everything the next finalize computes -- are the bits of the
// engine pass with the same epilogue. No neighbour is read: any slab, split grids included.
// ---------------------------------------------------------------------------------------------
template <int V, int TY, class Epi>
__global__ __launch_bounds__(kThreads) void tiled_epi_kernel(Geo g, const double* __restrict__ cf,
                                                             const double* __restrict__ wf, Epi ep0,
                                                             double* parts,
                                                             const int* __restrict__ skip) {
  if (skip && *skip) return;
  Epi ep = ep0;
  ep.prepare();
  constexpr int NS = Epi::NS, NE = Epi::NE;
  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0;
  const int lane = threadIdx.x & 63, wid = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int b = xcd_block(g.remap);
  const int seg = b % g.nsegx;
  b /= g.nsegx;
  const int tile = b % g.ntile;
  const int chunk = b / g.ntile;
  const int j0 = (tile * kWaves + wid) * TY;
  const int kb = g.k_lo + chunk * g.kstride;
  const int ke = min(kb + g.kc, g.k_hi);
  const int i0 = seg * 64 * V + lane * V;
  if (i0 < g.nx && j0 < g.ny) {
    const unsigned boff = (unsigned)i0 * 8u;
    for (int k = kb; k < ke; ++k) {
      const int64_t base = (int64_t)k * g.plane;
#pragma unroll
      for (int t = 0; t < TY; ++t) {
        const RowIx ix{base + (int64_t)(j0 + t) * g.nx, boff};
        double c[V], w[V], op[NE][V];
        load_row_nt<V>(cf, ix, c);
        load_row_nt<V>(wf, ix, w);
#pragma unroll
        for (int a = 0; a < NE; ++a) load_row_nt<V>(ep.src(a), ix, op[a]);
        ep.template put<V>(ix, c, w, op, acc, g.nt);
      }
    }
  }
  block_partials<NS>(acc, parts);
}

template <int V, int TY, class Epi>
static int launch_tiled_t(pb_grid* g, const double* cf, const double* wf, const Epi& ep,
                          const int* skip, int* nb_out) {
  Geo geo = make_geo(g, V, TY, PLANES_ALL, 0, Epi::WGCU, tune("engine_kc_skew", 0));
  const int64_t nblocks = (int64_t)geo.nsegx * geo.ntile * geo.nchunk;
  if (nblocks * Epi::NS > g->ctx->partials_cap)
    return set_error(PB_ERR_UNSUPPORTED, "tiled grid of %lld blocks exceeds partials capacity",
                     (long long)nblocks);
  hipLaunchKernelGGL((tiled_epi_kernel<V, TY, Epi>), dim3((unsigned)nblocks), dim3(kThreads), 0,
                     g->ctx->stream, geo, cf, wf, ep, g->ctx->d_partials, skip);
  PB_HIP(hipGetLastError());
  *nb_out = (int)nblocks;
  return PB_OK;
}

// the engine's tile shape (for_tile_shape) for an epilogue without the WIDE8 / TALL traits
template <class Epi>
static int launch_tiled(pb_grid* g, const double* cf, const double* wf, const Epi& ep,
                        const int* skip, int* nb_out) {
  static_assert(!Wide8Of<Epi>::v && !TallOf<Epi>::v, "launch_any would choose 8-row tiles");
  return for_tile_shape<Epi>(g, 0, [&](auto tile, int) {
    return launch_tiled_t<decltype(tile)::V, decltype(tile)::TY>(g, cf, wf, ep, skip, nb_out);
  });
}

}  // namespace pb
