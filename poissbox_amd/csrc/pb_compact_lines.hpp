// pb_compact_lines.hpp -- device pieces of the register-resident compact line solves, shared by
// the factorised Laplacian's passes (pb_compact_lines.hip) and the half-operator passes of grad /
// div / interp (pb_compact_ops.hip): the per-lane explicit RHS, the periodic (alpha, 1, alpha)
// solve, and the LDS tile transpose with its global <-> LDS copies; and the host pieces both
// launch sides share: the list of line lengths (for_line_c), the 16-byte alignment test
// (aligned16) and the tiled passes' launcher (launch_lines_tiled). Include after
// pb_internal.hpp / pb_device.hpp; the arithmetic is written for contraction, so the including
// file sets `#pragma clang fp contract(fast)` first (as this header does for itself).
#pragma once
#include <cmath>
#include <cstdint>
#include <type_traits>

#pragma clang fp contract(fast)

namespace pb {

// The line lengths the register solves are compiled for, n = 64*C: f(integral_constant<int, C>)
// for n's C, PB_ERR_UNSUPPORTED (no error text set) for any other n. The only copy of the list.
template <class F>
static int for_line_c(int64_t n, F&& f) {
  switch (n % 64 ? 0 : n / 64) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    case 4: return f(std::integral_constant<int, 4>{});
    case 6: return f(std::integral_constant<int, 6>{});
    case 8: return f(std::integral_constant<int, 8>{});
    case 12: return f(std::integral_constant<int, 12>{});
    case 16: return f(std::integral_constant<int, 16>{});
  }
  return PB_ERR_UNSUPPORTED;
}

// every pointer on a 16-byte boundary (the 16-byte moves' condition; nullptr counts as aligned)
template <class... P>
static bool aligned16(const P*... p) {
  return ((((uintptr_t)p & 15) == 0) && ...);
}

struct LineOp {
  double a, b, sign;  // explicit 4-point RHS (src/compact_schemes.f90:332-372)
  double mq;          // -q
  double inv_kappa;
  double corr;        // 1 / (1 - G^64) if the scan wraps the whole line, else 1
  double gs[6];       // G^(2^s)
  double pw[16];      // (-q)^(m+1)
  int nsteps;
};

struct LinePass {
  const double* in0;
  const double* in1;
  double* out0;
  double* out1;
  int64_t li, lo, es;  // address of (outer, inner line, element e) = outer*lo + inner*li + e*es
  int ninner, ntiles_inner, nouter, TL, P;
  int ablate;  // tuning only (PB_LINES_ABLATE=1): copy lines through, no solves (the build flag
               // -DPB_LINES_ABLATE_TRAFFIC=1 drops the tiled passes' global loads / stores instead)
  int remap;   // XCD-aware tile order: off (Z pass 0.74-0.78 vs 0.715-0.72 ms with it at 512^3,
               // profiles/r02/ab_remap_compact.jsonl)
  LineOp J, L;
  const int* skip;  // pb_ctx::op_skip (exit at entry once set)
  // CG fusions (CgFuse): Z pass forming p from in0 = z and in1 = p_old (CGP kernels), X pass
  // taking p . w partial sums (DOT kernels)
  double* p_out;
  const CgState* st;
  int first;
  const double* dot_p;
  double* parts;
  // blocked inputs (lo_in > 0): the decomposed Y pass reads the all-to-all receive buffers --
  // outer stride lo_in, element e at (e >> esh_in) * ebs_in + (e & (2^esh_in - 1)) * es
  int64_t lo_in, ebs_in;
  int esh_in;
  // the self block of a blocked input (YSlabPlan::self_direct): block alt_blk of in0 / in1 is read
  // from alt0 / alt1 (the Z pass's y-slab outputs; the all-to-all did not copy it); -1: none
  const double* alt0 = nullptr;
  const double* alt1 = nullptr;
  int alt_blk = -1;
  // half-operator passes (pb_compact_ops.hip): J is the first term's operator, L the second
  // term's / second output's, both applied once at this stagger (-1: cell -> vertex, +1 back)
  int stagger = 0;
};

static LineOp make_line_op(int kind, int C, double h) {
  LineOp o{};
  double alpha;
  if (kind == 0) {  // J: interp (:303-305)
    o.a = 0.75;
    o.b = 1.0 / 20.0;
    o.sign = 1.0;
    alpha = 3.0 / 10.0;
  } else {  // L: grad / div (:188-190)
    o.a = 63.0 / 62.0 / h;
    o.b = 17.0 / 62.0 / (3.0 * h);
    o.sign = -1.0;
    alpha = 9.0 / 62.0;
  }
  const double q = 2.0 * alpha / (1.0 + std::sqrt(1.0 - 4.0 * alpha * alpha));
  o.mq = -q;
  o.inv_kappa = q / alpha;
  double p = 1.0;
  for (int m = 0; m < C; ++m) {
    p *= -q;
    o.pw[m] = p;
  }
  const double G = p;  // (-q)^C
  double g = G;
  int s = 0;
  for (; s < 6; ++s) {
    if (std::fabs(g) < 1e-24) break;
    o.gs[s] = g;
    g = g * g;
  }
  o.nsteps = s;
  o.corr = s == 6 ? 1.0 / (1.0 - g) : 1.0;  // g = G^64 here
  return o;
}

__device__ __forceinline__ double lane_shfl(double v, int src) { return __shfl(v, src & 63, 64); }
// the wave rotations by one lane as DPP moves (VALU, no LDS round trip like __shfl's
// ds_bpermute): lane l <- lane l-1 (lane 0 <- 63: wave_ror:1) / lane l+1 (lane 63 <- 0: wave_rol:1).
// The same values as lane_shfl(v, lane -/+ 1), so the results do not change.
template <int CTRL>
__device__ __forceinline__ double lane_rot(double v) {
  const long long b = __builtin_bit_cast(long long, v);
  const int lo = __builtin_amdgcn_mov_dpp((int)b, CTRL, 0xf, 0xf, false);
  const int hi = __builtin_amdgcn_mov_dpp((int)(b >> 32), CTRL, 0xf, 0xf, false);
  return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned)lo);
}
__device__ __forceinline__ double lane_from_lower(double v) { return lane_rot<0x13C>(v); }
__device__ __forceinline__ double lane_from_upper(double v) { return lane_rot<0x134>(v); }

// d <- explicit RHS of x (stagger -1: cell -> vertex, +1: vertex -> cell), eval_1d_rhs order
template <int C>
__device__ __forceinline__ void line_rhs(const double (&x)[C], double (&d)[C], const LineOp& o,
                                         int stagger, int lane) {
  double xm2, xm1, xp0, xp1;  // x at local offsets -2, -1, C, C+1
  (void)lane;
  xm1 = lane_from_lower(x[C - 1]);
  xp0 = lane_from_upper(x[0]);
  if constexpr (C >= 2) {
    if (stagger < 0) {
      xm2 = lane_from_lower(x[C - 2]);
      xp1 = 0.0;
    } else {
      xp1 = lane_from_upper(x[1]);
      xm2 = 0.0;
    }
  } else {
    if (stagger < 0) {
      xm2 = lane_from_lower(xm1);
      xp1 = 0.0;
    } else {
      xp1 = lane_from_upper(xp0);
      xm2 = 0.0;
    }
  }
  auto at = [&](int o2) -> double {  // o2 is a compile-time constant after unrolling
    if (o2 == -2) return xm2;
    if (o2 == -1) return xm1;
    if (o2 == C) return xp0;
    if (o2 == C + 1) return xp1;
    return x[o2];
  };
  const double a = o.a, b = o.b, s = o.sign;
#pragma unroll
  for (int m = 0; m < C; ++m) {
    if (stagger < 0)
      d[m] = a * (at(m) + s * at(m - 1)) + b * (at(m + 1) + s * at(m - 2));
    else
      d[m] = a * (at(m + 1) + s * at(m)) + b * (at(m + 2) + s * at(m - 1));
  }
}

// d <- (alpha, 1, alpha)^-1 d on the periodic line (64 lanes x C points)
template <int C>
__device__ __forceinline__ void line_solve(double (&d)[C], const LineOp& o, int lane) {
  const double mq = o.mq;
  // causal sweep y_i = d_i - q y_{i-1}
#pragma unroll
  for (int m = 1; m < C; ++m) d[m] = d[m] + mq * d[m - 1];
  double T = d[C - 1];
  // the scan's distance-1 step and the carries as DPP rotations (chains of them for distances 2
  // and 4 measured no faster than ds_bpermute, profiles/r03/compact_dpp_*.jsonl)
  if (o.nsteps > 0) T = T + o.gs[0] * lane_from_lower(T);
  for (int s = 1; s < o.nsteps; ++s) T = T + o.gs[s] * lane_shfl(T, lane - (1 << s));
  T *= o.corr;
  double cin = lane_from_lower(T);
#pragma unroll
  for (int m = 0; m < C; ++m) d[m] = d[m] + o.pw[m] * cin;
  // anti-causal sweep z_i = y_i - q z_{i+1}
#pragma unroll
  for (int m = C - 2; m >= 0; --m) d[m] = d[m] + mq * d[m + 1];
  T = d[0];
  if (o.nsteps > 0) T = T + o.gs[0] * lane_from_upper(T);
  for (int s = 1; s < o.nsteps; ++s) T = T + o.gs[s] * lane_shfl(T, lane + (1 << s));
  T *= o.corr;
  cin = lane_from_upper(T);
#pragma unroll
  for (int m = 0; m < C; ++m) d[m] = (d[m] + o.pw[C - 1 - m] * cin) * o.inv_kappa;
}

// r <- (I+ I-) x  (J or L: cell -> vertex half, then vertex -> cell half)
template <int C>
__device__ __forceinline__ void line_op(const double (&x)[C], double (&r)[C], const LineOp& o,
                                        int lane, int ablate) {
  if (ablate) {
#pragma unroll
    for (int m = 0; m < C; ++m) r[m] = x[m];
    return;
  }
  double t[C];
  line_rhs<C>(x, t, o, -1, lane);
  line_solve<C>(t, o, lane);
  line_rhs<C>(t, r, o, +1, lane);
  line_solve<C>(r, o, lane);
}

// LDS word of (line l, element e): lanes own C consecutive points; chunk pitch odd -> no conflicts
template <int C>
struct Lds {
  static constexpr int CP = (C % 2 == 0) ? C + 1 : C;
  // line pitch (doubles): 64 CP + 1 = 1 mod 16, so the tile copies' 16-lane groups (8 lines x 2
  // elements) hit 16 distinct banks; the r01/r02 pitch 64 CP + 4 put lines 0, 4, 8, 12 on one bank
  // (4-way conflicts on every tile write: 4x the LDS write cycles of the copy, by a bank model)
  static constexpr int LP = 64 * CP + 1;
  __device__ static __forceinline__ int word(int l, int e) { return l * LP + (e / C) * CP + (e % C); }
};

// global <-> LDS tile copies, fully unrolled so every load of the tile is in flight at once.
// LAYOUT 0: lines run across rows (li == 1, coalesced along l); LAYOUT 1: lines contiguous
// (es == 1, li == n). V = 2 moves 16-byte pairs along the contiguous direction (needs an even
// row length); the pair (l, l+1) of LAYOUT 0 sits in two different LDS lines.
typedef double dv2 __attribute__((ext_vector_type(2)));

template <int C, int LAYOUT, int TL, int V>
__device__ __forceinline__ void tile_coord(int f, int& l, int& e) {
  constexpr int n = 64 * C;
  if (LAYOUT == 0) {
    l = (f % (TL / V)) * V;
    e = f / (TL / V);
  } else {
    l = (f * V) / n;
    e = (f * V) % n;
  }
}

template <int C, int LAYOUT, int TL, int V, int NT>
struct TileRegs {
  static constexpr int NF = TL * 64 * C / V;  // pairs (or singles) in the tile
  static constexpr int R = (NF + NT - 1) / NT;
  double v[R][V];
};

// issue every global load of the tile (no wait: the registers are consumed by tile_put later).
// Every load is unconditional, from a valid address (pairs past the tile re-load line 0 / the
// tile's first element; tile_put ignores them): a load under a runtime `if` made the compiler
// wait for each load before issuing the next (s_waitcnt vmcnt(0) ahead of every
// global_load_dwordx4 in the r02 ISA of the persistent Z / Y passes), i.e. one HBM round trip per
// pair instead of the whole tile in flight.
#ifndef PB_LINES_ABLATE_TRAFFIC
#define PB_LINES_ABLATE_TRAFFIC 0  // timing builds only: no global loads / stores in tiled passes
#endif
// BLK: the input is an all-to-all receive buffer in its blocked layout (LinePass::lo_in, esh_in,
// ebs_in; the decomposed Y pass, PASS 4); base is the output layout's
template <bool BLK = false, int C, int LAYOUT, int TL, int V, int NT>
__device__ __forceinline__ void tile_fetch(const LinePass& p, const double* __restrict__ src,
                                           int64_t base, int nl, TileRegs<C, LAYOUT, TL, V, NT>& t) {
  using T = TileRegs<C, LAYOUT, TL, V, NT>;
  if (PB_LINES_ABLATE_TRAFFIC) return;
  int64_t b_in = base;
  if constexpr (BLK) {
    const int64_t outer = base / p.lo;
    b_in = outer * p.lo_in + (base - outer * p.lo);
  }
#pragma unroll
  for (int r = 0; r < T::R; ++r) {
    int l, e;
    const int f = threadIdx.x + NT * r;
    tile_coord<C, LAYOUT, TL, V>(f, l, e);
    const bool ok = (T::NF % NT == 0 || f < T::NF) && l < nl;
    const int lc = ok ? l : 0, ec = ok ? e : 0;  // selects, not a branch around the load
    int64_t eo = (int64_t)ec * p.es;
    const double* s = src;
    if constexpr (BLK) {
      eo = (int64_t)(ec >> p.esh_in) * p.ebs_in + (int64_t)(ec & ((1 << p.esh_in) - 1)) * p.es;
      if ((ec >> p.esh_in) == p.alt_blk) s = src == p.in0 ? p.alt0 : p.alt1;  // (a select)
    }
    const double* a = s + b_in + lc * p.li + eo;
    if (V == 2) {
      const dv2 w = __builtin_nontemporal_load((const dv2*)a);
      t.v[r][0] = w.x;
      t.v[r][V - 1] = w.y;
    } else {
      t.v[r][0] = __builtin_nontemporal_load(a);
    }
  }
}

template <int C, int LAYOUT, int TL, int V, int NT>
__device__ __forceinline__ void tile_put(double* lds, int nl, const TileRegs<C, LAYOUT, TL, V, NT>& t) {
  using T = TileRegs<C, LAYOUT, TL, V, NT>;
  constexpr int dl = LAYOUT == 0 ? 1 : 0, de = LAYOUT == 0 ? 0 : 1;  // step of the pair partner
#pragma unroll
  for (int r = 0; r < T::R; ++r) {
    int l, e;
    const int f = threadIdx.x + NT * r;
    tile_coord<C, LAYOUT, TL, V>(f, l, e);
    if ((T::NF % NT == 0 || f < T::NF) && l < nl) {
      lds[Lds<C>::word(l, e)] = t.v[r][0];
      if (V == 2) lds[Lds<C>::word(l + dl, e + de)] = t.v[r][V - 1];
    }
  }
}

template <int C, int LAYOUT, int TL, int V, int NT>
__device__ __forceinline__ void tile_store(const LinePass& p, double* __restrict__ dst,
                                           const double* lds, int64_t base, int nl) {
  constexpr int NF = TL * 64 * C / V;
  constexpr int R = (NF + NT - 1) / NT;
  constexpr int dl = LAYOUT == 0 ? 1 : 0, de = LAYOUT == 0 ? 0 : 1;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    int l, e;
    const int f = threadIdx.x + NT * r;
    tile_coord<C, LAYOUT, TL, V>(f, l, e);
    if ((NF % NT == 0 || f < NF) && l < nl) {
      double* a = dst + base + l * p.li + e * p.es;
      if (V == 2) {
        dv2 w;
        w.x = lds[Lds<C>::word(l, e)];
        w.y = lds[Lds<C>::word(l + dl, e + de)];
        if (PB_LINES_ABLATE_TRAFFIC) {
          if (w.x == 12345.678) *a = w.y;  // keeps the LDS reads (never true on real data)
          continue;
        }
        __builtin_nontemporal_store(w, (dv2*)a);
      } else {
        __builtin_nontemporal_store(lds[Lds<C>::word(l, e)], a);
      }
    }
  }
}

// CGP: p = (dinv z - mu) + (beta / beta_old) p_old on the tile's pairs (z in `pre`, p_old in
// `pold`), written back into `pre` and stored to p_out at the pairs' own addresses. The products
// and sums round separately, as cg_gen_p_kernel's (built without contraction): bit-identical.
template <int C, int LAYOUT, int TL, int V, int NT>
__device__ __forceinline__ void cg_form_p(const LinePass& p, int64_t base, int nl,
                                          TileRegs<C, LAYOUT, TL, V, NT>& pre,
                                          const TileRegs<C, LAYOUT, TL, V, NT>& pold) {
  using T = TileRegs<C, LAYOUT, TL, V, NT>;
  const CgState* st = p.st;
  const double dinv = st->dinv, shift = -st->mu;
  const double bb = st->it == 0 ? 0.0 : st->beta / st->betaold;
#pragma unroll
  for (int r = 0; r < T::R; ++r) {
    int l, e;
    const int f = threadIdx.x + NT * r;
    tile_coord<C, LAYOUT, TL, V>(f, l, e);
#pragma unroll
    for (int q = 0; q < V; ++q) {
      const double z = __dadd_rn(__dmul_rn(dinv, pre.v[r][q]), shift);
      pre.v[r][q] = p.first ? z : __dadd_rn(z, __dmul_rn(bb, pold.v[r][q]));
    }
    if ((T::NF % NT == 0 || f < T::NF) && l < nl && !PB_LINES_ABLATE_TRAFFIC) {
      dv2 w;
      w.x = pre.v[r][0];
      w.y = pre.v[r][V - 1];
      __builtin_nontemporal_store(w, (dv2*)(p.p_out + base + l * p.li + e * p.es));
    }
  }
}

template <int C>
__device__ __forceinline__ void chunk_read(const double* lds, int l, int lane, double (&x)[C]) {
  const int w0 = l * Lds<C>::LP + lane * Lds<C>::CP;
#pragma unroll
  for (int m = 0; m < C; ++m) x[m] = lds[w0 + m];
}
template <int C>
__device__ __forceinline__ void chunk_write(double* lds, int l, int lane, const double (&x)[C]) {
  const int w0 = l * Lds<C>::LP + lane * Lds<C>::CP;
#pragma unroll
  for (int m = 0; m < C; ++m) lds[w0 + m] = x[m];
}

// K = launch shape: TL lines per tile, NW waves per block (NW divides TL), PF = 1 for persistent
// blocks that fetch the next input tile into registers while the current one is solved and
// stored (HBM reads overlap the line solves and the write-back), PF = 0 for one tile per block.
template <int TL_, int NW_, int PF_>
struct LineCfg {
  static constexpr int TL = TL_, NW = NW_, PF = PF_, NT = 64 * NW_, LPW = TL_ / NW_;
};

// Launch the tiled pass kernel Kern (launch shape K, lines of 64*C points) over p's tiles: the
// dynamic-LDS attribute and the occupancy are taken once per kernel (`occ` is one per
// instantiation, i.e. per Kern); persistent shapes (K::PF) get occupancy x CUs blocks at most,
// the others one block per tile.
template <auto Kern, class K, int C>
static int launch_lines_tiled(pb_ctx* ctx, LinePass& p, int64_t nouter) {
  p.TL = K::TL;
  p.P = Lds<C>::LP;
  p.ntiles_inner = (p.ninner + K::TL - 1) / K::TL;
  p.nouter = (int)nouter;
  const int64_t ntiles = (int64_t)p.ntiles_inner * nouter;
  const size_t lds = (size_t)K::TL * Lds<C>::LP * sizeof(double);
  static int occ = 0;
  if (!occ) {
    PB_HIP(hipFuncSetAttribute((const void*)Kern, hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
    PB_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, Kern, K::NT, lds));
    if (occ < 1) occ = 1;
  }
  int64_t nblocks = K::PF ? (int64_t)occ * ctx->num_cus : ntiles;
  if (nblocks > ntiles) nblocks = ntiles;
  hipLaunchKernelGGL(Kern, dim3((unsigned)nblocks), dim3(K::NT), lds, ctx->stream, p);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

// wave-private LDS strips: order the wave's own LDS writes and reads without a block barrier
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

}  // namespace pb
