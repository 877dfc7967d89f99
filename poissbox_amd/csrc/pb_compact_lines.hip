// pb_compact_lines.hip -- register-resident line solves for the 3-pass compact Laplacian.
//
// Same factorisation as pb_compact_fast.hip (lapl = Lx Jy Jz + Jx Ly Jz + Jx Jy Lz, SURVEY.md
// Appendix D; reference src/compact_schemes.f90:17-37), but each 1-D line of n = 64*C points is
// owned by ONE wave with C consecutive points per lane, so both the explicit RHS and the periodic
// (alpha, 1, alpha) solve run in registers:
//
//   (alpha,1,alpha) = kappa (1 + q S^-1)(1 + q S),  q = 2 alpha / (1 + sqrt(1 - 4 alpha^2)),
//                                                   kappa = alpha / q
// so the solve is a causal first-order recursion y_i = d_i - q y_{i-1} followed by the
// anti-causal z_i = y_i - q z_{i+1}, each periodic. A lane runs its chunk with zero initial state,
// then the chunk-end values are combined across lanes by a cyclic Kogge-Stone scan with
// multiplier G = (-q)^C (truncated once G^(2^s) < 1e-24, or the exact periodic factor
// 1/(1 - G^64) when the scan covers the whole line), and each point is corrected by
// (-q)^(m+1) * carry. Nothing touches LDS except the tile transpose that gives coalesced HBM
// rows for the strided (Y, Z) passes. HBM traffic is the 80 B/DoF of the factorisation.
//
// Line sets: Z pass (lines along k, tile = TL consecutive i at fixed j), Y pass (along j, tile =
// TL consecutive i at fixed k), X pass (along i, tile = TL consecutive contiguous lines).
// The results match the reference to rounding (operation order differs from Thomas + Sherman-
// Morrison in src/tridsol.f90:34-74); the bit-exact reference-order path stays in pb_compact.hip.
#include <algorithm>
#include <cmath>

#include "pb_internal.hpp"
#include "pb_device.hpp"

#pragma clang fp contract(fast)

#include "pb_compact_lines.hpp"

namespace pb {

// PASS 0 (Z): out0 = J in0, out1 = L in0.   PASS 1 (Y): out0 = J in0, out1 = L in0 + J in1.
// PASS 2 (X): out0 = L in0 + J in1.   (launch shapes K: LineCfg, pb_compact_lines.hpp)
// CGP (PASS 0, V = 2): in0 = z, in1 = p_old; the tile's input is p = (dinv z - mu) + beta/
// beta_old p_old (cg_gen_p_kernel's operations, unfused roundings: bit-identical), also stored to
// p_out as it goes into LDS
// PASS_ 4: PASS 1 with its inputs read from the all-to-all receive buffers (tile_fetch BLK)
template <int C, int LAYOUT, int PASS_, class K, int V, bool CGP = false>
__global__ __launch_bounds__(K::NT) void compact_lines_kernel(LinePass p) {
  constexpr bool BLK = PASS_ == 4;
  constexpr int PASS = BLK ? 1 : PASS_;
  static_assert(!CGP || (PASS == 0 && V == 2 && K::PF == 1), "CGP: Z pass, pairs, prefetch");
  if (p.skip && *p.skip) return;
  extern __shared__ __attribute__((aligned(16))) double lds[];
  constexpr int TL = K::TL, LPW = K::LPW, NT = K::NT;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ntiles = p.ntiles_inner * p.nouter;
  auto tile_of = [&](int t, int64_t& base, int& nl) {
    const int outer = t / p.ntiles_inner;
    const int inner0 = (t % p.ntiles_inner) * TL;
    nl = min(TL, p.ninner - inner0);
    base = (int64_t)outer * p.lo + (int64_t)inner0 * p.li;
  };
  int t = xcd_block(p.remap);
  if (t >= ntiles) return;
  double keep[LPW][C];
  TileRegs<C, LAYOUT, TL, V, NT> pold;  // CGP: p_old of the prefetched tile (dead otherwise)
  // one tile: its input registers `pre` go to LDS, then (PF) tile tn's input is fetched into them
  // while this tile is solved and stored
  auto step = [&](int t, TileRegs<C, LAYOUT, TL, V, NT>& pre, int tn) {
    int64_t base, base_n = 0;
    int nl, nl_n = 0;
    tile_of(t, base, nl);
    if (K::PF && tn < ntiles) tile_of(tn, base_n, nl_n);
    __syncthreads();  // previous tile's LDS reads are done
    if (!K::PF) tile_fetch<BLK>(p, p.in0, base, nl, pre);
    if constexpr (CGP) cg_form_p<C, LAYOUT, TL, V, NT>(p, base, nl, pre, pold);
    tile_put(lds, nl, pre);
    __syncthreads();
    if (K::PF) {
      if (PASS == 0 || PASS == 3) {
        if (tn < ntiles) {
          tile_fetch<BLK>(p, p.in0, base_n, nl_n, pre);
          // (the first iteration of a lazy-start solve has no p_old: p = z - mu, 8 B/DoF fewer)
          if constexpr (CGP)
            if (!p.first) tile_fetch<BLK>(p, p.in1, base_n, nl_n, pold);
        }
      } else {
        tile_fetch<BLK>(p, p.in1, base, nl, pre);
      }
    }
#pragma unroll
    for (int j = 0; j < LPW; ++j) {
      const int l = wave * LPW + j;
      if (l >= nl) continue;
      double x[C], r[C];
      chunk_read<C>(lds, l, lane, x);
      if (PASS == 3) {  // batched (alpha, 1, alpha) periodic solve
#pragma unroll
        for (int m = 0; m < C; ++m) r[m] = x[m];
        line_solve<C>(r, p.J, lane);
        chunk_write<C>(lds, l, lane, r);
        continue;  // (per line)
      }
      if (PASS != 2) {
        line_op<C>(x, r, p.J, lane, p.ablate);
        chunk_write<C>(lds, l, lane, r);
      }
      line_op<C>(x, keep[j], p.L, lane, p.ablate);
    }
    __syncthreads();
    if (PASS == 3) {
      tile_store<C, LAYOUT, TL, V, NT>(p, p.out0, lds, base, nl);
      return;
    }
    if (PASS == 0) {
      tile_store<C, LAYOUT, TL, V, NT>(p, p.out0, lds, base, nl);
      __syncthreads();
#pragma unroll
      for (int j = 0; j < LPW; ++j) {
        const int l = wave * LPW + j;
        if (l < nl) chunk_write<C>(lds, l, lane, keep[j]);
      }
      __syncthreads();
      tile_store<C, LAYOUT, TL, V, NT>(p, p.out1, lds, base, nl);
      return;
    }
    if (PASS == 1) {
      tile_store<C, LAYOUT, TL, V, NT>(p, p.out0, lds, base, nl);
      __syncthreads();
    }
    if (!K::PF) tile_fetch<BLK>(p, p.in1, base, nl, pre);
    tile_put(lds, nl, pre);
    __syncthreads();
    if (K::PF && tn < ntiles) tile_fetch<BLK>(p, p.in0, base_n, nl_n, pre);
#pragma unroll
    for (int j = 0; j < LPW; ++j) {
      const int l = wave * LPW + j;
      if (l >= nl) continue;
      double x[C], r[C];
      chunk_read<C>(lds, l, lane, x);
      line_op<C>(x, r, p.J, lane, p.ablate);
#pragma unroll
      for (int m = 0; m < C; ++m) r[m] = keep[j][m] + r[m];
      chunk_write<C>(lds, l, lane, r);
    }
    __syncthreads();
    tile_store<C, LAYOUT, TL, V, NT>(p, PASS == 1 ? p.out1 : p.out0, lds, base, nl);
  };
  if constexpr (K::PF == 2) {  // two tiles' inputs in flight (single-input passes)
    static_assert(PASS == 0 || PASS == 3, "PF = 2: single-input passes only");
    const int G = gridDim.x;
    TileRegs<C, LAYOUT, TL, V, NT> ra, rb;
    int64_t b0;
    int n0;
    tile_of(t, b0, n0);
    tile_fetch<BLK>(p, p.in0, b0, n0, ra);
    if (t + G < ntiles) {
      tile_of(t + G, b0, n0);
      tile_fetch<BLK>(p, p.in0, b0, n0, rb);
    }
    for (; t < ntiles; t += 2 * G) {
      step(t, ra, t + 2 * G);
      if (t + G >= ntiles) break;
      step(t + G, rb, t + 3 * G);
    }
  } else {
    TileRegs<C, LAYOUT, TL, V, NT> pre;
    if (K::PF) {
      int64_t b0;
      int n0;
      tile_of(t, b0, n0);
      tile_fetch<BLK>(p, p.in0, b0, n0, pre);
      if constexpr (CGP)
        if (!p.first) tile_fetch(p, p.in1, b0, n0, pold);
    }
    for (; t < ntiles; t += gridDim.x) step(t, pre, t + gridDim.x);
  }
}

// X pass without block barriers: the lines are contiguous, so each wave owns whole lines and
// re-distributes them through a wave-private LDS strip (coalesced 16-byte loads -> C consecutive
// points per lane -> coalesced stores). One wave per line: out = L in0 + J in1.

template <int C, bool DOT>
__device__ __forceinline__ void x_direct_line(const LinePass& p, int64_t line, double* sl,
                                              int lane, double& acc) {
  constexpr int LP = Lds<C>::LP, CP = Lds<C>::CP;
  const int64_t off = line * (64 * C);
  constexpr int NP = 32 * C;  // 16-byte pieces per line
  constexpr int R = (NP + 63) / 64;
  dv2 a[R], b[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int q = lane + 64 * r;
    if (NP % 64 == 0 || q < NP) {
      a[r] = __builtin_nontemporal_load((const dv2*)(p.in0 + off) + q);
      b[r] = __builtin_nontemporal_load((const dv2*)(p.in1 + off) + q);
    }
  }
  auto w = [&](int e) { return (e / C) * CP + (e % C); };
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int q = lane + 64 * r;
    if (NP % 64 == 0 || q < NP) {
      sl[w(2 * q)] = a[r].x;
      sl[w(2 * q + 1)] = a[r].y;
      sl[LP + w(2 * q)] = b[r].x;
      sl[LP + w(2 * q + 1)] = b[r].y;
    }
  }
  wave_sync();
  double x[C], y[C], r1[C], r2[C];
#pragma unroll
  for (int m = 0; m < C; ++m) {
    x[m] = sl[lane * CP + m];
    y[m] = sl[LP + lane * CP + m];
  }
  line_op<C>(x, r1, p.L, lane, p.ablate);
  line_op<C>(y, r2, p.J, lane, p.ablate);
  wave_sync();
#pragma unroll
  for (int m = 0; m < C; ++m) sl[lane * CP + m] = r1[m] + r2[m];
  wave_sync();
  dv2 pp[R];
  if constexpr (DOT) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int q = lane + 64 * r;
      pp[r] = __builtin_nontemporal_load((const dv2*)(p.dot_p + off) + (NP % 64 == 0 || q < NP ? q : 0));
    }
  }
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int q = lane + 64 * r;
    if (NP % 64 == 0 || q < NP) {
      dv2 o;
      o.x = sl[w(2 * q)];
      o.y = sl[w(2 * q + 1)];
      __builtin_nontemporal_store(o, (dv2*)(p.out0 + off) + q);
      if constexpr (DOT) {
        acc += o.x * pp[r].x;
        acc += o.y * pp[r].y;
      }
    }
  }
  wave_sync();  // the strip is reused by the wave's next line
}

// DOT: CG's p . w partial sums as w is written (p = p.dot_p): the waves walk lines
// grid-stride (line = 4 block + wave + 4 grid k), each lane sums its w p products in order, then a
// fixed-order block reduction (lane butterflies, waves in order) -> p.parts[block]
template <int C, bool DOT = false>
__global__ __launch_bounds__(256) void compact_lines_x_direct(LinePass p, int64_t nlines) {
  if (p.skip && *p.skip) return;
  constexpr int LP = Lds<C>::LP;
  __shared__ double strip[4][2 * LP];
  __shared__ double red[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double acc = 0.0;
  for (int64_t line = (int64_t)blockIdx.x * 4 + wave; line < nlines;
       line += DOT ? (int64_t)gridDim.x * 4 : nlines) {
    x_direct_line<C, DOT>(p, line, strip[wave], lane, acc);
  }
  if constexpr (DOT) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
    if (lane == 0) red[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) p.parts[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
  }
}


template <int C>
static int launch_x_direct(pb_ctx* ctx, LinePass& p, int64_t nlines) {
  CgFuse* cf = ctx->cg_fuse;
  if (cf && cf->dot_p) {  // p . w partial sums: a fixed grid of at most 16 blocks per CU
    // (x_dot_cu, A/B: blocks per CU of that grid; 0: one line per wave like the plain X pass)
    const int per_cu = tune("x_dot_cu", 16);
    const int64_t nb = per_cu > 0 ? std::min<int64_t>((nlines + 3) / 4, (int64_t)ctx->num_cus * per_cu)
                                   : (nlines + 3) / 4;
    if (nb > ctx->partials_cap) return set_error(PB_ERR_UNSUPPORTED, "x pass: partials");
    p.dot_p = cf->dot_p;
    p.parts = ctx->d_partials;
    hipLaunchKernelGGL((compact_lines_x_direct<C, true>), dim3((unsigned)nb), dim3(256), 0,
                       ctx->stream, p, nlines);
    PB_HIP(hipGetLastError());
    cf->nparts = (int)nb;
    cf->fused_dot = true;
    return PB_OK;
  }
  hipLaunchKernelGGL(compact_lines_x_direct<C>, dim3((unsigned)((nlines + 3) / 4)), dim3(256), 0,
                     ctx->stream, p, nlines);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

// batched solve on contiguous lines (element stride 1, line stride li): one wave per line,
// redistributed through a wave-private LDS strip like the X pass
template <int C>
__global__ __launch_bounds__(256) void lines_solve_direct(LinePass p, int64_t nlines) {
  if (p.skip && *p.skip) return;
  constexpr int LP = Lds<C>::LP, CP = Lds<C>::CP;
  __shared__ double strip[4][LP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t line = (int64_t)blockIdx.x * 4 + wave;
  if (line >= nlines) return;
  double* sl = strip[wave];
  const int64_t off = line * p.li;
  constexpr int NP = 32 * C;
  constexpr int R = (NP + 63) / 64;
  dv2 a[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int q = lane + 64 * r;
    if (NP % 64 == 0 || q < NP) a[r] = __builtin_nontemporal_load((const dv2*)(p.in0 + off) + q);
  }
  auto w = [&](int e) { return (e / C) * CP + (e % C); };
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int q = lane + 64 * r;
    if (NP % 64 == 0 || q < NP) {
      sl[w(2 * q)] = a[r].x;
      sl[w(2 * q + 1)] = a[r].y;
    }
  }
  wave_sync();
  double x[C];
#pragma unroll
  for (int m = 0; m < C; ++m) x[m] = sl[lane * CP + m];
  line_solve<C>(x, p.J, lane);
  wave_sync();
#pragma unroll
  for (int m = 0; m < C; ++m) sl[lane * CP + m] = x[m];
  wave_sync();
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int q = lane + 64 * r;
    if (NP % 64 == 0 || q < NP) {
      dv2 o;
      o.x = sl[w(2 * q)];
      o.y = sl[w(2 * q + 1)];
      __builtin_nontemporal_store(o, (dv2*)(p.out0 + off) + q);
    }
  }
}

template <int C>
static int launch_solve_direct(pb_ctx* ctx, LinePass& p, int64_t nlines) {
  hipLaunchKernelGGL(lines_solve_direct<C>, dim3((unsigned)((nlines + 3) / 4)), dim3(256), 0,
                     ctx->stream, p, nlines);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

static LineOp make_solve_op(double alpha, int C) {
  LineOp o{};
  const double q = 2.0 * alpha / (1.0 + std::sqrt(1.0 - 4.0 * alpha * alpha));
  o.mq = -q;
  o.inv_kappa = q / alpha;
  double pw = 1.0;
  for (int m = 0; m < C; ++m) {
    pw *= -q;
    o.pw[m] = pw;
  }
  double g = pw;
  int s = 0;
  for (; s < 6; ++s) {
    if (std::fabs(g) < 1e-24) break;
    o.gs[s] = g;
    g = g * g;
  }
  o.nsteps = s;
  o.corr = s == 6 ? 1.0 / (1.0 - g) : 1.0;
  return o;
}

// the CgFuse passes apply: one rank (no z-slab <-> y-slab transposes), register line solves in
// every direction, the Z pass with prefetch (lines of <= 512 points) on an even x extent, default
// launch shapes
// (the same conditions the Z and X passes test below and in compact_pass_*: the solver falls back
// to the unfused iteration when a pass reports it did not fuse)
bool compact_cg_fusable(const pb_grid* g) {
  return !grid_split(g) && !g->ctx->split && tune("compact_lines", 1) &&
         compact_lines_supported(g->n[0]) && compact_lines_supported(g->n[1]) &&
         compact_lines_supported(g->n[2]) && g->n[2] <= 512 && g->n[0] % 2 == 0 &&
         tune("cg_fuse", 1);
}

// split grids (z-slab <-> y-slab transposes, r06): p is formed by the pack of the transpose
// (pb_compact_dist.hip, even nx) and p . w taken by the X pass (register line solves in x);
// a pass that does not fuse is reported and the solver runs the separate kernels for it
bool compact_cg_fusable_split(const pb_grid* g) {
  return g->ctx->split && tune("compact_lines", 1) && compact_lines_supported(g->n[0]) &&
         g->n[0] % 2 == 0 && tune("cg_fuse", 1);
}

bool compact_lines_supported(int64_t n) {
  return for_line_c(n, [](auto) { return (int)PB_OK; }) == PB_OK;
}

// 16-byte pairs when the contiguous direction has even length (always for LAYOUT 1, n = 64*C)
template <int C, int LAYOUT, int PASS, class K>
static int launch_lines_k(pb_ctx* ctx, LinePass& p, int64_t nouter) {
  if (LAYOUT == 1 || (p.ninner % 2 == 0 && p.li == 1 && p.lo % 2 == 0 && p.es % 2 == 0 &&
                      aligned16(p.in0, p.out0)))
    return launch_lines_tiled<compact_lines_kernel<C, LAYOUT, PASS, K, 2>, K, C>(ctx, p, nouter);
  return launch_lines_tiled<compact_lines_kernel<C, LAYOUT, PASS, K, 1>, K, C>(ctx, p, nouter);
}

// Launch shapes (measured at 512^3, profiles/r01/tune_compact*.jsonl): strided passes use 16-line
// tiles (128-B row segments, two blocks per CU), the contiguous X pass 8-line tiles; the batched
// interleaved solve (PASS 3: little compute per tile to hide the next tile's loads under) 32-line
// tiles with two tiles' inputs in flight. C > 8 keeps 8-line tiles for LDS.
template <int C, int LAYOUT, int PASS>
static int launch_lines_c(pb_ctx* ctx, LinePass& p, int64_t nouter) {
  if constexpr (LAYOUT == 0 && C <= 8 && PASS == 3)  // batched solve: 0.62 -> 0.48 ms at 512
    return launch_lines_k<C, LAYOUT, PASS, LineCfg<32, 16, 2>>(ctx, p, nouter);
  else if constexpr (LAYOUT == 0 && C <= 8)
    return launch_lines_k<C, LAYOUT, PASS, LineCfg<16, 16, 1>>(ctx, p, nouter);
  else
    return launch_lines_k<C, LAYOUT, PASS, LineCfg<8, 8, 0>>(ctx, p, nouter);
}

template <int LAYOUT, int PASS>
static int launch_lines(pb_ctx* ctx, LinePass& p, int64_t n, int64_t nouter) {
  if (!compact_lines_supported(n))
    return set_error(PB_ERR_UNSUPPORTED, "compact line solver: n = %lld", (long long)n);
  return for_line_c(n, [&](auto c) {
    return launch_lines_c<decltype(c)::value, LAYOUT, PASS>(ctx, p, nouter);
  });
}

// One pass of the factorised Laplacian with register line solves. axis: 2 = Z, 1 = Y, 0 = X.
int compact_lines_pass(pb_ctx* ctx, const int64_t dims[3], int axis, double h, const double* in0,
                       const double* in1, double* out0, double* out1, const YSlabPlan* blk_in) {
  const LineGeo q = line_geo(dims, axis);
  const int64_t nx = dims[0], nz = dims[2];
  const int C = (int)(q.n / 64);
  static const char* names[3] = {"compact_lines_x", "compact_lines_y", "compact_lines_z"};
  ScopedTimer tm(ctx, names[axis]);
  LinePass p{};
  p.skip = ctx->op_skip;
  p.remap = 0;
  const int ablate = PB_ABLATE_LINES;
  p.ablate = ablate;
  p.in0 = in0;
  p.in1 = in1;
  p.out0 = out0;
  p.out1 = out1;
  p.J = make_line_op(0, C, h);
  p.L = make_line_op(1, C, h);
  p.li = q.li;
  p.lo = q.lo;
  p.es = q.es;
  p.ninner = q.ninner;
  if (axis == 2) {
    CgFuse* cf = ctx->cg_fuse;
    if (cf && cf->z && C <= 8 && nx % 2 == 0 && aligned16(cf->z, out0)) {
      // CG's p formed by the Z pass from z and p_old (CgFuse); in0 is not read
      p.in0 = cf->z;
      p.in1 = cf->p_old;
      p.p_out = cf->p_out;
      p.st = cf->st;
      p.first = cf->first;
      const int rc = for_line_c(q.n, [&](auto c) {
        constexpr int CC = decltype(c)::value;
        using K = LineCfg<16, 16, 1>;
        if constexpr (CC <= 8)  // (the CGP kernels exist up to C = 8)
          return launch_lines_tiled<compact_lines_kernel<CC, 0, 0, K, 2, true>, K, CC>(ctx, p, q.nouter);
        else
          return (int)PB_ERR_UNSUPPORTED;
      });
      if (rc == PB_OK) cf->fused_z = true;
      return rc;
    }
    return launch_lines<0, 0>(ctx, p, q.n, q.nouter);
  }
  if (axis == 1) {
    if (blk_in) {  // row (kl, j) at block j >> k, row kl * nyl + (j & (nyl - 1))
      const int64_t nyl = blk_in->nyl[0];
      int sh = 0;
      while (((int64_t)1 << sh) < nyl) ++sh;
      p.lo_in = nyl * nx;
      p.esh_in = sh;
      p.ebs_in = nz * nyl * nx;
      if (blk_in->self_direct) {
        p.alt_blk = blk_in->me;
        p.alt0 = blk_in->alt0;
        p.alt1 = blk_in->alt1;
      }
      return launch_lines<0, 4>(ctx, p, q.n, q.nouter);
    }
    return launch_lines<0, 1>(ctx, p, q.n, q.nouter);
  }
  if (blk_in) return set_error(PB_ERR_ARG, "compact lines: blocked input on the Y pass only");
  if (!compact_lines_supported(nx))
    return set_error(PB_ERR_UNSUPPORTED, "compact lines: X extent %lld", (long long)nx);
  const int64_t nlines = (int64_t)q.ninner * q.nouter;
  return for_line_c(nx, [&](auto c) { return launch_x_direct<decltype(c)::value>(ctx, p, nlines); });
}

// Batched periodic (alpha, 1, alpha) solve, in place, n = 64*C points per line: contiguous
// lines (elem_stride 1) one wave each; interleaved lines (line_stride 1) through the LDS tile
// transpose. Returns PB_ERR_UNSUPPORTED for other layouts (the caller falls back to LDS PCR).
int lines_solve_batched(pb_ctx* ctx, int64_t n, int64_t nbatch, int64_t line_stride,
                        int64_t elem_stride, double alpha, double* d) {
  if (!compact_lines_supported(n) || !(alpha > 0.0 && alpha < 0.5))
    return PB_ERR_UNSUPPORTED;
  const int C = (int)(n / 64);
  LinePass p{};
  p.skip = ctx->op_skip;
  p.remap = 0;
  p.in0 = d;
  p.out0 = d;
  p.J = make_solve_op(alpha, C);
  if (elem_stride == 1 && line_stride % 2 == 0 && aligned16(d) && line_stride >= n) {
    p.li = line_stride;
    return for_line_c(n, [&](auto c) {
      return launch_solve_direct<decltype(c)::value>(ctx, p, nbatch);
    });
  }
  if (line_stride == 1 && elem_stride >= nbatch) {
    p.li = 1;
    p.lo = 0;
    p.es = elem_stride;
    p.ninner = (int)nbatch;
    return launch_lines<0, 3>(ctx, p, n, 1);
  }
  return PB_ERR_UNSUPPORTED;
}

}  // namespace pb
