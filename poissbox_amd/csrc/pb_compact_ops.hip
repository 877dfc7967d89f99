// pb_compact_ops.hip -- bandwidth-oriented compact grad, div and interp (factorised line passes).
//
// The reference evaluates grad (src/compact_schemes.f90:42-88), div (:207-257) and interp (:93-152)
// as families of 1-D periodic tridiagonal line solves, one sweep after the other. Every 1-D
// operator is circulant, so the axes commute and each call is a short chain
// of line passes that read and write whole lines once. With I = interp_1d and D_a = grad_1d along
// axis a, all at the call's stagger (-1 grad, +1 div):
//
//   grad (Z -> Y -> X, 112 B/DoF)            div (X -> Y -> Z, 112 B/DoF)
//     Z: a = I f, c = D_z f      1 -> 2        X: g1 = D_x f1              1 -> 1
//     Y: e1 = I a, e2 = D_y a    1 -> 2        X: g2 = I f2                1 -> 1
//     Y: e3 = I c                1 -> 1        X: g3 = I f3                1 -> 1
//     X: df1 = D_x e1            1 -> 1        Y: h = I g1 + D_y g2        2 -> 1
//     X: df2 = I e2              1 -> 1        Y: h3 = I g3                1 -> 1
//     X: df3 = I e3              1 -> 1        Z: out = I h + D_z h3       2 -> 1
//   interp: three 1 -> 1 passes (Z, Y, X), 48 B/DoF.
//
// One primitive per axis, the half-operator line pass out0 = H0 in0 [+ H1 in1] with an optional
// out1 = H1 in0: a half operator is ONE explicit RHS (line_rhs) and ONE (alpha, 1, alpha) solve
// (line_solve), not the Laplacian's pair (line_op). Lines of n = 64*C points run in registers
// (tiled persistent kernels for the strided Y / Z passes, one wave per line for the contiguous X
// pass, pb_compact_lines.hpp); other lengths go to the LDS-PCR kernel's half-operator term
// (pb_compact_fast.hip). The X pass is only ever 1 -> 1 in these chains, and a wave reads its whole
// line before it stores, so it runs in place: grad keeps e1..e3 in the caller's df vectors.
// Results match the reference to rounding (operation order differs); the bit-exact
// reference-order calls stay in pb_compact.hip.
#include <algorithm>
#include <cmath>
#include <type_traits>

#include "pb_internal.hpp"
#include "pb_device.hpp"

#pragma clang fp contract(fast)

#include "pb_compact_lines.hpp"

namespace pb {

// r <- H x: the explicit RHS at the stagger, then the periodic solve
template <int C>
__device__ __forceinline__ void line_half(const double (&x)[C], double (&r)[C], const LineOp& o,
                                          int stagger, int lane) {
  if (stagger < 0)
    line_rhs<C>(x, r, o, -1, lane);
  else
    line_rhs<C>(x, r, o, +1, lane);
  line_solve<C>(r, o, lane);
}

// Strided passes (Y, Z; lines run across rows, the tile transposed through LDS).
// SHAPE 0: out0 = J in0.   SHAPE 1: out0 = J in0, out1 = L in0.   SHAPE 2: out0 = J in0 + L in1.
// (J, L of the LinePass: the first term's and the second term's / output's half operator.)
// K::PF = 1: persistent blocks, the next tile's in0 (SHAPE 2: this tile's in1, then the next
// tile's in0) fetched into registers while the current tile is solved and stored.
template <int C, int SHAPE, class K, int V>
__global__ __launch_bounds__(K::NT) void half_lines_kernel(LinePass p) {
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
  int t = blockIdx.x;
  if (t >= ntiles) return;
  const int stagger = p.stagger;
  double keep[LPW][C];  // SHAPE 1: L in0 until out0 has left LDS; SHAPE 2: J in0 (the first term)
  using Tile = TileRegs<C, 0, TL, V, NT>;
  auto step = [&](int t, Tile& pre, int tn) {
    int64_t base, base_n = 0;
    int nl, nl_n = 0;
    tile_of(t, base, nl);
    if (K::PF && tn < ntiles) tile_of(tn, base_n, nl_n);
    __syncthreads();  // the previous tile's LDS reads are done
    if (!K::PF) tile_fetch(p, p.in0, base, nl, pre);
    tile_put(lds, nl, pre);
    __syncthreads();
    if (K::PF) {
      if (SHAPE == 2)
        tile_fetch(p, p.in1, base, nl, pre);
      else if (tn < ntiles)
        tile_fetch(p, p.in0, base_n, nl_n, pre);
    }
#pragma unroll
    for (int j = 0; j < LPW; ++j) {
      const int l = wave * LPW + j;
      if (l >= nl) continue;
      double x[C], r[C];
      chunk_read<C>(lds, l, lane, x);
      if (SHAPE == 2) {
        line_half<C>(x, keep[j], p.J, stagger, lane);
      } else {
        line_half<C>(x, r, p.J, stagger, lane);
        chunk_write<C>(lds, l, lane, r);  // (a wave's lines are its own)
        if (SHAPE == 1) line_half<C>(x, keep[j], p.L, stagger, lane);
      }
    }
    __syncthreads();
    if (SHAPE != 2) {
      tile_store<C, 0, TL, V, NT>(p, p.out0, lds, base, nl);
      if (SHAPE == 0) return;
      __syncthreads();
#pragma unroll
      for (int j = 0; j < LPW; ++j) {
        const int l = wave * LPW + j;
        if (l < nl) chunk_write<C>(lds, l, lane, keep[j]);
      }
      __syncthreads();
      tile_store<C, 0, TL, V, NT>(p, p.out1, lds, base, nl);
      return;
    }
    // SHAPE 2: the second input's tile through LDS, the first term still in registers
    if (!K::PF) tile_fetch(p, p.in1, base, nl, pre);
    tile_put(lds, nl, pre);
    __syncthreads();
    if (K::PF && tn < ntiles) tile_fetch(p, p.in0, base_n, nl_n, pre);
#pragma unroll
    for (int j = 0; j < LPW; ++j) {
      const int l = wave * LPW + j;
      if (l >= nl) continue;
      double x[C], r[C];
      chunk_read<C>(lds, l, lane, x);
      line_half<C>(x, r, p.L, stagger, lane);
#pragma unroll
      for (int m = 0; m < C; ++m) r[m] = keep[j][m] + r[m];
      chunk_write<C>(lds, l, lane, r);
    }
    __syncthreads();
    tile_store<C, 0, TL, V, NT>(p, p.out0, lds, base, nl);
  };
  Tile pre;
  if (K::PF) {
    int64_t b0;
    int n0;
    tile_of(t, b0, n0);
    tile_fetch(p, p.in0, b0, n0, pre);
  }
  for (; t < ntiles; t += gridDim.x) step(t, pre, t + gridDim.x);
}

// Contiguous X pass, 1 -> 1: one wave per line, re-distributed through a wave-private LDS strip
// (coalesced 16-byte loads -> C consecutive points per lane -> coalesced stores), no block
// barriers. The whole line is in registers before the first store: out0 may be in0.
template <int C>
__global__ __launch_bounds__(256) void half_x_direct(LinePass p, int64_t nlines) {
  if (p.skip && *p.skip) return;
  constexpr int LP = Lds<C>::LP, CP = Lds<C>::CP;
  __shared__ double strip[4][LP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t line = (int64_t)blockIdx.x * 4 + wave;
  if (line >= nlines) return;
  double* sl = strip[wave];
  const int64_t off = line * (64 * C);
  constexpr int NP = 32 * C;  // 16-byte pieces per line
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
  double x[C], y[C];
#pragma unroll
  for (int m = 0; m < C; ++m) x[m] = sl[lane * CP + m];
  line_half<C>(x, y, p.J, p.stagger, lane);
  wave_sync();
#pragma unroll
  for (int m = 0; m < C; ++m) sl[lane * CP + m] = y[m];
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

// the Laplacian's launch shapes (pb_compact_lines.hip): 16-line tiles, persistent with prefetch,
// up to C = 8; 8-line tiles, one per block, above (LDS). 16-byte row moves when the rows are even.
// (2 -> 1 at C = 8 with 8-byte moves, i.e. an odd x extent: the 1024-thread block's 128 VGPRs
// would spill 2 registers, so that one instantiation takes the 512-thread shape as well.)
template <int C, int SHAPE>
static int launch_half_c(pb_ctx* ctx, LinePass& p, int64_t nouter, bool pairs) {
  using K = std::conditional_t<(C <= 8), LineCfg<16, 16, 1>, LineCfg<8, 8, 0>>;
  using K1 = std::conditional_t<(C == 8 && SHAPE == 2), LineCfg<8, 8, 0>, K>;
  if (pairs) return launch_lines_tiled<half_lines_kernel<C, SHAPE, K, 2>, K, C>(ctx, p, nouter);
  return launch_lines_tiled<half_lines_kernel<C, SHAPE, K1, 1>, K1, C>(ctx, p, nouter);
}

template <int SHAPE>
static int launch_half(pb_ctx* ctx, LinePass& p, int64_t n, int64_t nouter, bool pairs) {
  if (!compact_lines_supported(n))
    return set_error(PB_ERR_UNSUPPORTED, "compact half pass: n = %d", (int)n);
  return for_line_c(n, [&](auto c) {
    return launch_half_c<decltype(c)::value, SHAPE>(ctx, p, nouter, pairs);
  });
}

template <int C>
static int launch_half_x(pb_ctx* ctx, LinePass& p, int64_t nlines) {
  hipLaunchKernelGGL(half_x_direct<C>, dim3((unsigned)((nlines + 3) / 4)), dim3(256), 0,
                     ctx->stream, p, nlines);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int compact_half_pass(pb_ctx* ctx, const int64_t d[3], int axis, double h, int stagger,
                      const HalfPass& a) {
  const LineGeo q = line_geo(d, axis);
  if (a.in1 && a.out1) return set_error(PB_ERR_ARG, "compact half pass: 2 -> 2");
  if (!(tune("compact_lines", 1) && compact_lines_supported(q.n)))
    return compact_half_pass_pcr(ctx, d, axis, h, stagger, a);
  const int C = (int)(q.n / 64);
  static const char* names[3] = {"compact_half_x", "compact_half_y", "compact_half_z"};
  ScopedTimer tm(ctx, names[axis]);
  LinePass p{};
  p.skip = ctx->op_skip;
  p.stagger = stagger;
  p.in0 = a.in0;
  p.in1 = a.in1;
  p.out0 = a.out0;
  p.out1 = a.out1;
  p.J = make_line_op(a.k0, C, h);
  p.L = make_line_op(a.k1, C, h);
  if (axis == 0) {
    // (the chains above only have 1 -> 1 X passes; the 16-byte moves need aligned fields)
    if (a.in1 || a.out1 || !aligned16(a.in0, a.out0))
      return compact_half_pass_pcr(ctx, d, axis, h, stagger, a);
    const int64_t nlines = (int64_t)q.ninner * q.nouter;
    return for_line_c(q.n, [&](auto c) { return launch_half_x<decltype(c)::value>(ctx, p, nlines); });
  }
  p.li = q.li;
  p.lo = q.lo;
  p.es = q.es;
  p.ninner = q.ninner;
  // (an absent in1 / out1 is nullptr: aligned)
  const bool pairs = d[0] % 2 == 0 && aligned16(a.in0, a.out0, a.in1, a.out1);
  if (a.in1) return launch_half<2>(ctx, p, q.n, q.nouter, pairs);
  if (a.out1) return launch_half<1>(ctx, p, q.n, q.nouter, pairs);
  return launch_half<0>(ctx, p, q.n, q.nouter, pairs);
}

namespace {

// Z passes on a split grid run on y-slabs (complete z-lines): plain pack / all-to-all / unpack
// transposes around the same line kernels on the same whole lines, so every line's arithmetic is
// the one-rank arithmetic. Scratch: three y-slab fields and the transpose staging.
int64_t ops_zsplit_len(const pb_grid* g) { return grid_split(g) ? yslab_fields_len(g, 3) : 0; }

// the Z pass `a` of a chain: in place on one rank, on y-slabs on a split grid
int half_pass_z(pb_grid* g, double h, int stagger, const HalfPass& a, double* zws) {
  if (!grid_split(g)) {
    const int64_t d[3] = {g->n[0], g->n[1], g->nzl};
    return compact_half_pass(g->ctx, d, 2, h, stagger, a);
  }
  YSlabFields z;
  PB_TRY(yslab_fields_begin(g, zws, 3, &z));
  HalfPass ay = a;
  PB_TRY(yslab_to(g, z.p, a.in0, z.y[0]));
  ay.in0 = z.y[0];
  if (a.in1) {  // 2 -> 1 (div): two fields over, one back
    PB_TRY(yslab_to(g, z.p, a.in1, z.y[1]));
    ay.in1 = z.y[1];
    ay.out0 = z.y[2];
  } else {  // 1 -> 1 (interp), 1 -> 2 (grad: the Laplacian's own shape)
    ay.out0 = z.y[1];
    if (a.out1) ay.out1 = z.y[2];
  }
  PB_TRY(compact_half_pass(g->ctx, z.b, 2, h, stagger, ay));
  PB_TRY(yslab_from(g, z.p, ay.out0, a.out0));
  if (a.out1) PB_TRY(yslab_from(g, z.p, ay.out1, a.out1));
  return PB_OK;
}

enum { H_INTERP = 0, H_GRAD = 1 };

HalfPass one(int k, const double* in, double* out) {
  HalfPass a;
  a.k0 = k;
  a.in0 = in;
  a.out0 = out;
  return a;
}

int check_extents(const pb_grid* g) {
  for (int a = 0; a < 3; ++a)
    if (g->n[a] > 4096)
      return set_error(PB_ERR_UNSUPPORTED, "compact fast path: n > %d", 4096);
  return PB_OK;
}

}  // namespace

// grad: scratch 2N (a, c) + the split-grid transposes; e1..e3 live in df1..df3
int compact_grad_fast(pb_grid* g, const double dx[3], const double* f, double* df1, double* df2,
                      double* df3, double* ws) {
  ScopedTimer tm(g->ctx, "compact_grad_fast");
  const int64_t N = g->nlocal;
  const int64_t d[3] = {g->n[0], g->n[1], g->nzl};
  double *a = ws, *c = ws + N, *zws = ws + 2 * N;
  const int s = -1;
  HalfPass z = one(H_INTERP, f, a);
  z.k1 = H_GRAD;
  z.out1 = c;
  PB_TRY(half_pass_z(g, dx[2], s, z, zws));
  HalfPass y = one(H_INTERP, a, df1);
  y.k1 = H_GRAD;
  y.out1 = df2;
  PB_TRY(compact_half_pass(g->ctx, d, 1, dx[1], s, y));
  PB_TRY(compact_half_pass(g->ctx, d, 1, dx[1], s, one(H_INTERP, c, df3)));
  PB_TRY(compact_half_pass(g->ctx, d, 0, dx[0], s, one(H_GRAD, df1, df1)));
  PB_TRY(compact_half_pass(g->ctx, d, 0, dx[0], s, one(H_INTERP, df2, df2)));
  return compact_half_pass(g->ctx, d, 0, dx[0], s, one(H_INTERP, df3, df3));
}

// div: scratch 5N (g1..g3, h, h3) + the split-grid transposes
int compact_div_fast(pb_grid* g, const double dx[3], const double* f1, const double* f2,
                     const double* f3, double* out, double* ws) {
  ScopedTimer tm(g->ctx, "compact_div_fast");
  const int64_t N = g->nlocal;
  const int64_t d[3] = {g->n[0], g->n[1], g->nzl};
  double *g1 = ws, *g2 = ws + N, *g3 = ws + 2 * N, *hh = ws + 3 * N, *h3 = ws + 4 * N;
  double* zws = ws + 5 * N;
  const int s = +1;
  PB_TRY(compact_half_pass(g->ctx, d, 0, dx[0], s, one(H_GRAD, f1, g1)));
  PB_TRY(compact_half_pass(g->ctx, d, 0, dx[0], s, one(H_INTERP, f2, g2)));
  PB_TRY(compact_half_pass(g->ctx, d, 0, dx[0], s, one(H_INTERP, f3, g3)));
  HalfPass y = one(H_INTERP, g1, hh);
  y.k1 = H_GRAD;
  y.in1 = g2;
  PB_TRY(compact_half_pass(g->ctx, d, 1, dx[1], s, y));
  PB_TRY(compact_half_pass(g->ctx, d, 1, dx[1], s, one(H_INTERP, g3, h3)));
  HalfPass z = one(H_INTERP, hh, out);
  z.k1 = H_GRAD;
  z.in1 = h3;
  return half_pass_z(g, dx[2], s, z, zws);
}

// interp: scratch N + the split-grid transposes; the Y pass writes fi, the X pass runs in place
int compact_interp_fast(pb_grid* g, int stagger, const double* f, double* fi, double* ws) {
  ScopedTimer tm(g->ctx, "compact_interp_fast");
  const int64_t N = g->nlocal;
  const int64_t d[3] = {g->n[0], g->n[1], g->nzl};
  PB_TRY(half_pass_z(g, 0.0, stagger, one(H_INTERP, f, ws), ws + N));
  PB_TRY(compact_half_pass(g->ctx, d, 1, 0.0, stagger, one(H_INTERP, ws, fi)));
  return compact_half_pass(g->ctx, d, 0, 0.0, stagger, one(H_INTERP, fi, fi));
}

}  // namespace pb

extern "C" int pb_compact_grad_fast(pb_grid* g, const double dx[3], const pb_vec* f,
                                    pb_vec* const df[3]) {
  using namespace pb;
  PB_CHECK_ARG(g && dx && f && df && df[0] && df[1] && df[2], "bad grad args");
  PB_CHECK_ARG(f != df[0] && f != df[1] && f != df[2], "grad: the input aliases an output");
  PB_CHECK_ARG(df[0] != df[1] && df[0] != df[2] && df[1] != df[2],
               "grad: the three components must be distinct");
  PB_TRY(check_extents(g));
  double* ws = nullptr;
  PB_TRY(ctx_scratch(g->ctx, (size_t)(2 * g->nlocal + ops_zsplit_len(g)), &ws));
  return compact_grad_fast(g, dx, f->d, df[0]->d, df[1]->d, df[2]->d, ws);
}

extern "C" int pb_compact_div_fast(pb_grid* g, const double dx[3], const pb_vec* const f[3],
                                   pb_vec* df) {
  using namespace pb;
  PB_CHECK_ARG(g && dx && f && f[0] && f[1] && f[2] && df, "bad div args");
  PB_CHECK_ARG(df != f[0] && df != f[1] && df != f[2], "div: an input aliases the output");
  PB_CHECK_ARG(f[0] != f[1] && f[0] != f[2] && f[1] != f[2],
               "div: the three components must be distinct");
  PB_TRY(check_extents(g));
  double* ws = nullptr;
  PB_TRY(ctx_scratch(g->ctx, (size_t)(5 * g->nlocal + ops_zsplit_len(g)), &ws));
  return compact_div_fast(g, dx, f[0]->d, f[1]->d, f[2]->d, df->d, ws);
}

extern "C" int pb_compact_interp_fast(pb_grid* g, int stagger, const pb_vec* f, pb_vec* fi) {
  using namespace pb;
  PB_CHECK_ARG(g && f && fi && f != fi, "bad interp args");
  PB_CHECK_ARG(stagger == -1 || stagger == 1, "stagger must be -1 or +1");
  PB_TRY(check_extents(g));
  double* ws = nullptr;
  PB_TRY(ctx_scratch(g->ctx, (size_t)(g->nlocal + ops_zsplit_len(g)), &ws));
  return compact_interp_fast(g, stagger, f->d, fi->d, ws);
}
