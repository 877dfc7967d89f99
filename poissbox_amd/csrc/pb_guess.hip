// pb_guess.hip -- multi-vector kernels (PETSc VecMDot / VecMAXPY analogues) behind pb_vec_mdot,
// pb_vec_maxpy and the projected initial guess (-ksp_guess_type fischer, pb_ksp_guess.cpp).
// One pass each: every stream is read once with 16-byte loads, two loads per stream in flight per
// thread; grid-stride with a block cap; an odd length ends in a scalar tail. Plain loads and
// stores: non-temporal stores measured no faster (profiles/guess_fischer/README.md). The sums are
// per-block partials in a fixed order (block_partials, then reduce_partials), so every result is
// deterministic run to run.
#include "pb_internal.hpp"
#include "pb_device.hpp"

namespace pb {

// blocks for n2 16-byte elements, two per thread and trip; capped like pb_vecops.hip's grid_for
static int guess_grid(pb_ctx* ctx, int64_t n2) {
  int64_t b = (n2 + 511) / 512;
  const int64_t cap = (int64_t)ctx->num_cus * 8;
  if (b > cap) b = cap;
  if (b < 1) b = 1;
  return (int)b;
}

template <int NV>
__device__ __forceinline__ void mdot_step(const dv2* x2, const VecTable& y, int64_t i,
                                          dv2 (&acc)[NV]) {
  const dv2 xv = x2[i];
  dv2 yv[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) yv[v] = reinterpret_cast<const dv2*>(y.p[v])[i];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] += xv * yv[v];
}

// parts[block * NV + v] = this block's share of sum_j x_j y[v]_j (y[v] may be x itself)
template <int NV>
__global__ __launch_bounds__(256) void mdot_kernel(const double* x, VecTable y, int64_t n,
                                                   double* parts) {
  const dv2* x2 = reinterpret_cast<const dv2*>(x);
  const int64_t n2 = n >> 1;
  const int64_t stride = (int64_t)gridDim.x * 256;
  dv2 acc[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) acc[v] = dv2{0.0, 0.0};
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + stride < n2; i += 2 * stride) {
    // both trips' loads first: two 16-byte loads of every stream in flight
    const dv2 xa = x2[i], xb = x2[i + stride];
    dv2 ya[NV], yb[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      ya[v] = reinterpret_cast<const dv2*>(y.p[v])[i];
      yb[v] = reinterpret_cast<const dv2*>(y.p[v])[i + stride];
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      acc[v] += xa * ya[v];
      acc[v] += xb * yb[v];
    }
  }
  if (i < n2) mdot_step<NV>(x2, y, i, acc);
  double s[NV];
#pragma unroll
  for (int v = 0; v < NV; ++v) s[v] = acc[v].x + acc[v].y;
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {  // odd length: the last element
    const double xt = x[n - 1];
#pragma unroll
    for (int v = 0; v < NV; ++v) s[v] += xt * y.p[v][n - 1];
  }
  block_partials<NV>(s, parts);
}

template <int NV>
__device__ __forceinline__ void maxpy_coefs(const MCoef& c, double* a) {
#pragma unroll
  for (int v = 0; v < NV; ++v) a[v] = c.dev ? c.sign * c.dev[v] : c.host[v];
}

// y = ((y + a0 x0) + a1 x1) + ...   (each product and each sum rounded: no FMA contraction; the
// same order in the vector body and in the tail). from_zero: y is not read, the chain starts at
// 0. y2: a second copy of the result. parts: per-block sums of y_new^2 (wsum: two wide, with the
// plain sum of y_new behind it). NV = 0: only those sums of y as it is (nothing stored).
template <int NV>
__global__ __launch_bounds__(256) void maxpy_kernel(double* y, double* y2, VecTable x, MCoef c,
                                                    int64_t n, int from_zero, double* parts,
                                                    int wsum) {
  constexpr int NA = NV > 0 ? NV : 1;
  double a[NA];
  maxpy_coefs<NV>(c, a);
  dv2* yv2 = reinterpret_cast<dv2*>(y);
  dv2* yo2 = reinterpret_cast<dv2*>(y2);
  const int64_t n2 = n >> 1;
  const int64_t stride = (int64_t)gridDim.x * 256;
  dv2 nrm = dv2{0.0, 0.0}, sm = dv2{0.0, 0.0};
  int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  for (; i + stride < n2; i += 2 * stride) {
    dv2 ya = dv2{0.0, 0.0}, yb = dv2{0.0, 0.0};
    if (!from_zero) {
      ya = yv2[i];
      yb = yv2[i + stride];
    }
    dv2 xa[NA], xb[NA];
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      xa[v] = reinterpret_cast<const dv2*>(x.p[v])[i];
      xb[v] = reinterpret_cast<const dv2*>(x.p[v])[i + stride];
    }
#pragma unroll
    for (int v = 0; v < NV; ++v) {
      ya = ya + a[v] * xa[v];
      yb = yb + a[v] * xb[v];
    }
    if constexpr (NV > 0) {
      yv2[i] = ya;
      yv2[i + stride] = yb;
      if (y2) {
        yo2[i] = ya;
        yo2[i + stride] = yb;
      }
    }
    nrm += ya * ya;
    nrm += yb * yb;
    sm += ya;
    sm += yb;
  }
  if (i < n2) {
    dv2 ya = dv2{0.0, 0.0};
    if (!from_zero) ya = yv2[i];
    dv2 xa[NA];
#pragma unroll
    for (int v = 0; v < NV; ++v) xa[v] = reinterpret_cast<const dv2*>(x.p[v])[i];
#pragma unroll
    for (int v = 0; v < NV; ++v) ya = ya + a[v] * xa[v];
    if constexpr (NV > 0) {
      yv2[i] = ya;
      if (y2) yo2[i] = ya;
    }
    nrm += ya * ya;
    sm += ya;
  }
  double s[2] = {nrm.x + nrm.y, sm.x + sm.y};
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {  // odd length: the last element
    double yt = from_zero ? 0.0 : y[n - 1];
#pragma unroll
    for (int v = 0; v < NV; ++v) yt = yt + a[v] * x.p[v][n - 1];
    if constexpr (NV > 0) {
      y[n - 1] = yt;
      if (y2) y2[n - 1] = yt;
    }
    s[0] += yt * yt;
    s[1] += yt;
  }
  // (uniform over the grid)
  if (parts && wsum) block_partials<2>(s, parts);
  else if (parts) block_partials<1>(s, parts);
}

// out = a - b
__global__ __launch_bounds__(256) void guess_diff_kernel(const double* __restrict__ a,
                                                         const double* __restrict__ b,
                                                         double* __restrict__ out, int64_t n) {
  const int64_t n2 = n >> 1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2; i += (int64_t)gridDim.x * 256)
    reinterpret_cast<dv2*>(out)[i] =
        reinterpret_cast<const dv2*>(a)[i] - reinterpret_cast<const dv2*>(b)[i];
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) out[n - 1] = a[n - 1] - b[n - 1];
}

// b = s b and xdst = s xsrc (xsrc may be xdst) in one launch
__global__ __launch_bounds__(256) void guess_scale_kernel(double* b, const double* xsrc,
                                                          double* xdst, double s, int64_t n) {
  const int64_t n2 = n >> 1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n2;
       i += (int64_t)gridDim.x * 256) {
    const dv2 bv = reinterpret_cast<dv2*>(b)[i], xv = reinterpret_cast<const dv2*>(xsrc)[i];
    reinterpret_cast<dv2*>(b)[i] = s * bv;
    reinterpret_cast<dv2*>(xdst)[i] = s * xv;
  }
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    b[n - 1] = s * b[n - 1];
    xdst[n - 1] = s * xsrc[n - 1];
  }
}

#define PB_NV_CASES(X)                                                                        \
  X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12) X(13) X(14) X(15) X(16)

int launch_mdot(pb_ctx* ctx, const double* x, int nv, const VecTable& y, int64_t n,
                double* d_out) {
  if (nv < 1 || nv > kMaxVecs) return set_error(PB_ERR_ARG, "multi-dot of %d vectors", nv);
  const int nb = guess_grid(ctx, n >> 1);
  if ((int64_t)nb * nv > ctx->partials_cap)
    return set_error(PB_ERR_UNSUPPORTED, "multi-dot: partial sums do not fit");
  {
    ScopedTimer tm(ctx, "guess_mdot");
    switch (nv) {
#define X(NV)                                                                                  \
  case NV:                                                                                     \
    hipLaunchKernelGGL(mdot_kernel<NV>, dim3(nb), dim3(256), 0, ctx->stream, x, y, n,          \
                       ctx->d_partials);                                                       \
    break;
      PB_NV_CASES(X)
#undef X
    }
    PB_HIP(hipGetLastError());
  }
  PB_TRY(reduce_partials(ctx, ctx->d_partials, nb, nv, d_out));
  return allreduce_device(ctx, d_out, nv);
}

int launch_maxpy(pb_ctx* ctx, double* y, double* y2, int nv, const VecTable& x, const MCoef& c,
                 int64_t n, bool from_zero, double* d_norm2, bool with_sum) {
  if (nv < 0 || nv > kMaxVecs) return set_error(PB_ERR_ARG, "multi-axpy of %d vectors", nv);
  const int nb = guess_grid(ctx, n >> 1);
  double* parts = d_norm2 ? ctx->d_partials : nullptr;
  {
    ScopedTimer tm(ctx, "guess_maxpy");
    switch (nv) {
#define X(NV)                                                                                  \
  case NV:                                                                                     \
    hipLaunchKernelGGL(maxpy_kernel<NV>, dim3(nb), dim3(256), 0, ctx->stream, y, y2, x, c, n,  \
                       from_zero ? 1 : 0, parts, with_sum ? 1 : 0);                            \
    break;
      X(0) PB_NV_CASES(X)
#undef X
    }
    PB_HIP(hipGetLastError());
  }
  if (!d_norm2) return PB_OK;
  const int width = with_sum ? 2 : 1;
  PB_TRY(reduce_partials(ctx, ctx->d_partials, nb, width, d_norm2));
  return allreduce_device(ctx, d_norm2, width);
}

int launch_guess_diff(pb_ctx* ctx, const double* a, const double* b, double* out, int64_t n) {
  hipLaunchKernelGGL(guess_diff_kernel, dim3(guess_grid(ctx, n >> 1)), dim3(256), 0, ctx->stream,
                     a, b, out, n);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

int launch_guess_scale(pb_ctx* ctx, double* b, const double* xsrc, double* xdst, double s,
                       int64_t n) {
  ScopedTimer tm(ctx, "guess_scale");
  hipLaunchKernelGGL(guess_scale_kernel, dim3(guess_grid(ctx, n >> 1)), dim3(256), 0,
                     ctx->stream, b, xsrc, xdst, s, n);
  PB_HIP(hipGetLastError());
  return PB_OK;
}

}  // namespace pb
