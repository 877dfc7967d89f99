// pb_stencil.hip -- the 7-point operator apply y = A x on the stencil engine (pb_star7.hpp):
// PlainLoad with the epilogue that stores the Laplacian. MatMult of the matrix-free operator, the
// seam-corrected assembled P (pb_assembled.hip) and every solver step that applies A on its own.
#include "pb_star7.hpp"

namespace pb {

// y = the Laplacian (the centre value is not used); 8-row tiles on large planes (TALL)
struct StoreY {
  static constexpr int NS = 0, NE = 0;
  static constexpr bool RAW = false, TALL = true;
  static constexpr int WGCU = 3;  // workgroups per CU the grid is sized for
  static constexpr bool PREFETCH = true;
  double* __restrict__ y;
  __device__ __forceinline__ void prepare() {}
  __device__ __forceinline__ const double* src(int) const { return nullptr; }
  template <int V>
  __device__ __forceinline__ void put(RowIx idx, const double (&c)[V], const double (&w)[V],
                                      double (&)[1][V], double*, int nt) const {
    store_row<V>(y, idx, w, nt);
    (void)c;
  }
};

// Timer names: a whole-grid launch is "<name>"; the two launches of a split apply (interior
// planes, then the boundary planes after the halo exchange) are "<name>_interior" and
// "<name>_boundary", and halo_overlap (pb_internal.hpp) times the apply as a whole under "<name>",
// so "<name>" always averages complete applies over all owned planes.
const char* timer_name(int mode, const char* all, const char* interior, const char* boundary) {
  return mode == PLANES_ALL ? all : (mode == PLANES_INTERIOR ? interior : boundary);
}

int launch_star7_apply(pb_grid* g, const Star& s, const double* x, double* y,
                       const StencilPlanes& gp, int mode) {
  ScopedTimer tm(g->ctx, timer_name(mode, "stencil", "stencil_interior", "stencil_boundary"));
  // alternate the march direction between applies (the boundary launch of a split apply is one
  // plane per chunk, direction-free, and does not flip it)
  const int rev = g->ctx->zflip;
  if (mode != PLANES_BOUNDARY) g->ctx->zflip ^= 1;
  Launch lc{g->ctx->op_skip, mode};
  lc.rev = rev;
  lc.wgcu = tune("stencil_wgcu", 0);
  return launch_any(g, s, PlainLoad{x}, gp, StoreY{y}, lc);
}

}  // namespace pb
