// pb_op.cpp -- the operator (MatShell analogue): pb_op_* and the ownership ranges.
#include "pb_ksp.hpp"

using namespace pb;

static int star7_apply(pb_op* op, const double* x, double* y) {
  pb_grid* g = op->grid;
  const Star s = star_of(op);
  const double* hi = x + (g->nzl - 1) * g->plane;
  StencilPlanes one;
  one.ghost_lo = hi;  // periodic wrap: no copy
  one.ghost_hi = x;
  // split grids: interior planes overlap the halo exchange; the two boundary planes follow it
  // (timed as one apply: interior launch, wait for the exchange, boundary launch)
  int none = 0;  // (no sums)
  return halo_overlap(g, x, hi, one, "stencil", 0, &none,
                      [&](int mode, const StencilPlanes& gp, int, int*) {
                        return launch_star7_apply(g, s, x, y, gp, mode);
                      });
}

int pb::op_apply_raw(pb_op* op, const double* x, double* y) {
  pb_grid* g = op->grid;
  if (op->kind == PB_OP_COMPACT) return compact_lapl_fast(g, op->deltas, x, y, op->work);
  PB_TRY(star7_apply(op, x, y));
  if (op->kind != PB_OP_ASSEMBLED27) return PB_OK;
  // assembled P: same 7 non-zeros; re-sum the seam / slab-boundary rows in AIJ order (the
  // ghost planes hold x's halo after the apply on a split grid)
  const Star s = star_of(op);
  const bool split = g->ctx->split;
  return launch_aij_seams(g, s, x, split ? g->ghost_lo : nullptr, split ? g->ghost_hi : nullptr, y);
}

extern "C" {

// ---------------------------------------------------------------------------------------------
// Operator (src/poissbox.f90:242-267 initialise_matrix_free; :300-322 mfmult)
// ---------------------------------------------------------------------------------------------
int pb_op_create(pb_grid* g, int kind, const double deltas[3], pb_op** out) {
  PB_CHECK_ARG(g && out, "bad op args");
  PB_CHECK_ARG(kind == PB_OP_STAR7 || kind == PB_OP_COMPACT || kind == PB_OP_ASSEMBLED27,
               "unknown operator kind");
  pb_op* op = new pb_op();
  op->grid = g;
  op->kind = kind;
  for (int d = 0; d < 3; ++d) op->deltas[d] = deltas ? deltas[d] : g->h[d];
  Star s = star_coeffs(op->deltas);
  op->cx = s.cx;
  op->cy = s.cy;
  op->cz = s.cz;
  op->cc = s.cc;
  if (kind == PB_OP_COMPACT) {
    op->work_len = compact_fast_work_len(g);
    if (hipMalloc(&op->work, (size_t)op->work_len * sizeof(double)) != hipSuccess) {
      delete op;
      return set_error(PB_ERR_ALLOC, "compact operator workspace: out of device memory");
    }
  }
  *out = op;
  return PB_OK;
}

int pb_op_set_deltas(pb_op* op, const double deltas[3]) {
  PB_CHECK_ARG(op && deltas, "bad args");
  for (int d = 0; d < 3; ++d) op->deltas[d] = deltas[d];
  Star s = star_coeffs(op->deltas);
  op->cx = s.cx;
  op->cy = s.cy;
  op->cz = s.cz;
  op->cc = s.cc;
  return PB_OK;
}

int pb_op_apply(pb_op* op, const pb_vec* x, pb_vec* y) {
  PB_CHECK_ARG(op && x && y, "bad apply args");
  PB_CHECK_ARG(x->grid == op->grid && y->grid == op->grid, "vector/operator grid mismatch");
  PB_CHECK_ARG(x != y, "MatMult requires distinct input and output vectors");
  return op_apply_raw(op, x->d, y->d);
}

int pb_op_get_ownership_range(const pb_op* op, int64_t* first, int64_t* next) {
  PB_CHECK_ARG(op && first && next, "bad args");
  const pb_grid* g = op->grid;
  *first = g->k0 * g->plane;
  *next = (g->k0 + g->nzl) * g->plane;
  return PB_OK;
}

int pb_vec_get_ownership_range(const pb_vec* v, int64_t* first, int64_t* next) {
  PB_CHECK_ARG(v && first && next, "bad args");
  const pb_grid* g = v->grid;
  *first = g->k0 * g->plane;
  *next = (g->k0 + g->nzl) * g->plane;
  return PB_OK;
}

int pb_op_get_diagonal(const pb_op* op, double* diag) {
  PB_CHECK_ARG(op && diag, "bad args");
  *diag = op->cc;
  return PB_OK;
}

int pb_op_destroy(pb_op* op) {
  if (!op) return PB_OK;
  if (op->work) {
    (void)wait_stream(op->grid->ctx, op->grid->ctx->stream, "pb_op_destroy");
    (void)hipFree(op->work);
  }
  delete op;
  return PB_OK;
}

}  // extern "C"
