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

// y = div(beta grad x) (pb_varcoef.hip). One rank: the wrap planes of x read in place; split
// grids: x's boundary planes through halo_overlap (beta's ghost planes are the operator's own).
// nparts != nullptr: the per-block partial sums of x . y ride along (*nparts blocks at block 0)
static int varcoef_apply(pb_op* op, const double* x, double* y, int* nparts) {
  pb_grid* g = op->grid;
  const VarCoef c = varcoef_of(op);
  int none = 0;
  return halo_overlap(g, x, x + (g->nzl - 1) * g->plane, wrap_planes(), "varcoef", 0,
                      nparts ? nparts : &none,
                      [&](int mode, const StencilPlanes& gp, int part_off, int* nb) {
                        return launch_varcoef_apply(g, c, x, y, gp, mode, nparts != nullptr,
                                                    part_off, nb);
                      });
}

int pb::op_apply_dot(pb_op* op, const double* p, double* w, int* nparts) {
  *nparts = 0;
  // (default 1: at 512^3 the fused form saves the dot kernel's 0.36 ms per iteration, six times the
  // unfused launches' own spread, and costs the operator's pass nothing)
  if (op->kind == PB_OP_VARCOEF && tune("varcoef_dot_fused", 1) != 0)
    return varcoef_apply(op, p, w, nparts);
  return op_apply_raw(op, p, w);
}

int pb::op_apply_raw(pb_op* op, const double* x, double* y) {
  pb_grid* g = op->grid;
  if (op->kind == PB_OP_VARCOEF) return varcoef_apply(op, x, y, nullptr);
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
  PB_CHECK_ARG(kind == PB_OP_STAR7 || kind == PB_OP_COMPACT || kind == PB_OP_ASSEMBLED27 ||
                   kind == PB_OP_VARCOEF,
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
  if (kind == PB_OP_VARCOEF) {
    // one field and two ghost planes; beta = 1 everywhere, the ghosts included
    const int64_t len = g->nlocal + 2 * g->plane;
    if (field_alloc(&op->beta_store, (size_t)len * sizeof(double)) != hipSuccess) {
      delete op;
      return set_error(PB_ERR_ALLOC, "variable-coefficient operator: out of device memory");
    }
    op->beta = op->beta_store + g->plane;
    if (const int rc = vec_fill(g->ctx, op->beta_store, len, 1.0)) {
      field_free(op->beta_store);
      delete op;
      return rc;
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
  ++op->change;  // what a KSP derived from the old deltas is rebuilt
  return PB_OK;
}

static int varcoef_only(const pb_op* op, const char* what) {
  if (op->kind != PB_OP_VARCOEF)
    return set_error(PB_ERR_STATE, "%s needs a PB_OP_VARCOEF operator", what);
  return PB_OK;
}

int pb_op_set_coefficient(pb_op* op, const pb_vec* beta, int mean) {
  PB_CHECK_ARG(op && beta, "bad args");
  PB_TRY(varcoef_only(op, "pb_op_set_coefficient"));
  if (op->in_solve > 0)
    return set_error(PB_ERR_STATE, "pb_op_set_coefficient inside a solve that holds the operator");
  PB_CHECK_ARG(mean == PB_COEF_ARITHMETIC || mean == PB_COEF_HARMONIC, "unknown coefficient mean");
  pb_grid* g = op->grid;
  PB_CHECK_ARG(beta->grid == g, "vector/operator grid mismatch");
  // checked on the caller's vector, over all ranks, before anything of the operator changes
  double bad = 0.0;
  PB_TRY(varcoef_count_bad(g, beta->d, false, &bad));
  if (bad != 0.0)
    return set_error(PB_ERR_ARG, "coefficient field: %.0f values are not finite and > 0", bad);
  pb_ctx* ctx = g->ctx;
  PB_HIP(hipMemcpyAsync(op->beta, beta->d, (size_t)g->nlocal * sizeof(double),
                        hipMemcpyDeviceToDevice, ctx->stream));
  // the ghost planes: the neighbouring ranks' boundary planes (one rank: the periodic wrap)
  PB_TRY(halo_exchange_n(g, op->beta, op->beta + (g->nzl - 1) * g->plane, 1, op->beta_store,
                         op->beta + g->nlocal));
  PB_SYNC(ctx, "pb_op_set_coefficient");
  op->mean = mean;
  ++op->change;
  return PB_OK;
}

int pb_op_get_coefficient(const pb_op* op, pb_vec* beta, int* mean) {
  PB_CHECK_ARG(op, "bad args");
  PB_TRY(varcoef_only(op, "pb_op_get_coefficient"));
  if (beta) {
    pb_grid* g = op->grid;
    PB_CHECK_ARG(beta->grid == g, "vector/operator grid mismatch");
    PB_HIP(hipMemcpyAsync(beta->d, op->beta, (size_t)g->nlocal * sizeof(double),
                          hipMemcpyDeviceToDevice, g->ctx->stream));
    PB_SYNC(g->ctx, "pb_op_get_coefficient");
  }
  if (mean) *mean = op->mean;
  return PB_OK;
}

int pb_op_set_mass(pb_op* op, const pb_vec* m, double s) {
  PB_CHECK_ARG(op, "bad args");
  PB_TRY(varcoef_only(op, "pb_op_set_mass"));
  if (op->in_solve > 0)
    return set_error(PB_ERR_STATE, "pb_op_set_mass inside a solve that holds the operator");
  PB_CHECK_ARG(s >= 0.0 && s < INFINITY, "the mass factor s must be finite and >= 0");
  pb_grid* g = op->grid;
  if (!m) {
    if (op->mass) {
      PB_SYNC(g->ctx, "pb_op_set_mass");  // (launches that read the field)
      field_free(op->mass);
      op->mass = nullptr;
    }
  } else {
    PB_CHECK_ARG(m->grid == g, "vector/operator grid mismatch");
    // checked on the caller's vector, over all ranks, before anything of the operator changes
    double bad = 0.0;
    PB_TRY(varcoef_count_bad(g, m->d, true, &bad));
    if (bad != 0.0)
      return set_error(PB_ERR_ARG, "mass field: %.0f values are not finite and >= 0", bad);
    const size_t bytes = (size_t)g->nlocal * sizeof(double);
    if (!op->mass && field_alloc(&op->mass, bytes) != hipSuccess) {
      op->mass = nullptr;
      return set_error(PB_ERR_ALLOC, "mass field: out of device memory");
    }
    PB_HIP(hipMemcpyAsync(op->mass, m->d, bytes, hipMemcpyDeviceToDevice, g->ctx->stream));
    PB_SYNC(g->ctx, "pb_op_set_mass");
  }
  op->mass_s = s;
  ++op->change;
  return PB_OK;
}

int pb_op_get_mass(const pb_op* op, pb_vec* m, double* s) {
  PB_CHECK_ARG(op, "bad args");
  PB_TRY(varcoef_only(op, "pb_op_get_mass"));
  if (m) {
    pb_grid* g = op->grid;
    PB_CHECK_ARG(m->grid == g, "vector/operator grid mismatch");
    if (op->mass)
      PB_HIP(hipMemcpyAsync(m->d, op->mass, (size_t)g->nlocal * sizeof(double),
                            hipMemcpyDeviceToDevice, g->ctx->stream));
    else
      PB_TRY(vec_fill(g->ctx, m->d, g->nlocal, 1.0));
    PB_SYNC(g->ctx, "pb_op_get_mass");
  }
  if (s) *s = op->mass_s;
  return PB_OK;
}

int pb_op_get_diagonal_vec(const pb_op* op, pb_vec* diag) {
  PB_CHECK_ARG(op && diag, "bad args");
  pb_grid* g = op->grid;
  PB_CHECK_ARG(diag->grid == g, "vector/operator grid mismatch");
  if (op->kind == PB_OP_COMPACT)
    return set_error(PB_ERR_UNSUPPORTED, "the compact operator has no stored diagonal");
  if (op->kind == PB_OP_VARCOEF) PB_TRY(launch_varcoef_diag(g, varcoef_of(op), diag->d, false));
  else PB_TRY(vec_fill(g->ctx, diag->d, g->nlocal, op->cc));
  PB_SYNC(g->ctx, "pb_op_get_diagonal_vec");
  return PB_OK;
}

int pb_op_apply(pb_op* op, const pb_vec* x, pb_vec* y) {
  PB_CHECK_ARG(op && x && y, "bad apply args");
  PB_CHECK_ARG(x->grid == op->grid && y->grid == op->grid, "vector/operator grid mismatch");
  PB_CHECK_ARG(x != y, "MatMult requires distinct input and output vectors");
  return op_apply_raw(op, x->d, y->d);
}

// ---------------------------------------------------------------------------------------------
// MAC-grid gradient, projection and divergence of the 7-point operators (pb_mac.hip)
// ---------------------------------------------------------------------------------------------
// the checks the three calls share: the kind, the face field's three distinct vectors of the
// operator's grid, the cell vector (another vector of that grid), a finite factor
static int mac_check(const pb_op* op, const pb_vec* cell, const pb_vec* const f[3], double s) {
  PB_CHECK_ARG(op && cell && f && f[0] && f[1] && f[2], "bad MAC args");
  if (op->kind != PB_OP_STAR7 && op->kind != PB_OP_VARCOEF)
    return set_error(PB_ERR_UNSUPPORTED,
                     "the MAC operators need a PB_OP_STAR7 or PB_OP_VARCOEF operator");
  PB_CHECK_ARG(cell->grid == op->grid, "vector/operator grid mismatch");
  for (int d = 0; d < 3; ++d) {
    PB_CHECK_ARG(f[d]->grid == op->grid, "vector/operator grid mismatch");
    PB_CHECK_ARG(f[d] != cell, "the cell vector is one of the face field's components");
  }
  PB_CHECK_ARG(f[0] != f[1] && f[0] != f[2] && f[1] != f[2],
               "the three components of a face field must be distinct vectors");
  PB_CHECK_ARG(s - s == 0.0, "the factor s must be finite");
  return PB_OK;
}

static int mac_grad(const pb_op* op, const pb_vec* p, double s, pb_vec* const u[3], bool project) {
  PB_TRY(mac_check(op, p, u, s));
  pb_grid* g = op->grid;
  const MacCoef c = mac_coef_of(op);
  double* const ud[3] = {u[0]->d, u[1]->d, u[2]->d};
  const double* pd = p->d;
  int none = 0;
  return halo_overlap(g, pd, pd + (g->nzl - 1) * g->plane, wrap_planes(),
                      project ? "mac_project" : "mac_grad", 0, &none,
                      [&](int mode, const StencilPlanes& gp, int, int*) {
                        return launch_mac_grad(g, c, pd, s, ud, project, gp, mode);
                      });
}

int pb_op_mac_grad(const pb_op* op, const pb_vec* p, pb_vec* const g[3]) {
  return mac_grad(op, p, 1.0, g, false);
}

int pb_op_mac_project(const pb_op* op, const pb_vec* p, double s, pb_vec* const u[3]) {
  return mac_grad(op, p, s, u, true);
}

int pb_op_mac_div(const pb_op* op, double s, const pb_vec* const u[3], pb_vec* out) {
  PB_TRY(mac_check(op, out, u, s));
  pb_grid* g = op->grid;
  const MacCoef c = mac_coef_of(op);
  const double* const ud[3] = {u[0]->d, u[1]->d, u[2]->d};
  int none = 0;
  return halo_overlap(g, ud[2], ud[2] + (g->nzl - 1) * g->plane, wrap_planes(), "mac_div", 0, &none,
                      [&](int mode, const StencilPlanes& gp, int, int*) {
                        return launch_mac_div(g, c, s, ud, out->d, gp, mode);
                      });
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
  if (op->kind == PB_OP_VARCOEF)
    return set_error(PB_ERR_UNSUPPORTED,
                     "the diagonal of PB_OP_VARCOEF is a field: use pb_op_get_diagonal_vec");
  *diag = op->cc;
  return PB_OK;
}

int pb_op_destroy(pb_op* op) {
  if (!op) return PB_OK;
  if (op->work || op->beta_store || op->mass)
    (void)wait_stream(op->grid->ctx, op->grid->ctx->stream, "pb_op_destroy");
  if (op->work) (void)hipFree(op->work);
  field_free(op->beta_store);
  field_free(op->mass);
  delete op;
  return PB_OK;
}

}  // extern "C"
