// pb_solver.cpp -- operator (MatShell analogue) and KSP (KSPSolve_CG analogue) host logic.
//
// The CG iteration runs as 2 fused stencil passes + 2 one-block finalize kernels per iteration
// (plus a plane-sized boundary kernel and, on several ranks, one halo exchange and two scalar
// allreduces). All CG scalars live on the device; the host never waits inside an iteration and
// polls a per-iteration "done" flag (host-mapped) every `check_every` iterations, lagged by one
// poll interval so that every rank stops after the same number of enqueued iterations.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <strings.h>
#include <string>
#include <vector>

#include "pb_internal.hpp"

using namespace pb;

namespace pb {
int compact_lapl(pb_grid* g, const double dx[3], const double* f, double* out, double* work);
int64_t compact_work_len(const pb_grid* g);
}

// the fused CG passes evaluate A p inside the stencil engine (reference order); the assembled P
// (AIJ order at the seams) runs the unfused iteration around its own MatMult
static bool fused_kind(int kind) { return kind == PB_OP_STAR7; }

struct pb_ksp {
  pb_op* A = nullptr;
  pb_op* P = nullptr;
  pb_ksp_opts opts;
  double* r = nullptr;
  // Jacobi / none on the fused operator: pass B forms and stores p and writes the residual to
  // the other buffer -- iteration i reads rbuf(i), writes rbuf(i + 1)
  double* r2 = nullptr;
  bool pst = false;
  double* rbuf(int64_t i) const { return (pst && (i & 1)) ? r2 : r; }
  // iteration i: p_old = pb[i % ns], p_new = pb[(i + 1) % ns]; ns = 2, or 4 with the depth-4
  // deferred x update (pb[2], pb[3] allocated on first use)
  double* pb[4] = {nullptr, nullptr, nullptr, nullptr};
  double* w = nullptr;   // generic (unfused) path only
  double* z = nullptr;   // generic path only
  // Richardson (-ksp_type richardson): update i reads xbuf(i) and writes xbuf(i + 1) -- the
  // engine pass forms x_new at a point's neighbours from x_old there, so x is never updated in
  // place; the caller's x is xbuf(even), and pb_ksp_end copies x2 back after an odd number of
  // updates (the device's count: launches that exited at entry flipped nothing). Jacobi / none:
  // r ping-pongs likewise (rich_rbuf), r_0 = b read in place from a zero guess
  double* x2 = nullptr;
  bool rich_guess = false;  // this solve started from a nonzero guess (r_0 is in r, not b)
  // Chebyshev (-ksp_type chebyshev) runs as Richardson does (rich() covers both) with one more
  // solution buffer: update i >= 1 reads y_i = xbuf(i) and y_(i-1) = xbuf(i - 1) and writes
  // xbuf(i + 1), the three rotating; the caller's x is xbuf(0 mod 3)
  double* x3 = nullptr;
  bool cheb() const { return opts.ksp_type == PB_KSP_CHEBYSHEV; }
  bool rich() const { return opts.ksp_type == PB_KSP_RICHARDSON || cheb(); }
  double* xbuf(int64_t i) const {
    if (cheb()) return i % 3 == 0 ? x->d : (i % 3 == 1 ? x2 : x3);
    return (i & 1) ? x2 : x->d;
  }
  // the bounds in use and what follows from them (KSPSolve_Chebyshev's scale, mu, omegaprod);
  // cheb_state: 0 = not set yet, 1 = the caller's, 2 = estimated for the deltas in cheb_deltas
  // (A's, then P's: the estimate runs again when either changed)
  pb_ksp_chebyshev_opts copts;  // pb_ksp_chebyshev_set_opts; the defaults from pb_ksp_create
  int cheb_state = 0;
  double cheb_emin = 0.0, cheb_emax = 0.0, cheb_scale = 0.0, cheb_mu = 0.0, cheb_omegaprod = 0.0;
  double cheb_deltas[6] = {0, 0, 0, 0, 0, 0};
  const double* rich_rbuf(int64_t i) const {
    return i == 0 && !rich_guess ? b->d : ((i & 1) ? r2 : r);
  }
  pb::Mg* mg = nullptr;  // SOR / multigrid preconditioner (PB_PC_SOR, PB_PC_MG)
  pb_pc_mg_opts mgopts;  // pb_ksp_pc_mg_set_opts; the defaults from pb_ksp_create
  pb::FftPc* fft = nullptr;  // spectral preconditioner (PB_PC_FFT)
  int fold_nparts_b = 0;     // partial-sum blocks of the last folded pass B
  bool stored_z() const { return mg || fft; }  // PCs whose z = M^-1 r is stored (not Jacobi)
  bool lazy0 = false;  // r0 = b, x0 = 0, p0 = 0 left implicit by pb_ksp_begin
  double* guess_bsums() const { return reinterpret_cast<double*>(d_st + 2); }
  CgState* d_st = nullptr;
  double* d_hist = nullptr;
  int64_t nhist = 0;
  int* h_done = nullptr;      // host-mapped, one flag per host iteration (+1)
  int* h_done_dev = nullptr;  // its device alias
  int64_t done_cap = 0;
  std::vector<hipEvent_t> ring;
  // solve state
  const pb_vec* b = nullptr;
  pb_vec* x = nullptr;
  int64_t host_iter = 0;
  bool stopped = false;
  bool begun = false;
  int defer_x = 4;  // x updated every defer_x-th iteration (PB_CG_DEFER_X = 0, 2 or 4)
  int pslots() const { return defer_x == 4 ? 4 : 2; }
  // single-reduction iteration (-ksp_cg_single_reduction on the fused operator, Jacobi / none):
  // the state alternates between the two slots d_st[0..1] within a pb_ksp_iterate batch (pass P
  // of the batch's n-th iteration reads slot n & 1 and writes the other); sr_nparts = pass S's
  // partial-sum blocks of the last iteration (folded: reduced by the next pass P's prologue)
  bool sr = false;
  int sr_nparts = 0;
  // projected initial guess (-ksp_guess_type fischer; PETSc KSPGuessFischer model 1): curl stored
  // pairs (xt[i], bt[i] = A xt[i]) with the bt orthonormal in the 2-norm, and the last formed
  // guess. d_coef: [0..15] the multi-dot's sums, [16] the new direction's norm^2
  struct Fischer {
    int maxl = 0, curl = 0;
    std::vector<double*> xt, bt;
    double* guess = nullptr;
    double* d_coef = nullptr;
  };
  Fischer* fg = nullptr;
};

static int sr_pass_s(pb_ksp* k, const double* r, const CgState* st, int* nparts, int64_t n);
static const double* sr_region(const pb_ctx* ctx, int64_t n);

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

static int star7_apply(pb_op* op, const double* x, double* y) {
  pb_grid* g = op->grid;
  Star s{op->cx, op->cy, op->cz, op->cc};
  StencilPlanes gp;
  if (!g->ctx->split) {
    gp.ghost_lo = x + (g->nzl - 1) * g->plane;  // periodic wrap: no copy
    gp.ghost_hi = x;
    return launch_star7_apply(g, s, x, y, gp, PLANES_ALL);
  }
  gp.ghost_lo = g->ghost_lo;
  gp.ghost_hi = g->ghost_hi;
  if (g->nzl < 3) {
    PB_TRY(halo_exchange(g, x, x + (g->nzl - 1) * g->plane));
    return launch_star7_apply(g, s, x, y, gp, PLANES_ALL);
  }
  // interior planes overlap the halo exchange; the two boundary planes follow it (timed as one
  // apply: interior launch, wait for the exchange, boundary launch)
  ScopedTimer tm(g->ctx, "stencil");
  PB_TRY(halo_begin(g, x, x + (g->nzl - 1) * g->plane));
  PB_TRY(launch_star7_apply(g, s, x, y, gp, PLANES_INTERIOR));
  PB_TRY(halo_end(g));
  return launch_star7_apply(g, s, x, y, gp, PLANES_BOUNDARY);
}

// KSP iterations enqueued ahead of the convergence poll: the operator kernels launched inside
// the guard's scope exit at entry once the KSP's device flag is set (pb_ctx::op_skip)
struct OpApplySkip {
  pb_ctx* ctx;
  OpApplySkip(pb_ctx* c, const int* flag) : ctx(c) { ctx->op_skip = flag; }
  ~OpApplySkip() { ctx->op_skip = nullptr; }
};

static int op_apply_raw(pb_op* op, const double* x, double* y) {
  pb_grid* g = op->grid;
  if (op->kind == PB_OP_COMPACT) return compact_lapl_fast(g, op->deltas, x, y, op->work);
  PB_TRY(star7_apply(op, x, y));
  if (op->kind != PB_OP_ASSEMBLED27) return PB_OK;
  // assembled P: same 7 non-zeros; re-sum the seam / slab-boundary rows in AIJ order (the
  // ghost planes hold x's halo after the apply on a split grid)
  Star s{op->cx, op->cy, op->cz, op->cc};
  const bool split = g->ctx->split;
  return launch_aij_seams(g, s, x, split ? g->ghost_lo : nullptr, split ? g->ghost_hi : nullptr, y);
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

// ---------------------------------------------------------------------------------------------
// Options (PETSc options database names, src/poissbox.f90:295 KSPSetFromOptions)
// ---------------------------------------------------------------------------------------------
int pb_ksp_opts_default(pb_ksp_opts* o) {
  PB_CHECK_ARG(o, "opts is NULL");
  o->rtol = 1e-5;
  o->atol = 1e-50;
  o->dtol = 1e5;
  o->max_it = 10000;
  o->ksp_type = PB_KSP_CG;
  o->pc_type = PB_PC_JACOBI;
  o->nullspace = 1;
  o->monitor = 0;
  o->converged_reason = 0;
  o->check_every = 8;
  o->mg_levels = 0;
  o->mg_coarse_its = 8;
  o->sor_omega = 1.0;
  o->cg_single_reduction = 0;
  o->initial_guess_nonzero = 0;
  o->converged_use_initial_residual_norm = 0;
  o->converged_use_min_initial_residual_norm = 0;
  o->guess_type = PB_GUESS_NONE;
  o->guess_fischer_model = 1;  // PETSc's -ksp_guess_fischer_model default "1,10"
  o->guess_fischer_maxl = 10;
  o->richardson_scale = 1.0;  // KSPRichardsonSetScale's default
  return PB_OK;
}

int pb_ksp_chebyshev_opts_default(pb_ksp_chebyshev_opts* o) {
  PB_CHECK_ARG(o, "opts is NULL");
  o->emin = 0.0;  // 0, 0: estimate
  o->emax = 0.0;
  const double tr[4] = {0.0, 0.1, 0.0, 1.1};  // KSPChebyshevEstEigSet's default transform
  for (int i = 0; i < 4; ++i) o->esteig[i] = tr[i];
  o->esteig_steps = 10;
  return PB_OK;
}

static bool parse_real_list(const char* v, int n, double* out);

int pb_pc_mg_opts_default(pb_pc_mg_opts* o) {
  PB_CHECK_ARG(o, "opts is NULL");
  o->levels_ksp_type = PB_MG_LEVELS_RICHARDSON;
  o->levels_pc_type = PB_MG_LEVELS_SOR;
  o->levels_ksp_max_it = 1;
  o->levels_richardson_scale = 1.0;
  o->levels_eigenvalues[0] = o->levels_eigenvalues[1] = 0.0;  // 0, 0: the transform of (0, 2)
  const double tr[4] = {0.0, 0.1, 0.0, 1.1};
  for (int i = 0; i < 4; ++i) o->levels_esteig[i] = tr[i];
  return PB_OK;
}

// the level smoother's Chebyshev interval: D^-1 A is positive semi-definite
static int check_mg_pair(double emin, double emax, const char* what) {
  if (!std::isfinite(emin) || !std::isfinite(emax) || !(emin > 0.0) || !(emax > emin))
    return set_error(PB_ERR_ARG, "%s: emin %g, emax %g are no finite bounds with 0 < emin < emax",
                     what, emin, emax);
  return PB_OK;
}

// the bounds the level smoother runs with: the caller's, or the esteig transform of D^-1 A's
// exact extremes (0, 2) on every level
static void mg_levels_bounds(const pb_pc_mg_opts* o, double* emin, double* emax) {
  if (o->levels_eigenvalues[0] != 0.0 || o->levels_eigenvalues[1] != 0.0) {
    *emin = o->levels_eigenvalues[0];
    *emax = o->levels_eigenvalues[1];
    return;
  }
  const double lo = 0.0, hi = 2.0;
  *emin = o->levels_esteig[0] * lo + o->levels_esteig[1] * hi;
  *emax = o->levels_esteig[2] * lo + o->levels_esteig[3] * hi;
}

static int check_mg_opts(const pb_pc_mg_opts* o) {
  const int kt = o->levels_ksp_type, pt = o->levels_pc_type;
  if (kt != PB_MG_LEVELS_RICHARDSON && kt != PB_MG_LEVELS_CHEBYSHEV)
    return set_error(PB_ERR_ARG, "unknown mg levels_ksp_type %d", kt);
  if (pt != PB_MG_LEVELS_SOR && pt != PB_MG_LEVELS_JACOBI)
    return set_error(PB_ERR_ARG, "unknown mg levels_pc_type %d", pt);
  if (o->levels_ksp_max_it < 1 || o->levels_ksp_max_it > 8)
    return set_error(PB_ERR_ARG, "-mg_levels_ksp_max_it %d outside 1..8", o->levels_ksp_max_it);
  if (!std::isfinite(o->levels_richardson_scale) || !(o->levels_richardson_scale > 0.0))
    return set_error(PB_ERR_ARG, "-mg_levels_ksp_richardson_scale %g is not finite and > 0",
                     o->levels_richardson_scale);
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(o->levels_esteig[i]))
      return set_error(PB_ERR_ARG, "mg levels_esteig[%d] is not finite", i);
  if (o->levels_eigenvalues[0] != 0.0 || o->levels_eigenvalues[1] != 0.0)
    PB_TRY(check_mg_pair(o->levels_eigenvalues[0], o->levels_eigenvalues[1],
                         "-mg_levels_ksp_chebyshev_eigenvalues"));
  if (kt == PB_MG_LEVELS_CHEBYSHEV) {
    if (pt == PB_MG_LEVELS_SOR)
      return set_error(PB_ERR_UNSUPPORTED,
                       "-mg_levels_ksp_type chebyshev with -mg_levels_pc_type sor: the polynomial "
                       "smoother runs over jacobi only");
    double emin, emax;
    mg_levels_bounds(o, &emin, &emax);
    PB_TRY(check_mg_pair(emin, emax, "-mg_levels_ksp_chebyshev_esteig transform of (0, 2)"));
  }
  if (pt == PB_MG_LEVELS_SOR && o->levels_richardson_scale != 1.0)
    return set_error(PB_ERR_UNSUPPORTED,
                     "-mg_levels_ksp_richardson_scale %g with -mg_levels_pc_type sor: only 1 "
                     "(the relaxation factor is -pc_sor_omega)", o->levels_richardson_scale);
  return PB_OK;
}

int pb_pc_mg_opts_parse(pb_pc_mg_opts* o, int argc, const char* const* argv) {
  PB_CHECK_ARG(o, "opts is NULL");
  for (int i = 0; i < argc; ++i) {
    const char* a = argv[i];
    const char* v = i + 1 < argc ? argv[i + 1] : nullptr;
    if (!a || strncmp(a, "-mg_", 4) || !v) continue;
    if (!strcmp(a, "-mg_levels_ksp_type")) {
      if (!strcmp(v, "richardson")) o->levels_ksp_type = PB_MG_LEVELS_RICHARDSON;
      else if (!strcmp(v, "chebyshev")) o->levels_ksp_type = PB_MG_LEVELS_CHEBYSHEV;
      else
        return set_error(PB_ERR_UNSUPPORTED, "-mg_levels_ksp_type %s: only richardson, chebyshev",
                         v);
      ++i;
    } else if (!strcmp(a, "-mg_levels_pc_type")) {
      if (!strcmp(v, "sor")) o->levels_pc_type = PB_MG_LEVELS_SOR;
      else if (!strcmp(v, "jacobi")) o->levels_pc_type = PB_MG_LEVELS_JACOBI;
      else return set_error(PB_ERR_UNSUPPORTED, "-mg_levels_pc_type %s: only sor, jacobi", v);
      ++i;
    } else if (!strcmp(a, "-mg_levels_ksp_max_it")) {
      const int n = atoi(v);
      if (n < 1 || n > 8)
        return set_error(PB_ERR_ARG, "-mg_levels_ksp_max_it %s: outside 1..8", v);
      o->levels_ksp_max_it = n;
      ++i;
    } else if (!strcmp(a, "-mg_levels_ksp_richardson_scale")) {
      const double s = atof(v);
      if (!std::isfinite(s) || !(s > 0.0))
        return set_error(PB_ERR_ARG, "-mg_levels_ksp_richardson_scale %s: not finite and > 0", v);
      o->levels_richardson_scale = s;
      ++i;
    } else if (!strcmp(a, "-mg_levels_ksp_chebyshev_eigenvalues")) {
      double e[2];
      if (!parse_real_list(v, 2, e))
        return set_error(PB_ERR_ARG, "-mg_levels_ksp_chebyshev_eigenvalues %s: expected emin,emax",
                         v);
      PB_TRY(check_mg_pair(e[0], e[1], "-mg_levels_ksp_chebyshev_eigenvalues"));
      o->levels_eigenvalues[0] = e[0];
      o->levels_eigenvalues[1] = e[1];
      ++i;
    } else if (!strcmp(a, "-mg_levels_ksp_chebyshev_esteig")) {
      double t[4];
      if (!parse_real_list(v, 4, t))
        return set_error(PB_ERR_ARG, "-mg_levels_ksp_chebyshev_esteig %s: expected a,b,c,d", v);
      for (int j = 0; j < 4; ++j) {
        if (!std::isfinite(t[j]))
          return set_error(PB_ERR_ARG, "-mg_levels_ksp_chebyshev_esteig %s: not finite", v);
        o->levels_esteig[j] = t[j];
      }
      ++i;
    } else if (!strcmp(a, "-mg_levels_ksp_rtol") || !strcmp(a, "-mg_coarse_sub_pc_type")) {
      ++i;  // accepted, no effect: fixed sweep counts, SOR sweeps on the coarsest level
    }
  }
  return check_mg_opts(o);
}

// Chebyshev's interval: finite, non-zero, of one sign (negative pairs are legal, as in PETSc: A is
// negative semi-definite, so M^-1 A is negative without a PC), emax > emin
static int check_cheb_pair(double emin, double emax, const char* what) {
  if (!std::isfinite(emin) || !std::isfinite(emax) || emin == 0.0 || emax == 0.0 ||
      (emin < 0.0) != (emax < 0.0) || !(emax > emin))
    return set_error(PB_ERR_ARG,
                     "%s: emin %g, emax %g are no finite, non-zero bounds of one sign with "
                     "emax > emin", what, emin, emax);
  return PB_OK;
}

static int check_cheb_opts(const pb_ksp_chebyshev_opts* o) {
  if (o->emin != 0.0 || o->emax != 0.0)
    PB_TRY(check_cheb_pair(o->emin, o->emax, "chebyshev eigenvalues"));
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(o->esteig[i]))
      return set_error(PB_ERR_ARG, "chebyshev esteig[%d] is not finite", i);
  if (o->esteig_steps < 1 || o->esteig_steps > 64)
    return set_error(PB_ERR_ARG, "chebyshev esteig_steps %d outside 1..64", o->esteig_steps);
  return PB_OK;
}

// exactly n comma-separated numbers
static bool parse_real_list(const char* v, int n, double* out) {
  for (int i = 0; i < n; ++i) {
    char* end = nullptr;
    out[i] = strtod(v, &end);
    if (end == v) return false;
    if (i + 1 < n) {
      if (*end != ',') return false;
      v = end + 1;
    } else if (*end != '\0') {
      return false;
    }
  }
  return true;
}

static int check_guess_opts(int model, int maxl) {
  if (model == 2 || model == 3)
    return set_error(PB_ERR_UNSUPPORTED, "-ksp_guess_fischer_model %d: only model 1", model);
  if (model != 1) return set_error(PB_ERR_ARG, "-ksp_guess_fischer_model %d: no such model", model);
  if (maxl < 1 || maxl > kMaxVecs)
    return set_error(PB_ERR_ARG, "-ksp_guess_fischer_model: maxl %d outside 1..%d", maxl, kMaxVecs);
  return PB_OK;
}

// KSPConvergedDefaultSetUIRNorm / SetUMIRNorm exclude each other (PETSc errors on the second)
static int check_ref_norm_opts(const pb_ksp_opts* o) {
  if (o->converged_use_initial_residual_norm && o->converged_use_min_initial_residual_norm)
    return set_error(PB_ERR_ARG,
                     "-ksp_converged_use_initial_residual_norm and "
                     "-ksp_converged_use_min_initial_residual_norm exclude each other");
  return PB_OK;
}

int pb_ksp_chebyshev_opts_parse(pb_ksp_chebyshev_opts* o, int argc, const char* const* argv) {
  PB_CHECK_ARG(o, "opts is NULL");
  for (int i = 0; i < argc; ++i) {
    const char* a = argv[i];
    const char* v = i + 1 < argc ? argv[i + 1] : nullptr;
    auto flag = [&](int* out) {  // PetscOptionsBool, as in pb_ksp_opts_parse
      auto is = [&](const char* w) { return v && !strcasecmp(v, w); };
      *out = 1;
      if (is("true") || is("yes") || is("on") || is("1")) {
        ++i;
      } else if (is("false") || is("no") || is("off") || is("0")) {
        *out = 0;
        ++i;
      }
    };
    if (!strcmp(a, "-ksp_chebyshev_eigenvalues") && v) {
      double e[2];
      if (!parse_real_list(v, 2, e))
        return set_error(PB_ERR_ARG, "-ksp_chebyshev_eigenvalues %s: expected emin,emax", v);
      PB_TRY(check_cheb_pair(e[0], e[1], "-ksp_chebyshev_eigenvalues"));
      o->emin = e[0];
      o->emax = e[1];
      ++i;
    } else if (!strcmp(a, "-ksp_chebyshev_esteig") && v) {
      double t[4];
      if (!parse_real_list(v, 4, t))
        return set_error(PB_ERR_ARG, "-ksp_chebyshev_esteig %s: expected a,b,c,d", v);
      for (int j = 0; j < 4; ++j) {
        if (!std::isfinite(t[j]))
          return set_error(PB_ERR_ARG, "-ksp_chebyshev_esteig %s: not finite", v);
        o->esteig[j] = t[j];
      }
      ++i;
    } else if (!strcmp(a, "-ksp_chebyshev_esteig_steps") && v) {
      const int n = atoi(v);
      if (n < 1 || n > 64)
        return set_error(PB_ERR_ARG, "-ksp_chebyshev_esteig_steps %s: outside 1..64", v);
      o->esteig_steps = n;
      ++i;
    } else if (!strcmp(a, "-ksp_chebyshev_esteig_noisy")) {
      int noisy = 1;
      flag(&noisy);
      if (!noisy)
        return set_error(PB_ERR_UNSUPPORTED,
                         "-ksp_chebyshev_esteig_noisy false: the estimate starts from noise");
    }
  }
  return PB_OK;
}

int pb_ksp_opts_parse(pb_ksp_opts* o, int argc, const char* const* argv) {
  PB_CHECK_ARG(o, "opts is NULL");
  for (int i = 0; i < argc; ++i) {
    const char* a = argv[i];
    const char* v = i + 1 < argc ? argv[i + 1] : nullptr;
    // PetscOptionsBool: a bare flag is true; an explicit value may follow
    // (PetscOptionsStringToBool: case-insensitive true/yes/on/1 and false/no/off/0)
    auto flag = [&](int* out) {
      auto is = [&](const char* w) { return v && !strcasecmp(v, w); };
      *out = 1;
      if (is("true") || is("yes") || is("on") || is("1")) {
        ++i;
      } else if (is("false") || is("no") || is("off") || is("0")) {
        *out = 0;
        ++i;
      }
    };
    if (!strcmp(a, "-ksp_type") && v) {
      if (!strcmp(v, "cg")) o->ksp_type = PB_KSP_CG;
      else if (!strcmp(v, "preonly")) o->ksp_type = PB_KSP_PREONLY;
      else if (!strcmp(v, "richardson")) o->ksp_type = PB_KSP_RICHARDSON;
      else if (!strcmp(v, "chebyshev")) o->ksp_type = PB_KSP_CHEBYSHEV;
      else
        return set_error(PB_ERR_UNSUPPORTED,
                         "-ksp_type %s: only cg, preonly, richardson, chebyshev", v);
      ++i;
    } else if (!strcmp(a, "-ksp_richardson_scale") && v) {
      o->richardson_scale = atof(v);
      if (!std::isfinite(o->richardson_scale))
        return set_error(PB_ERR_ARG, "-ksp_richardson_scale %s: not finite", v);
      ++i;
    } else if (!strcmp(a, "-ksp_richardson_self_scale")) {
      int self_scale = 0;
      flag(&self_scale);
      if (self_scale) return set_error(PB_ERR_UNSUPPORTED, "-ksp_richardson_self_scale");
    } else if (!strcmp(a, "-pc_type") && v) {
      if (!strcmp(v, "none")) o->pc_type = PB_PC_NONE;
      else if (!strcmp(v, "jacobi")) o->pc_type = PB_PC_JACOBI;
      else if (!strcmp(v, "sor")) o->pc_type = PB_PC_SOR;
      else if (!strcmp(v, "mg") || !strcmp(v, "gamg")) o->pc_type = PB_PC_MG;
      else if (!strcmp(v, "fft")) o->pc_type = PB_PC_FFT;
      else return set_error(PB_ERR_UNSUPPORTED, "-pc_type %s", v);
      ++i;
    } else if (!strcmp(a, "-ksp_rtol") && v) {
      o->rtol = atof(v);
      ++i;
    } else if (!strcmp(a, "-ksp_atol") && v) {
      o->atol = atof(v);
      ++i;
    } else if (!strcmp(a, "-ksp_divtol") && v) {
      o->dtol = atof(v);
      ++i;
    } else if (!strcmp(a, "-ksp_max_it") && v) {
      o->max_it = atoll(v);
      ++i;
    } else if (!strcmp(a, "-pc_mg_levels") && v) {
      o->mg_levels = atoi(v);
      ++i;
    } else if ((!strcmp(a, "-pc_mg_coarse_its") || !strcmp(a, "-mg_coarse_ksp_max_it")) && v) {
      o->mg_coarse_its = atoi(v);
      ++i;
    } else if (!strcmp(a, "-pc_sor_omega") && v) {
      o->sor_omega = atof(v);
      ++i;
    } else if (!strcmp(a, "-ksp_cg_single_reduction")) {
      flag(&o->cg_single_reduction);
    } else if (!strcmp(a, "-ksp_initial_guess_nonzero")) {
      flag(&o->initial_guess_nonzero);
    } else if (!strcmp(a, "-ksp_converged_use_initial_residual_norm")) {
      flag(&o->converged_use_initial_residual_norm);
    } else if (!strcmp(a, "-ksp_converged_use_min_initial_residual_norm")) {
      flag(&o->converged_use_min_initial_residual_norm);
    } else if (!strcmp(a, "-ksp_guess_type") && v) {
      if (!strcmp(v, "none")) o->guess_type = PB_GUESS_NONE;
      else if (!strcmp(v, "fischer")) o->guess_type = PB_GUESS_FISCHER;
      else return set_error(PB_ERR_UNSUPPORTED, "-ksp_guess_type %s: only none, fischer", v);
      ++i;
    } else if (!strcmp(a, "-ksp_guess_fischer_model") && v && v[0] >= '0' && v[0] <= '9') {
      // <model>[,<maxl>] (PetscOptionsIntArray: a bare model keeps maxl)
      const int model = atoi(v);
      const char* comma = strchr(v, ',');
      const int maxl = comma ? atoi(comma + 1) : o->guess_fischer_maxl;
      PB_TRY(check_guess_opts(model, maxl));
      o->guess_fischer_model = model;
      o->guess_fischer_maxl = maxl;
      ++i;
    } else if (!strcmp(a, "-ksp_monitor")) {
      o->monitor = 1;
    } else if (!strcmp(a, "-ksp_converged_reason")) {
      o->converged_reason = 1;
    }
  }
  // the -ksp_chebyshev_* options: their errors are reported here too (the values belong to
  // pb_ksp_chebyshev_opts_parse)
  pb_ksp_chebyshev_opts co;
  pb_ksp_chebyshev_opts_default(&co);
  PB_TRY(pb_ksp_chebyshev_opts_parse(&co, argc, argv));
  // likewise the -mg_levels_* options (pb_pc_mg_opts_parse keeps the values)
  pb_pc_mg_opts mo;
  pb_pc_mg_opts_default(&mo);
  PB_TRY(pb_pc_mg_opts_parse(&mo, argc, argv));
  return check_ref_norm_opts(o);
}

// ---------------------------------------------------------------------------------------------
// KSP
// ---------------------------------------------------------------------------------------------
int pb_ksp_create(pb_op* A, pb_op* P, const pb_ksp_opts* opts, pb_ksp** out) {
  PB_CHECK_ARG(A && out, "bad ksp args");
  if (!P) P = A;
  PB_CHECK_ARG(A->grid == P->grid, "A and P on different grids");
  pb_ksp* k = new pb_ksp();
  k->A = A;
  k->P = P;
  // every failure below releases what was built so far (pb_ksp_destroy takes a partial KSP:
  // each field, the PC objects and the state are freed only if they exist)
  auto fail = [k](int rc) {
    const std::string msg = pb_last_error();
    pb_ksp_destroy(k);
    return set_error(rc, "%s", msg.c_str());
  };
  if (opts) k->opts = *opts;
  else pb_ksp_opts_default(&k->opts);
  if (k->opts.check_every < 1) k->opts.check_every = 8;
  if (check_ref_norm_opts(&k->opts) != PB_OK) return fail(PB_ERR_ARG);
  const int kt = k->opts.ksp_type;
  if (kt != PB_KSP_CG && kt != PB_KSP_PREONLY && kt != PB_KSP_RICHARDSON &&
      kt != PB_KSP_CHEBYSHEV)
    return fail(set_error(PB_ERR_UNSUPPORTED, "unknown ksp_type %d", kt));
  pb_ksp_chebyshev_opts_default(&k->copts);
  pb_pc_mg_opts_default(&k->mgopts);
  if (!std::isfinite(k->opts.richardson_scale))
    return fail(set_error(PB_ERR_ARG, "richardson_scale is not finite"));
  if (kt == PB_KSP_PREONLY &&
      (k->opts.initial_guess_nonzero || k->opts.guess_type != PB_GUESS_NONE))
    return fail(set_error(PB_ERR_ARG,
                          "preonly doesn't make sense with a nonzero initial guess; you probably "
                          "want richardson"));
  // SOR / MG / FFT iterations are expensive and few: poll the device flag more often -- every
  // iteration with the spectral PC (1-3 iterations per solve: an iteration enqueued ahead of the
  // poll costs its skipped launches, ~0.15 ms of a 512^3 config-5 solve, more than the idle
  // stream time of waiting for each iteration)
  // (only clamped down: a caller's explicit smaller interval stands -- ADVICE r03)
  if ((k->opts.pc_type == PB_PC_SOR || k->opts.pc_type == PB_PC_MG) && k->opts.check_every > 2)
    k->opts.check_every = 2;
  if (k->opts.pc_type == PB_PC_FFT)
    k->opts.check_every = 1;
  const int pc = k->opts.pc_type;
  if (pc != PB_PC_NONE && pc != PB_PC_JACOBI && pc != PB_PC_SOR && pc != PB_PC_MG &&
      pc != PB_PC_FFT)
    return fail(set_error(PB_ERR_UNSUPPORTED, "unknown pc_type %d", pc));
  pb_grid* g = A->grid;
  const size_t vb = (size_t)g->nlocal * sizeof(double);
  if (pc == PB_PC_SOR || pc == PB_PC_MG) {
    // the smoother / coarse operators are the 7-point P (src/coefficients.f90 star)
    if (P->kind == PB_OP_COMPACT)
      return fail(set_error(PB_ERR_UNSUPPORTED, "SOR / MG preconditioning needs a 7-point P"));
    const int rc = mg_create(g, P->deltas, pc, k->opts.mg_levels, k->opts.mg_coarse_its,
                             k->opts.sor_omega, &k->mg);
    if (rc != PB_OK) return fail(rc);
  }
  if (pc == PB_PC_FFT) {
    // the symbol of P: the compact operator (config 5: A = P = compact) or the 7-point star
    const int rc = fftpc_create(g, P->deltas, P->kind == PB_OP_COMPACT, &k->fft);
    if (rc != PB_OK) return fail(rc);
  }
  if (field_alloc(&k->r, vb) != hipSuccess || field_alloc(&k->pb[0], vb) != hipSuccess ||
      field_alloc(&k->pb[1], vb) != hipSuccess)
    return fail(set_error(PB_ERR_ALLOC, "KSP work vectors: out of device memory"));
  if (!fused_kind(A->kind) || k->stored_z()) {
    if (field_alloc(&k->w, vb) != hipSuccess || field_alloc(&k->z, vb) != hipSuccess)
      return fail(set_error(PB_ERR_ALLOC, "KSP work vectors: out of device memory"));
  }
  // [1]: the folded iteration's second slot; behind them two doubles: the sums of M^-1 b a
  // stored-z setup from a nonzero guess takes for its reference norm (guess_bsums)
  if (hipMalloc(&k->d_st, 2 * sizeof(CgState) + 2 * sizeof(double)) != hipSuccess)
    return fail(set_error(PB_ERR_ALLOC, "KSP state: out of device memory"));
  if (k->opts.guess_type != PB_GUESS_NONE) {
    if (k->opts.guess_type != PB_GUESS_FISCHER)
      return fail(set_error(PB_ERR_UNSUPPORTED, "unknown guess_type %d", k->opts.guess_type));
    const int rc = check_guess_opts(k->opts.guess_fischer_model, k->opts.guess_fischer_maxl);
    if (rc != PB_OK) return fail(rc);
    // 2 maxl + 1 fields: xt[maxl], bt[maxl] and the last formed guess
    pb_ksp::Fischer* f = k->fg = new pb_ksp::Fischer();
    f->maxl = k->opts.guess_fischer_maxl;
    f->xt.assign(f->maxl, nullptr);
    f->bt.assign(f->maxl, nullptr);
    bool ok = field_alloc(&f->guess, vb) == hipSuccess;
    for (int i = 0; ok && i < f->maxl; ++i)
      ok = field_alloc(&f->xt[i], vb) == hipSuccess && field_alloc(&f->bt[i], vb) == hipSuccess;
    if (!ok)
      return fail(set_error(PB_ERR_ALLOC, "projected guess: %d vectors: out of device memory",
                            2 * f->maxl + 1));
    if (hipMalloc(&f->d_coef, (kMaxVecs + 1) * sizeof(double)) != hipSuccess)
      return fail(set_error(PB_ERR_ALLOC, "projected guess state: out of device memory"));
    if (hipMemsetAsync(f->guess, 0, vb, g->ctx->stream) != hipSuccess)
      return fail(set_error(PB_ERR_HIP, "projected guess: clearing the stored guess failed"));
  }
  *out = k;
  return PB_OK;
}

static int ensure_done_cap(pb_ksp* k, int64_t need) {
  if (need <= k->done_cap) return PB_OK;
  int64_t cap = need < 1024 ? 1024 : need * 2;
  int* h = nullptr;
  PB_HIP(hipHostMalloc(&h, (size_t)cap * sizeof(int), hipHostMallocMapped));
  memset(h, 0, (size_t)cap * sizeof(int));
  if (k->h_done) {
    PB_TRY(wait_stream(k->A->grid->ctx, k->A->grid->ctx->stream, "KSP flag buffer"));
    memcpy(h, k->h_done, (size_t)k->done_cap * sizeof(int));
    (void)hipHostFree(k->h_done);
  }
  k->h_done = h;
  PB_HIP(hipHostGetDevicePointer((void**)&k->h_done_dev, h, 0));
  k->done_cap = cap;
  return PB_OK;
}

// z = M^-1 r for the stored-z preconditioners; *np = residual-sum partial blocks written by the
// PC itself (MG's last sweep), 0 if the caller must take the sums
static int pc_apply_dev(pb_ksp* k, const double* r, double* z, const int* skip, int* np) {
  *np = 0;
  if (k->fft) return fftpc_apply(k->fft, r, z, skip, k->d_st, np);
  return mg_apply(k->mg, r, z, skip, k->d_st, np);
}

// Setup from a nonzero initial guess (-ksp_initial_guess_nonzero): r = b - A x0, p = 0, z0 and
// stage 0 with KSPConvergedDefault's reference norm; x0 is read only
static int guess_setup(pb_ksp* k, const double* b, const double* x0, double dinv) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const int ref = k->opts.converged_use_initial_residual_norm
                      ? 1
                      : (k->opts.converged_use_min_initial_residual_norm ? 2 : 0);
  int np = 0;
  if (k->stored_z()) {
    const double* bsums = nullptr;
    if (ref != 1) {
      // the reference norm ||N(M^-1 b)||: one more PC application, its sums kept aside
      PB_TRY(pc_apply_dev(k, b, k->z, nullptr, &np));
      if (np == 0) PB_TRY(launch_cg_pc_sums(g, k->z, b, k->d_st, &np));
      PB_TRY(cg_reduce_allreduce(ctx, ctx->d_partials, np, 4));
      PB_HIP(hipMemcpyAsync(k->guess_bsums(), ctx->d_scalars, 2 * sizeof(double),
                            hipMemcpyDeviceToDevice, ctx->stream));
      bsums = k->guess_bsums();
    }
    PB_TRY(op_apply_raw(k->A, x0, k->w));
    PB_TRY(launch_cg_guess_resid(g, b, k->w, k->r, k->pb[0], dinv, nullptr));
    PB_TRY(pc_apply_dev(k, k->r, k->z, nullptr, &np));
    if (np == 0) PB_TRY(launch_cg_pc_sums(g, k->z, k->r, k->d_st, &np));
    return cg_finalize_guess(ctx, np, 4, bsums, ref, k->d_st, k->d_hist, k->h_done_dev);
  }
  if (!fused_kind(k->A->kind)) {  // compact / assembled A with Jacobi / no PC
    PB_TRY(op_apply_raw(k->A, x0, k->w));
    PB_TRY(launch_cg_guess_resid(g, b, k->w, k->r, k->pb[0], dinv, &np));
    return cg_finalize_guess(ctx, np, 6, nullptr, ref, k->d_st, k->d_hist, k->h_done_dev);
  }
  // the fused pass; split grids exchange x0's boundary planes under the interior planes
  Star s{k->A->cx, k->A->cy, k->A->cz, k->A->cc};
  StencilPlanes gp;
  const double* hi = x0 + (g->nzl - 1) * g->plane;
  if (!ctx->split) {
    gp.ghost_lo = hi;  // periodic wrap: no copy
    gp.ghost_hi = x0;
    PB_TRY(launch_cg_guess_init(g, s, x0, b, k->r, k->pb[0], gp, dinv, PLANES_ALL, 0, &np));
  } else {
    gp.ghost_lo = g->ghost_lo;
    gp.ghost_hi = g->ghost_hi;
    if (g->nzl < 3) {
      PB_TRY(halo_exchange(g, x0, hi));
      PB_TRY(launch_cg_guess_init(g, s, x0, b, k->r, k->pb[0], gp, dinv, PLANES_ALL, 0, &np));
    } else {
      int nb1 = 0, nb2 = 0;
      ScopedTimer tm(ctx, "cg_init_guess");
      PB_TRY(halo_begin(g, x0, hi));
      PB_TRY(launch_cg_guess_init(g, s, x0, b, k->r, k->pb[0], gp, dinv, PLANES_INTERIOR, 0,
                                  &nb1));
      PB_TRY(halo_end(g));
      PB_TRY(launch_cg_guess_init(g, s, x0, b, k->r, k->pb[0], gp, dinv, PLANES_BOUNDARY, nb1,
                                  &nb2));
      np = nb1 + nb2;
    }
  }
  PB_TRY(cg_finalize_guess(ctx, np, 6, nullptr, ref, k->d_st, k->d_hist, k->h_done_dev));
  if (k->sr) {
    // KSPSolve_CG_SingleReduction's setup as from a zero guess: pass S over r0
    PB_TRY(sr_pass_s(k, k->r, k->d_st, &np, 0));
    PB_TRY(cg_sr_finalize(ctx, sr_region(ctx, 0), np, k->d_st, k->d_hist, k->h_done_dev, -1,
                          true));
  }
  return PB_OK;
}

// ---------------------------------------------------------------------------------------------
// Stationary solves: -ksp_type richardson, chebyshev, preonly
// ---------------------------------------------------------------------------------------------
// the 7-point operator on one rank: the engine pass reads the periodic wrap planes in place
static bool rich_engine(const pb_ksp* k) {
  return fused_kind(k->A->kind) && !k->A->grid->ctx->split;
}

// r_out = b - A x (+ the sums of dinv r_out - mean with Jacobi / no PC: *np blocks, else 0)
static int rich_residual(pb_ksp* k, const double* x, double* r_out, bool skip, int* np) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const bool sums = !k->stored_z();
  *np = 0;
  if (rich_engine(k)) {
    Star s{k->A->cx, k->A->cy, k->A->cz, k->A->cc};
    StencilPlanes gp;
    gp.ghost_lo = gp.ghost_hi = nullptr;
    gp.wrap = true;
    return launch_rich_update(g, s, x, nullptr, k->b->d, nullptr, r_out, gp, k->d_st, 0.0, sums,
                              skip, np);
  }
  {
    OpApplySkip guard(ctx, skip ? &k->d_st->done : nullptr);
    PB_TRY(op_apply_raw(k->A, x, k->w));
  }
  return launch_rich_resid(g, k->b->d, k->w, r_out, k->d_st, skip, sums ? np : nullptr);
}

// z = M^-1 r of a stored-z PC with the sums of z - mean (4 wide: the PC's own, or CG's sum kernel)
static int rich_pc(pb_ksp* k, const double* r, const int* skip, int* np) {
  PB_TRY(pc_apply_dev(k, r, k->z, skip, np));
  if (*np == 0) PB_TRY(launch_cg_pc_sums(k->A->grid, k->z, r, k->d_st, np));
  return PB_OK;
}

// ---------------------------------------------------------------------------------------------
// Chebyshev's interval
// ---------------------------------------------------------------------------------------------
// z = N(M^-1 r) with the KSP's PC and null space, host-driven (setup cost, not a hot path)
static int cheb_pc_n(pb_ksp* k, const double* r, double* z) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  if (k->mg) {
    PB_TRY(mg_apply(k->mg, r, z));
  } else if (k->fft) {
    PB_TRY(fftpc_apply(k->fft, r, z));
  } else {
    PB_HIP(hipMemcpyAsync(z, r, (size_t)g->nlocal * sizeof(double), hipMemcpyDeviceToDevice,
                          ctx->stream));
    if (k->opts.pc_type == PB_PC_JACOBI)
      PB_TRY(vec_update(ctx, 2, z, nullptr, g->nlocal, 1.0 / k->P->cc));
  }
  if (!k->opts.nullspace) return PB_OK;
  int np = 0;
  PB_TRY(launch_pre_scale_sum(g, z, nullptr, 1.0, &np));
  PB_TRY(rich_reduce(ctx, np, 2, nullptr));
  return launch_pre_shift(g, z, (double)(g->n[0] * g->n[1] * g->n[2]));
}

// The extreme eigenvalues of M^-1 A on the range of N from `steps` steps of preconditioned
// CG-Lanczos (poissbox_gpu.h, pb_ksp_chebyshev_get_eigenvalues). Uses r, pb[0], pb[1] and x2:
// nothing of a solve may be in them. *n_out = the steps the tridiagonal holds (0: none)
static int cheb_lanczos(pb_ksp* k, double* lo, double* hi, int* n_out) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const int64_t n = g->nlocal;
  const size_t vb = (size_t)n * sizeof(double);
  if (!k->x2 && field_alloc(&k->x2, vb) != hipSuccess)
    return set_error(PB_ERR_ALLOC, "Chebyshev solution buffer: out of device memory");
  double *r = k->r, *p = k->pb[0], *w = k->pb[1], *z = k->x2;
  const int steps = k->copts.esteig_steps;
  double diag[64], off[64], alpha_prev = 0.0, beta_prev = 0.0;
  int m = 0;
  PB_TRY(vec_random(ctx, r, n, PB_CHEBYSHEV_ESTEIG_SEED, g->k0 * g->plane));
  if (k->opts.nullspace) {  // r_0 = N(v): r then stays in A's range
    int np = 0;
    PB_TRY(launch_pre_scale_sum(g, r, nullptr, 1.0, &np));
    PB_TRY(rich_reduce(ctx, np, 2, nullptr));
    PB_TRY(launch_pre_shift(g, r, (double)(g->n[0] * g->n[1] * g->n[2])));
  }
  PB_TRY(cheb_pc_n(k, r, z));
  PB_HIP(hipMemcpyAsync(p, z, vb, hipMemcpyDeviceToDevice, ctx->stream));
  double rz = 0.0, rz0 = 0.0;
  PB_TRY(vec_reduce(ctx, 1, r, z, n, &rz));
  rz0 = rz;
  for (int j = 0; j < steps; ++j) {
    double pw = 0.0;
    PB_TRY(op_apply_raw(k->A, p, w));
    PB_TRY(vec_reduce(ctx, 1, p, w, n, &pw));
    const double alpha = rz / pw;
    if (!std::isfinite(alpha) || alpha == 0.0) break;
    diag[j] = 1.0 / alpha + (j > 0 ? beta_prev / alpha_prev : 0.0);
    m = j + 1;
    if (m == steps) break;
    PB_TRY(vec_update(ctx, 0, r, w, n, -alpha));
    PB_TRY(cheb_pc_n(k, r, z));
    double rz_new = 0.0;
    PB_TRY(vec_reduce(ctx, 1, r, z, n, &rz_new));
    const double beta = rz_new / rz;
    // the Krylov space is exhausted (-pc_type fft with A = P after one step), or the PC is not
    // definite on it
    if (!std::isfinite(beta) || beta <= 0.0 || std::fabs(rz_new) <= 1e-24 * std::fabs(rz0)) break;
    off[j] = std::sqrt(beta) / alpha;
    PB_TRY(vec_update(ctx, 1, p, z, n, beta));
    alpha_prev = alpha;
    beta_prev = beta;
    rz = rz_new;
  }
  *n_out = m;
  if (m == 0) return PB_OK;
  return pb_tridiag_extreme_eigenvalues(m, diag, off, lo, hi);
}

// the bounds of the next solve into k->cheb_*: the caller's, or the estimate (run once per pair of
// deltas) through the transform; an invalid pair is PB_ERR_ARG and leaves the KSP usable
static int cheb_bounds(pb_ksp* k) {
  const pb_ksp_chebyshev_opts& o = k->copts;
  double emin = o.emin, emax = o.emax;
  const bool given = emin != 0.0 || emax != 0.0;
  double dl[6];
  for (int d = 0; d < 3; ++d) {
    dl[d] = k->A->deltas[d];
    dl[3 + d] = k->P->deltas[d];
  }
  if (given) {
    PB_TRY(check_cheb_pair(emin, emax, "chebyshev eigenvalues"));
    k->cheb_state = 1;
  } else if (k->cheb_state != 2 || memcmp(dl, k->cheb_deltas, sizeof(dl)) != 0) {
    if (k->begun) return set_error(PB_ERR_STATE, "Chebyshev eigenvalue estimate inside a solve");
    double lo = 0.0, hi = 0.0;
    int m = 0;
    k->cheb_state = 0;
    PB_TRY(cheb_lanczos(k, &lo, &hi, &m));
    if (m == 0)
      return set_error(PB_ERR_ARG, "Chebyshev eigenvalue estimate: the Lanczos process broke down "
                                   "at its first step");
    emin = o.esteig[0] * lo + o.esteig[1] * hi;
    emax = o.esteig[2] * lo + o.esteig[3] * hi;
    if (check_cheb_pair(emin, emax, "estimate") != PB_OK)
      return set_error(PB_ERR_ARG,
                       "Chebyshev eigenvalue estimate: extremes %g, %g transform to emin %g, emax "
                       "%g, no valid bounds (a negative spectrum, as with -pc_type none, needs "
                       "-ksp_chebyshev_esteig weights that keep emax > emin, or explicit "
                       "-ksp_chebyshev_eigenvalues)", lo, hi, emin, emax);
    memcpy(k->cheb_deltas, dl, sizeof(dl));
    k->cheb_state = 2;
  } else {
    emin = k->cheb_emin;
    emax = k->cheb_emax;
  }
  k->cheb_emin = emin;
  k->cheb_emax = emax;
  // KSPSolve_Chebyshev's quantities
  k->cheb_scale = 2.0 / (emax + emin);
  const double alpha = 1.0 - k->cheb_scale * emin;
  k->cheb_mu = 1.0 / alpha;
  k->cheb_omegaprod = 2.0 / alpha;
  return PB_OK;
}

// KSPSolve_Richardson's setup: r_0 = b (read in place), x_0 = 0, or r_0 = b - A x_0 from a nonzero
// guess with CG's reference-norm rules; z_0, its norm, history[0] and the first test
static int rich_begin(pb_ksp* k, const pb_vec* b, pb_vec* x) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const size_t vb = (size_t)g->nlocal * sizeof(double);
  // b is read by every update (r = b - A x) while x is written
  PB_CHECK_ARG(b != x, k->cheb() ? "chebyshev needs distinct b and x"
                                   : "richardson needs distinct b and x");
  k->sr = false;
  k->pst = false;
  k->lazy0 = false;
  k->defer_x = 0;
  if (!k->x2 && field_alloc(&k->x2, vb) != hipSuccess)
    return set_error(PB_ERR_ALLOC, "Richardson solution buffer: out of device memory");
  if (k->cheb() && !k->x3 && field_alloc(&k->x3, vb) != hipSuccess)
    return set_error(PB_ERR_ALLOC, "Chebyshev solution buffer: out of device memory");
  if (!k->stored_z() && !k->r2 && field_alloc(&k->r2, vb) != hipSuccess)
    return set_error(PB_ERR_ALLOC, "Richardson residual buffer: out of device memory");
  if (!rich_engine(k) && !k->w && field_alloc(&k->w, vb) != hipSuccess)
    return set_error(PB_ERR_ALLOC, "Richardson work vector: out of device memory");
  // (the eigenvalue estimate, when it has to run, uses the work vectors: before anything of
  // this solve is in them; invalid bounds leave the KSP as it was)
  if (k->cheb()) PB_TRY(cheb_bounds(k));
  const double cmu = k->cheb() ? k->cheb_mu : 0.0, cop = k->cheb() ? k->cheb_omegaprod : 0.0;
  k->b = b;
  k->x = x;
  k->rich_guess = k->opts.initial_guess_nonzero != 0;
  const int width = k->stored_z() ? 4 : 2;
  int np = 0;
  if (!k->rich_guess) {
    PB_HIP(hipMemsetAsync(x->d, 0, vb, ctx->stream));
    if (k->stored_z()) PB_TRY(rich_pc(k, b->d, nullptr, &np));
    else PB_TRY(launch_rich_sums(g, b->d, k->d_st, &np));
    return rich_finalize(ctx, np, width, nullptr, 3, k->d_st, k->d_hist, k->h_done_dev, -1, cmu,
                         cop);
  }
  PB_TRY(check_ref_norm_opts(&k->opts));
  const int ref = k->opts.converged_use_initial_residual_norm
                      ? 1
                      : (k->opts.converged_use_min_initial_residual_norm ? 2 : 0);
  const double* bsums = nullptr;
  if (ref != 1) {  // the reference norm ||N(M^-1 b)||: the sums of M^-1 b kept aside
    if (k->stored_z()) PB_TRY(rich_pc(k, b->d, nullptr, &np));
    else PB_TRY(launch_rich_sums(g, b->d, k->d_st, &np));
    PB_TRY(rich_reduce(ctx, np, width, k->guess_bsums()));
    bsums = k->guess_bsums();
  }
  PB_TRY(rich_residual(k, x->d, k->r, false, &np));
  if (k->stored_z()) PB_TRY(rich_pc(k, k->r, nullptr, &np));
  return rich_finalize(ctx, np, width, bsums, ref, k->d_st, k->d_hist, k->h_done_dev, -1, cmu,
                       cop);
}

// one update: x_new = x + scale (M^-1 r - mean), r_new = b - A x_new, z_new and its sums, the
// norm and the test. On the 7-point operator (one rank) the first two are one engine pass
// (tuning rich_fused = 0: a vector kernel and the engine's residual pass, bit-identical)
static int enqueue_rich_iteration(pb_ksp* k) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const int64_t i = k->host_iter;
  const double* xin = k->xbuf(i);
  double* xout = k->xbuf(i + 1);
  const double* q = k->stored_z() ? k->z : k->rich_rbuf(i);
  double* r_out = k->stored_z() ? k->r : (((i + 1) & 1) ? k->r2 : k->r);
  // Chebyshev: update 0 is Richardson's with scale = 2 / (emax + emin); update i >= 1 reads
  // y_(i-1) too (host_iter is the device's update count while the state is not done, and every
  // launch of a done state exits at entry)
  const bool cheb = k->cheb();
  const double scale = cheb ? k->cheb_scale : k->opts.richardson_scale;
  const double* xm1 = cheb && i >= 1 ? k->xbuf(i - 1) : nullptr;
  const bool fused = rich_engine(k) && (cheb ? tune("cheb_fused", 1) : tune("rich_fused", 1)) != 0;
  int np = 0;
  if (fused) {
    Star s{k->A->cx, k->A->cy, k->A->cz, k->A->cc};
    StencilPlanes gp;
    gp.ghost_lo = gp.ghost_hi = nullptr;
    gp.wrap = true;
    if (xm1)
      PB_TRY(launch_cheb_update(g, s, xin, xm1, q, k->b->d, xout, r_out, gp, k->d_st, scale,
                                !k->stored_z(), &np));
    else
      PB_TRY(launch_rich_update(g, s, xin, q, k->b->d, xout, r_out, gp, k->d_st, scale,
                                !k->stored_z(), true, &np));
  } else {
    if (xm1) PB_TRY(launch_cheb_x(g, xin, xm1, q, xout, k->d_st, scale));
    else PB_TRY(launch_rich_x(g, xin, q, xout, k->d_st, scale));
    PB_TRY(rich_residual(k, xout, r_out, true, &np));
  }
  if (k->stored_z()) PB_TRY(rich_pc(k, r_out, &k->d_st->done, &np));
  return rich_finalize(ctx, np, k->stored_z() ? 4 : 2, nullptr, 0, k->d_st, k->d_hist,
                       k->h_done_dev, i, cheb ? k->cheb_mu : 0.0, cheb ? k->cheb_omegaprod : 0.0);
}

// KSPSolve_PREONLY: x = N(M^-1 b). No norm, no reduction but the mean's, no NaN check. The
// spectral PC zeroes mode 0 itself: its result keeps its rounding-level mean (poissbox_gpu.h)
static int solve_preonly(pb_ksp* k, const pb_vec* b, pb_vec* x, pb_ksp_result* res) {
  PB_CHECK_ARG(k && b && x, "bad solve args");
  pb_grid* g = k->A->grid;
  PB_CHECK_ARG(b->grid == g && x->grid == g, "vector/operator grid mismatch");
  PB_CHECK_ARG(b != x, "preonly needs distinct b and x");
  pb_ctx* ctx = g->ctx;
  int np = 0;
  if (k->fft) {
    PB_TRY(fftpc_apply(k->fft, b->d, x->d));
  } else {
    if (k->mg) {
      PB_TRY(mg_apply(k->mg, b->d, x->d));
      if (k->opts.nullspace) PB_TRY(launch_pre_scale_sum(g, x->d, nullptr, 1.0, &np));
    } else {
      const double dinv = k->opts.pc_type == PB_PC_JACOBI ? 1.0 / k->P->cc : 1.0;
      PB_TRY(launch_pre_scale_sum(g, b->d, x->d, dinv, &np));
    }
    if (k->opts.nullspace) {
      PB_TRY(rich_reduce(ctx, np, 2, nullptr));
      PB_TRY(launch_pre_shift(g, x->d, (double)(g->n[0] * g->n[1] * g->n[2])));
    }
  }
  PB_SYNC(ctx, "pb_ksp_solve (preonly)");
  if (res) {
    res->reason = PB_KSP_CONVERGED_ITS;
    res->its = 1;
    res->rnorm = 0.0;
    res->rnorm0 = 0.0;
    res->nhist = 0;
  }
  if (ctx->rank == 0 && k->opts.converged_reason) {
    printf("Linear solve converged due to CONVERGED_ITS iterations 1\n");
    fflush(stdout);
  }
  return PB_OK;
}

static int preonly_split_form(const pb_ksp* k) {
  if (k && k->opts.ksp_type == PB_KSP_PREONLY)
    return set_error(PB_ERR_UNSUPPORTED,
                     "-ksp_type preonly has no split form: use pb_ksp_solve or pb_solve");
  return PB_OK;
}

int pb_ksp_begin(pb_ksp* k, const pb_vec* b, pb_vec* x) {
  PB_CHECK_ARG(k && b && x, "bad begin args");
  PB_TRY(preonly_split_form(k));
  pb_grid* g = k->A->grid;
  PB_CHECK_ARG(b->grid == g && x->grid == g, "vector/operator grid mismatch");
  pb_ctx* ctx = g->ctx;
  // history buffer: max_it + 1 entries
  const int64_t nh = k->opts.max_it + 1;
  if (nh > k->nhist) {
    if (k->d_hist) (void)hipFree(k->d_hist);
    PB_HIP(hipMalloc(&k->d_hist, (size_t)nh * sizeof(double)));
    k->nhist = nh;
  }
  PB_TRY(ensure_done_cap(k, 1024));
  memset(k->h_done, 0, (size_t)k->done_cap * sizeof(int));
  CgState st;
  memset(&st, 0, sizeof(st));
  st.rtol = k->opts.rtol;
  st.atol = k->opts.atol;
  st.dtol = k->opts.dtol;
  st.max_it = k->opts.max_it;
  st.nhist = k->nhist;
  st.pc = k->opts.pc_type;
  st.nullspace = k->opts.nullspace;
  // PCJacobi stores the reciprocal of diag(P) (src/coefficients.f90:44-46 centre coefficient);
  // with SOR / MG the sums are taken over z = M^-1 r itself (dinv = 1)
  st.dinv = k->opts.pc_type == PB_PC_JACOBI ? 1.0 / k->P->cc : 1.0;
  st.ntot = (double)(g->n[0] * g->n[1] * g->n[2]);
  if (k->rich()) {
    PB_HIP(hipMemcpyAsync(k->d_st, &st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
    PB_TRY(rich_begin(k, b, x));
    PB_SYNC(ctx, "pb_ksp_begin");
    k->host_iter = 0;
    k->stopped = k->h_done[0] != 0;
    k->begun = true;
    return PB_OK;
  }
  // depth 4 (default): 58 instead of 60 B/DoF per iteration, measured 3 % faster at 512^3
  // (profiles/r01/ab_defer_x.txt); the x update sums four alpha p terms instead of adding them
  // one per iteration (rounding-level difference in x only: the history is unaffected)
  const int dx = tune("cg_defer_x", 4);
  k->defer_x = dx == 0 ? 0 : (dx == 2 ? 2 : 4);
  if (!fused_kind(k->A->kind)) k->defer_x = 0;  // generic path: x every iteration
  st.defer_x = k->defer_x;
  // p stored by pass B (default): pass A read-only, 56 instead of 58 B/DoF per iteration and
  // the passes closer to their patterns' rates -- 1.29 vs 1.36 ms/iteration at 512^3 on one box
  // (profiles/r02/ab_pst_defer_512.jsonl); with a stored-z PC pass A stores p (the r01 split)
  k->pst = fused_kind(k->A->kind) && !k->stored_z();
  // single reduction: the fused operator with Jacobi / no PC (pass P forms p from r on load);
  // elsewhere the KSPSolve_CG iteration runs (equal in exact arithmetic; pb_ksp_opts)
  k->sr = k->opts.cg_single_reduction != 0 && fused_kind(k->A->kind) && !k->stored_z();
  st.sr = k->sr ? 1 : 0;
  if (k->sr) k->pst = true;  // r ping-pongs between r and r2 (pass P reads r_i, writes r_i+1)
  if (k->pst && !k->r2) {
    const size_t vb = (size_t)g->nlocal * sizeof(double);
    if (field_alloc(&k->r2, vb) != hipSuccess)
      return set_error(PB_ERR_ALLOC, "CG residual buffer: out of device memory");
  }
  if (k->defer_x == 4 && !k->pb[2]) {
    const size_t vb = (size_t)g->nlocal * sizeof(double);
    if (field_alloc(&k->pb[2], vb) != hipSuccess || field_alloc(&k->pb[3], vb) != hipSuccess)
      return set_error(PB_ERR_ALLOC, "CG direction buffers: out of device memory");
  }
  PB_HIP(hipMemcpyAsync(k->d_st, &st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
  // stored z with an operator without a stencil engine (compact A): r0 = b, x0 = 0 and p0 = 0 are
  // implicit -- the setup reads b in place of r, and the first iteration writes p = z, x = alpha p
  // and r = b - alpha w without reading them (three vector passes fewer)
  k->lazy0 = k->stored_z() && !fused_kind(k->A->kind) && tune("ksp_lazy0", 1) != 0;
  if (k->opts.initial_guess_nonzero) {
    // (read on every begin: a reused KSP warm-starts each solve of a time loop from its x)
    PB_CHECK_ARG(b != x, "a nonzero initial guess needs distinct b and x");
    PB_TRY(check_ref_norm_opts(&k->opts));
    k->lazy0 = false;  // x0 is not 0: every update accumulates onto it, none may overwrite
    PB_TRY(guess_setup(k, b->d, x->d, st.dinv));
  } else if (k->stored_z()) {
    // r = b, x = 0, p = 0; z = M^-1 r; sums of z (KSPSolve_CG setup, PC_LEFT)
    const size_t vb = (size_t)g->nlocal * sizeof(double);
    const double* r0 = k->lazy0 ? b->d : k->r;
    if (!k->lazy0) {
      PB_HIP(hipMemcpyAsync(k->r, b->d, vb, hipMemcpyDeviceToDevice, ctx->stream));
      PB_HIP(hipMemsetAsync(x->d, 0, vb, ctx->stream));
      PB_HIP(hipMemsetAsync(k->pb[0], 0, vb, ctx->stream));
    }
    int np = 0;
    PB_TRY(pc_apply_dev(k, r0, k->z, nullptr, &np));
    if (np == 0) PB_TRY(launch_cg_pc_sums(g, k->z, r0, k->d_st, &np));
    PB_TRY(cg_finalize_init(ctx, np, k->d_st, k->d_hist, k->h_done_dev));
  } else {
    PB_TRY(launch_cg_init(g, b->d, x->d, k->r, k->pb[0], k->d_st, st.dinv, k->d_hist,
                          k->h_done_dev));
    if (k->sr) {
      // KSPSolve_CG_SingleReduction's setup: S = A z, delta = z'S (pass S over r0 = b)
      int np = 0;
      PB_TRY(sr_pass_s(k, k->r, k->d_st, &np, 0));
      PB_TRY(cg_sr_finalize(ctx, sr_region(ctx, 0), np, k->d_st, k->d_hist, k->h_done_dev, -1,
                            true));
    }
  }
  PB_SYNC(ctx, "pb_ksp_begin");
  k->b = b;
  k->x = x;
  k->host_iter = 0;
  k->stopped = k->h_done[0] != 0;
  k->begun = true;
  return PB_OK;
}

// Unfused iteration for operators without a stencil engine (PB_OP_COMPACT): one vector pass
// for p, the operator, a dot pass, an x/r pass (same device scalar logic as the fused path).
static int enqueue_generic_iteration(pb_ksp* k) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  double* p = k->pb[0];
  int np = 0;
  PB_TRY(launch_cg_generic_p(g, k->r, p, k->d_st));
  {
    OpApplySkip guard(ctx, &k->d_st->done);
    PB_TRY(op_apply_raw(k->A, p, k->w));
  }
  PB_TRY(launch_cg_generic_dot(g, p, k->w, k->d_st, &np));
  PB_TRY(cg_finalize_pass_a(ctx, np, k->d_st));
  PB_TRY(launch_cg_generic_xr(g, p, k->w, k->x->d, k->r, k->d_st, &np));
  return cg_finalize_stage2(ctx, np, k->d_st, k->d_hist, k->h_done_dev, k->host_iter);
}

// Preconditioned iteration (SOR / MG): p = (z - mu) + b/b0 p, w = A p, p.w, x/r update,
// z = M^-1 r, sums of z -- PETSc KSPSolve_CG order with PC_LEFT and the null-space shift.
static int enqueue_pc_iteration(pb_ksp* k) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  double* p = k->pb[0];
  int np = 0;
  const int first = k->lazy0 && k->host_iter == 0;  // r0 = b, x0 = 0, p0 = 0 implicit
  if (k->A->kind == PB_OP_COMPACT && (compact_cg_fusable(g) || compact_cg_fusable_split(g))) {
    // the compact operator forms p in its Z pass (split grids: in the pack of the z -> y
    // transpose) and takes p . w in its X pass (CgFuse): two vector passes fewer (cg_gen_p,
    // cg_gen_dot), 16 B/DoF less per iteration
    CgFuse cf;
    cf.z = k->z;
    cf.p_old = p;
    cf.p_out = p;
    cf.st = k->d_st;
    cf.first = first;
    cf.dot_p = p;
    {
      OpApplySkip guard(ctx, &k->d_st->done);
      struct Set {
        pb_ctx* c;
        ~Set() { c->cg_fuse = nullptr; }
      } set{ctx};
      ctx->cg_fuse = &cf;
      PB_TRY(op_apply_raw(k->A, p, k->w));
    }
    np = cf.nparts;
    if (!cf.fused_z) {
      // a pass did not take the fusion (a launch shape the predicate cannot see): the operator
      // ran on p_old -- form p and apply again, unfused
      PB_TRY(launch_cg_generic_p(g, k->z, p, k->d_st, first));
      OpApplySkip guard(ctx, &k->d_st->done);
      PB_TRY(op_apply_raw(k->A, p, k->w));
    }
    if (!cf.fused_z || !cf.fused_dot) PB_TRY(launch_cg_generic_dot(g, p, k->w, k->d_st, &np));
  } else {
    PB_TRY(launch_cg_generic_p(g, k->z, p, k->d_st, first));  // dinv = 1: z - mu
    {
      OpApplySkip guard(ctx, &k->d_st->done);
      PB_TRY(op_apply_raw(k->A, p, k->w));
    }
    PB_TRY(launch_cg_generic_dot(g, p, k->w, k->d_st, &np));
  }
  PB_TRY(cg_finalize_pass_a(ctx, np, k->d_st));
  const double* r_in = first ? k->b->d : k->r;
  const int rupd = tune("fft_rupd", 1);
  if (k->fft && rupd && fftpc_fuses_r_update(k->fft)) {
    // r = r_in - alpha w formed by the spectral PC's first pass as it loads r, x = x + alpha p
    // beside it (8 B/DoF and one vector pass fewer)
    const RUpdate ru{r_in, k->w, k->r, p, k->x->d, first, k->d_st};
    np = 0;
    PB_TRY(fftpc_apply(k->fft, k->r, k->z, &k->d_st->done, k->d_st, &np, &ru));
  } else {
    PB_TRY(launch_cg_pc_xr(g, p, k->w, k->x->d, r_in, k->r, k->d_st, first));
    PB_TRY(pc_apply_dev(k, k->r, k->z, &k->d_st->done, &np));
  }
  if (np == 0) PB_TRY(launch_cg_pc_sums(g, k->z, k->r, k->d_st, &np));
  return cg_finalize_stage2(ctx, np, k->d_st, k->d_hist, k->h_done_dev, k->host_iter);
}

// the single-reduction iteration's two partial-sum regions (5 wide): iteration n of a batch
// writes region n & 1 and its folded prologue reduces region (n - 1) & 1, so a launch never
// overwrites the partials its own blocks may still be reading (part_off in 5-wide blocks)
static int64_t sr_region_off(const pb_ctx* ctx, int64_t n) {
  return (n & 1) * (ctx->partials_cap / 10);
}
static const double* sr_region(const pb_ctx* ctx, int64_t n) {
  return ctx->d_partials + sr_region_off(ctx, n) * 5;
}

// pass S over r (t = dinv r - mu of state st): split grids exchange r's boundary planes (raw;
// the loader transforms ghosts too) under the interior planes. Every launch is bounded by the
// end of region n & 1 (a grid that does not fit is PB_ERR_UNSUPPORTED, not a spill into the
// region the next prologue reads)
static int sr_pass_s(pb_ksp* k, const double* r, const CgState* st, int* nparts, int64_t n) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  Star s{k->A->cx, k->A->cy, k->A->cz, k->A->cc};
  StencilPlanes gp;
  const int off = (int)sr_region_off(ctx, n);
  const int end = off + (int)(ctx->partials_cap / 10);
  if (!ctx->split) {
    gp.ghost_lo = gp.ghost_hi = nullptr;
    gp.wrap = true;
    return launch_cg_sr_pass_s(g, s, r, gp, st, PLANES_ALL, off, end, nparts);
  }
  gp.ghost_lo = g->ghost_lo;
  gp.ghost_hi = g->ghost_hi;
  const double* hi = r + (g->nzl - 1) * g->plane;
  if (g->nzl < 3) {
    PB_TRY(halo_exchange(g, r, hi));
    return launch_cg_sr_pass_s(g, s, r, gp, st, PLANES_ALL, off, end, nparts);
  }
  int nb1 = 0, nb2 = 0;
  ScopedTimer tm(ctx, "cg_sr_s");
  PB_TRY(halo_begin(g, r, hi));
  PB_TRY(launch_cg_sr_pass_s(g, s, r, gp, st, PLANES_INTERIOR, off, end, &nb1));
  PB_TRY(halo_end(g));
  PB_TRY(launch_cg_sr_pass_s(g, s, r, gp, st, PLANES_BOUNDARY, off + nb1, end, &nb2));
  *nparts = nb1 + nb2;
  return PB_OK;
}

// One single-reduction iteration (PETSc KSPSolve_CG_SingleReduction): pass P, pass S, and -- unless
// folded into the next pass P's prologue (one rank) -- the reduction + residual-sum stage.
// n = the iteration's index inside this pb_ksp_iterate batch (state slot parity).
static int enqueue_sr_iteration(pb_ksp* k, bool fold, int64_t n) {
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  Star s{k->A->cx, k->A->cy, k->A->cz, k->A->cc};
  const int64_t i = k->host_iter;
  const int ns = k->pslots();
  const double* p_prev[3] = {k->pb[i % ns], k->pb[(i + ns - 1) % ns], k->pb[(i + ns - 2) % ns]};
  double* p_new = k->pb[(i + 1) % ns];
  double* r = k->rbuf(i);
  double* r_out = k->rbuf(i + 1);
  // one rank: the state alternates between the slots by the batch index's parity; split grids:
  // slot 0 holds the state after the residual-sum stage (written by the boundary-plane kernel's
  // folded prologue, or copied there unfolded), slot 1 after the top of the iteration (pass P)
  CgState* st_in = ctx->split ? k->d_st : k->d_st + (n & 1);
  CgState* st_out = ctx->split ? k->d_st + 1 : k->d_st + ((n + 1) & 1);
  SrFold f;
  f.fold_sums = fold && n > 0 && !ctx->split;
  f.nparts_s = k->sr_nparts;
  f.parts = sr_region(ctx, n - 1);
  f.in = st_in;
  f.out = st_out;
  f.hist = k->d_hist;
  f.h_done = k->h_done_dev;
  StencilPlanes gp;
  // one pass per iteration where it applies: one rank, depth-4 x deferral; the iterations that
  // carry the x update run the two passes (pass P's x-update form streams at the copy rate)
  if (cg_sr1_supported(g) && k->defer_x == 4 && i % 4 != 3) {
    PB_TRY(launch_cg_sr1(g, s, r, p_prev[0], p_new, r_out, f, f.parts, const_cast<double*>(sr_region(ctx, n)), i,
                         &k->sr_nparts));
    if (!fold)
      PB_TRY(cg_sr_finalize(ctx, sr_region(ctx, n), k->sr_nparts, st_out, k->d_hist,
                            k->h_done_dev, i));
    return PB_OK;
  }
  if (!ctx->split) {
    gp.ghost_lo = gp.ghost_hi = nullptr;
    gp.wrap = true;
    PB_TRY(launch_cg_sr_pass_p(g, s, r, p_prev, p_new, k->x->d, r_out, gp, f, PLANES_ALL, i,
                               k->defer_x));
  } else {
    // p's boundary planes -> halo, under the interior planes. Folded: the boundary-plane kernel
    // first runs the previous iteration's residual-sum stage from pass S's allreduced sums (a
    // one-block partial, slot 1 -> slot 0); pass P then runs the top (slot 0 -> slot 1)
    Fold fb;
    if (fold && n > 0) {
      fb.stage = 2;
      fb.nparts = 1;
      fb.width = 5;
      fb.parts = ctx->d_scalars;
      fb.in = k->d_st + 1;
      fb.out = k->d_st;
      fb.hist = k->d_hist;
      fb.h_done = k->h_done_dev;
      fb.host_iter = i - 1;
    }
    gp.ghost_lo = g->ghost_lo;
    gp.ghost_hi = g->ghost_hi;
    PB_TRY(launch_cg_boundary(g, r, p_prev[0], st_in, fb));
    if (g->nzl < 3) {
      PB_TRY(halo_exchange(g, g->bnd_lo, g->bnd_hi));
      PB_TRY(launch_cg_sr_pass_p(g, s, r, p_prev, p_new, k->x->d, r_out, gp, f, PLANES_ALL, i,
                                 k->defer_x));
    } else {
      ScopedTimer tm(ctx, "cg_sr_p_split");
      PB_TRY(halo_begin(g, g->bnd_lo, g->bnd_hi));
      PB_TRY(launch_cg_sr_pass_p(g, s, r, p_prev, p_new, k->x->d, r_out, gp, f, PLANES_INTERIOR,
                                 i, k->defer_x));
      PB_TRY(halo_end(g));
      PB_TRY(launch_cg_sr_pass_p(g, s, r, p_prev, p_new, k->x->d, r_out, gp, f, PLANES_BOUNDARY,
                                 i, k->defer_x));
    }
  }
  PB_TRY(sr_pass_s(k, r_out, st_out, &k->sr_nparts, n));
  if (fold && ctx->split) return cg_reduce_allreduce(ctx, sr_region(ctx, n), k->sr_nparts, 5);
  if (!fold)
    PB_TRY(cg_sr_finalize(ctx, sr_region(ctx, n), k->sr_nparts, st_out, k->d_hist,
                          k->h_done_dev, i));
  if (!fold && ctx->split)  // the next boundary-plane kernel reads slot 0
    PB_HIP(hipMemcpyAsync(k->d_st, st_out, sizeof(CgState), hipMemcpyDeviceToDevice,
                          ctx->stream));
  return PB_OK;
}

// fold: the finalize steps run in the passes' prologues (one rank, Jacobi; fold_a = pass A also
// folds, i.e. this is not the first iteration of the batch)
static int enqueue_iteration(pb_ksp* k, bool fold, bool fold_a) {
  if (!fused_kind(k->A->kind))
    return k->stored_z() ? enqueue_pc_iteration(k) : enqueue_generic_iteration(k);
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  Star s{k->A->cx, k->A->cy, k->A->cz, k->A->cc};
  const int64_t i = k->host_iter;  // == device iteration index until convergence
  const int ns = k->pslots();
  double* p_old = k->pb[i % ns];
  double* p_new = k->pb[(i + 1) % ns];
  // p of iterations i-1, i-2, i-3 (depth-4 deferral reads all three at i % 4 == 3)
  const double* p_prev[3] = {p_old, k->pb[(i + ns - 1) % ns], k->pb[(i + ns - 2) % ns]};
  // Jacobi: pass A builds z = dinv*r - mu on the fly; SOR / MG: z is stored (dinv = 1)
  double* r = k->rbuf(i);
  const double* zsrc = k->stored_z() ? k->z : r;
  // Jacobi / none: pass A read-only, pass B stores p and the residual into the other buffer
  PStore ps;
  if (k->pst) {
    ps.zsrc = zsrc;
    ps.r_out = k->rbuf(i + 1);
  }
  const bool store_a = !k->pst;
  StencilPlanes gp;
  int nparts = 0;
  const bool fold_split = fold && ctx->split;
  if (fold && !ctx->split) {
    gp.ghost_lo = gp.ghost_hi = nullptr;
    gp.wrap = true;
    if (fold_a)
      PB_TRY(launch_cg_pass_a_folded(g, s, zsrc, p_old, p_new, gp, k->d_st, k->fold_nparts_b,
                                     k->d_hist, k->h_done_dev, i, &nparts, store_a));
    else
      PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_ALL, 0, &nparts,
                              store_a));
    return launch_cg_pass_b_folded(g, s, p_new, p_prev, k->x->d, r, gp, k->d_st, nparts, i,
                                   k->defer_x, &k->fold_nparts_b, ps);
  }
  if (fold_split) {
    // split grids, folded (r05): the previous iteration's stage 2 runs in the prologues of the
    // boundary-plane kernel and pass A (from pass B's allreduced sums, a one-block partial), stage
    // 1 in pass B's (from pass A's); only the reductions before each allreduce stay separate
    // launches (bit-identical to unfolded)
    Fold fb;
    if (fold_a) {
      fb.stage = 2;
      fb.nparts = 1;
      fb.width = 4;
      fb.parts = ctx->d_scalars;
      fb.in = k->d_st + 1;
      fb.out = k->d_st;
      fb.hist = k->d_hist;
      fb.h_done = k->h_done_dev;
      fb.host_iter = i - 1;
    }
    gp.ghost_lo = g->ghost_lo;
    gp.ghost_hi = g->ghost_hi;
    if (g->nzl >= 3) {
      // the boundary-plane kernel runs on the comm stream ahead of the exchange, beside pass A's
      // interior planes, from the stage-2 state in its registers; pass A's interior launch runs the
      // same stage 2 in its prologue and writes the state (the boundary launch reads it)
      Fold fbr = fb;
      fbr.out = nullptr;
      fbr.hist = nullptr;
      fbr.h_done = nullptr;
      int nb1 = 0, nb2 = 0;
      ScopedTimer tm(ctx, "cg_pass_a");
      PB_TRY(halo_begin_after(g, g->bnd_lo, g->bnd_hi, [&](hipStream_t sm) {
        return launch_cg_boundary(g, zsrc, p_old, k->d_st, fbr, sm);
      }));
      if (fold_a)
        PB_TRY(launch_cg_pass_a_fold(g, s, zsrc, p_old, p_new, gp, fb, PLANES_INTERIOR, 0, &nb1,
                                     store_a));
      else
        PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_INTERIOR, 0, &nb1,
                                store_a));
      if (ctx->comm) {
        // the two boundary planes on the comm stream right after the exchange (beside the
        // interior planes), from the stage-2 state in registers as well
        EngineOn eo(ctx, ctx->comm_stream);
        if (fold_a)
          PB_TRY(launch_cg_pass_a_fold(g, s, zsrc, p_old, p_new, gp, fbr, PLANES_BOUNDARY, nb1,
                                       &nb2, store_a));
        else
          PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_BOUNDARY, nb1,
                                  &nb2, store_a));
        PB_HIP(hipEventRecord(ctx->ev_done, ctx->comm_stream));
        PB_TRY(halo_end(g));
      } else {
        PB_TRY(halo_end(g));
        PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_BOUNDARY, nb1,
                                &nb2, store_a));
      }
      nparts = nb1 + nb2;
    } else {
      PB_TRY(launch_cg_boundary(g, zsrc, p_old, k->d_st, fb));
      PB_TRY(halo_exchange(g, g->bnd_lo, g->bnd_hi));
      PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_ALL, 0, &nparts,
                              store_a));
    }
    PB_TRY(cg_reduce_allreduce(ctx, nparts, 1, false));
    PB_TRY(launch_cg_pass_b_folded(g, s, p_new, p_prev, k->x->d, r, gp, k->d_st, 1, i,
                                   k->defer_x, &k->fold_nparts_b, ps, ctx->d_scalars));
    return cg_reduce_allreduce(ctx, k->fold_nparts_b, 4, true);
  }
  if (!ctx->split) {
    // periodic wrap read in place: pass A combines r, p_old of the wrap planes itself and pass B
    // reads p_new's wrap planes (no boundary-plane kernel on one rank)
    gp.ghost_lo = gp.ghost_hi = nullptr;
    gp.wrap = true;
    PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_ALL, 0, &nparts,
                            store_a));
  } else if (g->nzl < 3) {
    PB_TRY(launch_cg_boundary(g, zsrc, p_old, k->d_st));
    PB_TRY(halo_exchange(g, g->bnd_lo, g->bnd_hi));
    gp.ghost_lo = g->ghost_lo;
    gp.ghost_hi = g->ghost_hi;
    PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_ALL, 0, &nparts,
                            store_a));
  } else {
    // the p-plane halo exchange (RCCL, comm stream) overlaps pass A's interior planes
    PB_TRY(launch_cg_boundary(g, zsrc, p_old, k->d_st));
    gp.ghost_lo = g->ghost_lo;
    gp.ghost_hi = g->ghost_hi;
    int nb1 = 0, nb2 = 0;
    ScopedTimer tm(ctx, "cg_pass_a");  // the whole pass A (both launches and the wait)
    PB_TRY(halo_begin(g, g->bnd_lo, g->bnd_hi));
    PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_INTERIOR, 0, &nb1,
                            store_a));
    PB_TRY(halo_end(g));
    PB_TRY(launch_cg_pass_a(g, s, zsrc, p_old, p_new, gp, k->d_st, PLANES_BOUNDARY, nb1, &nb2,
                            store_a));
    nparts = nb1 + nb2;
  }
  PB_TRY(cg_finalize_pass_a(ctx, nparts, k->d_st));
  PB_TRY(launch_cg_pass_b(g, s, p_new, p_prev, k->x->d, r, gp, k->d_st, k->d_hist,
                          k->h_done_dev, i, k->defer_x, !k->stored_z(), ps));
  if (k->stored_z()) {  // z = M^-1 r, then the residual sums over z
    int np = 0;
    PB_TRY(pc_apply_dev(k, r, k->z, &k->d_st->done, &np));
    if (np == 0) PB_TRY(launch_cg_pc_sums(g, k->z, r, k->d_st, &np));
    PB_TRY(cg_finalize_stage2(ctx, np, k->d_st, k->d_hist, k->h_done_dev, i));
  }
  return PB_OK;
}

int pb_ksp_iterate(pb_ksp* k, int64_t iters) {
  PB_CHECK_ARG(k, "ksp is NULL");
  PB_TRY(preonly_split_form(k));
  if (!k->begun) return set_error(PB_ERR_STATE, "pb_ksp_iterate before pb_ksp_begin");
  pb_ctx* ctx = k->A->grid->ctx;
  const int C = k->opts.check_every;
  const int R = 4 * C;
  if ((int)k->ring.size() < R) {
    for (int i = (int)k->ring.size(); i < R; ++i) {
      hipEvent_t e;
      PB_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      k->ring.push_back(e);
    }
  }
  PB_TRY(ensure_done_cap(k, k->host_iter + iters + 2));
  // one rank, Jacobi, fused operator: the finalize steps ride in the passes' prologues
  // (PB_CG_FOLD=0 keeps the separate finalize launches)
  const bool fold = C >= 2 && !k->rich() && fused_kind(k->A->kind) && !k->stored_z() &&
                    tune("cg_fold", 1) != 0;
  int64_t n = 0;
  for (; n < iters && !k->stopped; ++n) {
    if (k->rich()) PB_TRY(enqueue_rich_iteration(k));
    else if (k->sr) PB_TRY(enqueue_sr_iteration(k, fold, n));
    else PB_TRY(enqueue_iteration(k, fold, fold && n > 0));
    const int64_t hi = k->host_iter++;
    // only the iterations the poll below waits for get an event (j = 0 mod C; folded j + 1): an
    // event record between two kernels costs the stream ~6 us of idle time (measured 5.9 us per
    // iteration with one record per iteration; profiles/r02/cg_gaps_*.txt)
    if (hi % C == (fold ? 1 : 0) % C)
      PB_HIP(hipEventRecord(k->ring[hi % R], ctx->stream));
    // lagged, rank-consistent poll: decide on the flag of iteration hi + 1 - C only (folded:
    // that flag is written by the next iteration's pass A, so wait for that iteration's event)
    if ((hi + 1) % C == 0 && hi + 1 >= C) {
      const int64_t j = hi + 1 - C;
      PB_TRY(wait_event(ctx, k->ring[(fold ? j + 1 : j) % R], "KSP convergence poll"));
      if (k->h_done[j + 1]) k->stopped = true;
    }
  }
  if (k->sr) {
    // the residual-sum stage of the batch's last iteration (folded runs), then the state back
    // into slot 0 for the next batch and the other entry points
    if (ctx->split) {  // (unfolded: the state is in slot 0 already)
      if (fold && n > 0) {
        PB_TRY(cg_stage2_from_sums(ctx, 5, k->d_st + 1, k->d_hist, k->h_done_dev,
                                   k->host_iter - 1));
        PB_HIP(hipMemcpyAsync(k->d_st, k->d_st + 1, sizeof(CgState), hipMemcpyDeviceToDevice,
                              ctx->stream));
      }
      return PB_OK;
    }
    if (fold && n > 0)
      PB_TRY(cg_sr_finalize(ctx, sr_region(ctx, n - 1), k->sr_nparts, k->d_st + (n & 1),
                            k->d_hist, k->h_done_dev, k->host_iter - 1));
    if (n & 1)
      PB_HIP(hipMemcpyAsync(k->d_st, k->d_st + 1, sizeof(CgState), hipMemcpyDeviceToDevice,
                            ctx->stream));
    return PB_OK;
  }
  if (fold && n > 0)
    PB_TRY(cg_fold_tail(ctx, k->fold_nparts_b, k->d_st, k->d_hist, k->h_done_dev,
                        k->host_iter - 1));
  return PB_OK;
}

static const char* reason_name(int r) {
  switch (r) {
    case PB_KSP_CONVERGED_RTOL: return "CONVERGED_RTOL";
    case PB_KSP_CONVERGED_ATOL: return "CONVERGED_ATOL";
    case PB_KSP_CONVERGED_ITS: return "CONVERGED_ITS";
    case PB_KSP_DIVERGED_ITS: return "DIVERGED_ITS";
    case PB_KSP_DIVERGED_DTOL: return "DIVERGED_DTOL";
    case PB_KSP_DIVERGED_NANORINF: return "DIVERGED_NANORINF";
    case PB_KSP_DIVERGED_INDEFINITE_MAT: return "DIVERGED_INDEFINITE_MAT";
    case PB_KSP_DIVERGED_INDEFINITE_PC: return "DIVERGED_INDEFINITE_PC";
    default: return "CONVERGED_ITERATING";
  }
}

int pb_ksp_end(pb_ksp* k, pb_ksp_result* res, double* history, int64_t cap) {
  PB_CHECK_ARG(k, "ksp is NULL");
  PB_TRY(preonly_split_form(k));
  if (!k->begun) return set_error(PB_ERR_STATE, "pb_ksp_end before pb_ksp_begin");
  pb_ctx* ctx = k->A->grid->ctx;
  PB_SYNC(ctx, "pb_ksp_end");
  if (k->lazy0 && k->host_iter == 0) {  // stopped at the setup: x = x0 = 0 was never written
    PB_HIP(hipMemsetAsync(k->x->d, 0, (size_t)k->A->grid->nlocal * sizeof(double), ctx->stream));
  }
  CgState st;
  PB_HIP(hipMemcpyAsync(&st, k->d_st, sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
  PB_SYNC(ctx, "pb_ksp_end");
  // Richardson after an odd number of updates, Chebyshev after one that is no multiple of 3: the
  // result is in another buffer than the caller's
  if (k->rich() && k->xbuf(st.its) != k->x->d) {
    PB_HIP(hipMemcpyAsync(k->x->d, k->xbuf(st.its), (size_t)k->A->grid->nlocal * sizeof(double),
                          hipMemcpyDeviceToDevice, ctx->stream));
    PB_SYNC(ctx, "pb_ksp_end");
  }
  if (!k->rich() && st.pend_iter >= 0) {  // apply the still-deferred alpha_m p_m (p_m lives in pb[(m+1) % ns])
    const int ns = k->pslots();
    for (int64_t m = 0; m < st.pend_count; ++m)
      PB_TRY(launch_cg_flush(k->A->grid, k->x->d, k->pb[(st.pend_iter + m + 1) % ns], st.pa[m]));
    PB_SYNC(ctx, "pb_ksp_end");
  }
  if (res) {
    res->reason = st.reason;
    res->its = st.its;
    res->rnorm = st.dp;
    res->rnorm0 = st.rnorm0;
    res->nhist = std::min<int64_t>(st.nlog, k->nhist);
  }
  // only the norms the device logged (a breakdown exit leaves the last iteration without one)
  const int64_t nh = std::min<int64_t>(st.nlog, k->nhist);
  std::vector<double> hist((size_t)std::max<int64_t>(nh, 1));
  if (nh > 0) {
    PB_HIP(hipMemcpyAsync(hist.data(), k->d_hist, (size_t)nh * sizeof(double), hipMemcpyDeviceToHost,
                          ctx->stream));
    PB_SYNC(ctx, "pb_ksp_end");
  }
  if (history && cap > 0) memcpy(history, hist.data(), (size_t)std::min(nh, cap) * sizeof(double));
  if (ctx->rank == 0) {
    if (k->opts.monitor)
      for (int64_t i = 0; i < nh; ++i)
        printf("  %3lld KSP Residual norm %14.12e \n", (long long)i, hist[i]);
    if (k->opts.converged_reason) {
      if (st.reason > 0)
        printf("Linear solve converged due to %s iterations %lld\n", reason_name(st.reason),
               (long long)st.its);
      else
        printf("Linear solve did not converge due to %s iterations %lld\n",
               reason_name(st.reason), (long long)st.its);
    }
    fflush(stdout);
  }
  k->begun = false;
  return PB_OK;
}

// ---------------------------------------------------------------------------------------------
// Projected initial guess (PETSc KSPGuessFischer, model 1; DESIGN.md "Projected initial guess")
// ---------------------------------------------------------------------------------------------
// x = sum_i (b . bt[i]) xt[i], and the same into f->guess: one multi-dot, one two-output
// multi-axpy onto 0 reading its coefficients from the device (no host round trip)
static int fischer_form(pb_ksp* k, const double* b, double* x) {
  pb_ksp::Fischer* f = k->fg;
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const size_t vb = (size_t)g->nlocal * sizeof(double);
  if (f->curl == 0) {
    PB_HIP(hipMemsetAsync(x, 0, vb, ctx->stream));
    PB_HIP(hipMemsetAsync(f->guess, 0, vb, ctx->stream));
    return PB_OK;
  }
  VecTable t;
  for (int i = 0; i < kMaxVecs; ++i) t.p[i] = i < f->curl ? f->bt[i] : nullptr;
  PB_TRY(launch_mdot(ctx, b, f->curl, t, g->nlocal, f->d_coef));
  for (int i = 0; i < f->curl; ++i) t.p[i] = f->xt[i];
  MCoef c{};
  c.dev = f->d_coef;
  c.sign = 1.0;
  return launch_maxpy(ctx, x, f->guess, f->curl, t, c, g->nlocal, true, nullptr);
}

// the norm the last pass left in d_coef[16] as its square: the one host read of an update
static int fischer_norm(pb_ksp* k, double* norm) {
  pb_ctx* ctx = k->A->grid->ctx;
  PB_HIP(hipMemcpyAsync(ctx->h_scalars, k->fg->d_coef + kMaxVecs, sizeof(double),
                        hipMemcpyDeviceToHost, ctx->stream));
  PB_SYNC(ctx, "projected guess update");
  *norm = sqrt(ctx->h_scalars[0]);
  return PB_OK;
}

static int fischer_matvec(pb_ksp* k, const double* x, double* y) {
  ScopedTimer tm(k->A->grid->ctx, "guess_matvec");
  return op_apply_raw(k->A, x, y);
}

// after a solve from f->guess: the new direction x - guess, its A-image orthonormalised against
// the stored ones; a direction that is 0 or not finite is not added
static int fischer_update(pb_ksp* k, const double* x) {
  pb_ksp::Fischer* f = k->fg;
  pb_grid* g = k->A->grid;
  pb_ctx* ctx = g->ctx;
  const int64_t n = g->nlocal;
  VecTable t;
  for (int i = 0; i < kMaxVecs; ++i) t.p[i] = nullptr;
  MCoef c{};
  double* nrm2 = f->d_coef + kMaxVecs;
  double norm = 0.0;
  if (f->curl == f->maxl) {  // space full: restart from this solution alone
    PB_TRY(fischer_matvec(k, x, f->bt[0]));
    PB_TRY(launch_maxpy(ctx, f->bt[0], nullptr, 0, t, c, n, false, nrm2));
    PB_TRY(fischer_norm(k, &norm));
    f->curl = 0;
    if (!std::isfinite(norm) || norm == 0.0) return PB_OK;
    PB_TRY(launch_guess_scale(ctx, f->bt[0], x, f->xt[0], 1.0 / norm, n));
    f->curl = 1;
    return PB_OK;
  }
  const int l = f->curl;
  double* xn = f->xt[l];
  double* bn = f->bt[l];
  if (l == 0)
    PB_HIP(hipMemcpyAsync(xn, x, (size_t)n * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
  else
    PB_TRY(launch_guess_diff(ctx, x, f->guess, xn, n));
  PB_TRY(fischer_matvec(k, xn, bn));
  if (l > 0) {
    // alpha[i] = -(bn . bt[i]); bn += sum alpha[i] bt[i] (its norm^2 in the same pass);
    // xn += sum alpha[i] xt[i]
    for (int i = 0; i < l; ++i) t.p[i] = f->bt[i];
    PB_TRY(launch_mdot(ctx, bn, l, t, n, f->d_coef));
    c.dev = f->d_coef;
    c.sign = -1.0;
    PB_TRY(launch_maxpy(ctx, bn, nullptr, l, t, c, n, false, nrm2));
    for (int i = 0; i < l; ++i) t.p[i] = f->xt[i];
    PB_TRY(launch_maxpy(ctx, xn, nullptr, l, t, c, n, false, nullptr));
  } else {
    PB_TRY(launch_maxpy(ctx, bn, nullptr, 0, t, c, n, false, nrm2));
  }
  PB_TRY(fischer_norm(k, &norm));
  if (!std::isfinite(norm) || norm == 0.0) return PB_OK;
  PB_TRY(launch_guess_scale(ctx, bn, xn, xn, 1.0 / norm, n));
  f->curl = l + 1;
  return PB_OK;
}

static int fischer_check(const pb_ksp* k, const pb_vec* b, const pb_vec* x) {
  PB_CHECK_ARG(k, "ksp is NULL");
  if (!k->fg) return set_error(PB_ERR_STATE, "KSP created without -ksp_guess_type fischer");
  PB_CHECK_ARG(b && x && b != x, "the projected guess needs distinct b and x");
  PB_CHECK_ARG(b->grid == k->A->grid && x->grid == k->A->grid, "vector/operator grid mismatch");
  return PB_OK;
}

int pb_ksp_guess_form(pb_ksp* k, const pb_vec* b, pb_vec* x) {
  PB_TRY(fischer_check(k, b, x));
  return fischer_form(k, b->d, x->d);
}

int pb_ksp_guess_update(pb_ksp* k, const pb_vec* b, const pb_vec* x) {
  PB_TRY(fischer_check(k, b, x));
  return fischer_update(k, x->d);
}

int pb_ksp_guess_reset(pb_ksp* k) {
  PB_CHECK_ARG(k, "ksp is NULL");
  if (!k->fg) return set_error(PB_ERR_STATE, "KSP created without -ksp_guess_type fischer");
  k->fg->curl = 0;
  return PB_OK;
}

int pb_ksp_guess_size(const pb_ksp* k, int* curl, int* maxl) {
  PB_CHECK_ARG(k, "ksp is NULL");
  if (!k->fg) return set_error(PB_ERR_STATE, "KSP created without -ksp_guess_type fischer");
  if (curl) *curl = k->fg->curl;
  if (maxl) *maxl = k->fg->maxl;
  return PB_OK;
}

// form, the solve exactly as with initial_guess_nonzero = 1 (also while the space is empty and
// x = 0: PETSc's guess_zero is false once the guess object touched x), update
static int solve_projected(pb_ksp* k, const pb_vec* b, pb_vec* x, pb_ksp_result* res,
                           double* history, int64_t cap) {
  PB_TRY(fischer_check(k, b, x));
  PB_TRY(fischer_form(k, b->d, x->d));
  const int user_flag = k->opts.initial_guess_nonzero;
  k->opts.initial_guess_nonzero = 1;
  const int rc = pb_ksp_begin(k, b, x);
  k->opts.initial_guess_nonzero = user_flag;
  PB_TRY(rc);
  PB_TRY(pb_ksp_iterate(k, k->opts.max_it + 2 * (int64_t)k->opts.check_every));
  pb_ksp_result r;
  PB_TRY(pb_ksp_end(k, &r, history, cap));
  if (res) *res = r;
  // a non-finite direction must never enter the basis
  if (r.reason == PB_KSP_DIVERGED_NANORINF) return PB_OK;
  return fischer_update(k, x->d);
}

int pb_ksp_solve(pb_ksp* k, const pb_vec* b, pb_vec* x, pb_ksp_result* res, double* history,
                 int64_t cap) {
  PB_CHECK_ARG(k, "ksp is NULL");
  ScopedTimer tm(k->A->grid->ctx, "KSPSolve");
  if (k->opts.ksp_type == PB_KSP_PREONLY) return solve_preonly(k, b, x, res);
  if (k->opts.guess_type != PB_GUESS_NONE) return solve_projected(k, b, x, res, history, cap);
  PB_TRY(pb_ksp_begin(k, b, x));
  PB_TRY(pb_ksp_iterate(k, k->opts.max_it + 2 * (int64_t)k->opts.check_every));
  return pb_ksp_end(k, res, history, cap);
}

int pb_ksp_destroy(pb_ksp* k) {
  if (!k) return PB_OK;
  (void)wait_stream(k->A->grid->ctx, k->A->grid->ctx->stream, "pb_ksp_destroy");
  field_free(k->r);
  field_free(k->r2);
  for (double* p : k->pb) field_free(p);
  field_free(k->w);
  field_free(k->z);
  field_free(k->x2);
  field_free(k->x3);
  if (k->mg) mg_destroy(k->mg);
  fftpc_destroy(k->fft);
  if (k->fg) {
    for (double* p : k->fg->xt) field_free(p);
    for (double* p : k->fg->bt) field_free(p);
    field_free(k->fg->guess);
    if (k->fg->d_coef) (void)hipFree(k->fg->d_coef);
    delete k->fg;
  }
  if (k->d_st) (void)hipFree(k->d_st);
  if (k->d_hist) (void)hipFree(k->d_hist);
  if (k->h_done) (void)hipHostFree(k->h_done);
  for (hipEvent_t e : k->ring) (void)hipEventDestroy(e);
  delete k;
  return PB_OK;
}

int pb_ksp_pc_apply(pb_ksp* k, const pb_vec* r, pb_vec* z) {
  PB_CHECK_ARG(k && r && z && r != z, "bad pc apply args");
  pb_grid* g = k->A->grid;
  PB_CHECK_ARG(r->grid == g && z->grid == g, "vector/operator grid mismatch");
  pb_ctx* ctx = g->ctx;
  if (k->mg) {
    PB_TRY(mg_apply(k->mg, r->d, z->d));
  } else if (k->fft) {
    PB_TRY(fftpc_apply(k->fft, r->d, z->d));
  } else {
    PB_HIP(hipMemcpyAsync(z->d, r->d, (size_t)g->nlocal * sizeof(double),
                          hipMemcpyDeviceToDevice, ctx->stream));
    if (k->opts.pc_type == PB_PC_JACOBI)
      PB_TRY(vec_update(ctx, 2, z->d, nullptr, g->nlocal, 1.0 / k->P->cc));
  }
  PB_SYNC(ctx, "pb_ksp_pc_apply");
  return PB_OK;
}

int pb_ksp_pc_levels(const pb_ksp* k, int* levels) {
  PB_CHECK_ARG(k && levels, "bad args");
  *levels = k->mg ? mg_levels(k->mg) : 0;
  return PB_OK;
}

int pb_ksp_chebyshev_set_opts(pb_ksp* k, const pb_ksp_chebyshev_opts* o) {
  PB_CHECK_ARG(k && o, "bad args");
  if (!k->cheb()) return set_error(PB_ERR_STATE, "KSP created without -ksp_type chebyshev");
  if (k->begun) return set_error(PB_ERR_STATE, "pb_ksp_chebyshev_set_opts inside a solve");
  PB_TRY(check_cheb_opts(o));
  k->copts = *o;
  k->cheb_state = 0;
  return PB_OK;
}

int pb_ksp_pc_mg_set_opts(pb_ksp* k, const pb_pc_mg_opts* o) {
  PB_CHECK_ARG(k && o, "bad args");
  if (k->opts.pc_type != PB_PC_MG || !k->mg)
    return set_error(PB_ERR_STATE, "KSP created without -pc_type mg");
  if (k->begun) return set_error(PB_ERR_STATE, "pb_ksp_pc_mg_set_opts inside a solve");
  PB_TRY(check_mg_opts(o));
  MgSmoother sm;
  sm.ksp = o->levels_ksp_type;
  sm.pc = o->levels_pc_type;
  sm.nu = o->levels_ksp_max_it;
  sm.rich_scale = o->levels_richardson_scale;
  mg_levels_bounds(o, &sm.emin, &sm.emax);
  PB_TRY(mg_set_smoother(k->mg, sm));
  k->mgopts = *o;
  k->cheb_state = 0;  // an outer Chebyshev's estimate belongs to the old preconditioner
  return PB_OK;
}

int pb_ksp_pc_mg_get_opts(const pb_ksp* k, pb_pc_mg_opts* o) {
  PB_CHECK_ARG(k && o, "bad args");
  if (k->opts.pc_type != PB_PC_MG || !k->mg)
    return set_error(PB_ERR_STATE, "KSP created without -pc_type mg");
  *o = k->mgopts;
  return PB_OK;
}

int pb_ksp_chebyshev_get_eigenvalues(pb_ksp* k, double* emin, double* emax, int* estimated) {
  PB_CHECK_ARG(k, "ksp is NULL");
  if (!k->cheb()) return set_error(PB_ERR_STATE, "KSP created without -ksp_type chebyshev");
  PB_TRY(cheb_bounds(k));
  PB_SYNC(k->A->grid->ctx, "pb_ksp_chebyshev_get_eigenvalues");
  if (emin) *emin = k->cheb_emin;
  if (emax) *emax = k->cheb_emax;
  if (estimated) *estimated = k->cheb_state == 2 ? 1 : 0;
  return PB_OK;
}

// Bisection on the Sturm count (the number of eigenvalues below s = the number of negative pivots
// of T - s I), started from the Gershgorin interval; ends when the interval cannot be halved
int pb_tridiag_extreme_eigenvalues(int n, const double* diag, const double* off, double* lo,
                                   double* hi) {
  PB_CHECK_ARG(n >= 1 && n <= 64, "tridiagonal order outside 1..64");
  PB_CHECK_ARG(diag && lo && hi && (off || n == 1), "bad tridiagonal args");
  double gl = INFINITY, gu = -INFINITY;
  for (int i = 0; i < n; ++i) {
    const double a = i > 0 ? std::fabs(off[i - 1]) : 0.0, c = i + 1 < n ? std::fabs(off[i]) : 0.0;
    PB_CHECK_ARG(std::isfinite(diag[i]) && std::isfinite(a) && std::isfinite(c),
                 "tridiagonal entries must be finite");
    gl = std::min(gl, diag[i] - (a + c));
    gu = std::max(gu, diag[i] + (a + c));
  }
  PB_CHECK_ARG(std::isfinite(gl) && std::isfinite(gu), "tridiagonal entries too large");
  const double tiny = 1e-300 + 2.3e-16 * std::max(std::fabs(gl), std::fabs(gu));
  auto below = [&](double s) {
    int cnt = 0;
    double q = 1.0;
    for (int i = 0; i < n; ++i) {
      const double e = i > 0 ? off[i - 1] : 0.0;
      q = diag[i] - s - (i > 0 ? e * e / q : 0.0);
      if (std::fabs(q) < tiny) q = -tiny;
      if (q < 0.0) ++cnt;
    }
    return cnt;
  };
  // the index-th eigenvalue (ascending): the s where below(s) passes from <= index to > index
  auto kth = [&](int index) {
    double a = gl, b = gu;
    for (int it = 0; it < 2000; ++it) {
      const double m = a + 0.5 * (b - a);
      if (!(m > a && m < b)) break;
      if (below(m) > index) b = m;
      else a = m;
    }
    return a + 0.5 * (b - a);
  };
  *lo = kth(0);
  *hi = kth(n - 1);
  return PB_OK;
}

int pb_solve(pb_op* A, pb_op* P, const pb_ksp_opts* opts, const pb_vec* b, pb_vec* x,
             pb_ksp_result* res, double* history, int64_t cap) {
  return pb_solve_chebyshev(A, P, opts, nullptr, b, x, res, history, cap);
}

static int solve_once(pb_op* A, pb_op* P, const pb_ksp_opts* opts,
                      const pb_ksp_chebyshev_opts* cheb, const pb_pc_mg_opts* mgo, const pb_vec* b,
                      pb_vec* x, pb_ksp_result* res, double* history, int64_t cap);

int pb_solve_chebyshev(pb_op* A, pb_op* P, const pb_ksp_opts* opts,
                       const pb_ksp_chebyshev_opts* cheb, const pb_vec* b, pb_vec* x,
                       pb_ksp_result* res, double* history, int64_t cap) {
  return solve_once(A, P, opts, cheb, nullptr, b, x, res, history, cap);
}

int pb_solve_mg(pb_op* A, pb_op* P, const pb_ksp_opts* opts, const pb_pc_mg_opts* mgo,
                const pb_vec* b, pb_vec* x, pb_ksp_result* res, double* history, int64_t cap) {
  return solve_once(A, P, opts, nullptr, mgo, b, x, res, history, cap);
}

static int solve_once(pb_op* A, pb_op* P, const pb_ksp_opts* opts,
                      const pb_ksp_chebyshev_opts* cheb, const pb_pc_mg_opts* mgo, const pb_vec* b,
                      pb_vec* x, pb_ksp_result* res, double* history, int64_t cap) {
  pb_ksp* k = nullptr;
  pb_ksp_opts one;
  if (opts && opts->guess_type == PB_GUESS_FISCHER) {
    // this KSP lives for one solve and keeps no direction: one pair of vectors is enough
    PB_TRY(check_guess_opts(opts->guess_fischer_model, opts->guess_fischer_maxl));
    one = *opts;
    one.guess_fischer_maxl = 1;
    opts = &one;
  }
  PB_TRY(pb_ksp_create(A, P, opts, &k));
  int rc = cheb && k->cheb() ? pb_ksp_chebyshev_set_opts(k, cheb) : PB_OK;
  if (rc == PB_OK && mgo && k->opts.pc_type == PB_PC_MG) rc = pb_ksp_pc_mg_set_opts(k, mgo);
  if (rc == PB_OK) rc = pb_ksp_solve(k, b, x, res, history, cap);
  const std::string msg = rc != PB_OK ? pb_last_error() : "";
  pb_ksp_destroy(k);
  return rc != PB_OK ? set_error(rc, "%s", msg.c_str()) : PB_OK;
}

}  // extern "C"
