// pb_mg.hpp -- what the multigrid preconditioner's files share: pb_mg.cpp (the host path: the
// hierarchy, the level plan, the V-cycle driver and its legs) and pb_mg.hip (the per-pair,
// per-cell, polynomial and tail kernels, each behind the one launcher that names it) and
// pb_mg_varcoef.hip (the variable-coefficient levels). The fused sweeps (pb_mg_sweep.hip) and the
// engine passes (pb_mg_engine.hip): pb_internal.hpp.
#pragma once
#include <vector>

#include "pb_internal.hpp"

namespace pb {

struct MgGeo {
  int nx, ny, nzl;
  int64_t plane, nlocal, k0;
};

// The passes a level takes in one V-cycle: level_plan (pb_mg.cpp) computes it at the top of every
// apply; the legs and the launchers switch on it and nothing else re-derives it.
struct LevelPlan {
  // pre-smoothing from zero, residual and restriction in one pass | pre-smoothing and residual in
  // one pass | a launch each (half-sweeps, or the level smoother's steps)
  enum Pre { FusedRestrict, FusedResidual, Sweeps };
  // prolongation and both half-sweeps in one pass, xs -> x | prolongation into the residual
  // scratch, then both half-sweeps in one pass | in place, then a launch each
  enum Post { PostSweep, ProlongThenSweep2, ProlongThenHalves };
  bool engine = false;  // half-sweeps and residual on the stencil engine (else the pair kernels)
  Pre pre = Sweeps;
  Post post = ProlongThenHalves;
  bool march = false;  // transfers to / from the coarse level by the z-marching kernels
};

struct MgLevel {
  int64_t n[3];
  double h[3];
  Star s;
  pb_grid* g = nullptr;  // level grid (level 0: the caller's grid)
  bool own = false;
  double* x = nullptr;    // correction (level 0: the PC output z)
  double* b = nullptr;    // right-hand side (level 0: the PC input r)
  double* res = nullptr;  // residual scratch
  // fused post-smoothing (LevelPlan::PostSweep): the pre-smoothed x, kept apart from x so that
  // the prolongation + both half-sweeps can read it and write x in one pass
  double* xs = nullptr;
  // Jacobi-type smoothers (mg_set_smoother): two more iterate buffers and one more residual
  // buffer -- a step forms y_new at a point's neighbours from y, y_prev and r there, so it writes
  // to buffers it does not read; x, t1, t2 and res, r2 rotate
  double* t1 = nullptr;
  double* t2 = nullptr;
  double* r2 = nullptr;
  // the variable-coefficient PC (mg_set_coefficient; pb_mg_varcoef.hip): the level's beta and the
  // reciprocal diagonal of div(beta_l grad), each nzl + 2 planes with local plane 0 at the pointer
  // (planes -1 and nzl: the neighbouring ranks', one rank: the periodic wrap). Level 0's beta is
  // the operator's own storage; vs = the axis coefficients 1 / (2^l h_d)^2 of the operator's deltas
  const double* beta = nullptr;
  double* beta_own = nullptr;  // (below level 0: beta, writable)
  double* dinv = nullptr;
  // the mass term of the coefficient operator on this level (pb_op_set_mass): q_0 = s * m,
  // q_(l+1) the 8-child mean of q_l; point-local, no ghost planes. nullptr: none or the scalar qs
  // (a scalar-only mass stays s on every level)
  double* q = nullptr;
  double qs = 0.0;
  Star vs;
  LevelPlan plan;         // this apply's
  double* cur = nullptr;  // this apply's pre-smoothed iterate, from the down leg to the up leg
  int64_t size() const { return n[0] * n[1] * n[2]; }  // of the whole grid
  MgGeo geo() const {
    return MgGeo{(int)g->n[0], (int)g->n[1], (int)g->nzl, g->plane, g->nlocal, g->k0};
  }
};

// the tuning values of one apply, read once (mg_tunings, pb_mg.cpp)
struct MgTune {
  // SOR half-sweeps and residuals of levels whose planes hold >= engine_min_plane points run on
  // the z-marching stencil engine (smaller levels: per-pair kernels, whose short z-chunks would
  // not amortise the engine's prologue)
  int64_t engine_min_plane;
  // transfers: one thread per coarse column marching in z on coarse levels of this many columns
  // and more, one thread per coarse cell (prolongation) / point (restriction) below
  int64_t restrict_z_min_cols;
  int64_t tail_max;  // the one-launch tail: levels of at most this many points
  bool split_fused;  // decomposed grids: the unrolled fused passes with deep ghost planes
  bool poly_fused;   // Jacobi-type smoothers, one rank: a step and its residual in one pass
  // variable-coefficient levels: the zero-start red + black half-sweeps in one pass | the
  // half-sweep reads the stored dinv (else it forms it from its six faces)
  bool vc_pre_fused, vc_dinv_stored;
  int vc_kc;  // planes per chunk of the marching half-sweeps (0: by the level's size)
};

// CG's residual sums of the V-cycle's output, taken by its last pass where that pass can
struct MgSums {
  const CgState* st = nullptr;
  int* nparts = nullptr;
};

// a coarse correction that is not the coarse level's own x: the agglomerated level's, whose
// planes below and above this rank's are read in place
struct CoarsePlanes {
  const double *xc, *lo, *hi;
};

static constexpr int kTailMax = 12;  // levels the one-launch tail can take

struct Mg {
  pb_ctx* ctx = nullptr;
  std::vector<MgLevel> lv;
  double omega = 1.0;
  int coarse_its = 1;
  double* mem = nullptr;
  const int* skip = nullptr;  // device flag: when set, the kernels of this apply exit at entry
  MgTune tn;                  // this apply's tunings
  bool tail_attr = false;     // mg_tail_kernel's dynamic-LDS limit raised
  // Decomposed grids (r04): the coarse levels [La, L) are gathered onto every rank once per
  // V-cycle (one all-to-all of level La's right-hand side) and run there as the one-launch tail
  // on full-grid arrays -- instead of a latency-bound halo exchange per half-sweep, residual and
  // transfer on levels of a few thousand points. La = 0: none. Every rank computes the same
  // coarse correction (same kernels, same inputs) and prolongates from its own planes of it.
  int La = 0;
  double* agg = nullptr;                   // full-grid x, b, res of levels La .. L-1; send staging
  std::vector<MgGeo> ageo;                 // their full-grid geometry (k0 = 0)
  std::vector<double*> ax, ab, ares;
  double* agg_send = nullptr;              // P copies of this rank's level-La slab
  std::vector<int64_t> agg_sc, agg_rc;     // all-to-all counts (send: own slab; recv: rank q's)
  // the level smoother (pb_pc_mg_opts). custom(): anything but the default richardson + sor with
  // one sweep per leg -- a plan with every fusion, the tail and the agglomeration off
  MgSmoother sm;
  bool poly() const { return sm.pc == PB_MG_LEVELS_JACOBI; }
  bool custom() const { return poly() || sm.nu > 1 || coef; }
  double* pmem = nullptr;  // the levels' t1, t2, r2
  // pb_ksp_pc_set_coefficient_from: smoother, residual and coarse operators are div(beta_l grad)
  // of this PB_OP_VARCOEF operator (held, not owned). The levels' coefficients are rebuilt by the
  // first apply after coef->change moved on from coef_seen
  const pb_op* coef = nullptr;
  int64_t coef_seen = -1;
  int mean = PB_COEF_ARITHMETIC;  // coef's at the last build
  double* vmem = nullptr;         // the levels' beta (below level 0) and dinv
  double* qmem = nullptr;         // the levels' q, allocated by the first build with a mass field
};

// ---- the launchers (pb_mg.hip): one per pass, used by every path of the driver ----
#pragma GCC visibility push(hidden)
// mode 0: half-sweep of `color`; mode 1: zero-initialised red + black half-sweeps fused.
// sums (mode 0, engine path only): also take CG's residual sums of the output (*nparts set)
int level_smooth(Mg* mg, MgLevel& L, int color, int mode, MgSums sums = {});
int level_residual(Mg* mg, MgLevel& F, const double* x, double* res);  // res = F.b - A x
int level_restrict(Mg* mg, MgLevel& F, const double* res, MgLevel& C);  // C.b = R res
// xout = xf + P xc (another array than xf only on the z-marching kernel). cp: the coarse
// correction's planes where they are not C.x and its ghosts
int level_prolong(Mg* mg, MgLevel& F, const double* xf, double* xout, MgLevel& C,
                  const CoarsePlanes* cp = nullptr);
// One step of a Jacobi-type smoother on level F. y == nullptr: the zero start (r = b);
// yp == nullptr: no y_prev term. r_out == nullptr: the iterate alone (y_out may alias an input)
int poly_step(Mg* mg, MgLevel& F, const double* y, const double* yp, const double* r, double scale,
              double omega, double* y_out, double* r_out);
int launch_tail(Mg* mg, int Lt, bool agg);  // levels Lt .. L-1 in one launch (agg: gathered)
// ghost planes of v on level L: in place (1 rank) or exchanged (N ranks)
int level_ghosts(MgLevel& L, const double* v, const double** lo, const double** hi);
// ---- the variable-coefficient levels (pb_mg_varcoef.hip) ----
// the levels' beta (8-child arithmetic mean of the finer level's, then the ghost planes) and dinv
// from mg->coef as it is now
int vmg_build(Mg* mg);
// level_smooth's and level_residual's variable branches
int vmg_smooth(Mg* mg, MgLevel& L, int color, int mode);
int vmg_residual(Mg* mg, MgLevel& F, const double* x, double* res);
#pragma GCC visibility pop

}  // namespace pb
