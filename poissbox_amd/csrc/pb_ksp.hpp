// pb_ksp.hpp -- struct pb_ksp and what the KSP's host files share: pb_solver.cpp (the driver: create
// / begin / iterate / end / solve), pb_ksp_cg.cpp (cg), pb_ksp_stationary.cpp (richardson, chebyshev,
// preonly), pb_ksp_guess.cpp (the projected initial guess), pb_options.cpp (defaults, checks, parsers),
// pb_norm_type.cpp (-ksp_norm_type), pb_ksp_fgmres.cpp (fgmres), pb_ksp_pipecg.cpp (pipecg) and
// pb_op.cpp (the operator).
#pragma once
#include <vector>

#include "pb_internal.hpp"

namespace pb {
struct FgState;
struct PcgState;
}

struct pb_ksp {
  pb_op* A = nullptr;
  pb_op* P = nullptr;
  pb_ksp_opts opts;
  // -ksp_norm_type as set (pb_ksp_set_norm_type; pb_norm_type.cpp) and the one in force
  int norm_type = PB_KSP_NORM_DEFAULT;
  int norm() const {
    if (norm_type != PB_KSP_NORM_DEFAULT) return norm_type;
    if (opts.ksp_type == PB_KSP_FGMRES) return PB_KSP_NORM_UNPRECONDITIONED;
    return opts.ksp_type == PB_KSP_PREONLY ? PB_KSP_NORM_NONE : PB_KSP_NORM_PRECONDITIONED;
  }
  // none (KSPConvergedSkip): nothing but a breakdown ends the solve before max_it, so the host
  // neither polls nor enqueues past it
  bool norm_none() const { return norm() == PB_KSP_NORM_NONE; }
  bool norm_unp() const { return norm() == PB_KSP_NORM_UNPRECONDITIONED; }
  int64_t solve_iters() const {
    return norm_none() ? opts.max_it : opts.max_it + 2 * (int64_t)opts.check_every;
  }
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
  // r ping-pongs likewise (rich_rbuf), r_0 = b read in place from a zero guess.
  // Chebyshev (-ksp_type chebyshev) runs as Richardson does (rich() covers both) with one more
  // solution buffer: update i >= 1 reads y_i = xbuf(i) and y_(i-1) = xbuf(i - 1) and writes
  // xbuf(i + 1), the three rotating; the caller's x is xbuf(0 mod 3)
  struct Rich {
    double* x2 = nullptr;
    double* x3 = nullptr;
    bool guess = false;  // this solve started from a nonzero guess (r_0 is in r, not b)
  };
  Rich ri;
  bool cheb() const { return opts.ksp_type == PB_KSP_CHEBYSHEV; }
  bool rich() const { return opts.ksp_type == PB_KSP_RICHARDSON || cheb(); }
  double* xbuf(int64_t i) const {
    if (cheb()) return i % 3 == 0 ? x->d : (i % 3 == 1 ? ri.x2 : ri.x3);
    return (i & 1) ? ri.x2 : x->d;
  }
  const double* rich_rbuf(int64_t i) const {
    return i == 0 && !ri.guess ? b->d : ((i & 1) ? r2 : r);
  }
  // Chebyshev's bounds in use and what follows from them (KSPSolve_Chebyshev's scale, mu,
  // omegaprod); state: 0 = not set yet, 1 = the caller's, 2 = estimated for the deltas in `deltas`
  // (A's, then P's: the estimate runs again when either changed)
  struct Cheb {
    pb_ksp_chebyshev_opts opts;  // pb_ksp_chebyshev_set_opts; the defaults from pb_ksp_create
    int state = 0;
    double emin = 0.0, emax = 0.0, scale = 0.0, mu = 0.0, omegaprod = 0.0;
    double deltas[6] = {0, 0, 0, 0, 0, 0};
    // ... and for A's and P's change counters then (pb_op_set_coefficient moves them too)
    int64_t change[2] = {-1, -1};
  };
  Cheb ch;
  // Restarted flexible GMRES (-ksp_type fgmres). v[j] the orthonormal basis,
  // z[j] = N(M^-1 v[j]) the stored preconditioned directions, both allocated in chunks as a cycle
  // first reaches them (and cleared then). The unnormalised direction w alternates between pb[0]
  // and pb[1] (wbuf(cur): the engine pass that forms v, z and A z from it writes the other), A x
  // of a restart is r. pos = the host's cycle position: the device's (FgState::loc) as long as
  // the state is not done. d: the Hessenberg, rotations and sums (device)
  struct Fgmres {
    pb_ksp_fgmres_opts opts;  // pb_ksp_fgmres_set_opts; the defaults from pb_ksp_create
    std::vector<double*> v, z;
    pb::FgState* d = nullptr;
    int pos = 0;
    int cur = 0;
  };
  Fgmres fgm;
  bool fgmres() const { return opts.ksp_type == PB_KSP_FGMRES; }
  // Pipelined CG (-ksp_type pipecg). Beside x and b: r (r), u = N(M^-1 r)
  // (pb[0]), w = A u and the four recurrence vectors z, q, s, p. On the 7-point operator with
  // Jacobi / no PC (one rank) the engine pass of update i reads w from wbuf(i) and writes
  // wbuf(i + 1) (pb[1], w2): neighbouring waves still read w around a point. cur = the host's
  // parity, the device's as long as the state is not done (a launch that exited at entry wrote
  // nothing, and nothing reads w after the solve). Elsewhere w stays in pb[1] and m = N(M^-1 w),
  // n = A m are stored (the KSP's w and z fields). d: the sums and scalars (device)
  struct Pipecg {
    double* z = nullptr;
    double* q = nullptr;
    double* s = nullptr;
    double* p = nullptr;
    double* w2 = nullptr;
    pb::PcgState* d = nullptr;
    int cur = 0;
    bool fused = false;  // this solve runs the engine pass (decided by pb_ksp_begin)
  };
  Pipecg pcg;
  bool pipecg() const { return opts.ksp_type == PB_KSP_PIPECG; }
  double* pcg_wbuf(int i) const { return (i & 1) ? pcg.w2 : pb[1]; }
  // the default solver (pb_ksp_cg.cpp): the split form of every type that is none of the above
  bool cg() const { return !rich() && !fgmres() && !pipecg(); }
  pb::Mg* mg = nullptr;  // SOR / multigrid preconditioner (PB_PC_SOR, PB_PC_MG)
  pb_pc_mg_opts mgopts;  // pb_ksp_pc_mg_set_opts; the defaults from pb_ksp_create
  // pb_ksp_pc_set_coefficient_from: the PB_OP_VARCOEF operator the SOR / MG levels take their
  // coefficient from (held like A and P, not owned). pc_coef(): it, where a solve must hold it
  // beside A and P
  const pb_op* coef = nullptr;
  pb_op* pc_coef() const {
    return coef && coef != A && coef != P ? const_cast<pb_op*>(coef) : nullptr;
  }
  pb::FftPc* fft = nullptr;  // spectral preconditioner (PB_PC_FFT)
  int fold_nparts_b = 0;     // partial-sum blocks of the last folded pass B
  // -pc_type jacobi from a PB_OP_VARCOEF P: the diagonal is a field, so z = dinv o r is stored like
  // the PCs' above. dinv = 1.0 / diag(P), built when a solve first needs it and again when P's
  // change counter has moved on (pb_op_set_coefficient, pb_op_set_deltas)
  struct VarJacobi {
    bool on = false;
    double* dinv = nullptr;
    int64_t seen = -1;
  };
  VarJacobi vj;
  // PCs whose z = M^-1 r is stored (not the constant-coefficient Jacobi)
  bool stored_z() const { return mg || fft || vj.on; }
  bool lazy0 = false;  // r0 = b, x0 = 0, p0 = 0 left implicit by pb_ksp_begin
  double* guess_bsums() const { return reinterpret_cast<double*>(d_st + 2); }
  pb::CgState* d_st = nullptr;
  double* d_hist = nullptr;
  int64_t nhist = 0;
  int* h_done = nullptr;      // host-mapped, one flag per host iteration (+1)
  int* h_done_dev = nullptr;  // its device alias
  int64_t done_cap = 0;
  // what the scalar stages write: state slot 0 (1: the folded iterations' second), history, flags
  pb::KspLog log(int slot = 0) const { return pb::KspLog{d_st + slot, d_hist, h_done_dev}; }
  // KSPConvergedDefault's reference norm from a nonzero guess: REF_INITIAL, REF_MIN or REF_RHS
  // (pb_cg_device.hpp)
  int ref_norm() const {
    return opts.converged_use_initial_residual_norm
               ? 1
               : (opts.converged_use_min_initial_residual_norm ? 2 : 0);
  }
  std::vector<hipEvent_t> ring;
  // solve state
  const pb_vec* b = nullptr;
  pb_vec* x = nullptr;
  int64_t host_iter = 0;
  bool stopped = false;
  bool begun = false;
  int defer_x = 4;  // x updated every defer_x-th iteration (PB_CG_DEFER_X = 0, 2 or 4)
  int pslots() const { return defer_x == 4 ? 4 : 2; }
  // the vectors of CG's iteration i (= host_iter) on the fused operator: p of iterations i - 1
  // (p_old = p_prev[0]), i - 2, i - 3 (the depth-4 deferral reads all three at i % 4 == 3), the
  // direction and the residual it writes
  struct CgBufs {
    const double* p_prev[3];
    double *p_old, *p_new, *r, *r_out;
  };
  CgBufs cg_bufs() const {
    const int64_t i = host_iter;
    const int ns = pslots();
    return CgBufs{{pb[i % ns], pb[(i + ns - 1) % ns], pb[(i + ns - 2) % ns]},
                  pb[i % ns], pb[(i + 1) % ns], rbuf(i), rbuf(i + 1)};
  }
  // single-reduction iteration (-ksp_cg_single_reduction on the fused operator, Jacobi / none):
  // the state alternates between the two slots d_st[0..1] within a pb_ksp_iterate batch (pass P
  // of the batch's n-th iteration reads slot n & 1 and writes the other); nparts = pass S's
  // partial-sum blocks of the last iteration (folded: reduced by the next pass P's prologue)
  struct Sr {
    bool on = false;
    int nparts = 0;
  };
  Sr sr;
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

// (internal to the KSP's files: kept out of the library's dynamic symbols)
#pragma GCC visibility push(hidden)
namespace pb {

// the fused CG passes evaluate A p inside the stencil engine (reference order); the assembled P
// (AIJ order at the seams) runs the unfused iteration around its own MatMult
inline bool fused_kind(int kind) { return kind == PB_OP_STAR7; }

// ---- pb_op.cpp ----
// y = A x without the entry point's argument checks
int op_apply_raw(pb_op* op, const double* x, double* y);
// KSP iterations enqueued ahead of the convergence poll: the operator kernels launched inside
// the guard's scope exit at entry once the KSP's device flag is set (pb_ctx::op_skip)
struct OpApplySkip {
  pb_ctx* ctx;
  OpApplySkip(pb_ctx* c, const int* flag) : ctx(c) { ctx->op_skip = flag; }
  ~OpApplySkip() { ctx->op_skip = nullptr; }
};

// w = A p inside a CG iteration; *nparts = the blocks of p . w partial sums the operator's own pass
// left at ctx->d_partials (PB_OP_VARCOEF with tuning varcoef_dot_fused), 0: the caller takes them
int op_apply_dot(pb_op* op, const double* p, double* w, int* nparts);

// ---- pb_solver.cpp: the driver ----
int ensure_done_cap(pb_ksp* k, int64_t need);
// z = M^-1 r of a stored-z preconditioner, nothing else (no sums, no null-space shift)
int pc_stored_apply(pb_ksp* k, const double* r, double* z, const int* skip = nullptr);
// z = M^-1 r for the stored-z preconditioners; *np = residual-sum partial blocks written by the
// PC itself (MG's last sweep), 0 if the caller must take the sums
int pc_apply_dev(pb_ksp* k, const double* r, double* z, const int* skip, int* np);

// ---- pb_ksp_cg.cpp: -ksp_type cg ----
// pb_ksp_begin's setup (it uploads the state itself: st, the tolerances filled in, gets the form
// of this solve's iteration first); iteration n of a pb_ksp_iterate batch (fold: the finalize
// steps run in the passes' prologues); what completes a batch of n iterations (the folded last
// iteration's residual-sum stage, the state back into slot 0); pb_ksp_end's share from the final
// state st: the deferred part of the x update, x = 0 after a lazy start that never iterated
int cg_begin(pb_ksp* k, const pb_vec* b, pb_vec* x, CgState& st);
int enqueue_cg_iteration(pb_ksp* k, bool fold, int64_t n);
int cg_batch_end(pb_ksp* k, bool fold, int64_t n);
int cg_finish(pb_ksp* k, const CgState& st);

// ---- pb_options.cpp: every range and compatibility rule of the option structs ----
// Chebyshev's interval: finite, non-zero, of one sign, emax > emin (`what` names it in the error)
int check_cheb_pair(double emin, double emax, const char* what);
int check_cheb_opts(const pb_ksp_chebyshev_opts* o);
int check_mg_opts(const pb_pc_mg_opts* o);
int check_guess_opts(int model, int maxl);
int check_ref_norm_opts(const pb_ksp_opts* o);
int check_richardson_scale(double scale);
// the bounds the level smoother runs with: the caller's, or the esteig transform of D^-1 A's
// exact extremes (0, 2) on every level
void mg_levels_bounds(const pb_pc_mg_opts* o, double* emin, double* emax);

// ---- pb_ksp_stationary.cpp: -ksp_type richardson | chebyshev (k->rich()) and preonly ----
// pb_ksp_begin's setup (the state with the tolerances is on its way to k->d_st), one update of
// pb_ksp_iterate, and pb_ksp_end's copy of the result into the caller's x after `its` updates
int rich_begin(pb_ksp* k, const pb_vec* b, pb_vec* x);
int enqueue_rich_iteration(pb_ksp* k);
int rich_copy_back(pb_ksp* k, int64_t its);
int solve_preonly(pb_ksp* k, const pb_vec* b, pb_vec* x, pb_ksp_result* res);

// ---- pb_ksp_fgmres.cpp: -ksp_type fgmres ----
// pb_ksp_begin's setup (as rich_begin), one Arnoldi step of pb_ksp_iterate (with the restart
// sequence after the cycle's last), pb_ksp_end's solution build from the cycle the solve ended
// in, and pb_ksp_destroy's share
int fgmres_create(pb_ksp* k);
int fgmres_begin(pb_ksp* k, const pb_vec* b, pb_vec* x);
int enqueue_fgmres_iteration(pb_ksp* k);
int fgmres_finish(pb_ksp* k);
void fgmres_destroy(pb_ksp* k);
int check_fgmres_opts(const pb_ksp_fgmres_opts* o);

// ---- pb_ksp_fgmres.hip: the small state and its kernels ----
constexpr int kFgMaxRestart = 64;
constexpr int kFgLd = kFgMaxRestart + 1;  // column stride of the Hessenberg
// Everything small of a cycle, device resident. Column k of the Hessenberg (rotated in place into
// the triangular factor) is hh[k * kFgLd .. + k + 1]. The tolerances, reason, done flag and
// history cursor are CgState's (pb_ksp::d_st)
struct FgState {
  double hh[kFgLd * kFgMaxRestart];
  double cs[kFgMaxRestart], sn[kFgMaxRestart];  // Givens cosines and sines
  double g[kFgLd];                              // the rotated right-hand side
  double y[kFgMaxRestart];                      // the triangular solve's result
  double dots[kFgLd], dots2[kFgLd];             // the multi-dot's sums (second: refinement pass)
  double nrm2;    // sum w^2 from the multi-axpy (a restart, the setup: sum r^2)
  double wsum;    // sum w beside it (nrm2, wsum: the multi-axpy's two sums, adjacent)
  double shift;   // Jacobi / no PC: the null-space shift of the next z, -(dinv (scale wsum)) / ntot
  double bsq;     // sum b^2 (the reference norm of a nonzero guess)
  double zsum;    // sum of M^-1 v_k: the null-space shift is -zsum / ntot
  double scale;   // 1 / h_(k+1,k) (a cycle's start: 1 / ||r||)
  double haptol;
  int loc;        // cycle position: steps done in this cycle = live entries of v, z, y
  int restart;
};
// at most kFgMaxRestart vectors by value in the kernel arguments
struct FgTable {
  const double* p[kFgMaxRestart];
};
// v = fs->scale w; exits at entry when the state is done (so do the two below)
int launch_fg_scale(pb_ctx* ctx, const double* w, double* v, const FgState* fs, const CgState* st,
                    int64_t n);
// the sum of z as a stored-z PC wrote it, reduced and allreduced into fs->zsum
int launch_fg_zsum(pb_ctx* ctx, const double* z, FgState* fs, const CgState* st, int64_t n);
// z = z + (-(fs->zsum / ntot)): MatNullSpaceRemove's VecShift
int launch_fg_shift(pb_ctx* ctx, double* z, const FgState* fs, const CgState* st, int64_t n);
// Jacobi / no PC: z = dinv v + fs->shift (nullspace = 0: no add) -- fg_z, the expression the
// engine pass forms on load
int launch_fg_pcshift(pb_ctx* ctx, const double* v, double* z, const FgState* fs,
                      const CgState* st, int64_t n, bool nullspace);
// The engine pass of a step on the 7-point operator with Jacobi / no PC (one rank, wrap planes;
// pb_ksp_fgmres.hip FgLoad / FgEpi): from the unnormalised direction wt, v = fs->scale wt and
// z = dinv v + fs->shift formed on load; stores v and z and writes w_out = A z (another buffer
// than wt). 8 B read, 24 B written per DoF; the bits of scale + pcshift + operator
int launch_fg_fused(pb_grid* g, const Star& s, const double* wt, double* v, double* z,
                    double* w_out, const FgState* fs, const CgState* st, bool nullspace);
// mode 0: the setup (||r_0|| from fs->nrm2, the reference from fs->bsq by ref = REF_*, history[0],
// the first test, restart / haptol into the state); mode 1: a restart (the recomputed ||r||
// tested at the same iteration count, not logged). Both start a cycle: loc = 0, g_0 = ||r||,
// scale = 1 / ||r||
int launch_fg_start(pb_ctx* ctx, const KspLog& lg, FgState* fs, int mode, int ref, int restart,
                    double haptol, int64_t host_iter);
// one Arnoldi step's scalar part: the column from the sums (passes = 2: dots + dots2), the
// happy-breakdown check, the rotations, the estimate logged and tested, the done flag
int launch_fg_step(pb_ctx* ctx, const KspLog& lg, FgState* fs, int passes, int64_t host_iter);
// y = the triangular solve over the live columns; x = x + (((0 + y_0 z_0) + y_1 z_1) + ...) over
// the live count read from the device. force = false: exit at entry when the state is done (a
// restart enqueued ahead); true: pb_ksp_end's build of the cycle the solve ended in
int launch_fg_trisolve(pb_ctx* ctx, const CgState* st, FgState* fs, bool force);
int launch_fg_build(pb_ctx* ctx, double* x, const FgTable& z, const FgState* fs, const CgState* st,
                    bool force, int64_t n);

// ---- pb_ksp_pipecg.cpp: -ksp_type pipecg ----
// pb_ksp_create's share, pb_ksp_begin's setup (as rich_begin), one iteration of pb_ksp_iterate
// (x is updated in place: pb_ksp_end has nothing to add) and pb_ksp_destroy's share
int pipecg_create(pb_ksp* k);
int pipecg_begin(pb_ksp* k, const pb_vec* b, pb_vec* x);
int enqueue_pipecg_iteration(pb_ksp* k);
void pipecg_destroy(pb_ksp* k);

// ---- pb_ksp_pipecg.hip: the small state and its kernels ----
constexpr int kPcgSums = 5;
// sums: gamma = r.u, delta = w.u, sum u^2, sum r^2, sum w of the current vectors -- one reduction
// (split contexts: one allreduce). The tolerances, reason, done flag, update count (CgState::it)
// and history cursor are CgState's (pb_ksp::d_st)
struct PcgState {
  double sums[kPcgSums];
  double bsums[kPcgSums];  // the same sums with b for r and N(M^-1 b) for u and w (nonzero guess)
  double gamma_old, alpha, beta;
  double zsum;  // sum of M^-1 w as a stored-z PC wrote it (the setup with Jacobi / no PC: sum r)
};
// the vectors of an update; w_out = w (in place) but in the engine pass
struct PcgVecs {
  double *z, *q, *s, *p, *x, *r, *u;
  const double* w;
  double* w_out;
};
// *dst = the global sum of v (exits at entry when skip and the state is done, as the two below)
int launch_pcg_sum(pb_ctx* ctx, const double* v, double* dst, const CgState* st, bool skip,
                   int64_t n);
// dst = dinv src + shift, shift = -((dinv *sum) / ntot) (nullspace = 0: no add): fg_z with
// pcg_shift, the expression the engine pass forms on load. dst may be src
int launch_pcg_pcshift(pb_ctx* ctx, const double* src, double* dst, const double* sum,
                       const CgState* st, bool skip, int64_t n, bool nullspace);
// the five sums of (r, u, w) as they are, reduced and allreduced into dst (the setup)
int launch_pcg_sums(pb_ctx* ctx, const double* r, const double* u, const double* w, double* dst,
                    int64_t n);
// One block: reduces the nparts x 5 partials of the update pass into ps->sums (nparts = 0: the
// sums are there already, allreduced), then the scalar step: the norm by -ksp_norm_type logged and
// tested (KSPConvergedDefault), the iteration limit, beta, alpha (the i = 0 branch from the
// device's update count), the done flag. setup: pb_ksp_begin's (ref = REF_*, its = 0), else the
// update count advances first
int launch_pcg_finalize(pb_ctx* ctx, const KspLog& lg, PcgState* ps, const double* parts,
                        int nparts, bool setup, int ref, int64_t host_iter);
// ---- pb_ksp_pipecg.hip: the update pass on the stencil engine (pb_star7.hpp) ----
// The iteration on the 7-point operator with Jacobi / no PC (one rank, wrap planes; PcgLoad /
// PcgEpi): m = dinv w + shift formed on load, n = A m, the eight updates and the five sums of the
// new values; v.w_out is another buffer than v.w. 64 B read, 64 B written per DoF
int launch_pcg_fused(pb_grid* g, const Star& s, const PcgVecs& v, const PcgState* ps,
                     const CgState* st, bool nullspace, int* nparts);
// The same updates and sums from stored m and n, in the engine's tiles, chunks and order of
// summation (the bits of the engine pass): the stored-z PCs, the compact and assembled operators,
// N ranks, tuning pipecg_fused = 0. 80 B read, 64 B written per DoF
int launch_pcg_update(pb_grid* g, const double* m, const double* n, const PcgVecs& v,
                      const PcgState* ps, const CgState* st, int* nparts);

// ---- pb_ksp_guess.cpp: -ksp_guess_type fischer ----
int solve_projected(pb_ksp* k, const pb_vec* b, pb_vec* x, pb_ksp_result* res, double* history,
                    int64_t cap);

}  // namespace pb
#pragma GCC visibility pop
