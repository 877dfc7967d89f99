/* poissbox_gpu.h -- C ABI of the MI355X-native poissbox KSPSolve hot path.
 *
 * Drop-in boundary for 3decomp/poissbox (reference @ /root/reference). The reference is Fortran
 * driving PETSc; each entry point below names the reference interface it replaces. Callers bind
 * it from Fortran through iso_c_binding (poissbox_amd/fortran/poissbox_gpu.f90) or from Python
 * through ctypes (poissbox_amd/api.py). Plain pointers, sizes and opaque handles only.
 *
 * Conventions
 *  - Every function returns int: 0 = PB_OK, > 0 = PB_ERR_*; pb_last_error() describes the last
 *    failure of the calling thread. The reference never checks ierr; we always return it.
 *    Solver divergence is a KSP reason code in pb_ksp_result, not an error.
 *  - Layout: Fortran column-major (i,j,k), i fastest == C [k][j][i]; fp64 everywhere
 *    (src/constants.f90:15 pb_dp). Each rank owns a z-slab of whole planes, with the remainder
 *    planes on the low ranks; the rank-contiguous global order therefore equals natural order.
 *  - One process per GPU. A context spans one GPU; multi-GPU runs create one context per rank
 *    and connect them with RCCL (pb_comm_unique_id + pb_ctx_create). Every "vector" call is
 *    collective over the ranks of the context, exactly like PETSc calls on PETSC_COMM_WORLD.
 *  - Host buffers are borrowed for the duration of a call. The library owns device memory.
 */
#ifndef POISSBOX_GPU_H
#define POISSBOX_GPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PB_VERSION_MAJOR 0
#define PB_VERSION_MINOR 2

enum pb_error {
  PB_OK = 0,
  PB_ERR_ARG = 1,         /* invalid argument / shape */
  PB_ERR_HIP = 2,         /* HIP runtime error (device fault, launch failure) */
  PB_ERR_COMM = 3,        /* RCCL / transport error */
  PB_ERR_ALLOC = 4,       /* out of device or host memory */
  PB_ERR_UNSUPPORTED = 5, /* option or configuration not implemented */
  PB_ERR_STATE = 6        /* call out of order */
};

typedef struct pb_ctx pb_ctx;   /* device + rank + communicator + stream          */
typedef struct pb_grid pb_grid; /* DMDA analogue: periodic 3-D grid, z-slab layout */
typedef struct pb_vec pb_vec;   /* DMCreateGlobalVector analogue (owned slab)      */
typedef struct pb_op pb_op;     /* MatShell(MATOP_MULT = mfmult) analogue           */
typedef struct pb_ksp pb_ksp;   /* KSP analogue                                    */

const char* pb_last_error(void);
int pb_version(int* major, int* minor);
/* src/coefficients.f90:22-48: lapl_1d_coeffs (c = [1, -2, 1] / dx^2) and lapl_star_coeffs (the
 * 3x3x3 box, column-major, of the 7-point star) -- the coefficients every operator here uses. */
int pb_lapl_1d_coeffs(double dx, double c[3]);
int pb_lapl_star_coeffs(double dx, double dy, double dz, double c[27]);

/* ---- context / communicator (replaces MPI_Init + PetscInitialize, src/example.f90:43-47) ---- */
/* 128-byte RCCL unique id; rank 0 creates it and the caller broadcasts it (any channel). */
int pb_comm_unique_id(unsigned char uid[128]);
/* nranks == 1: uid may be NULL. nranks > 1: uid from rank 0's pb_comm_unique_id. The RCCL
 * communicator init is bounded by PB_COMM_TIMEOUT_MS: if not every rank joins in time (a peer
 * died during start-up, or holds another id) the call returns PB_ERR_COMM instead of blocking.
 * The init then still runs on a helper thread inside RCCL's start-up handshake (RCCL's blocking
 * init cannot be cancelled; its non-blocking form would make every later RCCL call of the hot
 * path asynchronous): after PB_ERR_COMM from pb_ctx_create the process should exit rather than
 * retry in-process. */
int pb_ctx_create(int device, int rank, int nranks, const unsigned char* uid, pb_ctx** ctx);
/* Test transport: route halo exchange and allreduce through host callbacks instead of RCCL
 * (lets several ranks share one GPU in tests). Must be called before any grid is created.
 * sendrecv: send `send_lo` (first owned plane) to rank-1 and `send_hi` (last owned plane) to
 * rank+1 (periodic), receive the plane below into recv_lo and the plane above into recv_hi.
 * allreduce: in-place SUM of `count` doubles over all ranks. Return 0 on success. */
typedef int (*pb_sendrecv_fn)(void* user, const double* send_lo, const double* send_hi,
                              double* recv_lo, double* recv_hi, int64_t count);
typedef int (*pb_allreduce_fn)(void* user, double* vals, int count);
int pb_ctx_set_host_transport(pb_ctx* ctx, pb_sendrecv_fn sendrecv, pb_allreduce_fn allreduce,
                              void* user);
/* Host all-to-all for the compact operators' z-slab <-> y-slab transposes: send_counts[p]
 * doubles go to rank p (blocks contiguous in rank order in `send`), recv_counts[p] arrive from
 * rank p (contiguous in rank order in `recv`). Needed only for the compact operator on a split
 * grid with the host transport; RCCL contexts use grouped ncclSend/ncclRecv. */
typedef int (*pb_alltoallv_fn)(void* user, const double* send, const int64_t* send_counts,
                               double* recv, const int64_t* recv_counts);
int pb_ctx_set_host_alltoallv(pb_ctx* ctx, pb_alltoallv_fn alltoallv, void* user);
int pb_ctx_get_rank(const pb_ctx* ctx, int* rank, int* nranks);
/* Launcher-agnostic start (≙ MPI_Init + MPI_Comm_rank/size, src/example.f90:43-47): the rank
 * layout comes from RANK/WORLD_SIZE/LOCAL_RANK (torchrun --no-python), OMPI_COMM_WORLD_* (mpirun)
 * or PMI_RANK/PMI_SIZE; one process = rank 0 of 1 on `device` (-1: LOCAL_RANK). Several ranks
 * take GPU LOCAL_RANK mod visible GPUs (PB_DEVICE overrides) and connect over
 *   PB_TRANSPORT=rccl (default when every rank has its own GPU): rank 0's unique id is passed in
 *     a file PB_RENDEZVOUS_DIR/pb_uid_<job> (default /tmp; job = PB_JOB_ID, else MASTER_PORT,
 *     plus torchrun's TORCHELASTIC_RESTART_COUNT), removed once the communicator is up; a file
 *     last written more than PB_RENDEZVOUS_SLACK_S (120) before the reading process started is
 *     taken for a crashed run's leftover and ignored, with a line on stderr -- until the reader
 *     itself has waited longer than the slack, when it takes the file (a rank started late; a
 *     stale id then fails the bounded init with PB_ERR_COMM) (likewise the shm segment below);
 *   PB_TRANSPORT=shm (default when ranks outnumber GPUs): a built-in POSIX shared-memory host
 *     transport (halo planes and scalar sums; ranks may share one GPU; no all-to-all, so the
 *     compact operators need RCCL or a host alltoallv callback on a split grid). */
int pb_ctx_create_from_env(int device, pb_ctx** ctx);
/* In-place SUM over all ranks of `count` (<= 32) host doubles (≙ MPI_Allreduce(MPI_SUM) of the
 * reference driver's checks, src/example.f90:108,137-147,194). */
int pb_ctx_allreduce_host(pb_ctx* ctx, double* vals, int count);
int pb_ctx_sync(pb_ctx* ctx);  /* stream synchronize (≙ MPI_Barrier for device work) */
int pb_ctx_barrier(pb_ctx* ctx); /* synchronize + all ranks rendezvous */
/* Failure handling on multi-rank contexts (the reference's MPI calls would hang or abort): every
 * host wait is bounded by PB_COMM_TIMEOUT_MS (default 180000) and checks RCCL's asynchronous
 * error; a timeout, an RCCL error or a failing host-transport callback aborts the communicator
 * (ncclCommAbort) and returns PB_ERR_COMM, and every later communicating call on the context
 * returns PB_ERR_COMM at once. *failed = 1 after such a failure. */
int pb_ctx_comm_status(const pb_ctx* ctx, int* failed);
/* What the context communicates over (≙ MPI_Comm_size of PETSC_COMM_WORLD as the transport
 * itself sees it): PB_TRANSPORT_RCCL with the communicator's own ncclCommCount /
 * ncclCommUserRank, PB_TRANSPORT_HOST (host callbacks or the shm transport) with the context's
 * rank layout, or PB_TRANSPORT_NONE (one rank, wrap planes in place) with 1 / 0. */
enum pb_transport { PB_TRANSPORT_NONE = 0, PB_TRANSPORT_RCCL = 1, PB_TRANSPORT_HOST = 2 };
int pb_ctx_comm_info(const pb_ctx* ctx, int* transport, int* comm_nranks, int* comm_rank);
int pb_ctx_destroy(pb_ctx* ctx);
/* Per-kernel timing with HIP events on the context's stream (off by default). */
int pb_ctx_set_timing(pb_ctx* ctx, int enable);
/* Timing restricted to the comma-separated phase names in `only` (NULL or "": every phase), and
 * to one launch in `every` of each such phase: a timed region keeps its event records off the
 * other launches (bench.py times its roofline kernel inside the timed steps this way). */
int pb_ctx_set_timing_filter(pb_ctx* ctx, int enable, const char* only, int every);
/* name: "stencil", "cg_pass_a", "cg_pass_b", ...; returns total ms and launch count since reset */
int pb_ctx_get_timing(pb_ctx* ctx, const char* name, double* total_ms, int64_t* count);
/* The per-launch durations behind pb_ctx_get_timing (the first 65536 since the last reset):
 * copies min(cap, *count) of them into ms; *count = how many there are. Lets a caller tell the
 * launches that ran from those that exited at entry (a converged solve's enqueued-ahead work). */
int pb_ctx_get_timing_samples(pb_ctx* ctx, const char* name, float* ms, int64_t cap,
                              int64_t* count);
int pb_ctx_reset_timing(pb_ctx* ctx);
/* HBM calibration of this process's device (no reference counterpart; bench.py reports it beside
 * the matvec's rate): a flat fp64 copy of n doubles -- 16-B loads, non-temporal 16-B stores, the
 * standalone matvec's access mix without its stencil -- `reps` timed launches after two warm-ups;
 * GB/s counted as 16 B per element. Allocates and frees its own 2 x n doubles. */
int pb_ctx_copy_probe(pb_ctx* ctx, int64_t n, int reps, double* best_gbps, double* median_gbps);
/* The same copy from x into y (both of one grid; y is overwritten): the matvec's own buffers,
 * so a placement-dependent rate shows up beside the matvec x -> y. */
int pb_vec_copy_probe(const pb_vec* x, pb_vec* y, int reps, double* best_gbps,
                      double* median_gbps);

/* ---- tuning (kernel selection and launch shapes; no reference counterpart) ----
 * Process-wide table of the launchers' parameters (INTEGRATION.md lists the names: z-march
 * alternation, tile heights, multigrid kernel thresholds, spectral-PC tile shapes, ...). Unset
 * names take the measured defaults; every setting selects kernels that give the same results to
 * the bits (or, for tile heights, to the reduction order of the CG sums), so it is a speed knob,
 * never a correctness one. The library reads no such setting from the environment. Unknown names
 * return PB_ERR_ARG. Set before the calls it should affect; not thread-safe against running calls. */
int pb_tune_set(const char* name, int value);
int pb_tune_get(const char* name, int* value, int* is_set);
int pb_tune_reset(void);

/* ---- slab partition (replaces DMDACreate3d's PETSC_DECIDE split, src/poissbox.f90:191-202) ---- */
/* Pure host function: remainder planes go to the low ranks (README.md:30-32's 22/21/21). */
int pb_slab_partition(int64_t nz, int nranks, int rank, int64_t* kstart, int64_t* nk);

/* ---- grid (replaces initialise_grid, src/poissbox.f90:183-204) ---- */
/* Periodic in x, y, z; spacing h = L/n (src/example.f90:33-35). n >= 3 in every direction. */
int pb_grid_create(pb_ctx* ctx, const int64_t n[3], const double L[3], pb_grid** grid);
/* ≙ DMDAGetCorners (src/poissbox.f90:107): 0-based start and owned size of this rank */
int pb_grid_get_corners(const pb_grid* grid, int64_t start[3], int64_t size[3]);
int pb_grid_get_info(const pb_grid* grid, int64_t n[3], double h[3], int64_t* nlocal);
int pb_grid_destroy(pb_grid* grid);

/* ---- vectors (replace DMCreateGlobalVector/VecDuplicate/VecSet/VecCopy/VecAXPY/VecAYPX/
 *      VecScale/VecDot/VecNorm/VecSum/DMDAVecGetArrayF90, src/example.f90:79-83,175-195,217-231) */
int pb_vec_create(pb_grid* grid, pb_vec** v);
int pb_vec_duplicate(const pb_vec* v, pb_vec** out);
int pb_vec_destroy(pb_vec* v);
int pb_vec_set(pb_vec* v, double alpha);
int pb_vec_copy(const pb_vec* src, pb_vec* dst);
int pb_vec_axpy(pb_vec* y, double alpha, const pb_vec* x);  /* y = y + alpha*x */
int pb_vec_aypx(pb_vec* y, double beta, const pb_vec* x);   /* y = x + beta*y  */
int pb_vec_scale(pb_vec* v, double alpha);
int pb_vec_dot(const pb_vec* x, const pb_vec* y, double* out); /* global sum x.y   */
int pb_vec_norm2(const pb_vec* v, double* out);              /* global ||v||_2    */
int pb_vec_sum(const pb_vec* v, double* out);                /* global sum v      */
/* ≙ VecMDot / VecMAXPY: nv vectors (0 <= nv <= 16, else PB_ERR_ARG; nv = 0 returns at once) of
 * x's / y's grid (else PB_ERR_ARG) in ONE pass over memory; collective over the ranks.
 * pb_vec_mdot: out[i] = global sum x . y[i]; y[i] may be x. x and every y[i] are read once
 * (8 (nv + 1) B/DoF); per-block partial sums reduced in a fixed order, one allreduce of all nv
 * values, one copy to the host: deterministic run to run.
 * pb_vec_maxpy: y += sum_i alpha[i] x[i]; no x[i] may be y (PB_ERR_ARG). 8 (nv + 2) B/DoF. Every
 * element is evaluated in the order ((y + a0 x0) + a1 x1) + ... with every product and every sum
 * rounded (no FMA contraction), in the vector body and in the tail of an odd length alike. */
int pb_vec_mdot(const pb_vec* x, int nv, const pb_vec* const* y, double* out);
int pb_vec_maxpy(pb_vec* y, int nv, const double* alpha, const pb_vec* const* x);
/* Owned values in natural (i fastest) order of this rank's slab; count = nlocal. */
int pb_vec_set_values_host(pb_vec* v, const double* owned);
int pb_vec_get_values_host(const pb_vec* v, double* owned);
/* Synthetic input: v[g] = 2*(0.5 - U), U = SplitMix64(seed ^ g) >> 11 * 2^-53,
 * g = global linear index; decomposition independent (src/example.f90:180-181 distribution). */
int pb_vec_set_random(pb_vec* v, uint64_t seed);
/* Borrowed device pointer to the owned slab (≙ DMDAVecGetArrayF90 on device memory). */
int pb_vec_device_ptr(pb_vec* v, double** dptr, int64_t* nlocal);

/* ---- operator (replaces MatCreateShell + MatShellSetOperation(MATOP_MULT, mfmult),
 *      src/poissbox.f90:242-267, and mfmult itself, :300-322) ---- */
enum pb_op_kind {
  PB_OP_STAR7 = 0,       /* 2nd-order 7-point star, compute_lapl_pointwise (:84-148)        */
  PB_OP_COMPACT = 1,     /* 6th-order compact lapl = div(grad f), compact_schemes.f90:17-37  */
  PB_OP_ASSEMBLED27 = 2, /* assembled BOX AIJ P (coefficients.f90:50-113), 27-entry rows     */
  PB_OP_VARCOEF = 3      /* 7-point div(beta grad), beta per cell (no reference counterpart:  */
                         /* what a caller's own MATOP_MULT supplies there, :226-267)          */
};
/* PB_OP_VARCOEF: y = div(beta grad x) in flux form, beta cell-centred on the operator's grid, the
 * face value between two cells their arithmetic or harmonic mean. With c_d = 1 / h_d^2 (the axis
 * coefficients of pb_lapl_1d_coeffs for the operator's deltas), the neighbours n taken in the
 * 7-point operator's order without the centre (z-, y-, x-, x+, y+, z+) and every product, sum and
 * quotient rounded:
 *   face(a, b) = 0.5 * (a + b)   |   (2.0 * (a * b)) / (a + b)
 *   g_n = c_d * face(beta_n, beta_c),   t_n = g_n * (x_n - x_c)
 *   y_c    = ((((t_z- + t_y-) + t_x-) + t_x+) + t_y+) + t_z+
 *   diag_c = -(((((g_z- + g_y-) + g_x-) + g_x+) + g_y+) + g_z+)
 * The matrix is symmetric to the bit and constants are in its null space to the bit (KSP's constant
 * null-space handling applies unchanged). 24 B/DoF per apply: x and beta read, y written; the
 * operator keeps one field and two ghost planes of beta. A fresh operator has beta = 1, arithmetic.
 * As A of a KSP it runs every ksp_type through the unfused iterations with any constant-coefficient
 * P behind every pc_type (the classic pairing: -pc_type mg | fft from a PB_OP_STAR7 P with
 * representative deltas); as P it supports -pc_type none and jacobi (z = r / diag, the reciprocal
 * diagonal stored by the KSP and rebuilt after pb_op_set_coefficient / pb_op_set_deltas); sor, mg
 * and fft from a variable P return PB_ERR_UNSUPPORTED at pb_ksp_create. -ksp_cg_single_reduction
 * runs the KSPSolve_CG iteration on it. */
enum pb_coef_mean { PB_COEF_ARITHMETIC = 0, PB_COEF_HARMONIC = 1 };
/* PB_OP_ASSEMBLED27 applies P x with PETSc's AIJ row sums: stored columns ascending on one rank
 * (MatMult_SeqAIJ), owned columns then off-rank columns on several (MatMult_MPIAIJ) -- so rows on
 * the periodic seams and slab boundaries differ from PB_OP_STAR7 at rounding level, and
 * src/example.f90:235-261's ||A x - P x|| is the reference's rounding-level value, not 0. As a
 * KSP operator (A = P, src/example.f90:62-64) it runs the unfused CG iteration. */
int pb_op_create(pb_grid* grid, int kind, const double deltas[3], pb_op** op);
int pb_op_apply(pb_op* op, const pb_vec* x, pb_vec* y); /* ≙ MatMult(A, x, y) */
/* ≙ assemble_laplacian(da, dx, dy, dz, M) (src/coefficients.f90:50-113): (re)set the spacings
 * the operator's coefficients are built from (lapl_star_coeffs). */
int pb_op_set_deltas(pb_op* op, const double deltas[3]);
/* (PB_ERR_UNSUPPORTED on PB_OP_VARCOEF, whose diagonal is a field: pb_op_get_diagonal_vec) */
int pb_op_get_diagonal(const pb_op* op, double* diag);  /* constant diagonal of the 7-pt P */
/* Sets the coefficient of a PB_OP_VARCOEF operator (PB_ERR_STATE on another kind, or between
 * pb_ksp_begin and pb_ksp_end of a KSP that holds the operator). Collective. beta is copied into
 * storage the operator owns and its two ghost planes are filled by one halo exchange; the caller's
 * vector is not kept. Every value must be finite and > 0 (a device reduction over all ranks checks
 * it); PB_ERR_ARG for a value that is not, a vector of another grid or a mean outside
 * pb_coef_mean. An error leaves the operator as it was. A KSP holding the operator may be reused:
 * what it derived from the old coefficient is rebuilt by its next solve. */
int pb_op_set_coefficient(pb_op* op, const pb_vec* beta, int mean);
/* The coefficient (copied into beta, a vector of the operator's grid) and the mean in force;
 * either may be NULL. PB_ERR_STATE on another kind. */
int pb_op_get_coefficient(const pb_op* op, pb_vec* beta, int* mean);
/* The mass term of a PB_OP_VARCOEF operator: A = div(beta grad) - q with q_c = s * m_c (m NULL:
 * q_c = s), the operator of an implicit diffusion / viscous / heat step (rho/dt) u - div(mu grad u)
 * up to the sign. Every operation rounded:
 *   y_c    = S6_c - q_c * x_c        S6_c: the six-term flux sum above
 *   diag_c = (-G6_c) - q_c           G6_c: the six-term sum of the g_n above
 * A stays symmetric to the bit, A 1 = -q to the bit, and A is negative definite as soon as q > 0
 * somewhere. The term is on iff s != 0; with it off every launch is the one without the term. A
 * scalar mass moves the 24 B/DoF of the plain apply, a field 32 B/DoF.
 * Collective. PB_ERR_STATE on another kind, or between pb_ksp_begin and pb_ksp_end of a KSP that
 * holds the operator. m is copied into storage the operator owns (one field, no ghost planes: q is
 * point-local; freed when a later call passes NULL). Every value of m must be finite and >= 0 (zero:
 * a region without mass; a device reduction over all ranks checks it), s finite and >= 0;
 * PB_ERR_ARG otherwise or for a vector of another grid. An error leaves the operator as it was. A
 * fresh operator has m absent and s = 0. A KSP holding the operator may be reused: the variable
 * Jacobi's diagonal, the variable sor / mg levels (pb_ksp_pc_set_coefficient_from: q_0 = s * m,
 * q_(l+1) the mean of a cell's 8 children) and Chebyshev's estimated bounds are rebuilt by its next
 * solve -- a time loop with a changing dt calls pb_op_set_mass(op, rho, 1 / dt) per step.
 * A KSP whose A has the term on solves a nonsingular system: with the option nullspace = 1
 * pb_ksp_solve / pb_ksp_begin return PB_ERR_STATE before anything is enqueued; create it with
 * nullspace = 0. The rule reads A only (a mass in P or in the PC's coefficient operator alone is a
 * nonsingular preconditioner of a singular A). */
int pb_op_set_mass(pb_op* op, const pb_vec* m, double s);
/* The mass field (copied into m; ones where the operator's is absent) and s; either may be NULL. */
int pb_op_get_mass(const pb_op* op, pb_vec* m, double* s);
/* ≙ MatGetDiagonal: diag_c above (with the mass term) for PB_OP_VARCOEF, the constant diagonal broadcast for
 * PB_OP_STAR7 / PB_OP_ASSEMBLED27 (PB_ERR_UNSUPPORTED for PB_OP_COMPACT). */
int pb_op_get_diagonal_vec(const pb_op* op, pb_vec* diag);
/* MAC-grid (staggered) gradient, projection and divergence of PB_OP_VARCOEF and PB_OP_STAR7
 * (beta = 1): the operators G (cell to face) and D (face to cell) with D G = A to rounding, the two
 * parts of a projection step around the solve. A face field is three cell-indexed vectors of the
 * operator's grid; u_d(c) lives on the face between cell c and cell c + e_d (the plus face). All
 * axes periodic. With r_d = 1.0 / h_d from the operator's deltas (one rounded division), face() the
 * operator's mean above, and every product, sum and quotient rounded:
 *   G_d(c) = (r_d * face(beta_(c+e_d), beta_c)) * (p_(c+e_d) - p_c)      pb_op_mac_grad
 *   u_d(c) <- u_d(c) - (s * G_d(c))                                      pb_op_mac_project, in place
 *   D(c)   = s * ((((ux(c) - ux(c-ex)) * r_x) + ((uy(c) - uy(c-ey)) * r_y))
 *                 + ((uz(c) - uz(c-ez)) * r_z))                          pb_op_mac_div
 * On PB_OP_STAR7 G_d(c) = r_d * (p_(c+e_d) - p_c), the bits of a PB_OP_VARCOEF with beta = 1 under
 * either mean. The operator's mass term is no part of G: it is ignored. Because G uses the
 * operator's own face coefficients (the same mean, beta and deltas) and D is the adjoint difference,
 * a field projected with the solved p is discretely divergence-free to the solve's residual.
 * The projection step of a variable-density flow (beta = 1 / rho, pb_op_set_coefficient):
 *   pb_op_mac_div(A, 1 / dt, ustar, b);        b = (1/dt) div u*
 *   pb_ksp_solve(ksp, b, p);                   div(beta grad p) = b
 *   pb_op_mac_project(A, p, dt, ustar);        u = u* - dt beta_f grad p
 * Collective (split grids: one halo exchange of p for grad / project, of uz for div, none of u in
 * project). They only read the operator and may be called between pb_ksp_begin and pb_ksp_end.
 * Stream ordered like pb_op_apply. grad: 16 B read + 24 B written per DoF (PB_OP_STAR7: 8 + 24),
 * project 64 B/DoF (56), div 24 + 8. PB_ERR_UNSUPPORTED for PB_OP_COMPACT and PB_OP_ASSEMBLED27;
 * PB_ERR_ARG for a vector of another grid, three components that are not distinct vectors, p among
 * g / u, out among u, or a non-finite s. An error leaves every output untouched. */
int pb_op_mac_grad(const pb_op* op, const pb_vec* p, pb_vec* const g[3]);           /* g_d = G_d(p)    */
int pb_op_mac_project(const pb_op* op, const pb_vec* p, double s, pb_vec* const u[3]); /* u_d -= s G_d(p) */
int pb_op_mac_div(const pb_op* op, double s, const pb_vec* const u[3], pb_vec* out);   /* out = s D(u)    */
int pb_op_destroy(pb_op* op);
/* ≙ MatGetOwnershipRange / VecGetOwnershipRange (src/example.f90:137-147): global row range
 * [first, next) owned by this rank (rank-contiguous natural order of the z-slab split). */
int pb_op_get_ownership_range(const pb_op* op, int64_t* first, int64_t* next);
int pb_vec_get_ownership_range(const pb_vec* v, int64_t* first, int64_t* next);

/* ---- KSP (replaces solve(P, A, x, b), src/poissbox.f90:269-298 -> KSPSolve) ---- */
/* -ksp_type (src/poissbox.f90:269-298: solve hands its KSP to KSPSetFromOptions, so the type is the
 * caller's choice; the reference README puts richardson on the multigrid levels).
 *  PB_KSP_PREONLY (PETSc KSPSolve_PREONLY): x = N(M^-1 b), one PC application and the constant
 *    null-space removal KSP adds (nullspace = 1). its = 1, reason PB_KSP_CONVERGED_ITS, rnorm =
 *    rnorm0 = 0, nhist = 0: no norm, no reduction, no NaN check. b and x must be distinct
 *    (PB_ERR_ARG). With PB_PC_FFT the mean subtraction is skipped: P^+ zeroes mode 0 itself, the
 *    result's mean is at rounding level (|mean| / max|x| = 1.2e-19 on the CPU oracle at 32x40x48),
 *    and subtracting it would add a 24 B/DoF pass (sum, then subtract) to a 5-pass solve. With
 *    -pc_type fft this is the direct solve of P's symbol. initial_guess_nonzero or a guess_type is
 *    PB_ERR_ARG at pb_ksp_create (PETSc: "preonly doesn't make sense with nonzero initial guess;
 *    you probably want richardson"); pb_ksp_begin / iterate / end return PB_ERR_UNSUPPORTED.
 *  PB_KSP_RICHARDSON (PETSc KSPSolve_Richardson, PC_LEFT, preconditioned norm, default test):
 *    x += richardson_scale N(M^-1 (b - A x)); iteration i logs ||z_i||, tests it with its = i,
 *    and updates if the test gives nothing; after max_it updates one more norm is logged and
 *    tested before PB_KSP_DIVERGED_ITS: nhist = its + 1 always. b and x must be distinct
 *    (PB_ERR_ARG: b is read by every update). Works with every operator, PC,
 *    initial_guess_nonzero, guess_type fischer and the split form, as PB_KSP_CG does.
 *  PB_KSP_CHEBYSHEV (PETSc KSPSolve_Chebyshev, PC_LEFT, preconditioned norm, default test): the
 *    accelerated stationary iteration for a spectrum of M^-1 A inside [emin, emax] -- no inner
 *    product but the norm's. With scale = 2 / (emax + emin), alpha = 1 - scale emin,
 *    mu = 1 / alpha, omegaprod = 2 / alpha: iteration i logs ||z_i||, z_i = N(M^-1 (b - A y_i)), and tests it with
 *    its = i exactly as PB_KSP_RICHARDSON does (nhist = its + 1 always); update 0 is Richardson's
 *    with richardson_scale = scale, y_1 = y_0 + scale z_0; update i >= 1 is
 *    y_(i+1) = omega_i ((y_i - y_(i-1)) + scale z_i) + y_(i-1), omega_i = omegaprod rho_i,
 *    rho_i = 1 / (2 mu - rho_(i-1)), rho_0 = 1 / mu. rho_i is PETSc's c_i / c_(i+1): its recurrence
 *    c_(k+1) = 2 mu c_k - c_(k-1) overflows in long runs, the ratio does not.
 *    Bounds: pb_ksp_chebyshev_opts emin / emax, both negative with -pc_type none (A is the Laplacian,
 *    negative semi-definite; Jacobi's diagonal is negative too, so M^-1 A is positive with it).
 *    Left at 0, 0 they are estimated once per operator pair (pb_ksp_chebyshev_get_eigenvalues).
 *    b and x must be distinct (PB_ERR_ARG). Works with every operator, PC, initial_guess_nonzero,
 *    guess_type fischer and the split form, as PB_KSP_RICHARDSON does; every solve and every
 *    pb_ksp_begin restarts rho.
 *  PB_KSP_FGMRES (PETSc KSPSolve_FGMRES / KSPFGMRESCycle: restarted flexible GMRES, classical
 *    Gram-Schmidt, right preconditioning only): the one type here that tolerates a preconditioner
 *    that is not one fixed symmetric linear operator. Step k of a cycle stores z_k = N(M^-1 v_k),
 *    forms w = A z_k, h_j = <w, v_j> (j <= k), w -= sum h_j v_j, h_(k+1,k) = ||w||, rotates the
 *    column with the stored Givens rotations and forms the new one; |g_(k+1)| -- the true residual
 *    norm ||b - A x|| in exact arithmetic -- is the iteration's norm, logged and tested by the
 *    default test. After `restart` steps (pb_ksp_fgmres_opts, default 30) x += sum y_j z_j from
 *    the triangular solve, r = b - A x is recomputed, and its norm starts the next cycle: it is
 *    tested at the same iteration count and not logged as an extra entry (nhist = its + 1;
 *    entry k is the estimate after k iterations). max_it reached inside a cycle builds the
 *    solution from the partial cycle: PB_KSP_DIVERGED_ITS. The norm type is unpreconditioned (the
 *    default here) or none; the reference norm with a nonzero guess is the one
 *    -ksp_norm_type unpreconditioned gives PB_KSP_CG (||b||, and the two
 *    converged_use_*_initial_residual_norm switches). b and x must be distinct. guess_type
 *    fischer is PB_ERR_UNSUPPORTED with it. The KSP keeps up to 2 restart fields beside its
 *    work vectors (allocated in chunks as a cycle first reaches them). On the
 *    7-point operator with Jacobi / no PC (one rank) a step starts with one engine pass that forms
 *    and stores v_k and z_k and writes A z_k; there the mean of z_k is taken from the sum of the
 *    unnormalised direction (equal in exact arithmetic to the mean over z_k).
 *  PB_KSP_PIPECG (PETSc KSPSolve_PIPECG, Ghysels & Vanroose: pipelined CG, PC_LEFT, default test):
 *    CG in exact arithmetic with ONE reduction per iteration, on every operator and with every
 *    PC (the PC is applied to a stored vector like any other) -- what cg_single_reduction gives
 *    the 7-point operator with Jacobi / no PC only. r = b - A x, u = N(M^-1 r), w = A u; iteration
 *    i: gamma = r.u, delta = w.u and the norm's sum in one reduction; m = N(M^-1 w), n = A m;
 *    the norm is logged and tested with its = i; beta = gamma / gamma_old (0 at i = 0),
 *    alpha = gamma / (delta - (beta / alpha_old) gamma) (gamma / delta at i = 0); z = n + beta z,
 *    q = m + beta q, s = w + beta s, p = u + beta p; x += alpha p, r -= alpha s, u -= alpha q,
 *    w -= alpha z. nhist = its + 1 always; entry k is the norm after k updates. After max_it
 *    updates one more norm is logged and tested before PB_KSP_DIVERGED_ITS (PETSc's loop makes
 *    one more update first: a deviation). All four norm types (preconditioned
 *    ||u||, the default; unpreconditioned ||r||; natural sqrt|gamma|; none) come out of the one
 *    reduction; the reference norm with a nonzero guess follows PB_KSP_CG's rules. There is no
 *    indefinite-PC or indefinite-matrix test (PETSc's pipecg has none): a zero or non-finite
 *    denominator surfaces as PB_KSP_DIVERGED_NANORINF at the next test. b and x must be
 *    distinct. guess_type fischer is PB_ERR_UNSUPPORTED with it. It moves 128 B/DoF per
 *    iteration where CG moves 56: on one GPU CG is faster; the type is there for what it does
 *    between ranks and for callers who want the method. With sor / mg / fft the mean of M^-1 w
 *    is a second, one-double allreduce. The KSP keeps 8 fields (9 off the engine path;
 *    INTEGRATION.md). Parity unpinned: written from knowledge of pipecg.c, pinned to a numpy
 *    restatement (tests/pipecg_restatement.py).
 * cg_single_reduction is a CG option: the other types ignore it. */
enum pb_ksp_type {
  PB_KSP_CG = 0, PB_KSP_PREONLY = 1, PB_KSP_RICHARDSON = 2, PB_KSP_CHEBYSHEV = 3,
  PB_KSP_FGMRES = 4, PB_KSP_PIPECG = 5
};
/* seed of the noise vector (pb_vec_set_random) the Chebyshev eigenvalue estimate starts from */
#define PB_CHEBYSHEV_ESTEIG_SEED 20240607ULL
/* PB_PC_FFT (-pc_type fft): z = P^+ r by separable Hartley transforms with P's symbol (the compact
 * operator's when P is PB_OP_COMPACT, else the 7-point star's); periodic, power-of-two extents in
 * 64..1024. Not in the reference: the spectrally exact PC for config 5. */
enum pb_pc_type { PB_PC_NONE = 0, PB_PC_JACOBI = 1, PB_PC_SOR = 2, PB_PC_MG = 3, PB_PC_FFT = 4 };
/* -ksp_guess_type (PETSc KSPGuess): how pb_ksp_solve forms its initial guess */
enum pb_guess_type { PB_GUESS_NONE = 0, PB_GUESS_FISCHER = 1 };
/* PETSc KSPConvergedReason values */
enum pb_ksp_reason {
  PB_KSP_ITERATING = 0, PB_KSP_CONVERGED_RTOL = 2, PB_KSP_CONVERGED_ATOL = 3,
  PB_KSP_CONVERGED_ITS = 4, PB_KSP_DIVERGED_ITS = -3, PB_KSP_DIVERGED_DTOL = -4,
  PB_KSP_DIVERGED_INDEFINITE_PC = -8, PB_KSP_DIVERGED_NANORINF = -9,
  PB_KSP_DIVERGED_INDEFINITE_MAT = -10,
  /* PB_KSP_FGMRES: the new direction vanished (||w|| below the happy-breakdown bound) -- with
   * -ksp_norm_type none that ends the solve as converged, otherwise the default test sees the
   * estimate 0 first and DIVERGED_BREAKDOWN is left for a test that still gives nothing */
  PB_KSP_DIVERGED_BREAKDOWN = -5, PB_KSP_CONVERGED_HAPPY_BREAKDOWN = 7
};
typedef struct {
  double rtol;       /* -ksp_rtol   (PETSc default 1e-5)  */
  double atol;       /* -ksp_atol   (1e-50)               */
  double dtol;       /* -ksp_divtol (1e5)                 */
  int64_t max_it;    /* -ksp_max_it (10000)               */
  int ksp_type;      /* -ksp_type cg|preonly|richardson|chebyshev|fgmres|pipecg */
  int pc_type;       /* -pc_type none|jacobi|sor|mg       */
  int nullspace;     /* constant null space (src/poissbox.f90:285-291), default 1 */
  int monitor;       /* -ksp_monitor: print ||z_k|| per iteration after the solve (rank 0) */
  int converged_reason; /* -ksp_converged_reason */
  int check_every;   /* host polls the device convergence flag every N iterations (default 8) */
  int mg_levels;     /* -pc_mg_levels: multigrid levels (0 = as many as the grid allows)      */
  int mg_coarse_its; /* -pc_mg_coarse_its: symmetric red-black sweeps on the coarsest level (8) */
  double sor_omega;  /* -pc_sor_omega: SOR relaxation factor (1.0 = Gauss-Seidel)              */
  int cg_single_reduction; /* -ksp_cg_single_reduction (PETSc KSPCGUseSingleReduction): the
                        iteration of KSPSolve_CG_SingleReduction -- one reduction per iteration
                        (z'z, z'r, z'Az together), p'w by its recurrence. Equal to KSPSolve_CG in
                        exact arithmetic. Runs as two engine passes on the 7-point operator with
                        -pc_type jacobi|none; with other operators / PCs the KSPSolve_CG iteration
                        runs (default 0) */
  int initial_guess_nonzero; /* -ksp_initial_guess_nonzero (KSPSetInitialGuessNonzero): the solve
                        starts from the x passed in, r0 = b - A x0 (x0 is taken as it is: no
                        null-space projection), and x accumulates onto it. The stopping reference
                        is then not ||z_0|| but the preconditioned, null-space-removed norm of
                        the right-hand side ||N(M^-1 b)|| (KSPConvergedDefault), or ||z_0|| when
                        that is exactly 0; ttol = max(rtol * rnorm0, atol) and the dtol test use
                        it, pb_ksp_result.rnorm0 reports it; history[0] stays ||z_0|| of the
                        actual initial residual. 0 (default): x0 = 0, the x passed in is
                        overwritten */
  int converged_use_initial_residual_norm; /* -ksp_converged_use_initial_residual_norm
                        (KSPConvergedDefaultSetUIRNorm): with a nonzero guess the reference is
                        ||z_0|| of the initial residual (no extra PC application) */
  int converged_use_min_initial_residual_norm; /* -ksp_converged_use_min_initial_residual_norm
                        (KSPConvergedDefaultSetUMIRNorm): min(||N(M^-1 b)||, ||z_0||). Setting
                        both is PB_ERR_ARG, as in PETSc. Neither has an effect without a guess */
  int guess_type;    /* -ksp_guess_type none|fischer (PETSc KSPGuessFischer, model 1): pb_ksp_solve
                        projects b onto the span of the last solves' directions for its initial
                        guess, runs as with initial_guess_nonzero = 1 (whatever that field says; the
                        x passed in is ignored and overwritten), and adds the solution's new
                        direction afterwards. The KSP keeps 2 maxl + 1 vectors. Default none */
  int guess_fischer_model; /* -ksp_guess_fischer_model <model>[,<maxl>]: only model 1 (2 and 3:
                        PB_ERR_UNSUPPORTED) */
  int guess_fischer_maxl;  /* stored directions, 1..16 (else PB_ERR_ARG), default 10; when the
                        space is full the next solve restarts it from its solution alone */
  double richardson_scale; /* -ksp_richardson_scale (PETSc KSPRichardsonSetScale), default 1.0;
                        must be finite (PB_ERR_ARG). -ksp_richardson_self_scale is parsed and
                        PB_ERR_UNSUPPORTED */
} pb_ksp_opts;
/* The settings of PB_KSP_CHEBYSHEV (PETSc KSPChebyshevSetEigenvalues, KSPChebyshevEstEigSet).
 * They have a struct of their own, set on the KSP after pb_ksp_create (pb_ksp_chebyshev_set_opts),
 * because the layout of pb_ksp_opts is pinned: a KSP that was given none runs with the defaults. */
typedef struct {
  double emin, emax; /* -ksp_chebyshev_eigenvalues emin,emax: finite, non-zero, of one sign,
                        emax > emin (else PB_ERR_ARG); 0, 0 (default): estimate them */
  double esteig[4];  /* -ksp_chebyshev_esteig a,b,c,d (0, 0.1, 0, 1.1): emin = a min + b max,
                        emax = c min + d max of the estimated extremes; finite */
  int esteig_steps;  /* -ksp_chebyshev_esteig_steps: Lanczos steps of the estimate, 1..64 (else
                        PB_ERR_ARG), default 10. -ksp_chebyshev_esteig_noisy false is
                        PB_ERR_UNSUPPORTED: the estimate always starts from noise */
} pb_ksp_chebyshev_opts;
/* The level smoother of PB_PC_MG (PETSc's -mg_levels_* family; the reference README.md:43-44
 * puts richardson + sor on the levels). Like pb_ksp_chebyshev_opts a struct of its own, set on the
 * KSP after pb_ksp_create (pb_ksp_pc_mg_set_opts): a KSP that was given none, or the defaults,
 * runs the V(1,1) red-black SOR cycle with its fused passes, one-launch tail and agglomeration.
 *  richardson + sor: max_it red-black sweeps per leg, pre-smoothing max_it x (red, black),
 *    post-smoothing max_it x (black, red), omega = -pc_sor_omega. levels_richardson_scale must
 *    be 1 (else PB_ERR_UNSUPPORTED).
 *  richardson + jacobi: damped Jacobi, y += s D^-1 (b - A y), s = levels_richardson_scale.
 *  chebyshev + jacobi: PB_KSP_CHEBYSHEV's recurrence above with M = D, restarted at every
 *    smoothing call (rho_0 = 1 / mu), no null-space projection, no norm:
 *    y_1 = y_0 + scale D^-1 r_0, y_(i+1) = omega_i ((y_i - y_(i-1)) + scale D^-1 r_i) + y_(i-1),
 *    every operation rounded. Pre-smoothing starts from zero (y_1 = scale D^-1 b).
 *  chebyshev + sor: PB_ERR_UNSUPPORTED.
 * Bounds of chebyshev: levels_eigenvalues, or (0, 0) the esteig transform of (0, 2) -- D^-1 A of
 * the periodic 7-point operator with even extents has the smallest eigenvalue 0 and the largest
 * exactly 2 on every level, so emin = 2 b, emax = 2 d: [0.2, 2.2] by default. Deviation from
 * PETSc, which estimates the largest eigenvalue with a Krylov run per level: no estimation pass
 * runs here, the bounds are the same on every level, every rank and every run.
 * A non-default smoother (or max_it > 1) runs per-level launches: the one-launch coarse tail and
 * the agglomerated coarse levels of a decomposed grid are bypassed. The coarsest level stays
 * -pc_mg_coarse_its symmetric red-black SOR sweeps whatever the level smoother is. */
enum pb_mg_levels_ksp { PB_MG_LEVELS_RICHARDSON = 0, PB_MG_LEVELS_CHEBYSHEV = 1 };
enum pb_mg_levels_pc { PB_MG_LEVELS_SOR = 0, PB_MG_LEVELS_JACOBI = 1 };
typedef struct {
  int levels_ksp_type;      /* -mg_levels_ksp_type richardson|chebyshev   (richardson) */
  int levels_pc_type;       /* -mg_levels_pc_type sor|jacobi              (sor)        */
  int levels_ksp_max_it;    /* -mg_levels_ksp_max_it: sweeps / steps per leg, 1..8 (1)  */
  double levels_richardson_scale; /* -mg_levels_ksp_richardson_scale (1.0), finite, > 0 */
  double levels_eigenvalues[2];   /* -mg_levels_ksp_chebyshev_eigenvalues emin,emax; 0,0: derive */
  double levels_esteig[4];        /* -mg_levels_ksp_chebyshev_esteig a,b,c,d (0, 0.1, 0, 1.1) */
} pb_pc_mg_opts;
/* The settings of PB_KSP_FGMRES (PETSc KSPGMRESSetRestart, KSPGMRESSetHapTol,
 * KSPGMRESSetCGSRefinementType): a struct of their own, set on the KSP after pb_ksp_create
 * (pb_ksp_fgmres_set_opts), as pb_ksp_chebyshev_opts is. */
enum pb_fgmres_refine { PB_FGMRES_REFINE_NEVER = 0, PB_FGMRES_REFINE_ALWAYS = 2 };
typedef struct {
  int restart;        /* -ksp_gmres_restart: steps per cycle, 1..64 (else PB_ERR_ARG), default 30 */
  double haptol;      /* -ksp_gmres_haptol: happy-breakdown tolerance, finite and > 0 (1e-30) */
  int cgs_refinement; /* -ksp_gmres_cgs_refinement_type refine_never|refine_always
                         (PB_FGMRES_REFINE_*; refine_ifneeded: PB_ERR_UNSUPPORTED). refine_always
                         runs the multi-dot / multi-axpy pair twice per step and adds the second
                         coefficients into the Hessenberg column */
} pb_ksp_fgmres_opts;
typedef struct {
  int reason;
  int64_t its;
  double rnorm;      /* the last norm of the KSP's norm type (pb_ksp_set_norm_type): ||z||_2 by
                        default (KSP_NORM_PRECONDITIONED), ||r||_2, sqrt(|r.z|), or 0 with none */
  double rnorm0;     /* the stopping reference, in the same norm */
  int64_t nhist;     /* residual norms logged (≙ KSPGetResidualHistory's count): its + 1, or its
                        after a breakdown exit (beta = 0, indefinite PC / matrix) */
} pb_ksp_result;
int pb_ksp_opts_default(pb_ksp_opts* opts);
/* Parses PETSc-style options (-ksp_type cg|preonly|richardson|chebyshev|fgmres|pipecg,
 * -ksp_richardson_scale,
 * -pc_type,
 * -ksp_rtol, -ksp_atol, -ksp_divtol, -ksp_max_it, -ksp_monitor, -ksp_converged_reason, -pc_mg_levels, -pc_mg_coarse_its,
 * -pc_sor_omega, and the PetscOptionsBool flags -ksp_cg_single_reduction,
 * -ksp_initial_guess_nonzero, -ksp_converged_use_initial_residual_norm,
 * -ksp_converged_use_min_initial_residual_norm [true|false]), -ksp_guess_type none|fischer and
 * -ksp_guess_fischer_model <model>[,<maxl>]; unknown options are ignored. The -ksp_chebyshev_*
 * options are checked here as pb_ksp_chebyshev_opts_parse checks them (the same errors), but
 * their values are kept by that call only.
 * Likewise the -mg_levels_* options of -pc_type mg's level smoother: checked here, kept by
 * pb_pc_mg_opts_parse only.
 * -pc_type sor: one symmetric red-black SOR sweep (PETSc PCSOR default: 1 local symmetric sweep,
 * here in red-black order). -pc_type mg (or gamg): geometric V(1,1) multigrid with red-black SOR
 * smoothing on the 7-point P (README.md:40-45 recommends GAMG + SOR). Both need even extents. */
int pb_ksp_opts_parse(pb_ksp_opts* opts, int argc, const char* const* argv);

/* KSPCreate + KSPSetOperators(ksp, A, P) + options. P supplies the Jacobi diagonal. */
int pb_ksp_create(pb_op* A, pb_op* P, const pb_ksp_opts* opts, pb_ksp** ksp);
/* KSPSolve(ksp, b, x): x0 = 0 (guess_zero; x is overwritten), or x0 = the x passed in with
 * initial_guess_nonzero (b and x must then be distinct vectors). A KSP may be reused: every
 * solve reads the flag and x afresh (a time loop warm-starts from the previous step's x).
 * history (optional, may be NULL): the res->nhist logged norms (k = 0 .. nhist-1) in the KSP's norm
 * type -- ||z_k|| by default, ||r_k||, sqrt(|r_k.z_k|), or 0.0 with none (pb_ksp_set_norm_type) --
 * at most history_cap entries written. */
int pb_ksp_solve(pb_ksp* ksp, const pb_vec* b, pb_vec* x, pb_ksp_result* res, double* history,
                 int64_t history_cap);
/* Split form used by benchmarks: setup (r = b, or b - A x0 with a nonzero guess; z, ||z0||), then
 * exactly `iters` iterations (continuing from the current state; stopping test applies unless
 * disabled by options). */
int pb_ksp_begin(pb_ksp* ksp, const pb_vec* b, pb_vec* x);
int pb_ksp_iterate(pb_ksp* ksp, int64_t iters);
int pb_ksp_end(pb_ksp* ksp, pb_ksp_result* res, double* history, int64_t history_cap);
int pb_ksp_destroy(pb_ksp* ksp);
/* ≙ KSPSetNormType / -ksp_norm_type: the number the solve logs, tests and returns (history,
 * pb_ksp_result.rnorm, rnorm0). z = N(M^-1 r) and the iteration (alpha, beta, p, x, r) are the same
 * under every type; the values are PETSc's KSPNormType.
 *   preconditioned (the default of cg / richardson / chebyshev / pipecg): ||z_i||_2; from a nonzero guess the
 *     reference is ||N(M^-1 b)||. PB_KSP_FGMRES is right-preconditioned: its default is
 *     unpreconditioned, and preconditioned / natural are PB_ERR_UNSUPPORTED on it
 *   unpreconditioned: ||r_i||_2 = ||b - A x_i||_2, the plain 2-norm (no mean shift); reference ||b||_2
 *   natural (cg and pipecg only): sqrt(|r_i . z_i|); reference sqrt(|b . N(M^-1 b)|)
 *   none: no norm and no test (KSPConvergedSkip): the solve runs max_it iterations and ends with
 *     PB_KSP_CONVERGED_ITS, its = max_it, rnorm = rnorm0 = 0 and its + 1 history entries of 0.0;
 *     breakdown and NaN exits of the dots stay. pb_ksp_solve enqueues every iteration and waits once.
 * ttol = max(rtol * rnorm0, atol), the rtol / atol / dtol / NaN tests and the reference-norm
 * switches apply to the chosen number unchanged. No type adds a pass, a launch or a reduction to
 * an iteration: ||r||^2 and r.z follow from the sums the passes already take (sor / mg / fft:
 * sum r^2 is taken where the pass that forms r holds it in registers). One exception: the spectral
 * PC's fused r update (compact A) gives way to the unfused pair under unpreconditioned. */
enum pb_ksp_norm_type {
  PB_KSP_NORM_DEFAULT = -1, PB_KSP_NORM_NONE = 0, PB_KSP_NORM_PRECONDITIONED = 1,
  PB_KSP_NORM_UNPRECONDITIONED = 2, PB_KSP_NORM_NATURAL = 3
};
/* -ksp_norm_type none|preconditioned|unpreconditioned|natural|default from the same argument list
 * as pb_ksp_opts_parse (which skips the option); the last occurrence wins, other options are
 * ignored, the option as the last token without a value is skipped. An unknown word is
 * PB_ERR_UNSUPPORTED and leaves *type as it was. */
int pb_ksp_norm_type_parse(int* type, int argc, const char* const* argv);
/* ≙ KSPSetNormType. PB_ERR_ARG for a value outside the enum; PB_ERR_UNSUPPORTED for natural on
 * richardson / chebyshev (as PETSc refuses it), for preconditioned / natural on fgmres and for
 * anything but default / none on preonly;
 * PB_ERR_STATE between pb_ksp_begin and pb_ksp_end. An error leaves the KSP as it was. */
int pb_ksp_set_norm_type(pb_ksp* ksp, int type);
/* ≙ KSPGetNormType. *set: the value as set (PB_KSP_NORM_DEFAULT after create); *effective: the one
 * in force (default: preconditioned for cg / richardson / chebyshev / pipecg, unpreconditioned for
 * fgmres, none for preonly). Either may be NULL. */
int pb_ksp_get_norm_type(const pb_ksp* ksp, int* set, int* effective);
/* -ksp_chebyshev_eigenvalues emin,emax, -ksp_chebyshev_esteig a,b,c,d,
 * -ksp_chebyshev_esteig_steps n, -ksp_chebyshev_esteig_noisy [bool] from the same argument list
 * as pb_ksp_opts_parse; other options are ignored. */
int pb_ksp_chebyshev_opts_default(pb_ksp_chebyshev_opts* opts);
int pb_ksp_chebyshev_opts_parse(pb_ksp_chebyshev_opts* opts, int argc, const char* const* argv);
/* Sets them on a PB_KSP_CHEBYSHEV KSP (PB_ERR_STATE on another type, PB_ERR_ARG for invalid
 * values, which leave the KSP as it was); an estimate made before is forgotten. */
int pb_ksp_chebyshev_set_opts(pb_ksp* ksp, const pb_ksp_chebyshev_opts* opts);
/* pb_solve with these settings (cheb may be NULL: the defaults) */
int pb_solve_chebyshev(pb_op* A, pb_op* P, const pb_ksp_opts* opts,
                       const pb_ksp_chebyshev_opts* cheb, const pb_vec* b, pb_vec* x,
                       pb_ksp_result* res, double* history, int64_t history_cap);
/* -ksp_gmres_restart n, -ksp_gmres_haptol h, -ksp_gmres_cgs_refinement_type <type>,
 * -ksp_gmres_classicalgramschmidt (no effect: it is the only orthogonalisation),
 * -ksp_gmres_modifiedgramschmidt [bool] (PB_ERR_UNSUPPORTED when true) and -ksp_gmres_preallocate
 * (accepted: the basis is allocated in chunks whatever it says) from the same argument list as
 * pb_ksp_opts_parse, which skips them; other options are ignored, an option that is the last
 * token without its value is skipped, and an error leaves *opts as it was. */
int pb_ksp_fgmres_opts_default(pb_ksp_fgmres_opts* opts);
int pb_ksp_fgmres_opts_parse(pb_ksp_fgmres_opts* opts, int argc, const char* const* argv);
/* Sets them on a PB_KSP_FGMRES KSP (PB_ERR_STATE on another type or between pb_ksp_begin and
 * pb_ksp_end; PB_ERR_ARG / PB_ERR_UNSUPPORTED for invalid values, which leave the KSP as it was) */
int pb_ksp_fgmres_set_opts(pb_ksp* ksp, const pb_ksp_fgmres_opts* opts);
int pb_ksp_fgmres_get_opts(const pb_ksp* ksp, pb_ksp_fgmres_opts* opts);
/* pb_solve with these settings (fg may be NULL: the defaults) */
int pb_solve_fgmres(pb_op* A, pb_op* P, const pb_ksp_opts* opts, const pb_ksp_fgmres_opts* fg,
                    const pb_vec* b, pb_vec* x, pb_ksp_result* res, double* history,
                    int64_t history_cap);
/* -mg_levels_ksp_type, -mg_levels_pc_type, -mg_levels_ksp_max_it,
 * -mg_levels_ksp_richardson_scale, -mg_levels_ksp_chebyshev_eigenvalues emin,emax and
 * -mg_levels_ksp_chebyshev_esteig a,b,c,d from the same argument list as pb_ksp_opts_parse (which
 * reports the same errors and keeps no value); other options are ignored. -mg_levels_ksp_rtol
 * and -mg_coarse_sub_pc_type are accepted and have no effect: the sweep count is fixed and the
 * coarsest level runs -pc_mg_coarse_its SOR sweeps. Bounds that are given must be finite and
 * positive with emax > emin (PB_ERR_ARG: D^-1 A is positive semi-definite). */
int pb_pc_mg_opts_default(pb_pc_mg_opts* opts);
int pb_pc_mg_opts_parse(pb_pc_mg_opts* opts, int argc, const char* const* argv);
/* Sets them on a KSP with pc_type PB_PC_MG (PB_ERR_STATE on another PC or inside a solve;
 * PB_ERR_ARG / PB_ERR_UNSUPPORTED for invalid values, which leave the KSP as it was). The
 * Jacobi-type smoothers' extra level arrays are allocated here, not at pb_ksp_create. */
int pb_ksp_pc_mg_set_opts(pb_ksp* ksp, const pb_pc_mg_opts* opts);
int pb_ksp_pc_mg_get_opts(const pb_ksp* ksp, pb_pc_mg_opts* opts);
/* pb_solve with these settings (mg may be NULL: the defaults) */
int pb_solve_mg(pb_op* A, pb_op* P, const pb_ksp_opts* opts, const pb_pc_mg_opts* mg,
                const pb_vec* b, pb_vec* x, pb_ksp_result* res, double* history,
                int64_t history_cap);
/* The bounds the next PB_KSP_CHEBYSHEV solve uses (PB_ERR_STATE on a KSP of another type);
 * *estimated = 0 for the caller's own. Without given bounds this runs the estimate if it has not
 * run for the operators' current deltas (so it is collective over the ranks):
 * esteig_steps steps of preconditioned CG-Lanczos on A and the PC, from r_0 = N(v),
 * v = pb_vec_set_random with
 * PB_CHEBYSHEV_ESTEIG_SEED (decomposition independent); the Lanczos tridiagonal (diagonal
 * 1 / alpha_j + beta_(j-1) / alpha_(j-1), off-diagonal sqrt(beta_j) / alpha_j) gives the extremes
 * through pb_tridiag_extreme_eigenvalues, esteig transforms them. It stops early on a
 * beta that is 0, negative or not finite, and once r'z has fallen below 1e-24 of its first value
 * (-pc_type fft with A = P: one step is all there is). PETSc's default estimator is GMRES in the
 * Euclidean inner product; this is its -esteig_ksp_type cg counterpart. Transformed bounds that
 * are no valid pair (-pc_type none with the default transform: the spectrum is negative) return
 * PB_ERR_ARG, here and from the solve; the KSP stays usable. */
int pb_ksp_chebyshev_get_eigenvalues(pb_ksp* ksp, double* emin, double* emax, int* estimated);
/* Smallest and largest eigenvalue of the symmetric tridiagonal matrix with diagonal diag[0..n-1]
 * and off-diagonal off[0..n-2] (off may be NULL when n = 1), by bisection on Sturm counts. Pure
 * host code, 1 <= n <= 64 and finite entries (else PB_ERR_ARG). */
int pb_tridiag_extreme_eigenvalues(int n, const double* diag, const double* off, double* lo,
                                   double* hi);
/* PCApply(KSPGetPC(ksp), r, z): z = M^-1 r of the configured preconditioner (Jacobi: D^-1 r;
 * SOR / MG: from a zero initial guess), without the null-space removal KSP adds. */
int pb_ksp_pc_apply(pb_ksp* ksp, const pb_vec* r, pb_vec* z);
/* number of multigrid levels in use (1 for SOR, 0 for Jacobi / none) */
int pb_ksp_pc_levels(const pb_ksp* ksp, int* levels);
/* The variable-coefficient SOR / multigrid preconditioner. -pc_type sor | mg only (else
 * PB_ERR_STATE), on a KSP created with a constant-coefficient 7-point P. C: a PB_OP_VARCOEF
 * operator of the KSP's grid (usually A; another kind or grid: PB_ERR_ARG); NULL returns to the
 * constant-coefficient PC. From the next solve / pb_ksp_pc_apply on, the smoother, the residual and
 * every coarse operator are div(beta_l grad) with C's mean and C's deltas (h_l = 2^l h), beta_0 =
 * C's coefficient and beta_(l+1) the arithmetic mean of a cell's 8 children; P's deltas are no
 * longer read by the PC. The KSP holds C as it holds A and P (pb_op_set_coefficient(C) inside a
 * solve is PB_ERR_STATE; C must outlive the KSP or be unset first); the levels are rebuilt by the
 * first apply after pb_op_set_coefficient(C) / pb_op_set_deltas(C). Level smoothers: richardson +
 * sor with 1..8 sweeps; a Jacobi-type level smoother together with a coefficient is
 * PB_ERR_UNSUPPORTED, from whichever of the two calls comes second. PB_ERR_STATE inside a solve.
 * Every error leaves the KSP as it was. */
int pb_ksp_pc_set_coefficient_from(pb_ksp* ksp, const pb_op* C);
int pb_ksp_pc_get_coefficient_from(const pb_ksp* ksp, const pb_op** C);
/* Projected initial guess (guess_type = PB_GUESS_FISCHER; every call returns PB_ERR_STATE on a
 * KSP created without it). pb_ksp_solve calls form before and update after the solve by itself;
 * callers of the split form (pb_ksp_begin with initial_guess_nonzero = 1) call them around it.
 *   form(b, x):   x = the projection of b's solution onto the stored directions (x as passed in is
 *                 ignored; 0 while nothing is stored); a copy stays inside the KSP for update.
 *   update(b, x): after a solve of b from the formed guess: adds the direction x - guess (A-image
 *                 orthonormalised against the stored ones) unless it is 0 or not finite; a full
 *                 space restarts from x alone. b is not read (model 1).
 *   reset:        forget every direction. size: directions stored now / at most. */
int pb_ksp_guess_form(pb_ksp* ksp, const pb_vec* b, pb_vec* x);
int pb_ksp_guess_update(pb_ksp* ksp, const pb_vec* b, const pb_vec* x);
int pb_ksp_guess_reset(pb_ksp* ksp);
int pb_ksp_guess_size(const pb_ksp* ksp, int* curl, int* maxl);
/* One-shot convenience: ≙ solve(P, A, x, b). Accepts guess_type too, but its KSP lives for one
 * solve: no direction is kept, the solve runs from x = 0 as a nonzero guess. */
int pb_solve(pb_op* A, pb_op* P, const pb_ksp_opts* opts, const pb_vec* b, pb_vec* x,
             pb_ksp_result* res, double* history, int64_t history_cap);

/* ---- tridiagonal (replaces tdma / tdma_periodic / fwd_sweep / bwd_sweep, src/tridsol.f90) ----
 * Batched over `nbatch` independent lines. Element e of line l sits at
 *   ptr[l * line_stride + e * elem_stride]        (device pointers).
 * Argument order follows the reference code: a = sub-diagonal, b = diagonal, c = super-diagonal,
 * d = rhs -> solution. tdma overwrites b and d (like the reference); tdma_periodic leaves b
 * unchanged. periodic: a[0] couples x[n-1], c[n-1] couples x[0] (src/tridsol.f90:34-74). */
int pb_tdma_batched(pb_ctx* ctx, int64_t n, int64_t nbatch, int64_t line_stride,
                    int64_t elem_stride, const double* a, double* b, const double* c, double* d,
                    int periodic);
/* fwd_sweep (which = 1: a, b, c, d -> modified b, d) or bwd_sweep (which = 2: b, c, d -> x in d;
 * a unused) alone, src/tridsol.f90:76-115 (exported by the reference for its tests). */
int pb_tdma_sweeps_batched(pb_ctx* ctx, int64_t n, int64_t nbatch, int64_t line_stride,
                           int64_t elem_stride, const double* a, double* b, const double* c,
                           double* d, int which);
/* Constant-coefficient periodic (alpha, 1, alpha) systems -- the compact-scheme solves
 * (src/compact_schemes.f90:197,312) -- by parallel cyclic reduction, in place on d. */
int pb_pcr_alpha_batched(pb_ctx* ctx, int64_t n, int64_t nbatch, int64_t line_stride,
                         int64_t elem_stride, double alpha, double* d);

/* ---- compact schemes (replace src/compact_schemes.f90:9-13 public API) ----
 * 3-D fields on the grid; grad/div take 3-component vectors as three pb_vec. stagger: -1
 * cell->vertex, +1 vertex->cell. Reference operation order (bit-identical to the reference). On a
 * split grid the Z steps run on y-slabs with complete z-lines (all-to-all transposes, as
 * pb_compact_lapl_fast), so every rank's result is bit-identical to the single-domain one. */
int pb_compact_grad(pb_grid* grid, const double dx[3], const pb_vec* f, pb_vec* const df[3]);
int pb_compact_div(pb_grid* grid, const double dx[3], const pb_vec* const f[3], pb_vec* df);
int pb_compact_interp(pb_grid* grid, int stagger, const pb_vec* f, pb_vec* fi);
int pb_compact_lapl(pb_grid* grid, const double dx[3], const pb_vec* f, pb_vec* out);
/* Same operator by the 3-pass factorisation lapl = Lx Jy Jz + Jx Ly Jz + Jx Jy Lz (SURVEY.md
 * App. D) with PCR line solves in LDS: ~80 B/DoF instead of 16 line-solve families; agrees with
 * pb_compact_lapl to rounding. This is what PB_OP_COMPACT applies inside CG. */
int pb_compact_lapl_fast(pb_grid* grid, const double dx[3], const pb_vec* f, pb_vec* out);
/* Bandwidth-oriented grad, div and interp: the same factorisation into line passes, one half
 * operator (explicit RHS + one (alpha, 1, alpha) solve) per axis, register line solves where the
 * line length is 64*{1,2,3,4,6,8,12,16} and the LDS-PCR kernel otherwise. Arguments and staggering
 * as pb_compact_grad / pb_compact_div / pb_compact_interp (interp_div is stagger +1). They match
 * the reference to rounding, NOT to the bit (operation order differs); the bit-exact calls above
 * stay as they are. They accept every grid pb_compact_lapl_fast accepts and return its errors
 * beyond; inputs must not alias outputs and the three components must be distinct vectors
 * (PB_ERR_ARG). On a split grid the Z pass runs on y-slabs (all-to-all transposes) and every
 * rank's slab is bit-identical to the one-rank result. N = the grid's local size; on a split
 * grid each call also takes three y-slab fields and the transpose staging from the context.
 *   pb_compact_grad_fast   replaces src/compact_schemes.f90:42-88;  Z -> Y -> X, 112 B/DoF,
 *                          context scratch 2N (the X passes run in place in df)
 *   pb_compact_div_fast    replaces src/compact_schemes.f90:207-257; X -> Y -> Z, 112 B/DoF,
 *                          context scratch 5N
 *   pb_compact_interp_fast replaces src/compact_schemes.f90:93-152;  Z -> Y -> X, 48 B/DoF,
 *                          context scratch N */
int pb_compact_grad_fast(pb_grid* grid, const double dx[3], const pb_vec* f, pb_vec* const df[3]);
int pb_compact_div_fast(pb_grid* grid, const double dx[3], const pb_vec* const f[3], pb_vec* df);
int pb_compact_interp_fast(pb_grid* grid, int stagger, const pb_vec* f, pb_vec* fi);
/* 1-D line operators on device arrays, batched like pb_tdma_batched (grad_1d/div_1d/interp_1d/
 * interp_1d_div: kind 0 = derivative, 1 = interpolation). */
int pb_compact_1d_batched(pb_ctx* ctx, int kind, int stagger, double dx, int64_t n,
                          int64_t nbatch, int64_t line_stride, int64_t elem_stride,
                          const double* f, double* out);

/* ---- host-array forms of the module procedures (src/tridsol.f90:16-18, compact_schemes.f90:9-13):
 * the reference works on process-local Fortran arrays, so these take host pointers, stage them
 * through device memory, run the kernels above and copy back (synchronous). The Fortran modules
 * `tridsol` and `compact_schemes` in poissbox_amd/fortran wrap them with the reference's
 * assumed-shape signatures. 3-D fields are whole arrays of shape n (never split, whatever the
 * context); vector fields are (nx, ny, nz, 3) with the component slowest. ---- */
int pb_tdma_batched_host(pb_ctx* ctx, int64_t n, int64_t nbatch, int64_t line_stride,
                         int64_t elem_stride, const double* a, double* b, const double* c,
                         double* d, int periodic);
int pb_tdma_sweeps_batched_host(pb_ctx* ctx, int64_t n, int64_t nbatch, int64_t line_stride,
                                int64_t elem_stride, const double* a, double* b, const double* c,
                                double* d, int which);
int pb_compact_1d_batched_host(pb_ctx* ctx, int kind, int stagger, double dx, int64_t n,
                               int64_t nbatch, int64_t line_stride, int64_t elem_stride,
                               const double* f, double* out);
int pb_compact_grad_host(pb_ctx* ctx, const int64_t n[3], const double dx[3], const double* f,
                         double* df);
int pb_compact_div_host(pb_ctx* ctx, const int64_t n[3], const double dx[3], const double* f,
                        double* df);
int pb_compact_interp_host(pb_ctx* ctx, const int64_t n[3], int stagger, const double* f,
                           double* fi);
int pb_compact_lapl_host(pb_ctx* ctx, const int64_t n[3], const double dx[3], const double* f,
                         double* out);

#ifdef __cplusplus
}
#endif
#endif /* POISSBOX_GPU_H */
