"""Python host side of the poissbox KSPSolve path, mirroring the reference's Fortran/PETSc interface.

Reference (3decomp/poissbox) -> here:
  MPI_Init + PetscInitialize (src/example.f90:43-47)        -> Context(device, rank, nranks, uid)
  initialise_grid(nglobal, da) (src/poissbox.f90:183-204)   -> initialise_grid(ctx, nglobal) -> DA
  DMDAGetCorners (src/poissbox.f90:107)                     -> DA.get_corners()
  initialise_linear_system(da, ctx, P, A, x, b) (:206-240)  -> initialise_linear_system(da, deltas)
  MatCreateShell + MATOP_MULT = mfmult (:242-267, :300-322) -> Mat(kind=STAR7) .mult(x, y)
  compute_lapl_pointwise(da, grid_deltas, x, b) (:84-126)   -> compute_lapl_pointwise(da, deltas, x, b)
  solve(P, A, x, b) (:269-298) + KSPSetFromOptions          -> solve(P, A, x, b, options=argv)
  Vec* (VecAXPY/VecNorm/VecSum/VecDuplicate/...)            -> Vec methods
  tdma / tdma_periodic (src/tridsol.f90)                    -> tdma_batched(...)
  grad/div/interp/interp_div/lapl (src/compact_schemes.f90) -> compact_* functions

All compute runs in libpoissbox_gpu.so (HIP kernels for gfx950); there is no CPU fallback.
"""
import ctypes as C

import numpy as np

from . import _lib as L

STAR7, COMPACT, ASSEMBLED27 = 0, 1, 2
# div(beta grad) with beta per cell (Mat.set_coefficient); the face value between two cells is
# their arithmetic or harmonic mean (pb_coef_mean)
VARCOEF = 3
COEF_ARITHMETIC, COEF_HARMONIC = 0, 1
PC_NONE, PC_JACOBI, PC_SOR, PC_MG, PC_FFT = 0, 1, 2, 3, 4
# -ksp_type: preonly = one PC application (with -pc_type fft the direct solve), richardson =
# x += scale M^-1 (b - A x) (ksp_options(richardson_scale=...) or -ksp_richardson_scale)
# chebyshev = the accelerated stationary iteration for a spectrum of M^-1 A in [emin, emax]
# (-ksp_chebyshev_eigenvalues emin,emax; estimated when not given: KSP.chebyshev_eigenvalues())
# fgmres = restarted flexible GMRES (right-preconditioned: the tested number is ||b - A x||;
# -ksp_gmres_restart, -ksp_gmres_haptol, -ksp_gmres_cgs_refinement_type: pb_ksp_fgmres_opts)
# pipecg = pipelined CG (KSPPIPECG): CG in exact arithmetic with one reduction per iteration on
# every operator and PC; no options of its own
KSP_CG, KSP_PREONLY, KSP_RICHARDSON, KSP_CHEBYSHEV, KSP_FGMRES, KSP_PIPECG = 0, 1, 2, 3, 4, 5
FGMRES_REFINE_NEVER, FGMRES_REFINE_ALWAYS = 0, 2
# -mg_levels_ksp_type / -mg_levels_pc_type: the level smoother of -pc_type mg (pb_pc_mg_opts)
MG_LEVELS_RICHARDSON, MG_LEVELS_CHEBYSHEV = 0, 1
# pb_ksp_norm_type (PETSc's KSPNormType values)
KSP_NORM_DEFAULT, KSP_NORM_NONE, KSP_NORM_PRECONDITIONED = -1, 0, 1
KSP_NORM_UNPRECONDITIONED, KSP_NORM_NATURAL = 2, 3
MG_LEVELS_SOR, MG_LEVELS_JACOBI = 0, 1

REASONS = {0: "CONVERGED_ITERATING", 2: "CONVERGED_RTOL", 3: "CONVERGED_ATOL",
           4: "CONVERGED_ITS", -3: "DIVERGED_ITS", -4: "DIVERGED_DTOL",
           -8: "DIVERGED_INDEFINITE_PC", -9: "DIVERGED_NANORINF",
           -10: "DIVERGED_INDEFINITE_MAT", -5: "DIVERGED_BREAKDOWN",
           7: "CONVERGED_HAPPY_BREAKDOWN"}


def _i64_3(v):
    return (C.c_int64 * 3)(*[int(t) for t in v])


def _d_3(v):
    return (C.c_double * 3)(*[float(t) for t in v])


def _dptr(a):
    assert a.dtype == np.float64 and a.flags.c_contiguous
    return a.ctypes.data_as(L.P_d)


def comm_unique_id():
    buf = C.create_string_buffer(128)
    L.call("pb_comm_unique_id", buf)
    return bytes(buf.raw)


def slab_partition(nz, nranks, rank):
    k0, nk = C.c_int64(), C.c_int64()
    L.call("pb_slab_partition", int(nz), int(nranks), int(rank), C.byref(k0), C.byref(nk))
    return k0.value, nk.value


def tune_set(name, value):
    """pb_tune_set: a kernel-selection / launch-shape parameter (INTEGRATION.md lists them)."""
    L.call("pb_tune_set", name.encode(), int(value))


def tune_get(name):
    """The value set for a tuning parameter, or None when it runs at its measured default."""
    v, s = C.c_int(), C.c_int()
    L.call("pb_tune_get", name.encode(), C.byref(v), C.byref(s))
    return v.value if s.value else None


def tune_reset():
    L.call("pb_tune_reset")


class Context:
    """One GPU, one rank. nranks > 1 needs either an RCCL unique id (uid, from rank 0's
    comm_unique_id()) or a host transport (set_host_transport) before the grid is created."""

    def __init__(self, device=0, rank=0, nranks=1, uid=None):
        h = C.c_void_p()
        L.call("pb_ctx_create", int(device), int(rank), int(nranks), uid, C.byref(h))
        self.h = h
        self.device = device
        self.rank, self.nranks = rank, nranks
        self._keep = []

    @classmethod
    def from_env(cls, device=-1):
        """pb_ctx_create_from_env: rank layout from the launcher's environment (torchrun / mpirun /
        PMI), RCCL or the built-in shared-memory transport (PB_TRANSPORT)."""
        self = cls.__new__(cls)
        h = C.c_void_p()
        L.call("pb_ctx_create_from_env", int(device), C.byref(h))
        self.h = h
        self.device = device
        r, n = C.c_int(), C.c_int()
        L.call("pb_ctx_get_rank", h, C.byref(r), C.byref(n))
        self.rank, self.nranks = r.value, n.value
        self._keep = []
        return self

    def allreduce_sum(self, vals):
        """SUM over ranks of a few host doubles (MPI_Allreduce of the reference's checks)."""
        a = np.ascontiguousarray(vals, dtype=np.float64).reshape(-1).copy()
        L.call("pb_ctx_allreduce_host", self.h, _dptr(a), a.size)
        return a

    def set_host_transport(self, sendrecv, allreduce, alltoallv=None):
        """sendrecv(send_lo, send_hi) -> (recv_lo, recv_hi) numpy arrays; allreduce(vals) -> vals;
        alltoallv(list of per-rank send blocks, list of per-rank receive sizes) -> list of
        per-rank received blocks (optional; the compact operator on a split grid needs it)."""

        def _sr(user, s_lo, s_hi, r_lo, r_hi, count):
            try:
                a = np.ctypeslib.as_array(s_lo, shape=(count,)).copy()
                b = np.ctypeslib.as_array(s_hi, shape=(count,)).copy()
                lo, hi = sendrecv(a, b)
                np.ctypeslib.as_array(r_lo, shape=(count,))[:] = lo
                np.ctypeslib.as_array(r_hi, shape=(count,))[:] = hi
                return 0
            except Exception as e:  # pragma: no cover - reported through the C error path
                print("host sendrecv failed:", e)
                return 1

        def _ar(user, vals, count):
            try:
                v = np.ctypeslib.as_array(vals, shape=(count,))
                v[:] = allreduce(v.copy())
                return 0
            except Exception as e:  # pragma: no cover
                print("host allreduce failed:", e)
                return 1

        f1, f2 = L.SENDRECV_FN(_sr), L.ALLREDUCE_FN(_ar)
        self._keep += [f1, f2]
        L.call("pb_ctx_set_host_transport", self.h, f1, f2, None)
        if alltoallv is None:
            return

        def _a2a(user, send, scount, recv, rcount):
            try:
                P = self.nranks
                sc = [int(scount[p]) for p in range(P)]
                rc = [int(rcount[p]) for p in range(P)]
                sa = np.ctypeslib.as_array(send, shape=(max(sum(sc), 1),))
                so = np.concatenate([[0], np.cumsum(sc)])
                blocks = [sa[so[p]:so[p + 1]].copy() for p in range(P)]
                got = alltoallv(blocks, rc)
                ra = np.ctypeslib.as_array(recv, shape=(max(sum(rc), 1),))
                ro = np.concatenate([[0], np.cumsum(rc)])
                for p in range(P):
                    assert got[p].size == rc[p], (p, got[p].size, rc[p])
                    ra[ro[p]:ro[p + 1]] = got[p]
                return 0
            except Exception as e:  # pragma: no cover
                print("host alltoallv failed:", e)
                return 1

        f3 = L.ALLTOALLV_FN(_a2a)
        self._keep.append(f3)
        L.call("pb_ctx_set_host_alltoallv", self.h, f3, None)

    def sync(self):
        L.call("pb_ctx_sync", self.h)

    def barrier(self):
        L.call("pb_ctx_barrier", self.h)

    @property
    def comm_failed(self):
        """True after a communication failure (timeout, RCCL error, failing host callback)."""
        v = C.c_int(0)
        L.call("pb_ctx_comm_status", self.h, C.byref(v))
        return bool(v.value)

    TRANSPORTS = {0: "none", 1: "rccl", 2: "host"}

    def comm_info(self):
        """(transport, communicator size, rank in it) as the transport itself reports them:
        RCCL's ncclCommCount / ncclCommUserRank, the host transport's rank layout, or
        ("none", 1, 0) on one rank (pb_ctx_comm_info)."""
        t, n, r = C.c_int(), C.c_int(), C.c_int()
        L.call("pb_ctx_comm_info", self.h, C.byref(t), C.byref(n), C.byref(r))
        return self.TRANSPORTS.get(t.value, t.value), n.value, r.value

    def set_timing(self, on=True, only=None, every=1):
        """HIP-event timing of the library's phases; only: phase names (str or list) to time,
        every: time one launch in `every` of each (pb_ctx_set_timing_filter)."""
        if isinstance(only, (list, tuple)):
            only = ",".join(only)
        L.call("pb_ctx_set_timing_filter", self.h, int(bool(on)),
               only.encode() if only else None, int(every))

    def timing(self, name):
        ms, cnt = C.c_double(), C.c_int64()
        L.call("pb_ctx_get_timing", self.h, name.encode(), C.byref(ms), C.byref(cnt))
        return ms.value, cnt.value

    def timing_samples(self, name):
        """Per-launch durations (ms) of a timed phase since the last reset (numpy float32)."""
        cnt = C.c_int64()
        L.call("pb_ctx_get_timing_samples", self.h, name.encode(), None, 0, C.byref(cnt))
        out = np.zeros(cnt.value, dtype=np.float32)
        if cnt.value:
            L.call("pb_ctx_get_timing_samples", self.h, name.encode(),
                   out.ctypes.data_as(C.POINTER(C.c_float)), cnt.value, C.byref(cnt))
        return out

    def copy_probe(self, n=1 << 27, reps=10):
        """HBM calibration: (best, median) GB/s of a flat fp64 copy of n doubles."""
        best, med = C.c_double(), C.c_double()
        L.call("pb_ctx_copy_probe", self.h, int(n), int(reps), C.byref(best), C.byref(med))
        return best.value, med.value

    def reset_timing(self):
        L.call("pb_ctx_reset_timing", self.h)

    def destroy(self):
        if self.h:
            L.call("pb_ctx_destroy", self.h)
            self.h = None


class DA:
    """DMDA analogue: periodic grid, z-slab per rank (src/poissbox.f90:191-202)."""

    def __init__(self, ctx, nglobal, L_=(1.0, 1.0, 1.0)):
        h = C.c_void_p()
        L.call("pb_grid_create", ctx.h, _i64_3(nglobal), _d_3(L_), C.byref(h))
        self.h, self.ctx = h, ctx
        n, hh, nl = (C.c_int64 * 3)(), (C.c_double * 3)(), C.c_int64()
        L.call("pb_grid_get_info", h, n, hh, C.byref(nl))
        self.n = tuple(n)
        self.spacing = tuple(hh)
        self.nlocal = nl.value

    def get_corners(self):
        """0-based (start, size) of the owned block, like DMDAGetCorners."""
        s, z = (C.c_int64 * 3)(), (C.c_int64 * 3)()
        L.call("pb_grid_get_corners", self.h, s, z)
        return tuple(s), tuple(z)

    def create_global_vector(self):
        return Vec(self)

    def destroy(self):
        if self.h:
            L.call("pb_grid_destroy", self.h)
            self.h = None


class Vec:
    def __init__(self, da, _handle=None):
        self.da = da
        if _handle is None:
            h = C.c_void_p()
            L.call("pb_vec_create", da.h, C.byref(h))
            _handle = h
        self.h = _handle

    def duplicate(self):
        return Vec(self.da)

    def set(self, a):
        L.call("pb_vec_set", self.h, float(a))
        return self

    def copy_to(self, dst):
        L.call("pb_vec_copy", self.h, dst.h)

    def axpy(self, a, x):  # VecAXPY(self, a, x): self = self + a*x
        L.call("pb_vec_axpy", self.h, float(a), x.h)

    def aypx(self, b, x):  # VecAYPX(self, b, x): self = x + b*self
        L.call("pb_vec_aypx", self.h, float(b), x.h)

    def scale(self, a):
        L.call("pb_vec_scale", self.h, float(a))

    def dot(self, y):
        out = C.c_double()
        L.call("pb_vec_dot", self.h, y.h, C.byref(out))
        return out.value

    def mdot(self, ys):
        """VecMDot: numpy array of self . y for the up to 16 vectors ys, in one pass."""
        out = np.zeros(len(ys))
        arr = (C.c_void_p * max(len(ys), 1))(*[y.h.value for y in ys])
        L.call("pb_vec_mdot", self.h, len(ys), arr, _dptr(out))
        return out

    def maxpy(self, alphas, xs):
        """VecMAXPY: self += sum_i alphas[i] xs[i] (up to 16 vectors) in one pass."""
        a = np.ascontiguousarray(alphas, dtype=np.float64).reshape(-1)
        if a.size != len(xs):
            raise ValueError(f"{a.size} coefficients for {len(xs)} vectors")
        a = np.concatenate([a, [0.0]])  # (a valid pointer also for no vectors)
        arr = (C.c_void_p * max(len(xs), 1))(*[x.h.value for x in xs])
        L.call("pb_vec_maxpy", self.h, len(xs), _dptr(a), arr)

    def norm(self):
        out = C.c_double()
        L.call("pb_vec_norm2", self.h, C.byref(out))
        return out.value

    def sum(self):
        out = C.c_double()
        L.call("pb_vec_sum", self.h, C.byref(out))
        return out.value

    def set_values(self, owned):
        a = np.ascontiguousarray(owned, dtype=np.float64).reshape(-1)
        if a.size != self.da.nlocal:
            raise ValueError(f"expected {self.da.nlocal} owned values, got {a.size}")
        L.call("pb_vec_set_values_host", self.h, _dptr(a))

    def get_values(self):
        a = np.empty(self.da.nlocal)
        L.call("pb_vec_get_values_host", self.h, _dptr(a))
        return a

    def set_random(self, seed):
        L.call("pb_vec_set_random", self.h, C.c_uint64(int(seed)))

    def copy_probe(self, y, reps=10):
        """HBM calibration over this vector's and y's own buffers (y is overwritten): flat copy
        self -> y, the matvec's access mix. Returns (best, median) GB/s."""
        best, med = C.c_double(), C.c_double()
        L.call("pb_vec_copy_probe", self.h, y.h, int(reps), C.byref(best), C.byref(med))
        return best.value, med.value

    def device_ptr(self):
        p, n = C.c_void_p(), C.c_int64()
        L.call("pb_vec_device_ptr", self.h, C.byref(p), C.byref(n))
        return p.value, n.value

    def destroy(self):
        if self.h:
            L.call("pb_vec_destroy", self.h)
            self.h = None


class Mat:
    """MatShell analogue (kind STAR7 = mfmult's compute_lapl_pointwise) or the assembled P."""

    def __init__(self, da, kind=STAR7, deltas=None):
        h = C.c_void_p()
        d = _d_3(deltas) if deltas is not None else None
        L.call("pb_op_create", da.h, int(kind), d, C.byref(h))
        self.h, self.da, self.kind = h, da, kind

    def mult(self, x, y):  # MatMult(self, x, y)
        L.call("pb_op_apply", self.h, x.h, y.h)

    def diagonal(self):
        d = C.c_double()
        L.call("pb_op_get_diagonal", self.h, C.byref(d))
        return d.value

    def set_deltas(self, deltas):
        """(Re)set the spacings the coefficients are built from (assemble_laplacian)."""
        L.call("pb_op_set_deltas", self.h, _d_3(deltas))

    def set_coefficient(self, beta, mean=COEF_ARITHMETIC):
        """VARCOEF: copy the cell-centred coefficient (a Vec of the operator's grid, every value
        finite and > 0) into the operator; collective."""
        L.call("pb_op_set_coefficient", self.h, beta.h, int(mean))

    def coefficient(self, beta=None):
        """VARCOEF: the mean in force; beta (a Vec), if given, receives the coefficient."""
        m = C.c_int()
        L.call("pb_op_get_coefficient", self.h, beta.h if beta is not None else None, C.byref(m))
        return m.value

    def set_mass(self, m=None, s=0.0):
        """VARCOEF: the mass term A = div(beta grad) - s m (m a Vec of the operator's grid, every
        value finite and >= 0, copied; None: ones; s finite and >= 0, 0 switches the term off);
        collective. A KSP whose A has the term on needs nullspace = 0."""
        L.call("pb_op_set_mass", self.h, m.h if m is not None else None, float(s))

    def mass(self, m=None):
        """VARCOEF: s; m (a Vec), if given, receives the mass field (ones if none is set)."""
        s = C.c_double()
        L.call("pb_op_get_mass", self.h, m.h if m is not None else None, C.byref(s))
        return s.value

    def diagonal_vec(self, v):
        """MatGetDiagonal into the Vec v (VARCOEF: the diagonal field; 7-point kinds: broadcast)."""
        L.call("pb_op_get_diagonal_vec", self.h, v.h)
        return v

    # MAC-grid gradient, projection and divergence (STAR7, VARCOEF; include/poissbox_gpu.h): a
    # face field is a sequence of three Vecs, component d on the plus face along axis d
    @staticmethod
    def _vec3(v3):
        if len(v3) != 3:
            raise ValueError("a face field is three Vecs")
        return (C.c_void_p * 3)(*[v.h.value for v in v3])

    def mac_grad(self, p, g3):
        """g3[d] = G_d(p), the operator's own face flux: (r_d face(beta)) (p_+ - p_c); collective."""
        L.call("pb_op_mac_grad", self.h, p.h, self._vec3(g3))

    def mac_project(self, p, s, u3):
        """u3[d] -= s G_d(p) in place (the projection's correction, s = dt); collective."""
        L.call("pb_op_mac_project", self.h, p.h, float(s), self._vec3(u3))

    def mac_div(self, u3, out, s=1.0):
        """out = s D(u3), the adjoint difference of mac_grad (the projection's right-hand side,
        s = 1 / dt): D G = A to rounding; collective."""
        L.call("pb_op_mac_div", self.h, float(s), self._vec3(u3), out.h)

    def destroy(self):
        if self.h:
            L.call("pb_op_destroy", self.h)
            self.h = None


def MatMult(A, x, y):
    A.mult(x, y)


class KspOptions(L.KspOpts):
    """pb_ksp_opts (the same layout: no field added) together with the Chebyshev settings, which
    the C interface keeps in a struct of their own (pb_ksp_chebyshev_opts; `.chebyshev`); KSP()
    sets them after pb_ksp_create. chebyshev_emin / _emax / _esteig / _esteig_steps read and write
    that struct. Likewise the multigrid's level smoother (pb_pc_mg_opts; `.mg`): mg_levels_ksp_type
    (MG_LEVELS_RICHARDSON | _CHEBYSHEV), mg_levels_pc_type (MG_LEVELS_SOR | _JACOBI),
    mg_levels_ksp_max_it, mg_levels_richardson_scale, mg_levels_eigenvalues, mg_levels_esteig;
    KSP() sets them on a -pc_type mg KSP once one of them was touched or parsed. Likewise
    -ksp_norm_type (`.norm_type`, KSP_NORM_*; the C interface keeps it on the KSP object): KSP()
    sets it unless it is KSP_NORM_DEFAULT. Likewise the settings of -ksp_type fgmres
    (pb_ksp_fgmres_opts; `.fgmres`, with fgmres_restart / _haptol / _cgs_refinement): KSP() sets
    them on a KSP of that type."""

    norm_type = property(lambda s: s.__dict__.get("norm_type", KSP_NORM_DEFAULT),
                         lambda s, v: s.__dict__.__setitem__("norm_type", int(v)))

    def _mg(self):
        if "mg" not in self.__dict__:
            m = L.PcMgOpts()
            L.call("pb_pc_mg_opts_default", C.byref(m))
            self.__dict__["mg"] = m
        return self.__dict__["mg"]

    mg = property(_mg)
    mg_levels_ksp_type = property(lambda s: s._mg().levels_ksp_type,
                                  lambda s, v: setattr(s._mg(), "levels_ksp_type", v))
    mg_levels_pc_type = property(lambda s: s._mg().levels_pc_type,
                                 lambda s, v: setattr(s._mg(), "levels_pc_type", v))
    mg_levels_ksp_max_it = property(lambda s: s._mg().levels_ksp_max_it,
                                    lambda s, v: setattr(s._mg(), "levels_ksp_max_it", v))
    mg_levels_richardson_scale = property(
        lambda s: s._mg().levels_richardson_scale,
        lambda s, v: setattr(s._mg(), "levels_richardson_scale", v))

    @property
    def mg_levels_eigenvalues(self):
        return self._mg().levels_eigenvalues

    @mg_levels_eigenvalues.setter
    def mg_levels_eigenvalues(self, v):
        self._mg().levels_eigenvalues = (C.c_double * 2)(*v)

    @property
    def mg_levels_esteig(self):
        return self._mg().levels_esteig

    @mg_levels_esteig.setter
    def mg_levels_esteig(self, v):
        self._mg().levels_esteig = (C.c_double * 4)(*v)

    def _fgmres(self):
        if "fgmres" not in self.__dict__:
            f = L.KspFgmresOpts()
            L.call("pb_ksp_fgmres_opts_default", C.byref(f))
            self.__dict__["fgmres"] = f
        return self.__dict__["fgmres"]

    fgmres = property(_fgmres)
    fgmres_restart = property(lambda s: s._fgmres().restart,
                              lambda s, v: setattr(s._fgmres(), "restart", v))
    fgmres_haptol = property(lambda s: s._fgmres().haptol,
                             lambda s, v: setattr(s._fgmres(), "haptol", v))
    fgmres_cgs_refinement = property(lambda s: s._fgmres().cgs_refinement,
                                     lambda s, v: setattr(s._fgmres(), "cgs_refinement", v))

    def _cheb(self):
        if "chebyshev" not in self.__dict__:
            c = L.KspChebyshevOpts()
            L.call("pb_ksp_chebyshev_opts_default", C.byref(c))
            self.__dict__["chebyshev"] = c
        return self.__dict__["chebyshev"]

    chebyshev = property(_cheb)
    chebyshev_emin = property(lambda s: s._cheb().emin, lambda s, v: setattr(s._cheb(), "emin", v))
    chebyshev_emax = property(lambda s: s._cheb().emax, lambda s, v: setattr(s._cheb(), "emax", v))
    chebyshev_esteig_steps = property(lambda s: s._cheb().esteig_steps,
                                      lambda s, v: setattr(s._cheb(), "esteig_steps", v))

    @property
    def chebyshev_esteig(self):
        return self._cheb().esteig

    @chebyshev_esteig.setter
    def chebyshev_esteig(self, v):
        self._cheb().esteig = (C.c_double * 4)(*v)


def ksp_options(argv=(), **kw):
    o = KspOptions()
    L.call("pb_ksp_opts_default", C.byref(o))
    if argv:
        arr = (C.c_char_p * len(argv))(*[str(a).encode() for a in argv])
        L.call("pb_ksp_opts_parse", C.byref(o), len(argv), arr)
        L.call("pb_ksp_chebyshev_opts_parse", C.byref(o.chebyshev), len(argv), arr)
        L.call("pb_ksp_fgmres_opts_parse", C.byref(o.fgmres), len(argv), arr)
        if any(str(a).startswith("-mg_") for a in argv):
            L.call("pb_pc_mg_opts_parse", C.byref(o.mg), len(argv), arr)
        nt = C.c_int(KSP_NORM_DEFAULT)
        L.call("pb_ksp_norm_type_parse", C.byref(nt), len(argv), arr)
        o.norm_type = nt.value
    for k, v in kw.items():
        setattr(o, k, v)
    return o


def pc_mg_options(argv=(), **kw):
    """pb_pc_mg_opts: the defaults, then -mg_levels_* options from argv, then fields by keyword."""
    m = L.PcMgOpts()
    L.call("pb_pc_mg_opts_default", C.byref(m))
    if argv:
        arr = (C.c_char_p * len(argv))(*[str(a).encode() for a in argv])
        L.call("pb_pc_mg_opts_parse", C.byref(m), len(argv), arr)
    for k, v in kw.items():
        if k in ("levels_eigenvalues", "levels_esteig"):
            v = (C.c_double * len(v))(*v)
        setattr(m, k, v)
    return m


def tridiag_extreme_eigenvalues(diag, off=()):
    """(smallest, largest) eigenvalue of the symmetric tridiagonal matrix (host code, n <= 64)."""
    d = np.ascontiguousarray(diag, dtype=np.float64)
    e = np.ascontiguousarray(off if len(off) else [0.0], dtype=np.float64)
    if len(off) != max(d.size - 1, 0):
        raise ValueError("off-diagonal must have n - 1 entries")
    lo, hi = C.c_double(), C.c_double()
    L.call("pb_tridiag_extreme_eigenvalues", int(d.size), _dptr(d), _dptr(e), C.byref(lo),
           C.byref(hi))
    return lo.value, hi.value


class KSP:
    """KSPCreate + KSPSetOperators(ksp, A, P) + KSPSetFromOptions (src/poissbox.f90:293-295)."""

    def __init__(self, A, P=None, options=None):
        self.opts = options if isinstance(options, L.KspOpts) else ksp_options(options or ())
        h = C.c_void_p()
        L.call("pb_ksp_create", A.h, (P or A).h, C.byref(self.opts), C.byref(h))
        self.h = h
        if self.opts.ksp_type == KSP_CHEBYSHEV and isinstance(self.opts, KspOptions):
            try:
                L.call("pb_ksp_chebyshev_set_opts", h, C.byref(self.opts.chebyshev))
            except L.PbError:
                self.destroy()
                raise
        if self.opts.ksp_type == KSP_FGMRES and isinstance(self.opts, KspOptions):
            try:
                L.call("pb_ksp_fgmres_set_opts", h, C.byref(self.opts.fgmres))
            except L.PbError:
                self.destroy()
                raise
        # a KSP whose options never named the level smoother is given none (the default path)
        if self.opts.pc_type == PC_MG and "mg" in getattr(self.opts, "__dict__", {}):
            try:
                L.call("pb_ksp_pc_mg_set_opts", h, C.byref(self.opts.mg))
            except L.PbError:
                self.destroy()
                raise

        if getattr(self.opts, "norm_type", KSP_NORM_DEFAULT) != KSP_NORM_DEFAULT:
            try:
                self.set_norm_type(self.opts.norm_type)
            except L.PbError:
                self.destroy()
                raise

    def set_norm_type(self, norm_type):
        """KSPSetNormType: KSP_NORM_* (the number history, the tests and rnorm are taken in)."""
        L.call("pb_ksp_set_norm_type", self.h, int(norm_type))

    @property
    def norm_type(self):
        """(as set, in force): KSP_NORM_DEFAULT as set until set_norm_type; in force the default
        is preconditioned (cg, richardson, chebyshev, pipecg), unpreconditioned (fgmres) or none
        (preonly)."""
        s, e = C.c_int(), C.c_int()
        L.call("pb_ksp_get_norm_type", self.h, C.byref(s), C.byref(e))
        return s.value, e.value

    def pc_mg_set_opts(self, mg):
        """pb_ksp_pc_mg_set_opts: mg is a PcMgOpts (pc_mg_options())."""
        L.call("pb_ksp_pc_mg_set_opts", self.h, C.byref(mg))

    def pc_mg_get_opts(self):
        m = L.PcMgOpts()
        L.call("pb_ksp_pc_mg_get_opts", self.h, C.byref(m))
        return m

    def fgmres_set_opts(self, restart=None, haptol=None, cgs_refinement=None):
        """pb_ksp_fgmres_set_opts: the fields given replace the KSP's current ones."""
        f = self.fgmres_get_opts()
        for name, v in (("restart", restart), ("haptol", haptol),
                        ("cgs_refinement", cgs_refinement)):
            if v is not None:
                setattr(f, name, v)
        L.call("pb_ksp_fgmres_set_opts", self.h, C.byref(f))

    def fgmres_get_opts(self):
        f = L.KspFgmresOpts()
        L.call("pb_ksp_fgmres_get_opts", self.h, C.byref(f))
        return f

    def solve(self, b, x):
        """Returns (reason, its, history): the res.nhist logged norms (its + 1 of them, its
        after a breakdown exit)."""
        res = L.KspResult()
        hist = np.zeros(int(self.opts.max_it) + 1)
        L.call("pb_ksp_solve", self.h, b.h, x.h, C.byref(res), _dptr(hist), hist.size)
        self.result = res
        return res.reason, res.its, hist[: res.nhist].copy()

    def begin(self, b, x):
        L.call("pb_ksp_begin", self.h, b.h, x.h)

    def iterate(self, n):
        L.call("pb_ksp_iterate", self.h, int(n))

    def end(self):
        res = L.KspResult()
        hist = np.zeros(int(self.opts.max_it) + 1)
        L.call("pb_ksp_end", self.h, C.byref(res), _dptr(hist), hist.size)
        self.result = res
        return res.reason, res.its, hist[: res.nhist].copy()

    def guess_form(self, b, x):
        """-ksp_guess_type fischer: x = the projected guess for b (solve() does this itself)."""
        L.call("pb_ksp_guess_form", self.h, b.h, x.h)

    def guess_update(self, b, x):
        """Add the direction of the solution x of b (solved from the last formed guess)."""
        L.call("pb_ksp_guess_update", self.h, b.h, x.h)

    def guess_reset(self):
        L.call("pb_ksp_guess_reset", self.h)

    def guess_size(self):
        """(directions stored, most that are kept)."""
        curl, maxl = C.c_int(), C.c_int()
        L.call("pb_ksp_guess_size", self.h, C.byref(curl), C.byref(maxl))
        return curl.value, maxl.value

    def chebyshev_eigenvalues(self):
        """(emin, emax, estimated) of the next -ksp_type chebyshev solve; runs the estimate if the
        bounds were not given and it has not run yet (collective)."""
        lo, hi, est = C.c_double(), C.c_double(), C.c_int()
        L.call("pb_ksp_chebyshev_get_eigenvalues", self.h, C.byref(lo), C.byref(hi), C.byref(est))
        return lo.value, hi.value, bool(est.value)

    def pc_apply(self, r, z):
        """PCApply: z = M^-1 r (no null-space removal)."""
        L.call("pb_ksp_pc_apply", self.h, r.h, z.h)

    @property
    def pc_levels(self):
        v = C.c_int(0)
        L.call("pb_ksp_pc_levels", self.h, C.byref(v))
        return v.value

    def pc_set_coefficient_from(self, op):
        """pb_ksp_pc_set_coefficient_from: the -pc_type sor | mg levels become div(beta_l grad) of
        the VARCOEF Mat `op` (usually A); None returns to the constant-coefficient PC. The KSP
        holds op: keep it alive until the KSP is destroyed or the coefficient is unset."""
        L.call("pb_ksp_pc_set_coefficient_from", self.h, op.h if op is not None else None)
        self._pc_coef = op

    def pc_coefficient_from(self):
        """The Mat given to pc_set_coefficient_from, or None."""
        h = C.c_void_p()
        L.call("pb_ksp_pc_get_coefficient_from", self.h, C.byref(h))
        if not h.value:
            return None
        op = getattr(self, "_pc_coef", None)
        assert op is not None and op.h.value == h.value
        return op

    def destroy(self):
        if self.h:
            L.call("pb_ksp_destroy", self.h)
            self.h = None


# ---- reference-named entry points ----------------------------------------------------------
def initialise_grid(ctx, nglobal, L_=(1.0, 1.0, 1.0)):
    """src/poissbox.f90:183-204"""
    return DA(ctx, nglobal, L_)


def initialise_linear_system(da, grid_deltas, matrix_free=True):
    """src/poissbox.f90:206-240: returns (P, A, x, b); A is the matrix-free operator when
    matrix_free (src/example.f90:60-65), else A = P."""
    P = Mat(da, ASSEMBLED27, grid_deltas)
    A = Mat(da, STAR7, grid_deltas) if matrix_free else P
    return P, A, Vec(da), Vec(da)


def compute_lapl_pointwise(da, grid_deltas, x, b):
    """src/poissbox.f90:84-126 (one pass of the stencil, same kernel as mfmult)."""
    op = Mat(da, STAR7, grid_deltas)
    try:
        op.mult(x, b)
    finally:
        op.destroy()


def solve(P, A, x, b, options=("-ksp_type", "cg", "-pc_type", "jacobi")):
    """src/poissbox.f90:269-298: constant null space on A and P, KSPSolve(b -> x)."""
    ksp = KSP(A, P, options)
    try:
        return ksp.solve(b, x)
    finally:
        ksp.destroy()


# ---- tridiagonal / compact ------------------------------------------------------------------
def tdma_batched(ctx, n, nbatch, line_stride, elem_stride, a_ptr, b_ptr, c_ptr, d_ptr,
                 periodic=False):
    L.call("pb_tdma_batched", ctx.h, int(n), int(nbatch), int(line_stride), int(elem_stride),
           a_ptr, b_ptr, c_ptr, d_ptr, int(bool(periodic)))


def pcr_alpha_batched(ctx, n, nbatch, line_stride, elem_stride, alpha, d_ptr):
    L.call("pb_pcr_alpha_batched", ctx.h, int(n), int(nbatch), int(line_stride),
           int(elem_stride), float(alpha), d_ptr)


def compact_1d_batched(ctx, kind, stagger, dx, n, nbatch, line_stride, elem_stride, f_ptr,
                       out_ptr):
    L.call("pb_compact_1d_batched", ctx.h, int(kind), int(stagger), float(dx), int(n),
           int(nbatch), int(line_stride), int(elem_stride), f_ptr, out_ptr)


def compact_grad(da, dx, f, df3):
    arr = (C.c_void_p * 3)(*[v.h.value for v in df3])
    L.call("pb_compact_grad", da.h, _d_3(dx), f.h, arr)


def compact_div(da, dx, f3, df):
    arr = (C.c_void_p * 3)(*[v.h.value for v in f3])
    L.call("pb_compact_div", da.h, _d_3(dx), arr, df.h)


def compact_interp(da, stagger, f, fi):
    L.call("pb_compact_interp", da.h, int(stagger), f.h, fi.h)


def compact_lapl(da, dx, f, out):
    L.call("pb_compact_lapl", da.h, _d_3(dx), f.h, out.h)


# host-array forms (the reference's module procedures on process-local arrays)
def tdma_host(ctx, a, b, c, d, periodic=False):
    """tdma / tdma_periodic (src/tridsol.f90:22-74) on host arrays, batched over leading axes:
    the last axis is the line. b and d are updated in place like the reference."""
    for v in (a, b, c, d):
        assert v.dtype == np.float64 and v.flags.c_contiguous and v.shape == d.shape
    n = d.shape[-1]
    L.call("pb_tdma_batched_host", ctx.h, n, d.size // n, n, 1, _dptr(a), _dptr(b), _dptr(c),
           _dptr(d), int(bool(periodic)))


def compact_host(ctx, op, f, n, dx=(1.0, 1.0, 1.0), stagger=-1):
    """grad / div / interp / lapl (src/compact_schemes.f90) on whole host arrays (C order
    [c][k][j][i] == Fortran (i, j, k, c)); returns the result array."""
    f = np.ascontiguousarray(f, dtype=np.float64).reshape(-1)
    N = int(np.prod(n))
    out = np.empty(3 * N if op == "grad" else N)
    if op == "interp":
        L.call("pb_compact_interp_host", ctx.h, _i64_3(n), int(stagger), _dptr(f), _dptr(out))
    else:
        L.call(f"pb_compact_{op}_host", ctx.h, _i64_3(n), _d_3(dx), _dptr(f), _dptr(out))
    return out


def compact_lapl_fast(da, dx, f, out):
    """3-pass factorised compact Laplacian with PCR line solves (agrees with compact_lapl to
    rounding); the operator PB_OP_COMPACT applies."""
    L.call("pb_compact_lapl_fast", da.h, _d_3(dx), f.h, out.h)


def compact_grad_fast(da, dx, f, df3):
    """compact_grad by factorised half-operator line passes (112 B/DoF; agrees with compact_grad
    to rounding). f must not be one of df3, and the three df3 must be distinct."""
    arr = (C.c_void_p * 3)(*[v.h.value for v in df3])
    L.call("pb_compact_grad_fast", da.h, _d_3(dx), f.h, arr)


def compact_div_fast(da, dx, f3, df):
    """compact_div by factorised half-operator line passes (112 B/DoF; agrees with compact_div
    to rounding). df must not be one of f3, and the three f3 must be distinct."""
    arr = (C.c_void_p * 3)(*[v.h.value for v in f3])
    L.call("pb_compact_div_fast", da.h, _d_3(dx), arr, df.h)


def compact_interp_fast(da, stagger, f, fi):
    """compact_interp by three half-operator line passes (48 B/DoF; agrees with compact_interp
    to rounding)."""
    L.call("pb_compact_interp_fast", da.h, int(stagger), f.h, fi.h)
