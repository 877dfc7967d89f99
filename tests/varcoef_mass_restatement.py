"""numpy restatement of the mass term of PB_OP_VARCOEF (pb_op_set_mass):
A = div(beta grad) - q, the operator of an implicit diffusion, viscous or heat step
(rho / dt) u - div(mu grad u) up to the sign, with its diagonal, the variable Jacobi and the levels
of the variable -pc_type sor | mg. This file is the feature's definition; it subclasses
varcoef_restatement / varcoef_mg_restatement, which stay as they are. One rounded numpy operation
per arithmetic step; the library is built -ffp-contract=off.

m is a cell-centred field of the operator's grid or None (every m_c = 1), s a scalar:

    q_c    = s * m_c                      (m None: q_c = s)
    y_c    = S6_c - q_c * x_c             S6_c: varcoef_restatement.apply's six-term flux sum
    diag_c = (-G6_c) - q_c                G6_c: varcoef_restatement.diag's six-term sum of the g_n

The operators here are negative semi-definite (A is the Laplacian itself): subtracting q >= 0
keeps A symmetric to the bit -- q_c * x_c touches the diagonal alone -- and makes it negative
definite as soon as q > 0 somewhere; A 1 = -q to the bit (S6 of a constant is 0.0 and
0.0 - q * 1.0 = -q). The mass is on iff s != 0; with it off every function below returns what its
parent returns, bit for bit.

Levels of the variable sor / mg: q_0 = s * m, q_(l+1) = varcoef_mg_restatement.coarsen(q_l) (the
mean of a cell's 8 children, same order, factor 0.125); a scalar-only mass stays s on every level.
Each level's dinv = 1.0 / diag with the diag above, the half-sweep's nb is unchanged (off-diagonals
only), the residual is b - y with the y above; transfers, cycle, level plan, coarsest sweeps and
the zero-start formula are varcoef_mg_restatement's.
"""
import numpy as np

import varcoef_mg_restatement as VM
import varcoef_restatement as V


def q_of(m, s, n3):
    """the mass term of the finest grid, (nz, ny, nx), or the scalar s where m is None"""
    if m is None:
        return float(s)
    return float(s) * np.asarray(m, dtype=np.float64).reshape(n3[2], n3[1], n3[0])


def _flat(q):
    return q if np.isscalar(q) else q.reshape(-1)


def apply(x, beta, n3, h, mean=V.ARITHMETIC, m=None, s=0.0):
    """y = A x, flat in natural (x fastest) order."""
    y = V.apply(x, beta, n3, h, mean)
    if s == 0.0:
        return y
    return y - _flat(q_of(m, s, n3)) * np.asarray(x, dtype=np.float64).reshape(-1)


def diag(beta, n3, h, mean=V.ARITHMETIC, m=None, s=0.0):
    d = V.diag(beta, n3, h, mean)
    if s == 0.0:
        return d
    return d - _flat(q_of(m, s, n3))


def mass_uniform(n3, seed=20240911, lo=0.5, hi=1.5):
    """the mass field of the tests: uniform in [lo, hi]"""
    return np.random.default_rng(seed).uniform(lo, hi, int(np.prod(n3)))


def _set_mass_on(pb, da, A, m, s, n3):
    """A.set_mass with m cut to the planes this rank owns"""
    if m is None:
        A.set_mass(None, s)
        return
    (_, _, k0), (_, _, nk) = da.get_corners()
    mv = pb.Vec(da)
    mv.set_values(np.asarray(m, dtype=np.float64).reshape(n3[2], -1)[k0:k0 + nk])
    A.set_mass(mv, s)
    mv.destroy()


class MassProblem(V.VarProblem):
    """A = PB_OP_VARCOEF(beta, mean) with the mass (m, s); P = A with pc "none" | "vjacobi", or a
    constant P (V.VarProblem). nullspace 0 by default: A is nonsingular with the mass on."""

    def __init__(self, n3, beta, mean=V.ARITHMETIC, m=None, s=0.0, pc="vjacobi", p=None,
                 deltas=None, nullspace=0):
        super().__init__(n3, beta, mean, pc=pc, p=p, deltas=deltas, nullspace=nullspace)
        self.set_mass(m, s)

    def set_mass(self, m=None, s=0.0):
        self.m = None if m is None else np.asarray(m, dtype=np.float64)
        self.s = float(s)
        if self.pc == "vjacobi":
            self.dinv = 1.0 / diag(self.beta, self.n3, self.h, self.mean, self.m, self.s)

    def apply(self, x, nranks=1):
        return apply(x, self.beta, self.n3, self.h, self.mean, self.m, self.s)

    def set_beta(self, beta, mean=None):
        super().set_beta(beta, mean)
        self.set_mass(self.m, self.s)

    def mats(self, pb, da):
        P, A = super().mats(pb, da)
        _set_mass_on(pb, da, A, self.m, self.s, self.n3)
        return P, A


class MassLevel(VM.VarLevel):
    """VarLevel with the level's mass term q (an array of the level's shape, or a scalar)."""

    def __init__(self, n, h, beta, mean, q):
        super().__init__(n, h, beta, mean)
        self.q = q
        self.diag = self.diag - q
        self.dinv = 1.0 / self.diag  # (half_sweep: nb from the off-diagonals, t = (b - nb) * dinv)

    def apply(self, x):
        return super().apply(x) - self.q * x


class MassVCycle(VM.VarVCycle):
    """VarVCycle over MassLevels: q_0 = s * m, q_(l+1) = coarsen(q_l); a scalar mass stays s."""

    def __init__(self, n, h, beta, mean=V.ARITHMETIC, m=None, s=0.0, smoother=None, levels=0,
                 coarse_its=8, omega=1.0, pc="mg"):
        super().__init__(n, h, beta, mean, smoother, levels, coarse_its, omega, pc)
        if s == 0.0:
            return
        q = q_of(m, s, self.n)
        lv = []
        for l, v in enumerate(self.lv):
            if l > 0 and not np.isscalar(q):
                q = VM.coarsen(q)
            lv.append(MassLevel(v.n, v.h, v.beta, v.mean, q))
        self.lv = lv


class MassMgProblem(VM.VarMgProblem):
    """A = PB_OP_VARCOEF(beta, mean) with the mass (m, s), P a constant 7-point operator and the
    PC's levels taken from A: pc "vsor" | "vmg"."""

    def __init__(self, n3, beta, mean=V.ARITHMETIC, m=None, s=0.0, pc="vmg", deltas=None,
                 nullspace=0, smoother=None, coarse_its=8, omega=1.0, levels=0):
        self.m = None if m is None else np.asarray(m, dtype=np.float64)
        self.s = float(s)
        super().__init__(n3, beta, mean, pc=pc, deltas=deltas, nullspace=nullspace,
                         smoother=smoother, coarse_its=coarse_its, omega=omega, levels=levels)

    def _build(self):
        self.vc = MassVCycle(self.n3, self.h, self.beta, self.mean, self.m, self.s, self.smoother,
                             self.levels, self.coarse_its, self.omega, pc=self.pc)

    def set_mass(self, m=None, s=0.0):
        self.m = None if m is None else np.asarray(m, dtype=np.float64)
        self.s = float(s)
        self._build()

    def apply(self, x, nranks=1):
        return apply(x, self.beta, self.n3, self.h, self.mean, self.m, self.s)

    def mats(self, pb, da):
        P, A = super().mats(pb, da)
        _set_mass_on(pb, da, A, self.m, self.s, self.n3)
        return P, A
