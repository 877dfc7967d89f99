"""numpy restatement of the variable-coefficient -pc_type sor | mg (pb_ksp_pc_set_coefficient_from;
DESIGN.md §3.5): the V-cycle of mg_smoothers_restatement with every level's smoother, residual and
operator replaced by div(beta_l grad) of varcoef_restatement. This file is the feature's definition.
One rounded numpy operation per arithmetic step; the library is built -ffp-contract=off.

  levels      the plan of plan_levels; beta_0 = the operator's beta; the coarse cell (I, J, K) is
              beta_(l+1) = 0.125 * (((b000 + b100) + (b010 + b110)) + ((b001 + b101) + (b011 + b111)))
              with b_abc the fine cell (2I + a, 2J + b, 2K + c); c_d = 1 / (2^l h_d)^2, taken as
              varcoef_restatement.axis_coeffs of the level's spacing
  faces       g_n, diag_c and y = A x on a level: varcoef_restatement._faces / diag / apply
  half-sweep  dinv = 1.0 / diag_c; nb = ((((g_z- x_z- + g_y- x_y-) + g_x- x_x-) + g_x+ x_x+) +
              g_y+ x_y+) + g_z+ x_z+; t = (b - nb) * dinv; x = (1 - omega) * x + omega * t on the
              colour, red = (i + j + k) even. The zero-initialised first half-sweep has nb = 0.0 and
              xo = 0.0 in the same formula
  residual    b - apply(x), the flux form
  unchanged   the cycle order, the pre and post legs, the coarsest level's coarse_its symmetric
              sweeps, restrict, prolong_add and the nu repetition (VCycle); pc = sor is one level
"""
import numpy as np

import mg_smoothers_restatement as M
import varcoef_restatement as V


def coarsen(beta):
    """(nz, ny, nx) -> (nz/2, ny/2, nx/2): the arithmetic mean of a cell's 8 children."""
    b = lambda a, bb, c: beta[c::2, bb::2, a::2]
    lo = (b(0, 0, 0) + b(1, 0, 0)) + (b(0, 1, 0) + b(1, 1, 0))
    hi = (b(0, 0, 1) + b(1, 0, 1)) + (b(0, 1, 1) + b(1, 1, 1))
    return 0.125 * (lo + hi)


class VarLevel:
    def __init__(self, n, h, beta, mean):
        self.n = tuple(int(v) for v in n)
        self.h = tuple(float(d) for d in h)
        self.shape = (self.n[2], self.n[1], self.n[0])
        self.beta = np.asarray(beta, dtype=np.float64).reshape(self.shape)
        self.mean = mean
        self.g = V._faces(self.beta, self.n, self.h, mean)  # z-, y-, x-, x+, y+, z+
        self.diag = V.diag(self.beta, self.n, self.h, mean).reshape(self.shape)
        self.dinv = 1.0 / self.diag
        k, j, i = np.indices(self.shape)
        self.red = ((i + j + k) % 2) == 0

    def apply(self, x):
        return V.apply(x, self.beta, self.n, self.h, self.mean).reshape(self.shape)

    def half_sweep(self, x, b, omega, color, zero=False):
        sel = self.red if color == 0 else ~self.red
        if zero:  # the zero-initialised first half-sweep
            nb, xo = 0.0, 0.0
        else:
            g, xn = self.g, V._neighbours(x)
            nb = g[0] * xn[0] + g[1] * xn[1]
            for gn, xv in zip(g[2:], xn[2:]):
                nb = nb + gn * xv
            xo = x
        t = (b - nb) * self.dinv
        new = (1.0 - omega) * xo + omega * t
        return np.where(sel, new, x)


class VarVCycle(M.VCycle):
    """z = M^-1 r with variable-coefficient levels: M.VCycle's cycle over VarLevels."""

    def __init__(self, n, h, beta, mean=V.ARITHMETIC, smoother=None, levels=0, coarse_its=8,
                 omega=1.0, pc="mg"):
        self.n, self.h = tuple(n), tuple(h)
        self.sm = smoother or M.Smoother()
        assert self.sm.pc == "sor", "the variable-coefficient levels smooth with sor"
        self.coarse_its = max(1, int(coarse_its)) if pc == "mg" else 1
        self.omega = float(omega)
        self.L = M.plan_levels(self.n, levels) if pc == "mg" else 1
        b = np.asarray(beta, dtype=np.float64).reshape(self.n[2], self.n[1], self.n[0])
        self.lv = []
        for l in range(self.L):
            if l > 0:
                b = coarsen(b)
            self.lv.append(VarLevel([v >> l for v in self.n],
                                    [d * float(1 << l) for d in self.h], b, mean))

    def _pre(self, lv, b):
        w = self.omega
        x = np.zeros_like(b)
        for i in range(self.sm.nu):
            x = lv.half_sweep(x, b, w, 0, zero=i == 0)
            x = lv.half_sweep(x, b, w, 1)
        return x, b - lv.apply(x)

    def _coarsest(self, lv, b):
        w = self.omega
        x = np.zeros_like(b)
        x = lv.half_sweep(x, b, w, 0, zero=True)
        x = lv.half_sweep(x, b, w, 1)
        x = lv.half_sweep(x, b, w, 0)
        for _ in range(1, self.coarse_its):
            x = lv.half_sweep(x, b, w, 1)
            x = lv.half_sweep(x, b, w, 0)
        return x


class VarMgProblem(V.VarProblem):
    """A = PB_OP_VARCOEF(beta, mean), P a constant 7-point operator, and the PC's levels taken from
    A: pc "vsor" | "vmg" (other names than "sor" / "mg", which the restatements read as the
    constant-coefficient PCs of P)."""

    def __init__(self, n3, beta, mean=V.ARITHMETIC, pc="vmg", deltas=None, nullspace=1,
                 smoother=None, coarse_its=8, omega=1.0, levels=0):
        assert pc in ("vsor", "vmg")
        V.VarProblem.__init__(self, n3, beta, mean, pc="mg" if pc == "vmg" else "sor", p="const",
                              deltas=deltas, nullspace=nullspace)
        self.vpc, self.smoother = pc, smoother
        self.coarse_its, self.omega, self.levels = coarse_its, omega, levels
        self._build()

    def _build(self):
        self.vc = VarVCycle(self.n3, self.h, self.beta, self.mean, self.smoother, self.levels,
                            self.coarse_its, self.omega, pc=self.pc)

    def pc_apply(self, r, nranks=1):
        return self.vc.apply(r)

    def set_beta(self, beta, mean=None):
        V.VarProblem.set_beta(self, beta, mean)
        self._build()

    def after_create(self, ksp, P, A):
        """the hook of the tests' gpu_solve: the KSP's levels from A"""
        ksp.pc_set_coefficient_from(A)
