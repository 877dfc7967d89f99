"""numpy restatement of PB_OP_VARCOEF: the variable-coefficient 7-point operator
y = div(beta grad x) in flux form, its diagonal, the coefficient fields the tests use, and
`VarProblem`, which gives the KSP restatements (norm_type_restatement.cg,
ksp_types_restatement.richardson / preonly, chebyshev_restatement, fgmres_restatement,
pipecg_restatement) this operator.

This file is the operator's definition: the reference has no counterpart (there a caller's own
MATOP_MULT supplies such an operator, src/poissbox.f90:226-267). beta is cell-centred, arrays are
(nz, ny, nx) with x fastest, every axis periodic. With c_d = 1 / h_d^2 (what pb_lapl_1d_coeffs /
the star's coefficients give for the deltas), the six neighbours n in the 7-point operator's order
without the centre -- z-, y-, x-, x+, y+, z+ -- and every product, sum and quotient rounded (numpy
evaluates one operation at a time; the library is built -ffp-contract=off):

    face(a, b) = 0.5 * (a + b)              arithmetic
                 (2.0 * (a * b)) / (a + b)  harmonic
    g_n    = c_d * face(beta_n, beta_c)
    t_n    = g_n * (x_n - x_c)
    y_c    = ((((t_z- + t_y-) + t_x-) + t_x+) + t_y+) + t_z+
    diag_c = -(((((g_z- + g_y-) + g_x-) + g_x+) + g_y+) + g_z+)

Both means are commutative in IEEE arithmetic, so the face between two cells has the same bits
seen from either side: the matrix is symmetric to the bit, and x_n - x_c = 0 for a constant makes
A 1 = 0 to the bit.
"""
import numpy as np

from oracle import oracle as O
from ksp_types_restatement import Problem

ARITHMETIC, HARMONIC = 0, 1
MEANS = {"arithmetic": ARITHMETIC, "harmonic": HARMONIC}


def face(a, b, mean):
    if mean == HARMONIC:
        return (2.0 * (a * b)) / (a + b)
    return 0.5 * (a + b)


def axis_coeffs(h):
    """(cx, cy, cz) = 1 / h_d^2."""
    return tuple(1.0 / (d * d) for d in h)


def _neighbours(a):
    """the six neighbours of every cell of a (nz, ny, nx): z-, y-, x-, x+, y+, z+"""
    return (np.roll(a, 1, 0), np.roll(a, 1, 1), np.roll(a, 1, 2),
            np.roll(a, -1, 2), np.roll(a, -1, 1), np.roll(a, -1, 0))


def _faces(beta, n3, h, mean):
    cx, cy, cz = axis_coeffs(h)
    b = np.asarray(beta, dtype=np.float64).reshape(n3[2], n3[1], n3[0])
    return [c * face(bn, b, mean) for c, bn in zip((cz, cy, cx, cx, cy, cz), _neighbours(b))]


def apply(x, beta, n3, h, mean=ARITHMETIC):
    """y = A x, flat in natural (x fastest) order."""
    g = _faces(beta, n3, h, mean)
    xc = np.asarray(x, dtype=np.float64).reshape(n3[2], n3[1], n3[0])
    t = [gn * (xn - xc) for gn, xn in zip(g, _neighbours(xc))]
    y = t[0] + t[1]
    for tn in t[2:]:
        y = y + tn
    return y.reshape(-1)


def diag(beta, n3, h, mean=ARITHMETIC):
    g = _faces(beta, n3, h, mean)
    s = g[0] + g[1]
    for gn in g[2:]:
        s = s + gn
    return (-s).reshape(-1)


# ---------------------------------------------------------------------------------------------
# the coefficient fields of the tests (all seeded)
# ---------------------------------------------------------------------------------------------
def beta_one(n3):
    return np.ones(int(np.prod(n3)))


def beta_random(n3, seed=20240607, contrast=1e3):
    """log-uniform in [1 / contrast, 1]"""
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(-np.log(contrast), 0.0, int(np.prod(n3))))


def beta_sphere(n3, inside=1e-3, radius=0.3):
    """1 outside, `inside` inside the sphere of `radius` about the centre of the unit box (cell
    centres at (i + 1/2) / n)"""
    c = [(np.arange(m) + 0.5) / m - 0.5 for m in n3]
    z, y, x = np.meshgrid(c[2], c[1], c[0], indexing="ij")
    return np.where(x * x + y * y + z * z < radius * radius, inside, 1.0).reshape(-1)


FIELDS = {"one": beta_one, "random": beta_random, "sphere": beta_sphere}


class VarProblem(Problem):
    """A = PB_OP_VARCOEF(beta, mean); the preconditioner from P.

    p = "var": P = A, pc "none" or "vjacobi" (the Jacobi PC of the variable diagonal; another name
    than "jacobi" because the restatements read that as the constant diagonal O.diag(h));
    p = "const": P = the constant-coefficient 7-point operator of the same deltas, pc any of
    none, jacobi, sor, mg, fft (the existing restatements' PCs, unchanged)."""

    def __init__(self, n3, beta, mean=ARITHMETIC, pc="vjacobi", p=None, deltas=None, nullspace=1):
        super().__init__(n3, pc=pc, op="star7", deltas=deltas, nullspace=nullspace)
        self.beta = np.asarray(beta, dtype=np.float64)
        self.mean = mean
        self.p = p if p is not None else ("var" if pc in ("vjacobi", "none") else "const")
        assert pc in ("vjacobi", "none") if self.p == "var" else pc != "vjacobi", (self.p, pc)
        self.dinv = 1.0 / diag(self.beta, self.n3, self.h, mean) if pc == "vjacobi" else None

    @property
    def pc_argv(self):
        return "jacobi" if self.pc == "vjacobi" else self.pc

    def apply(self, x, nranks=1):
        return apply(x, self.beta, self.n3, self.h, self.mean)

    def rhs(self, seed=20231015, nranks=1):
        return self.apply(O.fill_random(self.N, seed), nranks)

    def pc_apply(self, r, nranks=1):
        if self.pc == "vjacobi":
            return self.dinv * r  # PCJacobi stores the reciprocal
        return super().pc_apply(r, nranks)

    def set_beta(self, beta, mean=None):
        self.beta = np.asarray(beta, dtype=np.float64)
        self.mean = self.mean if mean is None else mean
        if self.pc == "vjacobi":
            self.dinv = 1.0 / diag(self.beta, self.n3, self.h, self.mean)

    def mats(self, pb, da):
        """(P, A) on the GPU; beta cut to the planes this rank owns."""
        A = pb.Mat(da, pb.VARCOEF, self.h)
        (_, _, k0), (_, _, nk) = da.get_corners()
        bv = pb.Vec(da)
        bv.set_values(self.beta.reshape(self.n3[2], -1)[k0:k0 + nk])
        A.set_coefficient(bv, self.mean)
        bv.destroy()
        if self.p == "var":
            return A, A
        return pb.Mat(da, pb.STAR7 if self.pc == "fft" else pb.ASSEMBLED27, self.h), A
