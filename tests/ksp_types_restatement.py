"""numpy restatement of -ksp_type preonly and -ksp_type richardson on the
oracle's building blocks: the operators (O.stencil, O.lapl, O.assembled), the preconditioners
(O.diag, O.mg_apply, O.fft_pc_apply) and nothing else of the oracle's solver.

PETSc is not available here: this is KSPSolve_PREONLY / KSPSolve_Richardson (PC_LEFT, the
preconditioned norm, KSPConvergedDefault, the constant null space) as restated -- "parity
unpinned", like the nonzero-guess and projected-guess restatements.

preonly:    x = N(M^-1 b); N = the mean subtraction, skipped with the spectral PC (P^+ zeroes
            mode 0 itself). Result fields (4, 1, 0.0, 0.0, nhist 0).
richardson: r = b (x = 0) or b - A x0; i = 0, 1, ...: z = N(M^-1 r), rnorm = ||z||, logged as
            history[i]; non-finite -> -9 with its = i; the default test with its = i
            (ttol = max(rtol rnorm0, atol); the dtol test not at i = 0 of a zero guess, where
            rnorm is the reference itself); i = max_it -> -3; else x += scale z, r = b - A x.
            nhist = its + 1 always.
"""
import numpy as np

from oracle import oracle as O

TWO_PI = 2 * np.pi


class Problem:
    """One (operator, PC) pair as the GPU tests build it and as the restatement applies it."""

    def __init__(self, n3, pc="jacobi", op="star7", deltas=None, nullspace=1):
        self.n3, self.pc, self.op, self.nullspace = tuple(n3), pc, op, nullspace
        self.N = int(np.prod(n3))
        # config 5 (compact A = P, spectral PC) lives on the 2 pi box, as in test_gpu_parity
        self.L = (TWO_PI,) * 3 if (op, pc) == ("compact", "fft") else (1.0, 1.0, 1.0)
        self.h = tuple(deltas) if deltas else tuple(l / m for l, m in zip(self.L, n3))

    def apply(self, x, nranks=1):
        if self.op == "compact":
            return O.lapl(x, self.n3, self.h)
        if self.op == "assembled":
            return O.assembled(x, self.n3, self.h, nranks=nranks)
        return O.stencil(x, self.n3, self.h)

    def rhs(self, seed=20231015, nranks=1):
        return self.apply(O.fill_random(self.N, seed), nranks)

    def pc_apply(self, r, nranks=1):
        if self.pc == "none":
            return r.copy()
        if self.pc == "jacobi":
            return (1.0 / O.diag(self.h)) * r  # PCJacobi stores the reciprocal
        if self.pc == "fft":
            return O.fft_pc_apply(r, self.n3, self.h, compact=self.op == "compact")
        return O.mg_apply(r, self.n3, self.h, pc=self.pc, nranks=nranks)

    def remove(self, z):
        return z - z.mean() if self.nullspace else z

    def mats(self, pb, da):
        """(P, A) on the GPU, as tests/test_gpu_initial_guess.Case.mats."""
        if self.op == "compact":
            A = pb.Mat(da, pb.COMPACT, self.h)
            return (A if self.pc == "fft" else pb.Mat(da, pb.ASSEMBLED27, self.h)), A
        if self.op == "assembled":
            P = pb.Mat(da, pb.ASSEMBLED27, self.h)
            return P, P
        if self.pc == "fft":
            A = pb.Mat(da, pb.STAR7, self.h)
            return A, A
        return pb.Mat(da, pb.ASSEMBLED27, self.h), pb.Mat(da, pb.STAR7, self.h)


def preonly(prob, b, nranks=1):
    """(x, reason, its, history, rnorm0)"""
    z = prob.pc_apply(b, nranks)
    if prob.pc != "fft":
        z = prob.remove(z)
    return z, 4, 1, np.zeros(0), 0.0


def richardson(prob, b, x0=None, scale=1.0, rtol=1e-5, atol=1e-50, dtol=1e5, max_it=10000,
               mode="default", nranks=1):
    """(x, reason, its, history, rnorm0); x0 = None: the zero guess. mode: the stopping reference
    of a nonzero guess (default ||N(M^-1 b)||, ||z_0|| if that is 0; initial; min)."""
    guess = x0 is not None
    x = x0.copy() if guess else np.zeros_like(b)
    r = b - prob.apply(x, nranks) if guess else b.copy()
    hist, i, rn0, reason = [], 0, 0.0, 0
    while True:
        z = prob.remove(prob.pc_apply(r, nranks))
        rn = float(np.sqrt(np.sum(z * z)))
        if i == 0:
            rn0 = rn
            if guess and mode != "initial":
                zb = prob.remove(prob.pc_apply(b, nranks))
                nb = float(np.sqrt(np.sum(zb * zb)))
                rn0 = (nb if nb != 0.0 else rn) if mode == "default" else min(nb, rn)
        hist.append(rn)
        if not np.isfinite(rn):
            reason = -9
            break
        ttol = max(rtol * rn0, atol)
        if rn <= ttol:
            reason = 3 if rn < atol else 2
            break
        if (i > 0 or guess) and rn >= dtol * rn0:
            reason = -4
            break
        if i >= max_it:
            reason = -3
            break
        x = x + scale * z
        i += 1
        r = b - prob.apply(x, nranks)
    return x, reason, i, np.asarray(hist), rn0


def ttol_margin_ok(hist, rtol, rn0, atol=1e-50):
    """the last two logged norms are more than 1e-6 (relative) from ttol: the GPU's differently
    ordered sums cannot move the stopping iteration"""
    ttol = max(rtol * rn0, atol)
    return all(abs(v - ttol) > 1e-6 * ttol for v in hist[-2:])
