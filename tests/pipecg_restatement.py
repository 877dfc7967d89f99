"""numpy restatement of -ksp_type pipecg on the oracle's building blocks, as
tests/ksp_types_restatement.py restates Richardson (its Problem is reused): the operators and the
preconditioners (O.stencil, O.lapl, O.assembled, O.diag, O.mg_apply, O.fft_pc_apply) and nothing
of the oracle's solver.

PETSc is not available here: this is KSPSolve_PIPECG (pipecg.c; Ghysels & Vanroose) with PC_LEFT,
KSPConvergedDefault and the constant null space, written from knowledge of that file -- "parity
unpinned". N is the mean subtraction, applied after every PC application.

  r = b (x = 0) or b - A x0;  u = N(M^-1 r);  w = A u
  i = 0, 1, ...:
    gamma = r.u, delta = w.u, dp = ||u|| | ||r|| | sqrt|gamma| | 0 (preconditioned |
      unpreconditioned | natural | none), sum w -- one reduction
    m = N(M^-1 w);  n = A m
    history[i] = dp; non-finite -> -9 with its = i; the default test with its = i (ttol =
      max(rtol rnorm0, atol); the dtol test not at i = 0 of a zero guess); norm type none: no test
      but i >= max_it -> 4; i = max_it -> -3
    i = 0: alpha = gamma / delta;  z = n, q = m, s = w, p = u
    i > 0: beta = gamma / gamma_old;  alpha = gamma / (delta - (beta / alpha_old) gamma);
           z = n + beta z, q = m + beta q, s = w + beta s, p = u + beta p
    x += alpha p;  r -= alpha s;  u -= alpha q;  w -= alpha z;  gamma_old = gamma
  nhist = its + 1 always; entry k is the norm after k updates.

The reference norm of a nonzero guess follows CG's rules per norm type: the same norm of b
(||N(M^-1 b)||, ||b||, sqrt|b . N(M^-1 b)|; the initial norm if that is 0), the initial norm, or
the smaller (mode default / initial / min).

With Jacobi / no PC the mean of m = D^-1 w is not summed over m: m = D^-1 w + shift with
shift = -((D^-1 sum w) / N), sum w being one of the reduction's sums -- as the library forms it.

From memory, not from the source: (1) PETSc's loop runs `do ... while (i <= max_it)` with the
test inside and so makes one more update before DIVERGED_ITS than this, which ends with
its = max_it updates in x, as every other type of the project does: a deliberate deviation.
(2) PETSc's pipecg calls KSPCheckDot / KSPCheckNorm on its sums; here a non-finite gamma or delta
surfaces through the vectors as -9 at the next test. (3) PETSc's pipecg has no indefinite-PC /
indefinite-matrix test, and neither has this.

sums: how every inner product, norm and mean is summed -- "pairwise" (numpy's), "sequential"
(left to right) or "exact" (math.fsum), as tests/fgmres_restatement.py.
"""
import math

import numpy as np

from oracle import oracle as O
from fgmres_restatement import _SUMS


def pipecg(prob, b, x0=None, rtol=1e-5, atol=1e-50, dtol=1e5, max_it=10000, mode="default",
           norm="preconditioned", nranks=1, sums="pairwise"):
    """(x, reason, its, history, rnorm0); x0 = None: the zero guess."""
    ssum = _SUMS[sums]
    N = prob.N
    dinv = 1.0 / O.diag(prob.h) if prob.pc == "jacobi" else 1.0
    stored = prob.pc not in ("jacobi", "none")

    def pcn(v, sum_v=None):
        if stored:
            z = prob.pc_apply(v, nranks)
            return z + (-((1.0 * ssum(z)) / N)) if prob.nullspace else z
        if not prob.nullspace:
            return dinv * v
        s = ssum(v) if sum_v is None else sum_v
        return dinv * v + (-((dinv * s) / N))

    def five(r, u, w):
        return ssum(r * u), ssum(w * u), ssum(u * u), ssum(r * r), ssum(w)

    def dp_of(S):
        if norm == "preconditioned":
            return math.sqrt(max(S[2], 0.0)) if S[2] == S[2] else float("nan")
        if norm == "unpreconditioned":
            return math.sqrt(max(S[3], 0.0)) if S[3] == S[3] else float("nan")
        if norm == "natural":
            return math.sqrt(abs(S[0]))
        return 0.0

    guess = x0 is not None
    x = x0.copy() if guess else np.zeros_like(b)
    hist, i, reason, rn0, ttol = [], 0, 0, 0.0, 0.0
    with np.errstate(all="ignore"):
        r = b - prob.apply(x, nranks) if guess else b.copy()
        u = pcn(r)
        w = prob.apply(u, nranks)
        z = q = s = p = None
        g_old = a_old = 0.0
        while True:
            S = five(r, u, w)
            gamma, delta = S[0], S[1]
            dp = dp_of(S)
            if i == 0:
                rn0 = dp
                if guess and mode != "initial" and norm != "none":
                    if norm == "unpreconditioned":
                        bn = dp_of(five(b, b, b))
                    else:
                        ub = pcn(b)
                        bn = dp_of(five(b, ub, ub))
                    rn0 = (bn if bn != 0.0 else dp) if mode == "default" else min(bn, dp)
                ttol = max(rtol * rn0, atol)
            hist.append(dp)
            if not math.isfinite(dp):
                reason = -9
            elif norm == "none":
                reason = 4 if i >= max_it else 0
            elif dp <= ttol:
                reason = 3 if dp < atol else 2
            elif (i > 0 or guess) and dp >= dtol * rn0:
                reason = -4
            if not reason and i >= max_it:
                reason = -3
            if reason:
                break
            m = pcn(w, S[4])
            n = prob.apply(m, nranks)
            if i == 0:
                alpha = gamma / delta
                z, q, s, p = n, m, w.copy(), u.copy()
            else:
                beta = gamma / g_old
                alpha = gamma / (delta - (beta / a_old) * gamma)
                z = n + beta * z
                q = m + beta * q
                s = w + beta * s
                p = u + beta * p
            x = x + alpha * p
            r = r - alpha * s
            u = u - alpha * q
            w = w - alpha * z
            g_old, a_old = gamma, alpha
            i += 1
    return x, reason, i, np.asarray(hist), rn0
