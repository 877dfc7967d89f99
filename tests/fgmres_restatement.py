"""numpy restatement of -ksp_type fgmres on the oracle's building blocks, as
tests/ksp_types_restatement.py restates Richardson (its Problem is reused): the operators and the
preconditioners (O.stencil, O.lapl, O.assembled, O.diag, O.mg_apply, O.fft_pc_apply) and nothing
of the oracle's solver.

PETSc is not available here: this is KSPSolve_FGMRES / KSPFGMRESCycle / KSPFGMRESUpdateHessenberg /
KSPFGMRESBuildSoln (fgmres.c) with classical Gram-Schmidt, right preconditioning, the
unpreconditioned norm, KSPConvergedDefault and the constant null space, written from knowledge of
that file -- "parity unpinned".

  r = b (x = 0) or b - A x0; rn = ||r||, history[0], the default test with its = 0 (reference: rn,
  or with a nonzero guess ||b|| -- rn if that is 0 --, rn, or the smaller: mode default / initial /
  min; the dtol test not at the setup of a zero guess); g_0 = rn, v_0 = (1 / rn) r.
  step k of a cycle (its = i): z_k = N(M^-1 v_k) stored; w = A z_k; h_j = <w, v_j>, j <= k, all of
    w as it came; w = ((w - h_0 v_0) - h_1 v_1) - ...; refine: once more, the second h_j added;
    a non-finite h_j or ||w|| -> -9 with its = i; tt = ||w||; hapbnd = min(haptol, |tt / g_k|);
    happy = not tt > hapbnd; else v_(k+1) = (1 / tt) w; h_(k+1) = tt; the stored rotations on the
    column; c = h_k / d, s = h_(k+1) / d, d = sqrt(h_k^2 + h_(k+1)^2); g_(k+1) = -(s g_k),
    g_k = c g_k, h_k = c h_k + s h_(k+1); res = |g_(k+1)| (happy: 0, no rotation); its = i + 1,
    history[its] = res, the default test; happy and no reason: -5 (7 with the norm type none);
    its = max_it and no reason: -3.
  after `restart` steps without a reason, and at the end from the partial cycle: the back
    substitution, x = x + (((0 + y_0 z_0) + y_1 z_1) + ...); at a restart r = b - A x, rn = ||r||
    tested with the same its (not logged), g_0 = rn, v_0 = (1 / rn) r.
  norm type none: no test but its >= max_it -> 4; the estimates are logged all the same.

From memory, not from the source: (1) what PETSc logs around a restart -- its cycle logs the
recomputed norm of a new cycle's start where this logs the last estimate of the old one; the
project's history contract (entry k = the number tested after k iterations, nhist = its + 1) decides
here. (2) the happy-breakdown bound, hapbnd = min(haptol, |tt / g_k|) with the breakdown taken
when tt is not above it (older sources compare with <, which lets tt = 0 through).

sums: how every inner product, norm and mean is summed -- "pairwise" (numpy's), "sequential"
(left to right) or "exact" (math.fsum: the correctly rounded sum of the rounded products). The
spread between them is the measure of what a different summation order (the GPU's) may move.
"""
import math

import numpy as np

_SUMS = {"pairwise": lambda a: float(np.sum(a)),
         "sequential": lambda a: float(np.cumsum(a)[-1]) if a.size else 0.0,
         "exact": lambda a: math.fsum(a)}


def fgmres(prob, b, x0=None, restart=30, rtol=1e-5, atol=1e-50, dtol=1e5, max_it=10000,
           mode="default", refine=False, haptol=1e-30, norm_none=False, nranks=1,
           sums="pairwise", detail=None):
    """(x, reason, its, history, rnorm0); x0 = None: the zero guess. detail: a dict that receives
    the Hessenberg columns, g and the bases of the last cycle (the CPU tests' least-squares check)."""
    ssum = _SUMS[sums]
    dot = lambda a, c: ssum(a * c)
    nrm = lambda a: math.sqrt(ssum(a * a))

    def pcn(v):
        z = prob.pc_apply(v, nranks)
        return z + (-(ssum(z) / prob.N)) if prob.nullspace else z

    def test(rn, its, dtol_test):
        if not math.isfinite(rn):
            return -9
        if norm_none:
            return 4 if its >= max_it else 0
        if rn <= ttol:
            return 3 if rn < atol else 2
        if dtol_test and rn >= dtol * rn0:
            return -4
        return 0

    guess = x0 is not None
    x = x0.copy() if guess else np.zeros_like(b)
    with np.errstate(all="ignore"):
        r = b - prob.apply(x, nranks) if guess else b.copy()
        rn = nrm(r)
        rn0 = rn
        if guess and mode != "initial":
            bn = nrm(b)
            rn0 = (bn if bn != 0.0 else rn) if mode == "default" else min(bn, rn)
        ttol = max(rtol * rn0, atol)
        hist, its = [rn], 0
        reason = test(rn, 0, guess)
        if not reason and max_it <= 0:
            reason = -3
        V, Z, H, cs, sn, g = [], [], [], [], [], []

        def build():
            m = len(Z)
            y = [0.0] * m
            for k in range(m - 1, -1, -1):
                t = g[k]
                for j in range(k + 1, m):
                    t = t - H[j][k] * y[j]
                y[k] = t / H[k][k] if H[k][k] != 0.0 else 0.0
            t = np.zeros_like(b)
            for j in range(m):
                t = t + y[j] * Z[j]
            return x + t if m else x

        while not reason:
            # a cycle starts from r, rn
            V, Z, H, cs, sn = [(1.0 / rn) * r], [], [], [], []
            g = [rn]
            while not reason and len(Z) < restart:
                k = len(Z)
                Z.append(pcn(V[k]))
                w = prob.apply(Z[k], nranks)
                col = [0.0] * (k + 2)
                for _ in range(2 if refine else 1):
                    h = [dot(w, V[j]) for j in range(k + 1)]
                    for j in range(k + 1):
                        w = w + (-1.0 * h[j]) * V[j]
                        col[j] = col[j] + h[j] if _ else h[j]
                tt = nrm(w)
                if not all(math.isfinite(v) for v in col[:k + 1]) or not math.isfinite(tt):
                    Z.pop()  # the step did not complete: its direction is not live
                    reason = -9
                    break
                hapbnd = min(haptol, abs(tt / g[k])) if g[k] != 0.0 else haptol
                happy = not tt > hapbnd
                if not happy:
                    V.append((1.0 / tt) * w)
                col[k + 1] = tt
                for j in range(k):
                    t = col[j]
                    col[j] = cs[j] * t + sn[j] * col[j + 1]
                    col[j + 1] = cs[j] * col[j + 1] - sn[j] * t
                res = 0.0
                if not happy:
                    d = math.sqrt(col[k] * col[k] + col[k + 1] * col[k + 1])
                    c, s = col[k] / d, col[k + 1] / d
                    cs.append(c)
                    sn.append(s)
                    g.append(-(s * g[k]))
                    g[k] = c * g[k]
                    col[k] = c * col[k] + s * col[k + 1]
                    res = abs(g[k + 1])
                H.append(col)
                its += 1
                hist.append(res)
                reason = test(res, its, True)
                if not reason and happy:
                    reason = 7 if norm_none else -5
                if not reason and its >= max_it:
                    reason = -3
            if detail is not None:
                detail.update(V=list(V), Z=list(Z), H=[list(c) for c in H], g=list(g), x_in=x)
            x = build()
            if reason:
                break
            r = b - prob.apply(x, nranks)
            rn = nrm(r)
            reason = test(rn, its, True)
    return x, reason, its, np.asarray(hist), rn0
