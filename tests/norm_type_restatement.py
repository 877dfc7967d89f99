"""numpy restatement of -ksp_norm_type for cg, single-reduction cg, richardson
and chebyshev, on `Problem` (tests/ksp_types_restatement.py) and the oracle's building blocks only:
the operators and PC applications, nothing of the oracle's solver.

PETSc is not available here: this is KSPSolve_CG / KSPSolve_CG_SingleReduction /
KSPSolve_Richardson / KSPSolve_Chebyshev with KSPSetNormType and KSPConvergedDefault /
KSPConvergedSkip as restated -- "parity unpinned", like the other restatements. What pins it: with
norm_type = "preconditioned" cg() reproduces the oracle's own CG history (its sums run in the
oracle's order: sequential), and richardson() / chebyshev() return what the restatements they wrap
return.

z = N(M^-1 r) always; alpha, beta, p, x, r do not depend on the norm type. Only dp changes:
    preconditioned    ||z||_2                 reference from a nonzero guess ||N(M^-1 b)||
    unpreconditioned  ||r||_2 (no mean shift)                                ||b||_2
    natural           sqrt|r . z|                                            sqrt|b . N(M^-1 b)|
    none              0.0, no test: reason 4 (CONVERGED_ITS) once its >= max_it (max_it = 0: at
                      the setup); the NaN checks on CG's dots and the breakdown exits stay
The test runs before beta's checks, as KSPSolve_CG calls it.
Every solver returns (x, reason, its, history, rnorm0); nhist = len(history).
"""
import numpy as np

import chebyshev_restatement as CR
import ksp_types_restatement as KR
from ksp_types_restatement import Problem, ttol_margin_ok  # noqa: F401  (re-exported)

NORM_TYPES = ("preconditioned", "unpreconditioned", "natural", "none")
NORM_CODES = {"default": -1, "none": 0, "preconditioned": 1, "unpreconditioned": 2, "natural": 3}


def _sum(a):
    return float(np.cumsum(a)[-1])  # sequential, the oracle's vsum


def _dot(a, b):
    return _sum(b * a)              # the oracle's vdot


def _pcn(prob, r, nranks):
    """z = N(M^-1 r) as the oracle's pc_apply_any: z += VecSum(z) / (-N)."""
    z = prob.pc_apply(r, nranks)
    return z + _sum(z) / (-1.0 * prob.N) if prob.nullspace else z


def norm_of(norm_type, r, z):
    """dp of the residual r and z = N(M^-1 r)."""
    if norm_type == "preconditioned":
        return float(np.sqrt(_dot(z, z)))
    if norm_type == "unpreconditioned":
        return float(np.sqrt(_dot(r, r)))
    if norm_type == "natural":
        return float(np.sqrt(abs(_dot(z, r))))
    assert norm_type == "none", norm_type
    return 0.0


def _reference(prob, norm_type, b, dp, guess, mode, nranks):
    """rnorm0 of KSPConvergedDefault: dp from a zero guess; from a nonzero guess the norm of b in
    the same norm type (dp if that is exactly 0), dp (initial), or the smaller (min)."""
    if not guess or mode == "initial" or norm_type == "none":
        return dp
    nb = norm_of(norm_type, b, _pcn(prob, b, nranks) if norm_type != "unpreconditioned" else None)
    return (nb if nb != 0.0 else dp) if mode == "default" else min(nb, dp)


def cg(prob, b, x0=None, norm_type="preconditioned", single_reduction=False, rtol=1e-5,
       atol=1e-50, dtol=1e5, max_it=10000, mode="default", nranks=1):
    """KSPSolve_CG, or KSPSolve_CG_SingleReduction in the GPU pass's arithmetic (the oracle's form
    2: p'w by the recurrence delta - beta^2 dpiold / betaold^2 without KSPCheckDot on it, w = A p
    recomputed). x0 = None: the zero guess."""
    assert norm_type in NORM_TYPES
    skip = norm_type == "none"
    guess = x0 is not None
    x = x0.copy() if guess else np.zeros_like(b)
    hist = []
    with np.errstate(all="ignore"):
        r = b - prob.apply(x, nranks) if guess else b.copy()
        z = _pcn(prob, r, nranks)
        beta = _dot(z, r)
        dp = norm_of(norm_type, r, z)
        rn0 = _reference(prob, norm_type, b, dp, guess, mode, nranks)
        hist.append(dp)
        if not np.isfinite(dp):
            return x, -9, 0, np.asarray(hist), rn0
        ttol = max(rtol * rn0, atol)
        if skip:
            if max_it <= 0:
                return x, 4, 0, np.asarray(hist), rn0
        elif dp <= ttol:
            return x, (3 if dp < atol else 2), 0, np.asarray(hist), rn0
        elif guess and dp >= dtol * rn0:
            return x, -4, 0, np.asarray(hist), rn0
        if not np.isfinite(beta):
            return x, -9, 0, np.asarray(hist), rn0
        if beta != 0.0 and max_it <= 0:
            return x, -3, 0, np.asarray(hist), rn0
        delta = _dot(z, prob.apply(z, nranks)) if single_reduction else 0.0
        i, its, betaold, dpi, reason, p = 0, 0, 0.0, 0.0, 0, None
        while True:
            its = i + 1
            if beta == 0.0:
                reason = 3
                break
            if i > 0 and beta * betaold < 0.0:
                reason = -8
                break
            p = z.copy() if i == 0 else z + (beta / betaold) * p
            dpiold = dpi
            w = prob.apply(p, nranks)
            if single_reduction:
                dpi = delta if i == 0 else delta - beta * beta * dpiold / (betaold * betaold)
            else:
                dpi = _dot(p, w)
                if not np.isfinite(dpi):
                    reason = -9
                    break
            betaold = beta
            if dpi == 0.0 or (i > 0 and np.sign(dpi) * np.sign(dpiold) < 0):
                reason = -10
                break
            a = beta / dpi
            x = x + a * p
            r = r + (-a) * w
            z = _pcn(prob, r, nranks)
            beta = _dot(z, r)
            dp = norm_of(norm_type, r, z)
            hist.append(dp)
            if not np.isfinite(dp):
                reason = -9
                break
            if skip:
                if i + 1 >= max_it:
                    reason = 4
                    break
            elif dp <= ttol:
                reason = 3 if dp < atol else 2
                break
            elif dp >= dtol * rn0:
                reason = -4
                break
            if not np.isfinite(beta):
                reason = -9
                break
            if single_reduction:
                delta = _dot(z, prob.apply(z, nranks))
            i += 1
            if i >= max_it:
                reason = -3
                break
    return x, reason, its, np.asarray(hist), rn0


def _stationary(prob, b, step, norm_type, x0, rtol, atol, dtol, max_it, mode, nranks):
    """Richardson's and Chebyshev's frame (ksp_types_restatement.richardson's) with dp by norm
    type: unpreconditioned is ||b - A x_i||, none tests nothing. step(i, y, ym1, z) -> y_new."""
    skip = norm_type == "none"
    guess = x0 is not None
    y = x0.copy() if guess else np.zeros_like(b)
    ym1 = y
    r = b - prob.apply(y, nranks) if guess else b.copy()
    hist, i, rn0, reason = [], 0, 0.0, 0
    with np.errstate(all="ignore"):
        while True:
            z = prob.remove(prob.pc_apply(r, nranks))
            rn = {"preconditioned": lambda: float(np.sqrt(np.sum(z * z))),
                  "unpreconditioned": lambda: float(np.sqrt(np.sum(r * r))),
                  "none": lambda: 0.0}[norm_type]()
            if i == 0:
                rn0 = rn
                if guess and mode != "initial" and not skip:
                    if norm_type == "unpreconditioned":
                        nb = float(np.sqrt(np.sum(b * b)))
                    else:
                        zb = prob.remove(prob.pc_apply(b, nranks))
                        nb = float(np.sqrt(np.sum(zb * zb)))
                    rn0 = (nb if nb != 0.0 else rn) if mode == "default" else min(nb, rn)
            hist.append(rn)
            if not np.isfinite(rn):
                reason = -9
                break
            ttol = max(rtol * rn0, atol)
            if not skip and rn <= ttol:
                reason = 3 if rn < atol else 2
                break
            if not skip and (i > 0 or guess) and rn >= dtol * rn0:
                reason = -4
                break
            if i >= max_it:
                reason = 4 if skip else -3
                break
            ym1, y = y, step(i, y, ym1, z)
            i += 1
            r = b - prob.apply(y, nranks)
    return y, reason, i, np.asarray(hist), rn0


def richardson(prob, b, x0=None, scale=1.0, norm_type="preconditioned", rtol=1e-5, atol=1e-50,
               dtol=1e5, max_it=10000, mode="default", nranks=1):
    """ksp_types_restatement.richardson with a norm type (natural: PETSc refuses it)."""
    assert norm_type in ("preconditioned", "unpreconditioned", "none")
    if norm_type == "preconditioned":
        return KR.richardson(prob, b, x0=x0, scale=scale, rtol=rtol, atol=atol, dtol=dtol,
                             max_it=max_it, mode=mode, nranks=nranks)
    return _stationary(prob, b, lambda i, y, ym1, z: y + scale * z, norm_type, x0, rtol, atol,
                       dtol, max_it, mode, nranks)


def chebyshev(prob, b, emin, emax, x0=None, norm_type="preconditioned", rtol=1e-5, atol=1e-50,
              dtol=1e5, max_it=10000, mode="default", nranks=1):
    """chebyshev_restatement.chebyshev with a norm type: the same update (scale, mu, omegaprod of
    CR.coefficients; rho_0 = 1 / mu, rho_i = 1 / (2 mu - rho_(i-1)), omega_i = omegaprod rho_i)."""
    assert norm_type in ("preconditioned", "unpreconditioned", "none")
    if norm_type == "preconditioned":
        return CR.chebyshev(prob, b, emin, emax, x0=x0, rtol=rtol, atol=atol, dtol=dtol,
                            max_it=max_it, mode=mode, nranks=nranks)
    scale, mu, omegaprod = CR.coefficients(emin, emax)
    rho = [0.0]

    def step(i, y, ym1, z):
        if i == 0:
            rho[0] = 1.0 / mu
            return y + scale * z
        rho[0] = 1.0 / (2.0 * mu - rho[0])
        omega = omegaprod * rho[0]
        t = y - ym1
        u = scale * z
        t = t + u
        t = omega * t
        return t + ym1

    return _stationary(prob, b, step, norm_type, x0, rtol, atol, dtol, max_it, mode, nranks)
