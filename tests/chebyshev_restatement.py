"""numpy restatement of -ksp_type chebyshev on the oracle's building blocks, as
tests/ksp_types_restatement.py restates Richardson (its Problem is reused).

PETSc is not available here: this is KSPSolve_Chebyshev (PC_LEFT, the preconditioned norm,
KSPConvergedDefault, the constant null space) as restated -- "parity unpinned".

  scale = 2 / (emax + emin), alpha = 1 - scale emin, mu = 1 / alpha, omegaprod = 2 / alpha
  r = b (y = 0) or b - A y0; i = 0, 1, ...: z = N(M^-1 r), rnorm = ||z||, logged as history[i],
  tested with its = i exactly as Richardson's (no dtol test at i = 0 of a zero guess; i = max_it
  -> -3; nhist = its + 1 always); then
    i = 0:  y1 = y0 + scale z                       (Richardson's update, richardson_scale = scale)
    i >= 1: rho_i = 1 / (2 mu - rho_(i-1)), rho_0 = 1 / mu, omega = omegaprod rho_i
            t = y_i - y_(i-1); u = scale z; t = t + u; t = omega t; y_(i+1) = t + y_(i-1)
  every operation rounded. rho_i = c_i / c_(i+1) of PETSc's c_(k+1) = 2 mu c_k - c_(k-1), which
  overflows in long runs; the ratio stays in (0, 1].

The eigenvalue estimate: `steps` steps of preconditioned CG-Lanczos from r_0 = N(v),
v = fill_random(ESTEIG_SEED); the tridiagonal's extremes; emin = a min + b max, emax = c min + d max.
"""
import numpy as np

from oracle import oracle as O

ESTEIG_SEED = 20240607  # PB_CHEBYSHEV_ESTEIG_SEED
TRANSFORM = (0.0, 0.1, 0.0, 1.1)


def coefficients(emin, emax):
    scale = 2.0 / (emax + emin)
    alpha = 1.0 - scale * emin
    return scale, 1.0 / alpha, 2.0 / alpha  # scale, mu, omegaprod


def chebyshev(prob, b, emin, emax, x0=None, rtol=1e-5, atol=1e-50, dtol=1e5, max_it=10000,
              mode="default", nranks=1, trace=None):
    """(x, reason, its, history, rnorm0); x0 = None: the zero guess. mode: the stopping reference
    of a nonzero guess (default ||N(M^-1 b)||, ||z_0|| if that is 0; initial; min). trace: a list
    that receives y_0, y_1, ... (a run without a stopping test holds every shorter run)."""
    scale, mu, omegaprod = coefficients(emin, emax)
    guess = x0 is not None
    y = x0.copy() if guess else np.zeros_like(b)
    ym1 = None
    r = b - prob.apply(y, nranks) if guess else b.copy()
    hist, i, rn0, reason, rho = [], 0, 0.0, 0, 0.0
    with np.errstate(all="ignore"):
        while True:
            if trace is not None:
                trace.append(y)
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
            if i == 0:
                rho = 1.0 / mu
                ynew = y + scale * z
            else:
                rho = 1.0 / (2.0 * mu - rho)
                omega = omegaprod * rho
                t = y - ym1
                u = scale * z
                t = t + u
                t = omega * t
                ynew = t + ym1
            ym1, y = y, ynew
            i += 1
            r = b - prob.apply(y, nranks)
    return y, reason, i, np.asarray(hist), rn0


def petsc_c_recurrence(emin, emax, n):
    """c_k of PETSc's own recurrence after n updates (what the ratio form avoids)."""
    _, mu, _ = coefficients(emin, emax)
    ckm1, ck = 1.0, mu
    with np.errstate(all="ignore"):
        for _ in range(n):
            ckm1, ck = ck, 2.0 * mu * ck - ckm1
    return ck


def lanczos(prob, steps=10, seed=ESTEIG_SEED, dot=None, nranks=1):
    """(min, max, steps taken) of the Lanczos tridiagonal of N M^-1 A. dot: the inner product
    (default numpy's pairwise sums; the tests pass another summation order to measure how far the
    estimate moves)."""
    dot = dot or (lambda a, c: float(np.sum(a * c)))
    r = O.fill_random(prob.N, seed)
    if prob.nullspace:
        r = r - dot(r, np.ones_like(r)) / prob.N
    pcn = lambda v: _remove(prob, prob.pc_apply(v, nranks), dot)
    z = pcn(r)
    p = z.copy()
    rz = rz0 = dot(r, z)
    diag, off = [], []
    alpha_prev = beta_prev = 0.0
    with np.errstate(all="ignore"):
        for j in range(steps):
            w = prob.apply(p, nranks)
            alpha = rz / dot(p, w)
            if not np.isfinite(alpha) or alpha == 0.0:
                break
            diag.append(1.0 / alpha + (beta_prev / alpha_prev if j > 0 else 0.0))
            if len(diag) == steps:
                break
            r = r - alpha * w
            z = pcn(r)
            rz_new = dot(r, z)
            beta = rz_new / rz
            if not np.isfinite(beta) or beta <= 0.0 or abs(rz_new) <= 1e-24 * abs(rz0):
                break
            off.append(np.sqrt(beta) / alpha)
            p = z + beta * p
            alpha_prev, beta_prev, rz = alpha, beta, rz_new
    m = len(diag)
    if m == 0:
        return 0.0, 0.0, 0
    T = np.diag(diag) + np.diag(off[:m - 1], 1) + np.diag(off[:m - 1], -1)
    ev = np.linalg.eigvalsh(T)
    return float(ev[0]), float(ev[-1]), m


def _remove(prob, z, dot):
    return z - dot(z, np.ones_like(z)) / prob.N if prob.nullspace else z


def estimate(prob, steps=10, transform=TRANSFORM, **kw):
    """(emin, emax) as the library forms them from the Lanczos extremes."""
    lo, hi, _ = lanczos(prob, steps, **kw)
    a, b, c, d = transform
    return a * lo + b * hi, c * lo + d * hi


def jacobi_spectrum(prob):
    """(smallest non-zero, largest) eigenvalue of D^-1 A for the 7-point operator: the symbol
    sum_d c_d (1 - cos(2 pi k_d / n_d)) / sum_d c_d with c_d = 1 / h_d^2 (largest = 2 for even
    extents)."""
    c = [1.0 / (h * h) for h in prob.h]
    axes = [cd * (1.0 - np.cos(2 * np.pi * np.arange(n) / n)) for cd, n in zip(c, prob.n3)]
    lam = (axes[0][:, None, None] + axes[1][None, :, None] + axes[2][None, None, :]) / sum(c)
    lam = np.sort(lam.reshape(-1))
    return float(lam[1]), float(lam[-1])
