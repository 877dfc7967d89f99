"""numpy restatement of the -pc_type mg V-cycle with a selectable level smoother,
as the header of pb_mg.hip describes it, one rounded numpy operation per arithmetic step.

  levels        h_l = 2^l h, the 7-point coefficients of lapl_star_coeffs (O.star_coeffs); the
                level count of mg_plan_levels on one rank (plan_levels below)
  operator      per point z-, y-, x-, c, x+, y+, z+ (the reference order)
  restriction   weights 1/8, 3/8, 3/8, 1/8 over the fine cells 2I-1 .. 2I+2: x first, then y and z
                from 0.0
  prolongation  3/4 near, 1/4 far: x, then y, then z; x_f = x_f + (3/4 near + 1/4 far)
  sor           PCSOR form x = (1 - w) x + w ((b - sum_nb c x_nb) (1 / c)), neighbour sum in the
                order z-, y-, x-, x+, y+, z+; red = (i + j + k) even. Pre-smoothing nu x (red,
                black) from zero, post-smoothing nu x (black, red)
  coarsest      coarse_its symmetric sweeps from zero: red, black, red, (black, red) ...
  jacobi-type   y_new = omega ((y - yp) + scale ((1 / c) r)) + yp, r_new = b - A y_new.
                richardson: omega = 1, no yp, scale = the Richardson scale. chebyshev:
                scale = 2 / (emax + emin), alpha = 1 - scale emin, mu = 1 / alpha,
                omegaprod = 2 / alpha; step 0 is Richardson's; step i >= 1 has rho_i =
                1 / (2 mu - rho_(i-1)), rho_0 = 1 / mu, omega = omegaprod rho_i; restarted at
                every smoothing call. Pre-smoothing starts from zero (r_0 = b); post-smoothing
                from the corrected iterate and its residual.
Arrays are flat in natural order, [k][j][i] when shaped.
"""
import numpy as np

from oracle import oracle as O

ESTEIG = (0.0, 0.1, 0.0, 1.1)
W4 = (0.125, 0.375, 0.375, 0.125)


def plan_levels(n, levels_req=0):
    """mg_plan_levels on one rank"""
    cur, L = list(n), 1
    cap = levels_req if levels_req > 0 else 64
    while L < cap:
        ok = all(c % 4 == 0 for c in cur)
        if levels_req <= 0:
            ok = ok and min(cur) > 4
        if not ok:
            break
        cur = [c // 2 for c in cur]
        L += 1
    return L


def bounds(eigenvalues=(0.0, 0.0), esteig=ESTEIG):
    """The level smoother's Chebyshev interval: the caller's, or the transform of (0, 2)."""
    if eigenvalues[0] != 0.0 or eigenvalues[1] != 0.0:
        return float(eigenvalues[0]), float(eigenvalues[1])
    a, b, c, d = esteig
    return a * 0.0 + b * 2.0, c * 0.0 + d * 2.0


class Smoother:
    def __init__(self, ksp="richardson", pc="sor", nu=1, scale=1.0, eigenvalues=(0.0, 0.0),
                 esteig=ESTEIG):
        assert (ksp, pc) in (("richardson", "sor"), ("richardson", "jacobi"),
                             ("chebyshev", "jacobi"))
        self.ksp, self.pc, self.nu, self.scale = ksp, pc, int(nu), float(scale)
        self.emin, self.emax = bounds(eigenvalues, esteig)

    def argv(self):
        a = ["-mg_levels_ksp_type", self.ksp, "-mg_levels_pc_type", self.pc,
             "-mg_levels_ksp_max_it", str(self.nu)]
        if self.scale != 1.0:
            a += ["-mg_levels_ksp_richardson_scale", repr(self.scale)]
        return a

    def __repr__(self):
        return f"{self.ksp}-{self.pc}-nu{self.nu}" + (f"-s{self.scale:.4g}" if self.scale != 1 else "")


class Level:
    def __init__(self, n, h):
        self.n = tuple(int(v) for v in n)
        self.shape = (self.n[2], self.n[1], self.n[0])
        c = O.star_coeffs(h)
        self.cx, self.cy, self.cz, self.cc = float(c[12]), float(c[10]), float(c[4]), float(c[13])
        k, j, i = np.indices(self.shape)
        self.red = ((i + j + k) % 2) == 0

    def apply(self, x):
        s = self.cz * np.roll(x, 1, 0)
        s = s + self.cy * np.roll(x, 1, 1)
        s = s + self.cx * np.roll(x, 1, 2)
        s = s + self.cc * x
        s = s + self.cx * np.roll(x, -1, 2)
        s = s + self.cy * np.roll(x, -1, 1)
        s = s + self.cz * np.roll(x, -1, 0)
        return s

    def half_sweep(self, x, b, omega, color):
        nb = self.cz * np.roll(x, 1, 0)
        nb = nb + self.cy * np.roll(x, 1, 1)
        nb = nb + self.cx * np.roll(x, 1, 2)
        nb = nb + self.cx * np.roll(x, -1, 2)
        nb = nb + self.cy * np.roll(x, -1, 1)
        nb = nb + self.cz * np.roll(x, -1, 0)
        t = (b - nb) * (1.0 / self.cc)
        xn = (1.0 - omega) * x + omega * t
        return np.where(self.red if color == 0 else ~self.red, xn, x)


def restrict(r):
    def along(a, axis, first):
        n = a.shape[axis]
        ev = [slice(None)] * 3
        od = [slice(None)] * 3
        ev[axis] = slice(0, n, 2)
        od[axis] = slice(1, n, 2)
        ev, od = tuple(ev), tuple(od)
        v = (np.roll(a, 1, axis)[ev], a[ev], a[od], np.roll(a, -2, axis)[ev])
        if first:  # sx = w0 v0; sx = sx + w1 v1; ...
            s = W4[0] * v[0]
            for w, q in zip(W4[1:], v[1:]):
                s = s + w * q
        else:      # sy = 0.0; sy = sy + w sx; ...
            s = np.zeros_like(v[0])
            for w, q in zip(W4, v):
                s = s + w * q
        return s
    return along(along(along(r, 2, True), 1, False), 0, False)


def prolong_add(xf, xc):
    """xf + P xc"""
    def along(c, axis):
        n = c.shape[axis]
        shp = list(c.shape)
        shp[axis] = 2 * n
        f = np.empty(shp)
        ev = [slice(None)] * 3
        od = [slice(None)] * 3
        ev[axis] = slice(0, 2 * n, 2)
        od[axis] = slice(1, 2 * n, 2)
        f[tuple(ev)] = 0.75 * c + 0.25 * np.roll(c, 1, axis)
        f[tuple(od)] = 0.75 * c + 0.25 * np.roll(c, -1, axis)
        return f
    return xf + along(along(along(xc, 2), 1), 0)


def cheb_coefficients(emin, emax):
    scale = 2.0 / (emax + emin)
    alpha = 1.0 - scale * emin
    return scale, 1.0 / alpha, 2.0 / alpha  # scale, mu, omegaprod


def poly_smooth(lv, sm, b, y0):
    """nu steps from y0 (None: zero). Returns (y, r = b - A y)."""
    dinv = 1.0 / lv.cc
    cheb = sm.ksp == "chebyshev"
    scale, mu, omegaprod = cheb_coefficients(sm.emin, sm.emax) if cheb else (sm.scale, 0.0, 0.0)
    rho = 1.0 / mu if cheb else 0.0
    zero = y0 is None
    y = np.zeros_like(b) if zero else y0
    r = b if zero else b - lv.apply(y)
    yp = None
    for i in range(sm.nu):
        z = dinv * r
        u = scale * z
        if not cheb or i == 0:
            yn = 1.0 * (y + u)
        else:
            rho = 1.0 / (2.0 * mu - rho)
            omega = omegaprod * rho
            t = y - yp
            t = t + u
            t = omega * t
            yn = t + yp
        yp, y = y, yn
        r = b - lv.apply(y)
    return y, r


class VCycle:
    """z = M^-1 r of -pc_type mg on one rank."""

    def __init__(self, n, h, smoother=None, levels=0, coarse_its=8, omega=1.0):
        self.n, self.h = tuple(n), tuple(h)
        self.sm = smoother or Smoother()
        self.coarse_its, self.omega = max(1, int(coarse_its)), float(omega)
        self.L = plan_levels(self.n, levels)
        self.lv = [Level([v >> l for v in self.n], [d * float(1 << l) for d in self.h])
                   for l in range(self.L)]

    def _pre(self, lv, b):
        sm, w = self.sm, self.omega
        if sm.pc == "jacobi":
            return poly_smooth(lv, sm, b, None)
        x = np.zeros_like(b)
        for _ in range(sm.nu):
            x = lv.half_sweep(x, b, w, 0)
            x = lv.half_sweep(x, b, w, 1)
        return x, b - lv.apply(x)

    def _post(self, lv, b, x):
        sm, w = self.sm, self.omega
        if sm.pc == "jacobi":
            return poly_smooth(lv, sm, b, x)[0]
        for _ in range(sm.nu):
            x = lv.half_sweep(x, b, w, 1)
            x = lv.half_sweep(x, b, w, 0)
        return x

    def _coarsest(self, lv, b):
        w = self.omega
        x = np.zeros_like(b)
        x = lv.half_sweep(x, b, w, 0)
        x = lv.half_sweep(x, b, w, 1)
        x = lv.half_sweep(x, b, w, 0)
        for _ in range(1, self.coarse_its):
            x = lv.half_sweep(x, b, w, 1)
            x = lv.half_sweep(x, b, w, 0)
        return x

    def _cycle(self, l, b):
        lv = self.lv[l]
        if l == self.L - 1:
            return self._coarsest(lv, b)
        x, res = self._pre(lv, b)
        xc = self._cycle(l + 1, restrict(res))
        return self._post(lv, b, prolong_add(x, xc))

    def apply(self, r):
        with np.errstate(all="ignore"):
            return self._cycle(0, np.asarray(r, dtype=np.float64).reshape(self.lv[0].shape)
                               ).reshape(-1)


class MgProblem:
    """tests/ksp_types_restatement.Problem with the restated V-cycle as the PC (7-point A)."""

    def __init__(self, n3, h, smoother=None, coarse_its=8, omega=1.0, nullspace=1):
        self.n3, self.h, self.nullspace = tuple(n3), tuple(h), nullspace
        self.N = int(np.prod(n3))
        self.pc, self.op, self.L = "mg", "star7", (1.0, 1.0, 1.0)
        self.vc = VCycle(n3, h, smoother, coarse_its=coarse_its, omega=omega)

    def mats(self, pb, da):
        return pb.Mat(da, pb.ASSEMBLED27, self.h), pb.Mat(da, pb.STAR7, self.h)

    def apply(self, x, nranks=1):
        return O.stencil(x, self.n3, self.h)

    def rhs(self, seed=20231015, nranks=1):
        return self.apply(O.fill_random(self.N, seed))

    def pc_apply(self, r, nranks=1):
        return self.vc.apply(r)

    def remove(self, z):
        return z - z.mean() if self.nullspace else z


def cg(prob, b, rtol=1e-5, atol=1e-50, dtol=1e5, max_it=10000):
    """oracle.cg_solve's sequence (KSPSolve_CG, preconditioned norm) with prob's PC.
    Returns (x, reason, its, history)."""
    x = np.zeros_like(b)
    r = b.copy()
    with np.errstate(all="ignore"):
        z = prob.remove(prob.pc_apply(r))
        dp = float(np.sqrt(np.sum(z * z)))
        hist = [dp]
        if not np.isfinite(dp):
            return x, -9, 0, np.asarray(hist)
        ttol = max(rtol * dp, atol)
        rn0 = dp
        if dp <= ttol:
            return x, (3 if dp < atol else 2), 0, np.asarray(hist)
        beta = float(np.sum(z * r))
        if not np.isfinite(beta):
            return x, -9, 0, np.asarray(hist)
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
            w = prob.apply(p)
            dpi = float(np.sum(p * w))
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
            z = prob.remove(prob.pc_apply(r))
            dp = float(np.sqrt(np.sum(z * z)))
            hist.append(dp)
            if not np.isfinite(dp):
                reason = -9
                break
            if dp <= ttol:
                reason = 3 if dp < atol else 2
                break
            if dp >= dtol * rn0:
                reason = -4
                break
            beta = float(np.sum(z * r))
            if not np.isfinite(beta):
                reason = -9
                break
            i += 1
            if i >= max_it:
                reason = -3
                break
    return x, reason, its, np.asarray(hist)
