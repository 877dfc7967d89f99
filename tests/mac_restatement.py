"""numpy restatement of the MAC-grid gradient, projection and divergence of the 7-point operators
(pb_op_mac_grad / pb_op_mac_project / pb_op_mac_div; DESIGN.md §3.5 "Projection"), built on
varcoef_restatement's face() and _neighbours().

This file is the definition. A face field is three cell-indexed arrays (ux, uy, uz); u_d(c) lives
on the face between cell c and cell c + e_d (the plus face). Arrays are (nz, ny, nx) with x fastest,
every axis periodic. With r_d = 1.0 / h_d (one rounded division), face() the operator's mean and
every product, sum and quotient rounded (numpy evaluates one operation at a time; the library is
built -ffp-contract=off):

    G_d(c) = (r_d * face(beta_(c+e_d), beta_c)) * (p_(c+e_d) - p_c)
    u_d(c) <- u_d(c) - (s * G_d(c))
    D(c)   = s * ((((ux(c) - ux(c-ex)) * r_x) + ((uy(c) - uy(c-ey)) * r_y)) + ((uz(c) - uz(c-ez)) * r_z))

beta = None is PB_OP_STAR7: G_d(c) = r_d * (p_(c+e_d) - p_c), the bits of beta = 1 under either
mean (face(1, 1) = 1 and a multiplication by 1.0 are exact). D G = A to rounding: `ea` and `eu` are
the per-cell magnitudes the tests' rounding bounds are stated in.
"""
import numpy as np

import varcoef_restatement as V

# positions in V._neighbours()'s (z-, y-, x-, x+, y+, z+) of the minus / plus neighbour along x, y, z
_MINUS, _PLUS = (2, 1, 0), (3, 4, 5)


def recips(h):
    """(r_x, r_y, r_z) = 1.0 / h_d"""
    return tuple(1.0 / d for d in h)


def _cells(a, n3):
    return np.asarray(a, dtype=np.float64).reshape(n3[2], n3[1], n3[0])


def grad(p, beta, n3, h, mean=V.ARITHMETIC):
    """(G_x, G_y, G_z) of p, each flat in natural order; beta None: PB_OP_STAR7"""
    pc = _cells(p, n3)
    pn = V._neighbours(pc)
    b = None if beta is None else _cells(beta, n3)
    bn = None if beta is None else V._neighbours(b)
    out = []
    for r, plus in zip(recips(h), _PLUS):
        coef = r if beta is None else r * V.face(bn[plus], b, mean)
        out.append((coef * (pn[plus] - pc)).reshape(-1))
    return tuple(out)


def project(u3, p, s, beta, n3, h, mean=V.ARITHMETIC):
    """u_d - (s * G_d(p)), a new face field"""
    g3 = grad(p, beta, n3, h, mean)
    return tuple(np.asarray(u, dtype=np.float64).reshape(-1) - (s * g) for u, g in zip(u3, g3))


def div(u3, n3, h, s=1.0):
    """s D(u), flat"""
    rx, ry, rz = recips(h)
    ux, uy, uz = (_cells(u, n3) for u in u3)
    d = (ux - V._neighbours(ux)[_MINUS[0]]) * rx
    d = d + (uy - V._neighbours(uy)[_MINUS[1]]) * ry
    d = d + (uz - V._neighbours(uz)[_MINUS[2]]) * rz
    return (s * d).reshape(-1)


# ---------------------------------------------------------------------------------------------
# the magnitudes of the rounding bounds
# ---------------------------------------------------------------------------------------------
def ea(p, beta, n3, h, mean=V.ARITHMETIC):
    """EA_c = sum_n g_n (|p_n| + |p_c|), g_n the operator's six face coefficients"""
    g = V._faces(V.beta_one(n3) if beta is None else beta, n3, h, mean)
    pc = np.abs(_cells(p, n3))
    e = 0.0
    for gn, pn in zip(g, V._neighbours(pc)):
        e = e + gn * (pn + pc)
    return e.reshape(-1)


def eu(u3, p, s, beta, n3, h, mean=V.ARITHMETIC):
    """EU_c = sum_d r_d (m_d(c) + m_d(c - e_d)), m_d = |u_d| + |s G_d(p)|"""
    g3 = grad(p, beta, n3, h, mean)
    e = 0.0
    for r, minus, u, g in zip(recips(h), _MINUS, u3, g3):
        m = _cells(np.abs(u), n3) + _cells(np.abs(s * g), n3)
        e = e + r * (m + V._neighbours(m)[minus])
    return e.reshape(-1)
