"""numpy restatement of the damping of a cell scalar by del6_vt_flux and the divergence of its fluxes, written from the reference's Fortran
(sw_core_nlm.F90: del6_vt_flux, the routine the tangent code restates at sw_core_tlm.F90:3719-3801; its call for w and the divergence
that follows, sw_core_nlm.F90:941-952; copy_corners, tp_core_nlm.F90:214-289) -- not from the oracle and not from the product.
Real-valued: the operator is linear in the damped field, so the tangent plane goes through the same function.

Planes are [pj, pi] with the halo of 3 the product uses: Fortran index i sits at column i + 2 (isd = -2), one spare row / column at the
high end.  F(a) below gives a view indexed by Fortran (i, j)."""
import numpy as np

NG = 3


class F:
    """Fortran-indexed view of a padded plane: x[i, j] with isd = jsd = 1 - NG"""

    def __init__(self, a):
        self.a = a

    def __getitem__(self, ij):
        i, j = ij
        return self.a[j + NG - 1, i + NG - 1]

    def __setitem__(self, ij, v):
        i, j = ij
        self.a[j + NG - 1, i + NG - 1] = v


def copy_corners(q, npx, npy, direction):
    """tp_core_nlm.F90:214-289, all four corners present (a whole face); q: F view, changed in place"""
    ng = NG
    if direction == 1:
        for j in range(1 - ng, 1):
            for i in range(1 - ng, 1):
                q[i, j] = q[j, 1 - i]
        for j in range(1 - ng, 1):
            for i in range(npx, npx + ng):
                q[i, j] = q[npy - j, i - npx + 1]
        for j in range(npy, npy + ng):
            for i in range(npx, npx + ng):
                q[i, j] = q[j, 2 * npx - 1 - i]
        for j in range(npy, npy + ng):
            for i in range(1 - ng, 1):
                q[i, j] = q[npy - j, i - 1 + npx]
    else:
        for j in range(1 - ng, 1):
            for i in range(1 - ng, 1):
                q[i, j] = q[1 - j, i]
        for j in range(1 - ng, 1):
            for i in range(npx, npx + ng):
                q[i, j] = q[npy + j - 1, npx - i]
        for j in range(npy, npy + ng):
            for i in range(npx, npx + ng):
                q[i, j] = q[2 * npy - 1 - j, i]
        for j in range(npy, npy + ng):
            for i in range(1 - ng, 1):
                q[i, j] = q[j + 1 - npx, npy - i]


def del6_vt_flux(nord, nx, ny, damp, q_in, del6_u, del6_v, rarea, face):
    """-> fx2, fy2 (padded planes).  face: the tile is a whole cube face (copy_corners acts); otherwise no cube edge is in the tile"""
    npx, npy = nx + 1, ny + 1
    is_, ie, js, je = 1, nx, 1, ny
    d2a = np.zeros_like(q_in); fxa = np.zeros_like(q_in); fya = np.zeros_like(q_in)
    d2, fx2, fy2, q = F(d2a), F(fxa), F(fya), F(q_in)
    du, dv, ra = F(del6_u), F(del6_v), F(rarea)
    corners = (lambda d: copy_corners(d2, npx, npy, d)) if face else (lambda d: None)
    for j in range(js - 1 - nord, je + 1 + nord + 1):
        for i in range(is_ - 1 - nord, ie + 1 + nord + 1):
            d2[i, j] = damp * q[i, j]
    if nord > 0:
        corners(1)
    for j in range(js - nord, je + nord + 1):
        for i in range(is_ - nord, ie + nord + 2):
            fx2[i, j] = dv[i, j] * (d2[i - 1, j] - d2[i, j])
    if nord > 0:
        corners(2)
    for j in range(js - nord, je + nord + 2):
        for i in range(is_ - nord, ie + nord + 1):
            fy2[i, j] = du[i, j] * (d2[i, j - 1] - d2[i, j])
    for n in range(1, nord + 1):
        nt = nord - n
        for j in range(js - nt - 1, je + nt + 2):
            for i in range(is_ - nt - 1, ie + nt + 2):
                d2[i, j] = (fx2[i, j] - fx2[i + 1, j] + (fy2[i, j] - fy2[i, j + 1])) * ra[i, j]
        corners(1)
        for j in range(js - nt, je + nt + 1):
            for i in range(is_ - nt, ie + nt + 2):
                fx2[i, j] = dv[i, j] * (d2[i, j] - d2[i - 1, j])
        corners(2)
        for j in range(js - nt, je + nt + 2):
            for i in range(is_ - nt, ie + nt + 1):
                fy2[i, j] = du[i, j] * (d2[i, j] - d2[i, j - 1])
    return fxa, fya


def damping_increment(nord, nx, ny, damp, q, del6_u, del6_v, rarea, face):
    """dw of sw_core_nlm.F90:944-947 on is..ie, js..je (zero elsewhere) for one plane q [pj, pi]"""
    fxa, fya = del6_vt_flux(nord, nx, ny, damp, q.copy(), del6_u, del6_v, rarea, face)
    fx2, fy2, ra = F(fxa), F(fya), F(rarea)
    out = np.zeros_like(q); dw = F(out)
    for j in range(1, ny + 1):
        for i in range(1, nx + 1):
            dw[i, j] = ((fx2[i, j] - fx2[i + 1, j]) + (fy2[i, j] - fy2[i, j + 1])) * ra[i, j]
    return out


def dw_levels(nx, ny, levels, da_min_c, w, del6_u, del6_v, rarea, face):
    """levels: [(nord_w, damp_w)] per level; w [npz, pj, pi] -> dw [npz, pj, pi] with damp4 = (damp_w da_min_c)^(nord_w+1), nothing where
    damp_w <= 1e-5 (sw_core_nlm.F90:941-943)"""
    out = np.zeros_like(w)
    for k, (nord_w, damp_w) in enumerate(levels):
        if damp_w > 1.0e-5:
            out[k] = damping_increment(nord_w, nx, ny, (damp_w * da_min_c) ** (nord_w + 1), w[k], del6_u, del6_v, rarea, face)
    return out
