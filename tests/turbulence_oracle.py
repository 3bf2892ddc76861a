"""numpy restatement of the linearised boundary-layer turbulence (reference physics/turbulence/fv3jedi_lm_turbulence_mod.F90 and
turbulence/blsimp.F90), written from their description; line numbers are cited, nothing is copied.  Arrays are COMPACT with the level
axis third from the end, [..., lm, ny, nx]; every function is vectorised over the other axes (a sweep is lm array operations).

  pressures      compute_pressures, utils/fv3jedi_lm_utils_mod.F90:359-391
  vtrilupert     :583-601       LU factors: a the multipliers, b the inverse pivots
  vtrisolvepert  :605-674       phase 1 (tangent) / 2 (adjoint), ygswitch 1 / 0
  turbulence     step_nl / step_tl :218-282, step_ad :286-350: T <-> theta around the seven solves
  bl_simp        blsimp.F90:72-133
  diffusion_systems  generator of diffusion-shaped, diagonally dominant systems of chosen strength (the tests' diagonals (ii))"""
import numpy as np

P00 = 1.0e5
NL, TL, AD = 0, 1, 2


def _l(x, l):
    """level l (1-based) of x"""
    return x[..., l - 1, :, :]


def pressures(delp, ptop, kappa):
    """-> pe [..., lm+1, ny, nx] (pe[0] = ptop, pe(l) = pe(l-1) + delp(l) in double), pk [..., lm, ny, nx].
    pk is the reference's quotient of two differences, evaluated in extended precision and rounded once: in double the quotient
    itself loses 1 / (kappa ln(pe(l) / pe(l-1))) -- 270 at L127 -- of the precision of log and pow, and BL_simp, which differences pk
    and theta = T / pk of neighbouring layers again, amplifies that another ~1e3 times; the restatement must not carry an error of
    its own of the size of the tolerances it is used with."""
    top = np.full_like(delp[..., :1, :, :], ptop)
    pe = np.cumsum(np.concatenate([top, delp], axis=-3), axis=-3)
    pel = pe.astype(np.longdouble); kl = np.longdouble(kappa)
    lpe = np.log(pel); pek = pel ** kl
    pk = (pek[..., 1:, :, :] - pek[..., :-1, :, :]) / (kl * (lpe[..., 1:, :, :] - lpe[..., :-1, :, :]))
    return pe, pk.astype(np.float64)


def vtrilupert(a, b, c):
    a, b = a.copy(), b.copy()
    lm = a.shape[-3]
    _l(b, 1)[...] = 1.0 / _l(b, 1)
    for l in range(2, lm + 1):
        _l(a, l)[...] = _l(a, l) * _l(b, l - 1)
        _l(b, l)[...] = 1.0 / (_l(b, l) - _l(c, l - 1) * _l(a, l))
    return a, b


def vtrisolvepert(a, b, c, y, phase, ygswitch):
    """a, b the LU factors of vtrilupert, c the upper diagonal; -> the new y"""
    y = y.copy()
    lm = y.shape[-3]
    if phase == 1:
        for l in range(2, lm + 1):                                    # sweep down with the multipliers
            _l(y, l)[...] = _l(y, l) - _l(a, l) * _l(y, l - 1)
        if ygswitch == 1:
            _l(y, lm)[...] = _l(y, lm) * _l(b, lm)
        else:
            _l(y, lm)[...] = _l(y, lm) * _l(b, lm - 1) / (_l(b, lm - 1) - _l(a, lm) * (1.0 + _l(c, lm - 1) * _l(b, lm - 1)))
        for l in range(lm - 1, 0, -1):                                # sweep up; b holds the inverse of the main diagonal
            _l(y, l)[...] = _l(b, l) * (_l(y, l) - _l(c, l) * _l(y, l + 1))
        return y
    assert phase == 2
    if ygswitch == 1:
        _l(y, 1)[...] = _l(y, 1) * _l(b, 1)                           # U' down
        for l in range(2, lm + 1):
            _l(y, l)[...] = _l(b, l) * (_l(y, l) - _l(c, l - 1) * _l(y, l - 1))
        for l in range(lm - 1, 0, -1):                                # L' up
            _l(y, l)[...] = _l(y, l) - _l(a, l + 1) * _l(y, l + 1)
        return y
    for l in range(1, lm):                                            # line-by-line adjoint of the sweep up
        _l(y, l + 1)[...] = _l(y, l + 1) - _l(c, l) * _l(b, l) * _l(y, l)
        _l(y, l)[...] = _l(b, l) * _l(y, l)
    _l(y, lm)[...] = _l(b, lm - 1) * _l(y, lm) / (_l(b, lm - 1) - _l(a, lm) * (_l(c, lm - 1) * _l(b, lm - 1) + 1.0))
    for l in range(lm, 1, -1):                                        # adjoint of the sweep down
        _l(y, l - 1)[...] = _l(y, l - 1) - _l(a, l) * _l(y, l)
    return y


def factorise(diag):
    """diag = AKV BKV CKV AKS BKS CKS AKQ BKQ CKQ -> the nine arrays after vtrilupert"""
    out = []
    for s in range(3):
        a, b = vtrilupert(diag[3 * s], diag[3 * s + 1], diag[3 * s + 2])
        out += [a, b, np.array(diag[3 * s + 2], dtype=np.float64)]
    return out


def turbulence(mode, fac, pk, kappa, fields):
    """fields: dict u v pt q1 .. (compact); fac the nine factor arrays; -> dict of the new fields.  NL and TL are the same operator
    (on the trajectory / the perturbation), AD its adjoint."""
    phase = 2 if mode == AD else 1
    p00k = P00 ** kappa
    out = {}
    V, S, Q = fac[0:3], fac[3:6], fac[6:9]
    out["u"] = vtrisolvepert(*V, fields["u"], phase, 1)
    out["v"] = vtrisolvepert(*V, fields["v"], phase, 1)
    if phase == 1:
        th = p00k * fields["pt"] / pk
        out["pt"] = pk * vtrisolvepert(*S, th, 1, 1) / p00k
    else:
        th = pk * fields["pt"] / p00k
        out["pt"] = p00k * vtrisolvepert(*S, th, 2, 1) / pk
    n = 1
    while "q%d" % n in fields:
        out["q%d" % n] = vtrisolvepert(*Q, fields["q%d" % n], phase, 1 if n == 1 else 0)
        n += 1
    return out


def bl_simp(dt, u, v, ptt, qv, ql, qi, pe, pk, frocean, grav, vireps, kappa, cp, rgas):
    """-> (nine diagonals AKV BKV CKV AKS BKS CKS AKQ BKQ CKQ, dict of intermediates RI, KH on the interfaces L = 2..lm).
    pe [..., lm+1, ny, nx] with pe[0] the top; frocean [..., ny, nx]."""
    lm = u.shape[-3]
    pel = lambda l: pe[..., l, :, :]                                   # PET(0:LM)
    aks, bks, cks = np.zeros_like(u), np.zeros_like(u), np.zeros_like(u)
    ri_all, kh_all = np.zeros_like(u[..., 1:, :, :]), np.zeros_like(u[..., 1:, :, :])
    dmi = (grav * dt) / (pel(1) - pel(0))
    tvt = _l(ptt, 1) * _l(pk, 1) * (1.0 + vireps * _l(qv, 1) - _l(ql, 1) - _l(qi, 1))
    for L in range(2, lm + 1):
        pkh = pel(L) ** kappa
        dz = cp * (_l(ptt, L - 1) * (pkh - _l(pk, L - 1)) + _l(ptt, L) * (_l(pk, L) - pkh))
        ws = (_l(u, L - 1) - _l(u, L)) ** 2 + (_l(v, L - 1) - _l(v, L)) ** 2 + 0.01
        ri = grav * ((_l(ptt, L - 1) - _l(ptt, L)) / (0.5 * (_l(ptt, L - 1) + _l(ptt, L)))) * dz / ws
        rin = 30.0 * 30.0 * np.sqrt(ws) / dz
        unstable = np.maximum(0.01, rin * np.sqrt(np.maximum(1.0 - 18.0 * ri, 0.0)))
        stable = np.maximum(0.01, rin / (1.0 + 10.0 * ri * (1.0 + 8.0 * ri)))
        kh = np.where(ri < 0.0, unstable, stable)
        ri_all[..., L - 2, :, :] = ri; kh_all[..., L - 2, :, :] = kh
        tvb = _l(ptt, L) * _l(pk, L) * (1.0 + vireps * _l(qv, L) - _l(ql, L) - _l(qi, L))
        tve = 0.5 * (tvt + tvb)
        tvt = tvb
        ckx = -kh * pel(L) / (rgas * tve) / dz
        _l(cks, L - 1)[...] = ckx * dmi
        dmi = (grav * dt) / (pel(L) - pel(L - 1))
        _l(aks, L)[...] = ckx * dmi
        _l(bks, L - 1)[...] = 1.0 - (_l(aks, L - 1) + _l(cks, L - 1))
        if L == lm:
            _l(bks, L)[...] = 1.0 - (_l(aks, L) + _l(cks, L))
            bksq = _l(bks, L).copy()
            wsf = np.sqrt(_l(u, L) ** 2 + _l(v, L) ** 2 + 1.0)
            sea = frocean == 1.0
            cdrag = np.where(sea, 0.0015, 0.002); tcoef = np.where(sea, 1.0, 0.0)
            khs = -cdrag * dmi * wsf * pel(L) / (rgas * tvb)
            bksv = 1.0 - (_l(aks, L) + _l(cks, L) + khs)
            bkst = 1.0 - (_l(aks, L) + _l(cks, L) + khs * tcoef)
    akv, bkv, ckv = aks.copy(), bks.copy(), cks.copy()
    akq, bkq, ckq = aks.copy(), bks.copy(), cks.copy()
    _l(bkv, lm)[...] = bksv; _l(bks, lm)[...] = bkst; _l(bkq, lm)[...] = bksq
    return [akv, bkv, ckv, aks, bks, cks, akq, bkq, ckq], dict(ri=ri_all, kh=kh_all)


def bl_simp_of_state(opt, dt, T, frocean, real=np.longdouble):
    """BL_simp on a compact trajectory T (dict u v pt delp q1 q2 q3; pt = temperature) with the JEDI constants of the options, read as
    the product reads the routine: PTT = T / pk, PKT = pk.  Evaluated in `real` and rounded to double at the end: the routine
    differences pk and theta of neighbouring layers (DZ, RI), which in double costs ~1e3 of the precision (see pressures); in
    extended precision the restatement's own rounding stays far below the 1e-12 it is compared at."""
    R = lambda x: np.asarray(x, dtype=real)
    pe, _ = pressures(T["delp"], opt.ptop, opt.akap)
    pel = R(pe); kl = real(opt.akap)
    lpe = np.log(pel); pek = pel ** kl
    pk = (pek[..., 1:, :, :] - pek[..., :-1, :, :]) / (kl * (lpe[..., 1:, :, :] - lpe[..., :-1, :, :]))
    diag, mid = bl_simp(real(dt), R(T["u"]), R(T["v"]), R(T["pt"]) / pk, R(T["q1"]), R(T["q2"]), R(T["q3"]), pel, pk, frocean,
                        real(opt.grav_jedi), real(opt.zvir), kl, real(opt.cp), real(opt.cp) * kl)
    return [d.astype(np.float64) for d in diag], {k: v.astype(np.float64) for k, v in mid.items()}, pk.astype(np.float64)


def diffusion_systems(rng, shape, strength):
    """Nine diagonals of three diffusion-shaped, diagonally dominant systems on `shape` = [..., lm, ny, nx]:
    a(l) = -kap_l g_l, c(l-1) = -kap_l g_(l-1) for the interfaces l = 2..lm (kap > 0 the exchange coefficient of the interface, g > 0
    the inverse mass of the layer), b = 1 - (a + c), plus a non-negative surface term in b(lm) that differs between V, S and Q.
    `strength` scales kap: max|a| grows with it."""
    lm = shape[-3]
    g = 0.5 + rng.random(shape)
    base = strength * np.exp(rng.normal(0.0, 0.7, shape))              # interface l sits at index l - 1; index 0 unused
    out = []
    for s, (fac, surf) in enumerate(((1.0, 0.9), (0.8, 0.4), (1.2, 0.0))):
        kap = fac * base
        a, c = np.zeros(shape), np.zeros(shape)
        a[..., 1:, :, :] = -kap[..., 1:, :, :] * g[..., 1:, :, :]
        c[..., :-1, :, :] = -kap[..., 1:, :, :] * g[..., :-1, :, :]
        b = 1.0 - (a + c)
        b[..., lm - 1, :, :] += surf * rng.random(shape[:-3] + shape[-2:])
        out += [a, b, c]
    return out


def tridiagonal_matrix(a, b, c):
    """dense [lm, lm] matrix of one column's lower / main / upper diagonals (1-D arrays)"""
    return np.diag(b) + np.diag(a[1:], -1) + np.diag(c[:-1], 1)
