"""Second restatement of the non-hydrostatic column operators, in numpy, written from the reference's NONLINEAR files
(model/nh_utils_nlm.F90, model/nh_core_nlm.F90, model/dyn_core_nlm.F90) and from nothing in csrc/ or oracle/.  Columns are vectorised
(axis 0), levels are looped (axis 1, level k of the reference = index k-1).  Every routine is generic in the dtype of its inputs:
float64, longdouble and clongdouble all work, and the derivatives are complex steps of size 1e-30 in clongdouble -- the two switches
(max in the dz_min fix, max in the p_fac floor) compare real parts, so the step follows the branch the values take.
    dz_fix          tails of UPDATE_DZ_C / UPDATE_DZ_D: surface velocity, dz_min fix    nh_utils_nlm.F90:167-178, :282-293
    sim1_solver     SIM1_SOLVER                                                         nh_utils_nlm.F90:1177-1308
    sim_solver      SIM_SOLVER                                                          nh_utils_nlm.F90:1310-1466
    riem_solver_c   RIEM_SOLVER_C (a_imp > 0.5: SIM1_SOLVER)                            nh_utils_nlm.F90:297-404
    riem_solver3    RIEM_SOLVER3 with its dispatch and the last_call outputs            nh_core_nlm.F90:40-204
    edge_profile    EDGE_PROFILE, non-uniform levels, limiter = 0                       nh_utils_nlm.F90:1519-1625 (called :227-233)
    pk3_halo / pe_halo   one column of PK3_HALO / PE_HALO                               dyn_core_nlm.F90:1129-1181, :1232-1260
    zh_init         interface heights from delz at the first acoustic step              dyn_core_nlm.F90:328-352
    dp_ref          reference thicknesses handed to EDGE_PROFILE                        dyn_core_nlm.F90:216-219
Not preprocessed in: USE_COND, MOIST_CAPPA (the linearised model is built without them)."""
import numpy as np

DZ_MIN = 2.0           # nh_utils_nlm.F90: real, parameter:: dz_min = 2.
H = 1e-30              # complex step
LD, CLD = np.longdouble, np.clongdouble


def _re(x):
    return x.real if np.iscomplexobj(x) else x


def _max(a, b):
    """Fortran max on the values: returns (max, took_a)"""
    a, b = np.broadcast_arrays(a, b)
    ta = _re(a) >= _re(b)
    return np.where(ta, a, b), ta


class Consts:
    def __init__(self, dt, akap, ptop, rdgas, grav, a_imp, p_fac, scale_m):
        self.dt, self.akap, self.ptop, self.rdgas, self.grav = dt, akap, ptop, rdgas, grav
        self.a_imp, self.p_fac, self.scale_m = a_imp, p_fac, scale_m


def dp_ref(ak, bk):
    ak, bk = np.asarray(ak, dtype=LD), np.asarray(bk, dtype=LD)
    return (ak[1:] - ak[:-1]) + (bk[1:] - bk[:-1]) * LD(1.0e5)


def zh_init(delz, zs):
    km = delz.shape[1]
    zh = [None] * (km + 1)
    zh[km] = zs + 0 * delz[:, 0]
    for k in range(km - 1, -1, -1):
        zh[k] = zh[k + 1] - delz[:, k]
    return np.stack(zh, axis=1)


def dz_fix(zh, zs, dt, info=None):
    """ws = (zs - zh(km+1)) / dt;  zh(k) = max(zh(k), zh(k+1) + dz_min), k = km .. 1"""
    km = zh.shape[1] - 1
    ws = (zs - zh[:, km]) * (1.0 / dt)
    z = [None] * (km + 1)
    z[km] = zh[:, km]
    lifted = np.zeros((zh.shape[0], km), dtype=bool)
    margin = np.zeros((zh.shape[0], km))
    for k in range(km - 1, -1, -1):
        lim = z[k + 1] + DZ_MIN
        z[k], kept = _max(zh[:, k], lim)
        lifted[:, k] = ~kept
        margin[:, k] = np.abs(_re(zh[:, k]) - _re(lim))
    if info is not None:
        info["lifted"], info["lift_margin"] = lifted, margin
    return ws, np.stack(z, axis=1)


def _pp_edges(pe, dm2, km):
    """shared head of SIM1 / SIM (:1212-1240, :1349-1377): g_rat, bb and the interface perturbation pp(1..km+1)"""
    n = pe.shape[0]
    g_rat, bb, dd = [None] * km, [None] * km, [None] * km
    for k in range(km - 1):
        g_rat[k] = dm2[:, k] / dm2[:, k + 1]
        bb[k] = 2.0 * (1.0 + g_rat[k])
        dd[k] = 3.0 * (pe[:, k] + g_rat[k] * pe[:, k + 1])
    bet = bb[0] if km > 1 else None
    pp = [None] * (km + 1)
    gam = [None] * km
    pp[0] = 0 * pe[:, 0]
    pivots = []
    if km > 1:
        pp[1] = dd[0] / bet
        pivots.append(bet)
    bb[km - 1] = 2.0 + 0 * pe[:, 0]
    dd[km - 1] = 3.0 * pe[:, km - 1]
    if km == 1:         # not reached by the library (km >= 2), kept total
        pp[1] = dd[0] / bb[0]
    for k in range(1, km):
        gam[k] = g_rat[k - 1] / bet
        bet = bb[k] - gam[k]
        pivots.append(bet)
        pp[k + 1] = (dd[k] - pp[k]) / bet
    for k in range(km - 1, 0, -1):
        pp[k] = pp[k] - gam[k] * pp[k + 1]
    return g_rat, bb, pp, pivots


def _new_dz(C, pe, g_rat, bb, dm2, pm2, pt2, km, info):
    """tail of SIM1 / SIM (:1288-1306, :1439-1458): dz2 = -dm R pt exp(capa1 log(max(p_fac pm, p1 + pm)))"""
    capa1 = C.akap - 1.0
    r3 = 1.0 / (3.0 + 0 * _re(pe[0]))
    n = pe[0].shape[0]
    dz = [None] * km
    floored = np.zeros((n, km), dtype=bool)
    margin = np.zeros((n, km))
    p1 = (pe[km - 1] + 2.0 * pe[km]) * r3
    for k in range(km - 1, -1, -1):
        if k < km - 1:
            p1 = (pe[k] + bb[k] * pe[k + 1] + g_rat[k] * pe[k + 2]) * r3 - g_rat[k] * p1
        lo, hi = C.p_fac * pm2[:, k], p1 + pm2[:, k]
        mx, took_lo = _max(lo, hi)
        floored[:, k] = took_lo
        margin[:, k] = np.abs(_re(hi) - _re(lo)) / np.abs(_re(pm2[:, k]))
        dz[k] = -dm2[:, k] * C.rdgas * pt2[:, k] * np.exp(capa1 * np.log(mx))
    if info is not None:
        info["floored"], info["floor_margin"] = floored, margin
    return dz


def sim1_solver(C, dt, dm2, pm2, pem, w2, dz2, pt2, ws, info=None):
    km = dm2.shape[1]
    gama = 1.0 / (1.0 - C.akap)
    t1g, rdt = gama * 2.0 * dt * dt, 1.0 / dt
    w1 = w2
    pe = np.exp(gama * np.log(-dm2 / dz2 * C.rdgas * pt2)) - pm2
    g_rat, bb, pp, piv = _pp_edges(pe, dm2, km)
    aa = [None] * (km + 1)
    for k in range(1, km):
        aa[k] = t1g / (dz2[:, k - 1] + dz2[:, k]) * (pem[:, k] + pp[k])
    w = [None] * km
    gam = [None] * km
    bet = dm2[:, 0] - aa[1]
    piv.append(bet)
    w[0] = (dm2[:, 0] * w1[:, 0] + dt * pp[1]) / bet
    for k in range(1, km - 1):
        gam[k] = aa[k] / bet
        bet = dm2[:, k] - (aa[k] + aa[k + 1] + aa[k] * gam[k])
        piv.append(bet)
        w[k] = (dm2[:, k] * w1[:, k] + dt * (pp[k + 1] - pp[k]) - aa[k] * w[k - 1]) / bet
    k = km - 1
    p1 = t1g / dz2[:, k] * (pem[:, km] + pp[km])
    gam[k] = aa[k] / bet
    bet = dm2[:, k] - (aa[k] + p1 + aa[k] * gam[k])
    piv.append(bet)
    w[k] = (dm2[:, k] * w1[:, k] + dt * (pp[km] - pp[k]) - p1 * ws - aa[k] * w[k - 1]) / bet
    for k in range(km - 2, -1, -1):
        w[k] = w[k] - gam[k + 1] * w[k + 1]
    pe2 = [None] * (km + 1)
    pe2[0] = 0 * w[0]
    for k in range(km):
        pe2[k + 1] = pe2[k] + dm2[:, k] * (w[k] - w1[:, k]) * rdt
    dz = _new_dz(C, pe2, g_rat, bb, dm2, pm2, pt2, km, info)
    if info is not None:
        info["min_pivot"] = np.min(np.stack([_re(p) for p in piv], axis=1), axis=1)
    return np.stack(pe2, axis=1), np.stack(w, axis=1), np.stack(dz, axis=1)


def sim_solver(C, dt, dm2, pm2, pem, w2, dz2, pt2, ws, alpha, scale_m, info=None):
    km = dm2.shape[1]
    gama = 1.0 / (1.0 - C.akap)
    beta, ra, t2 = 1.0 - alpha, 1.0 / alpha, (1.0 - alpha) / alpha
    t1g, rdt = 2.0 * gama * (alpha * dt) ** 2, 1.0 / dt
    w1 = w2
    pe = np.exp(gama * np.log(-dm2 / dz2 * C.rdgas * pt2)) - pm2
    g_rat, bb, pp, piv = _pp_edges(pe, dm2, km)
    pf = [pem[:, k] + pp[k] for k in range(km + 1)]          # full p
    aa, wk = [None] * (km + 1), [None] * (km + 1)
    for k in range(1, km):
        a = t1g / (dz2[:, k - 1] + dz2[:, k]) * pf[k]
        wk[k] = t2 * a * (w1[:, k - 1] - w1[:, k])
        aa[k] = a - scale_m * dm2[:, 0]
    w, gam = [None] * km, [None] * km
    bet = dm2[:, 0] - aa[1]
    piv.append(bet)
    w[0] = (dm2[:, 0] * w1[:, 0] + dt * pp[1] + wk[1]) / bet
    for k in range(1, km - 1):
        gam[k] = aa[k] / bet
        bet = dm2[:, k] - (aa[k] + aa[k + 1] + aa[k] * gam[k])
        piv.append(bet)
        w[k] = (dm2[:, k] * w1[:, k] + dt * (pp[k + 1] - pp[k]) + wk[k + 1] - wk[k] - aa[k] * w[k - 1]) / bet
    k = km - 1
    wk1 = t1g / dz2[:, k] * pf[km]
    gam[k] = aa[k] / bet
    bet = dm2[:, k] - (aa[k] + wk1 + aa[k] * gam[k])
    piv.append(bet)
    w[k] = (dm2[:, k] * w1[:, k] + dt * (pp[km] - pp[k]) - wk[k] + wk1 * (t2 * w1[:, k] - ra * ws) - aa[k] * w[k - 1]) / bet
    for k in range(km - 2, -1, -1):
        w[k] = w[k] - gam[k + 1] * w[k + 1]
    pe2 = [None] * (km + 1)
    pe2[0] = 0 * w[0]
    for k in range(km):
        pe2[k + 1] = pe2[k] + (dm2[:, k] * (w[k] - w1[:, k]) * rdt - beta * (pp[k + 1] - pp[k])) * ra
    dz = _new_dz(C, pe2, g_rat, bb, dm2, pm2, pt2, km, info)
    for k in range(km + 1):
        pe2[k] = pe2[k] + beta * (pp[k] - pe2[k])
    if info is not None:
        info["min_pivot"] = np.min(np.stack([_re(p) for p in piv], axis=1), axis=1)
    return np.stack(pe2, axis=1), np.stack(w, axis=1), np.stack(dz, axis=1)


def _cum_pressure(C, delp):
    n, km = delp.shape
    pem = [None] * (km + 1)
    pem[0] = C.ptop + 0 * delp[:, 0]
    for k in range(km):
        pem[k + 1] = pem[k] + delp[:, k]
    return np.stack(pem, axis=1)


def riem_solver_c(C, X, hs, info=None):
    """X: gz_a (heights after the C-grid advection, km+1), wc, ptc, delpc; hs surface geopotential.  dt here is the half step.
    The tail of UPDATE_DZ_C runs first.  -> gz (geopotential), pkc (full pressure)"""
    dt = C.dt
    rgrav = 1.0 / C.grav
    ws, gz = dz_fix(X["gz_a"], hs * rgrav, dt, info)
    delp = X["delpc"]
    km = delp.shape[1]
    pem = _cum_pressure(C, delp)
    dz2 = gz[:, 1:] - gz[:, :-1]
    pm2 = delp / np.log(pem[:, 1:] / pem[:, :-1])
    dm = delp * rgrav
    pe2, _, dz = sim1_solver(C, dt, dm, pm2, pem, X["wc"], dz2, X["ptc"], ws, info)
    pef = np.concatenate([pem[:, :1], pe2[:, 1:] + pem[:, 1:]], axis=1)
    g = [None] * (km + 1)
    g[km] = hs + 0 * dz[:, 0]
    for k in range(km - 1, -1, -1):
        g[k] = g[k + 1] - dz[:, k] * C.grav
    return dict(gz=np.stack(g, axis=1), pkc=pef)


def riem_solver3(C, X, hs, last_call, info=None):
    """X: zh_a (heights after the D-grid advection, km+1), w_m, pt_o, delp_o.  The tail of UPDATE_DZ_D runs first.
    -> w_o, delz_o, zh_o, ppe, pk3 and, at the last acoustic step, pe, peln, pk, ws"""
    dt = C.dt
    rgrav = 1.0 / C.grav
    zs = hs * rgrav
    ws, zh = dz_fix(X["zh_a"], zs, dt, info)
    delp = X["delp_o"]
    km = delp.shape[1]
    pem = _cum_pressure(C, delp)
    peln2 = np.concatenate([np.log(C.ptop + 0 * _re(pem[:, :1])) + 0 * pem[:, :1], np.log(pem[:, 1:])], axis=1)
    pk3 = np.exp(C.akap * peln2)
    pm2 = delp / (peln2[:, 1:] - peln2[:, :-1])
    dm = delp * rgrav
    dz2 = zh[:, 1:] - zh[:, :-1]
    if C.a_imp > 0.999:
        pe2, w2, dz = sim1_solver(C, dt, dm, pm2, pem, X["w_m"], dz2, X["pt_o"], ws, info)
    elif C.a_imp > 0.5:
        pe2, w2, dz = sim_solver(C, dt, dm, pm2, pem, X["w_m"], dz2, X["pt_o"], ws, C.a_imp, C.scale_m, info)
    else:
        raise ValueError("a_imp <= 0.5: RIM_2D / SIM3 are not restated")
    z = [None] * (km + 1)
    z[km] = zs + 0 * dz[:, 0]
    for k in range(km - 1, -1, -1):
        z[k] = z[k + 1] - dz[:, k]
    out = dict(w_o=w2, delz_o=dz, zh_o=np.stack(z, axis=1), ppe=pe2, pk3=pk3)
    if last_call:
        out.update(pe=pem, peln=peln2, pk=pk3, ws=ws[:, None])
    return out


def edge_profile(q1, q2, dp0):
    """-> q1e, q2e (km+1); dp0: the reference thicknesses (km)"""
    km = q1.shape[1]
    dp0 = np.asarray(dp0, dtype=_re(q1[:1, :1]).dtype)
    out = []
    for q in (q1, q2):
        g0 = dp0[1] / dp0[0]
        xt1 = 2.0 * g0 * (g0 + 1.0)
        bet = g0 * (g0 + 0.5)
        qe, gam = [None] * (km + 1), [None] * (km + 1)
        qe[0] = (xt1 * q[:, 0] + q[:, 1]) / bet
        gam[0] = (1.0 + g0 * (g0 + 1.5)) / bet
        gk = g0
        for k in range(1, km):
            gk = dp0[k - 1] / dp0[k]
            bet = 2.0 + 2.0 * gk - gam[k - 1]
            qe[k] = (3.0 * (q[:, k - 1] + gk * q[:, k]) - qe[k - 1]) / bet
            gam[k] = gk / bet
        a_bot = 1.0 + gk * (gk + 1.5)
        xt1 = 2.0 * gk * (gk + 1.0)
        xt2 = gk * (gk + 0.5) - a_bot * gam[km - 1]
        qe[km] = (xt1 * q[:, km - 1] + q[:, km - 2] - a_bot * qe[km - 1]) / xt2
        for k in range(km - 1, -1, -1):
            qe[k] = qe[k] - gam[k] * qe[k + 1]
        out.append(np.stack(qe, axis=1))
    return out[0], out[1]


def pe_halo(C, delp):
    return _cum_pressure(C, delp)


def pk3_halo(C, delp):
    """levels 2 .. km+1 (level 1 belongs to RIEM_SOLVER3); level 1 is returned as ptop**akap for shape only"""
    return np.exp(C.akap * np.log(_cum_pressure(C, delp)))


# ------------------------------------------------------------------------------------------------ derivatives
def tangent(f, X, dX, cdtype=CLD):
    """complex step: f maps {name: [n, nk]} -> {name: [n, nk]}; -> (values, tangent).  cdtype = complex128 evaluates the same
    formulas in float64 (used to measure how far double arithmetic moves the result)"""
    real = LD if cdtype is CLD else np.float64
    Z = {n: np.asarray(X[n], dtype=cdtype) + 1j * real(H) * np.asarray(dX[n], dtype=real) for n in X}
    Y = f(Z)
    return {n: y.real for n, y in Y.items()}, {n: y.imag / real(H) for n, y in Y.items()}


def jt_s(f, X, S, cdtype=CLD):
    """J^T s entry by entry from the complex-step Jacobian (one evaluation per input entry, all columns at once)"""
    real = LD if cdtype is CLD else np.float64
    out = {}
    zero = {n: np.zeros(np.shape(X[n]), dtype=real) for n in X}
    for n in X:
        g = np.zeros(np.shape(X[n]), dtype=real)
        for k in range(np.shape(X[n])[1]):
            d = dict(zero)
            e = np.zeros(np.shape(X[n]), dtype=real)
            e[:, k] = 1.0
            d[n] = e
            _, t = tangent(f, X, d, cdtype)
            g[:, k] = sum(np.sum(np.asarray(S[o], dtype=real) * t[o], axis=1) for o in S)
        out[n] = g
    return out


def jt_s_entries(f, X, S, entries, cdtype=CLD, chunk=1200):
    """chosen entries of J^T s: entries = list of (column, input name, level index).  Every entry is one column evaluation with the
    unit vector e_k of that input, evaluated in chunks of gathered columns (f(Z, cols) gathers its per-column constants)
    -> (entries of J^T s, sum |s . J e_k| of each)"""
    real = LD if cdtype is CLD else np.float64
    res, sc = np.zeros(len(entries), dtype=real), np.zeros(len(entries), dtype=real)
    for c0 in range(0, len(entries), chunk):
        part = entries[c0:c0 + chunk]
        cols = np.array([e[0] for e in part])
        Xg = {n: np.asarray(X[n])[cols] for n in X}
        d = {n: np.zeros(Xg[n].shape, dtype=real) for n in X}
        for m, (_, n, k) in enumerate(part):
            d[n][m, k] = 1.0
        _, t = tangent(lambda Z: f(Z, cols), Xg, d, cdtype)
        res[c0:c0 + len(part)] = sum(np.sum(np.asarray(S[o], dtype=real)[cols] * t[o], axis=1) for o in S)
        sc[c0:c0 + len(part)] = sum(np.sum(np.abs(np.asarray(S[o], dtype=real)[cols] * t[o]), axis=1) for o in S)
    return res, sc
