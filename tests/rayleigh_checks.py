"""Checks of the Rayleigh damping of the upper layers (fv3lm_set_rayleigh; product csrc/rayleigh.h) shared by the host-emulation
(test_emul_rayleigh.py) and the MI355X (test_gpu_rayleigh.py) runs, against the numpy restatement tests/rayleigh_oracle.py:
  the profile rf(k), kmax; the unit alone (fv3lm_rayleigh) in the three modes; its place in fv_dynamics -- the product's step with
  tau > 0 on x equals the oracle's step (no damping) on R(x), its tangent the oracle's on R'(x) dx, its adjoint R'(x)^T (oracle adjoint);
  the non-hydrostatic step (pkz from the temperature before the heating, dot product, finite differences)."""
import numpy as np
from common import relerr
from oracle import NL, TL, AD
from rayleigh_oracle import Rayleigh
from fv3_jedi_linearmodel_amd import harness as H


def check_profile(c, tol=1e-15):
    rf, kmax = c.dy.rayleigh_profile()
    R = Rayleigh(c)
    assert kmax == R.kmax and 0 < kmax < c.npz, (kmax, R.kmax)
    assert np.all(rf[kmax:] == 0.0) and np.all(rf[:kmax] > 0.0), rf
    e = float(np.max(np.abs(rf - R.rf)) / np.max(R.rf))
    assert e <= tol, e
    return kmax


def _unit_state(c, seed=3):
    """trajectory and perturbation of u v pt (w) on the case's padded planes"""
    names = ["u", "v", "pt"] + ([] if c.opt.hydrostatic else ["w"])
    rng = np.random.default_rng(seed)
    T = {n: np.array(c.traj[n], dtype=np.float64) for n in ("u", "v", "pt")}
    P = {n: np.array(c.pert[n], dtype=np.float64) for n in ("u", "v")}
    P["pt"] = 20.0 * np.array(c.pert["pt"])
    if not c.opt.hydrostatic:
        T["w"] = 2.0 * rng.standard_normal(T["pt"].shape)
        P["w"] = 0.1 * rng.standard_normal(T["pt"].shape)
    return names, T, P


def check_unit(c, tol_nl=1e-13, tol_tl=1e-12, tol_ad=1e-12):
    """fv3lm_rayleigh alone: nonlinear, tangent, adjoint (dot-product identity and against the numpy transpose)"""
    names, T, P = _unit_state(c)
    R = Rayleigh(c)
    K, J, I = R.kmax, R.J, R.I
    nh = not c.opt.hydrostatic
    rfpt = lambda w: c.dy.get("rf_pt", w)[:, :K, J, I]
    # nonlinear
    for n in names:
        c.dy.put(n, T[n], 0)
    c.dy.rayleigh(NL)
    ref = R.nl(T)
    for n in names:
        got = c.dy.get(n, 0)
        assert relerr(got, ref[n]) <= tol_nl, (n, relerr(got, ref[n]))
        if np.abs(ref[n] - T[n]).max() > 0:            # the change itself (the heating is small beside pt)
            assert relerr(got - T[n], ref[n] - T[n]) <= tol_nl, (n, "increment", relerr(got - T[n], ref[n] - T[n]))
    assert np.abs(ref["u"] - T["u"]).max() > 0 and np.abs(ref["v"] - T["v"]).max() > 0
    if nh:
        assert np.array_equal(c.dy.get("pt", 0), T["pt"])       # pt_in's pkz comes from the temperature before the heating
        h0 = T["pt"][:, :K, J, I]
        assert relerr(rfpt(0) - h0, ref["rf_pt"] - h0) <= tol_nl
    else:
        assert np.abs(ref["pt"] - T["pt"]).max() > 0
    # tangent
    for n in names:
        c.dy.put(n, T[n], 0); c.dy.put(n, P[n], 1)
    c.dy.rayleigh(TL)
    dref = R.tl(T, P)
    for n in names:
        assert relerr(c.dy.get(n, 0), ref[n]) <= tol_nl, (n, "traj")
        assert relerr(c.dy.get(n, 1), dref[n]) <= tol_tl, (n, "tl", relerr(c.dy.get(n, 1), dref[n]))
    if nh:
        assert relerr(rfpt(1), dref["rf_pt"]) <= tol_tl
    Mdx = {n: c.dy.get(n, 1) for n in names}
    if nh:
        Mdx["rf_pt"] = rfpt(1)
    # adjoint
    rng = np.random.default_rng(11)
    y = {n: rng.standard_normal(T[n].shape) for n in names}
    for n in names:
        c.dy.put(n, T[n], 0)
    c.dy.rayleigh(NL)
    for n in names:
        c.dy.put(n, y[n], 1)
    if nh:
        yh = rng.standard_normal((c.dims.ntile, c.npz) + T["pt"].shape[2:])
        c.dy.put("rf_pt", yh, 1)
        y["rf_pt"] = yh[:, :K, J, I]
    c.dy.rayleigh(AD)
    xb = {n: c.dy.get(n, 1) for n in names}
    lhs = sum(float(np.sum(Mdx[n] * y[n])) for n in y)
    rhs = sum(float(np.sum(P[n] * xb[n])) for n in names)
    assert abs(lhs - rhs) <= tol_ad * abs(lhs), (lhs, rhs)
    aref = R.ad(T, y)
    for n in names:
        assert relerr(xb[n], aref[n]) <= tol_ad, (n, "ad", relerr(xb[n], aref[n]))
    return abs(lhs - rhs) / abs(lhs)


# ---- place in the step: product(tau > 0)(x) = oracle(R(x)), hydrostatic
def _step_state(c):
    if isinstance(c, H.CubeCase):
        T, P = H.cube_step_state(c)
        return T, P, (lambda a: a), (lambda a: a)
    T, P = H.step_state(c)
    return T, P, (lambda a: a[None]), (lambda a: a[0])


def check_composition(c, mode, tol):
    """fv_dynamics with the damping against the oracle's fv_dynamics (no damping) composed with the numpy damping"""
    from groups import rects, masked
    T, P, lift, drop = _step_state(c)
    nq = c.nq
    ins_n = ["u", "v", "pt", "delp", "pe", "peln", "pk", "pkz"] + ["q%d" % (n + 1) for n in range(nq)]
    outs = [("u", "U"), ("v", "V"), ("pt", "A"), ("delp", "A")] + [("q%d" % (n + 1), "A") for n in range(nq)]
    R = Rayleigh(c)
    assert R.kmax > 0
    X = {n: lift(T[n]) for n in ("u", "v", "pt")}
    RX = R.nl(X)
    i_t = [drop(RX[n]) if n in RX else T[n] for n in ins_n]
    a = (nq, c.dims.dt, c.dims.n_split, c.dims.k_split)
    for n in ins_n:
        c.dy.put(n, lift(T[n]), 0)
    if mode == TL:
        RP = R.tl(X, {n: lift(P[n]) for n in ("u", "v", "pt")})
        i_p = [drop(RP[n]) if n in RP else P[n] for n in ins_n]
        ot, op = c.oracle.fv_dynamics(TL, *a, i_t, i_p)
        for n in ins_n:
            c.dy.put(n, lift(P[n]), 1)
        c.dy.fv_dynamics(TL)
        worst = 0.0
        for (n, rk), x, y in zip(outs, ot, op):
            r = c.rect(*rects(c)[rk])
            e1, e2 = relerr(drop(c.dy.get(n, 0))[r], x[r]), relerr(drop(c.dy.get(n, 1))[r], y[r])
            assert e1 < min(tol, 1e-12), (n, "traj", e1)
            assert e2 < tol, (n, "tl", e2)
            worst = max(worst, e1, e2)
        return worst
    rng = np.random.default_rng(41)
    seeds = [masked(c, rng.standard_normal(T["u"].shape), rk) for n, rk in outs]
    _, iad = c.oracle.fv_dynamics(AD, *a, i_t, None, seeds)
    iad = dict(zip(ins_n, iad))
    want = R.ad(X, {n: lift(iad[n]) for n in ("u", "v", "pt")})
    c.dy.fv_dynamics(NL)
    for n in ins_n:
        c.dy.put(n, np.zeros(c.dy.shape(n)), 1)
    for (n, rk), s in zip(outs, seeds):
        c.dy.put(n, lift(s), 1)
    c.dy.fv_dynamics(AD)
    worst = 0.0
    for n in ins_n:
        if n in ("pe", "peln", "pk"):
            continue
        x = drop(want[n]) if n in want else iad[n]
        e = relerr(drop(c.dy.get(n, 1)), x)
        assert e < tol, (n, "ad", e)
        worst = max(worst, e)
    return worst


# ---- non-hydrostatic step
def _nh_put(c, T, P=None):
    from nh_checks import fv_names
    for n, t in zip(fv_names(c), T):
        c.dy.put(n, t[None], 0)
        c.dy.put(n, (P[fv_names(c).index(n)] if P is not None else np.zeros_like(t))[None], 1)


def check_nh_pkz_before_heating(c, c0):
    """npz <= 4 (no remap: pkz after fv_dynamics is pt_in's): with the damping on (c) pkz is that of the undamped case (c0), i.e. it is
    taken from the temperature before the heating, while pt_in's result differs"""
    from test_oracle_nh import nh_state_fv
    assert c.npz <= 4 and Rayleigh(c).kmax > 0
    T, _ = nh_state_fv(c)
    out = []
    for x in (c, c0):
        _nh_put(x, T)
        x.dy.fv_dynamics(NL)
        out.append((x.dy.get("pkz", 0), x.dy.get("pt", 0)))
    assert np.array_equal(out[0][0], out[1][0])
    assert np.abs(out[0][1] - out[1][1]).max() > 0


def check_nh_taylor(c, eps=(3e-2, 1e-2)):
    """tangent of fv_dynamics against central differences of the nonlinear step: the error falls like eps^2.  A mean wind keeps the
    upwind branches of the transport (sign of the Courant numbers) on one side under the perturbation; without it a branch switch
    shows up near eps ~ 4e-3, below which round-off already dominates."""
    from test_oracle_nh import nh_state_fv
    from nh_checks import fv_names, fv_dom
    T, P = nh_state_fv(c)
    T = [T[0] + 20.0, T[1] + 12.0] + list(T[2:])
    _nh_put(c, T, P)
    c.dy.fv_dynamics(TL)
    tl = {n: c.dy.get(n, 1)[0] for n in fv_names(c)}
    errs = []
    for e in eps:
        y = []
        for sgn in (1.0, -1.0):
            _nh_put(c, [t + sgn * e * p for t, p in zip(T, P)])
            c.dy.step_nl()
            y.append({n: c.dy.get(n, 0)[0] for n in fv_names(c)})
        num = sum(float(np.sum(((y[0][n] - y[1][n]) / (2 * e) - tl[n])[fv_dom(c, n)] ** 2)) for n in fv_names(c))
        den = sum(float(np.sum(tl[n][fv_dom(c, n)] ** 2)) for n in fv_names(c))
        errs.append(np.sqrt(num / den))
    ratio = errs[1] / errs[0]
    assert errs[0] < 1e-4 and ratio < 3.0 * (eps[1] / eps[0]) ** 2, (errs, ratio)
    return errs
