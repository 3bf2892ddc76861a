"""Column checks of the vertical remap (fv3lm_remap; product csrc/remap.h, nh.h) shared by the host-emulation (test_emul_remap_column.py)
and the MI355X (test_gpu_remap_column.py) runs, against the numpy restatement tests/remap_oracle.py.  The columns are built here:
  identity   the source levels are the target levels
  small      source layers within +-3 % of the target ones
  large      a target layer holding >= 8 source layers and a source layer holding >= 8 targets (npz >= 12; fewer levels: as many as fit)
  ratio      adjacent source thicknesses in ratios of 1e-3 .. 1e3
on every kind the surface pressure differs by up to 5 % between neighbouring columns, so the pressures of u and v (averaged across the edge)
match neither column; hard = True adds T_v below t_min = 184 K, tracers with exact zeros and negatives, winds of both signs, w with ws != 0.
Errors are measured per level: max |product - reference| over the level's points / max |reference| over them."""
import numpy as np
from oracle import NL, TL, AD
import remap_oracle as RO


def stretched_levels(npz, ptop=1.0, p0=1.0e5):
    """L127-like hybrid coefficients: layer thickness growing geometrically from about 1 Pa at the top to about 1500 Pa, then flat,
    pure pressure above 100 hPa"""
    kg = max(1, int(0.55 * npz))
    r = 1500.0 ** (1.0 / kg)
    dp = np.minimum(1500.0, r ** np.arange(npz))
    dp *= (p0 - ptop) / dp.sum()
    pref = ptop + np.concatenate([[0.0], np.cumsum(dp)])
    pref[-1] = p0
    bk = np.clip((pref - 1.0e4) / (p0 - 1.0e4), 0.0, 1.0) ** 2
    ak = pref - bk * p0
    ak[0], bk[0], ak[-1], bk[-1] = ptop, 0.0, 0.0, 1.0
    return ak, bk


def _warp(npz):
    """monotone source positions xi(0..npz) in units of target layers: a block of thin layers at the top, one thick layer in the middle"""
    if npz >= 12:
        inc = [0.1] * 10 + [1.0] * ((npz - 11) // 2) + [10.0] + [1.0] * (npz - 11 - (npz - 11) // 2)
    elif npz >= 5:
        inc = [0.25] * 4 + [1.0] * ((npz - 5) // 2) + [4.0] + [1.0] * (npz - 5 - (npz - 5) // 2)
    else:
        inc = list(np.diff(npz * (np.arange(npz + 1) / npz) ** 3))
    xi = np.concatenate([[0.0], np.cumsum(inc)])
    xi *= npz / xi[-1]
    return xi


def column_state(c, kind, seed=1, hard=False):
    """trajectory planes [nk, ny+7, nx+7] of every remap input of case c"""
    o, km = c.opt, c.npz
    pj, pi = c.ny + 7, c.nx + 7
    rng = np.random.default_rng(seed)
    ps = 1.0e5 * (1.0 + 0.025 * rng.uniform(-1.0, 1.0, (pj, pi)))
    ak, bk = np.asarray(c.ak), np.asarray(c.bk)
    pe2 = ak[:, None, None] + bk[:, None, None] * ps[None]
    pe2[0], pe2[km] = o.ptop, ps
    if kind == "identity":
        pe = pe2.copy()
    elif kind == "small":
        d = np.diff(pe2, axis=0) * (1.0 + 0.03 * rng.uniform(-1.0, 1.0, (km, pj, pi)))
        pe = o.ptop + np.concatenate([np.zeros((1, pj, pi)), np.cumsum(d, axis=0) * ((ps - o.ptop) / d.sum(axis=0))[None]], axis=0)
    elif kind == "large":
        xi = _warp(km)
        k0 = np.minimum(np.floor(xi).astype(int), km - 1)
        f = (xi - k0)[:, None, None]
        pe = pe2[k0] + f * (pe2[k0 + 1] - pe2[k0])
    elif kind == "ratio":
        e = 1.5 * np.where(np.arange(km) % 2 == 0, 1.0, -1.0)[:, None, None] * rng.uniform(0.6, 1.0, (km, pj, pi))
        d = 10.0 ** e
        pe = o.ptop + np.concatenate([np.zeros((1, pj, pi)), np.cumsum(d, axis=0) * ((ps - o.ptop) / d.sum(axis=0))[None]], axis=0)
    else:
        raise ValueError(kind)
    pe[0], pe[km] = o.ptop, ps
    peln = np.log(pe)
    pk = np.exp(o.akap * peln)
    pkz = np.diff(pk, axis=0) / (o.akap * np.diff(peln, axis=0))
    tv = 200.0 + 90.0 * rng.uniform(0.0, 1.0, (km, pj, pi))
    u = 25.0 * rng.uniform(-1.0, 1.0, (km, pj, pi)) if hard else 15.0 + 8.0 * rng.uniform(-1.0, 1.0, (km, pj, pi))
    v = 25.0 * rng.uniform(-1.0, 1.0, (km, pj, pi)) if hard else -5.0 + 4.0 * rng.uniform(-1.0, 1.0, (km, pj, pi))
    qs = []
    for n in range(c.nq):
        q = 1e-3 * (0.2 + rng.uniform(0.0, 1.0, (km, pj, pi)))
        if hard:
            q[rng.uniform(size=q.shape) < 0.25] = 0.0
            neg = rng.uniform(size=q.shape) < 0.1
            q[neg] = -1e-4 * rng.uniform(0.1, 1.0, int(neg.sum()))
        qs.append(q)
    if hard:
        cold = rng.uniform(size=tv.shape) < 0.3
        tv[cold] = 150.0 + 30.0 * rng.uniform(0.0, 1.0, int(cold.sum()))
    S = dict(pe=pe, peln=peln, pk=pk, pt=tv / pkz, u=u, v=v)
    for n in range(c.nq):
        S["q%d" % (n + 1)] = qs[n]
    if not o.hydrostatic:
        S["delp"] = np.diff(pe, axis=0)
        noise = 0.0 if kind == "ratio" else 0.05        # (-delz/delp stays positive through the ratio columns' unlimited profile only when smooth)
        S["delz"] = -(o.rdgas / o.grav) * tv * np.diff(peln, axis=0) * (1.0 + noise * rng.uniform(-1.0, 1.0, (km, pj, pi)))
        S["w"] = (3.0 if hard else 1.0) * rng.uniform(-1.0, 1.0, (km, pj, pi))
        S["ws"] = (0.5 + 0.5 * rng.uniform(0.0, 1.0, (1, pj, pi))) * np.where(rng.uniform(size=(1, pj, pi)) < 0.5, -1.0, 1.0)
    return S


def perturbation(S, seed=2, only=None):
    """tangent inputs on every point; only = a list of names: the others zero"""
    rng = np.random.default_rng(seed)
    sc = dict(pe=None, peln=1e-3, pk=1e-2, pt=1e-1, u=1.0, v=1.0, delp=None, delz=1.0, w=0.3, ws=0.3)
    P = {}
    for n, a in S.items():
        r = rng.standard_normal(a.shape)
        if n in ("pe", "delp"):
            d = np.diff(S["pe"], axis=0)
            ref = np.concatenate([d[:1], np.minimum(d[1:], d[:-1]), d[-1:]], axis=0) if n == "pe" else d
            P[n] = 0.05 * ref * r
        elif n.startswith("q"):
            P[n] = 1e-4 * r
        else:
            P[n] = sc[n] * r
        if only is not None and n not in only:
            P[n] = np.zeros_like(a)
    return P


# ------------------------------------------------------------------------------------------------ the product
def _put_inputs(c, S, which):
    for n, a in S.items():
        c.dy.put(n, np.asarray(a, dtype=np.float64)[None], which)


def product(c, mode, last, S, P=None, seeds=None):
    """NL: {output: plane}.  TL: ({output: values}, {output: tangent}).  AD: {input: adjoint plane} from the output seeds."""
    R = RO.Remap(c, last)
    _put_inputs(c, S, 0)
    if mode == NL:
        c.dy.remap(NL, last)
        return {n: c.dy.get(n, 0)[0] for n, _ in R.outputs}
    if mode == TL:
        _put_inputs(c, P, 1)
        c.dy.remap(TL, last)
        return {n: c.dy.get(n, 0)[0] for n, _ in R.outputs}, {n: c.dy.get(n, 1)[0] for n, _ in R.outputs}
    for n in set(R.inputs) | {o for o, _ in R.outputs}:
        c.dy.put(n, np.zeros(c.dy.shape(n)), 1)
    for n, _ in R.outputs:
        c.dy.put(n, seeds[n][None], 1)
    c.dy.remap(AD, last)
    return {n: c.dy.get(n, 1)[0] for n in R.inputs}


def make_seeds(c, R, seed=5):
    """output adjoints on each output's rectangle.  pe: the two end levels only -- the interior of pe after the remap is dead in
    fv_dynamics (the next geopk rebuilds it) and its adjoint is not taken (as in groups.check_remap)"""
    rng = np.random.default_rng(seed)
    out = {}
    for n, rk in R.outputs:
        s = np.zeros(c.dy.shape(n)[1:])
        i0, i1, j0, j1 = R.R[rk]
        s[:, j0 + 2:j1 + 3, i0 + 2:i1 + 3] = rng.standard_normal((s.shape[0], j1 - j0 + 1, i1 - i0 + 1))
        if n == "pe":
            s[1:-1] = 0.0
        out[n] = s
    return out


def on_rect(R, name, plane_):
    rk = dict(R.outputs)[name]
    i0, i1, j0, j1 = R.R[rk]
    return plane_[:, j0 + 2:j1 + 3, i0 + 2:i1 + 3]


def per_level(got, ref):
    """max over levels of max |got - ref| / max |ref| at that level (levels whose reference is all zero: the absolute error)"""
    got, ref = np.asarray(got, dtype=np.longdouble), np.asarray(ref, dtype=np.longdouble)
    e = 0.0
    for k in range(ref.shape[0]):
        s = np.max(np.abs(ref[k]))
        e = max(e, float(np.max(np.abs(got[k] - ref[k])) / (s if s > 0 else 1.0)))
    return e


# ------------------------------------------------------------------------------------------------ checks
def check_nl_tl(c, S, last, tol=1e-12, P=None, conditioned=False):
    """NL values and TL (values and tangent) of every output on its rectangle against the reference; -> measured maxima.
    conditioned = True (the 'ratio' columns): adjacent thickness ratios of 1e3 make the edge-value solve ill-conditioned, and the same
    reference evaluated in float64 moves by up to ~1e-10 from the longdouble one; the bound per output is then max(tol, 4 x that move):
    the product must be as accurate as double arithmetic on these formulas can be."""
    R = RO.Remap(c, last)
    P = P if P is not None else perturbation(S)
    ref = R.nl(S)
    rv, rt = R.tl(S, P)
    tl_nl, tl_tl = {n: tol for n, _ in R.outputs}, {n: tol for n, _ in R.outputs}
    if conditioned:
        R64 = RO.Remap(c, last, real=np.float64)
        r64 = R64.nl(S)
        _, t64 = R64.tl(S, P)
        for n, _ in R.outputs:
            tl_nl[n] = max(tol, 4.0 * per_level(r64[n], ref[n]))
            tl_tl[n] = max(tol, 4.0 * per_level(t64[n], rt[n]))
    got = product(c, NL, last, S)
    m = {}
    for n, _ in R.outputs:
        e = per_level(on_rect(R, n, got[n]), ref[n])
        m["nl." + n] = e
        assert e <= tl_nl[n], (n, "nl", e, tl_nl[n])
    gv, gt = product(c, TL, last, S, P)
    for n, _ in R.outputs:
        e1, e2 = per_level(on_rect(R, n, gv[n]), rv[n]), per_level(on_rect(R, n, gt[n]), rt[n])
        m["tl." + n] = e2
        assert e1 <= tl_nl[n], (n, "tl values", e1, tl_nl[n])
        assert e2 <= tl_tl[n], (n, "tl", e2, tl_tl[n])
    return m


def check_ad_dot(c, S, last, tol=1e-11, nx_=3):
    """<AD(s), x> = <s, TL_ref(x)> for several random x (no Jacobian: any size) -> largest relative mismatch"""
    R = RO.Remap(c, last)
    seeds = make_seeds(c, R)
    ad = product(c, AD, last, S, seeds=seeds)
    worst = 0.0
    for t in range(nx_):
        X = perturbation(S, seed=40 + t)
        _, y = R.tl(S, X)
        rhs = sum(float(np.sum(on_rect(R, n, seeds[n]) * y[n])) for n, _ in R.outputs)
        lhs = sum(float(np.sum(ad[n] * X[n])) for n in R.inputs)
        scale = sum(float(np.sum(np.abs(on_rect(R, n, seeds[n]) * y[n]))) for n, _ in R.outputs)
        e = abs(lhs - rhs) / scale
        worst = max(worst, e)
        assert e <= tol, (t, lhs, rhs, e)
    return worst


def check_ad_jacobian(c, S, last, tol=1e-11):
    """the adjoint entry by entry against J^T s of the reference tangent (small columns only) -> measured maxima"""
    R = RO.Remap(c, last)
    seeds = make_seeds(c, R)
    ad = product(c, AD, last, S, seeds=seeds)
    ref = R.jt_s(S, seeds)
    m = {}
    for n in R.inputs:
        e = per_level(ad[n], ref[n])
        m["ad." + n] = e
        assert e <= tol, (n, "ad", e)
    return m


# ------------------------------------------------------------------------------------------------ properties (no restatement)
def check_conservation(c, S, last=0, tol=1e-12):
    """sum q2 dp2 = sum q1 dp1 per column for tracers (in p), winds (in the averaged pressures) and T_v in log p (recovered from the
    outputs: T_v = pt * pkz on an other-step remap)"""
    assert not last
    R = RO.Remap(c, last)
    got = product(c, NL, last, S)
    A = R.R["A"]
    col = lambda a, r=A: RO.cols(a, r)
    pe1 = col(S["pe"])
    pe2 = col(got["pe"])
    worst = 0.0

    def cmp(q1, p1, q2, p2):
        m1 = np.sum(q1 * np.diff(p1, axis=1), axis=1)
        m2 = np.sum(q2 * np.diff(p2, axis=1), axis=1)
        sc = np.sum(np.abs(q1 * np.diff(p1, axis=1)), axis=1)
        return float(np.max(np.abs(m1 - m2) / sc))
    for n in range(c.nq):
        nm = "q%d" % (n + 1)
        worst = max(worst, cmp(col(S[nm]), pe1, col(got[nm]), pe2))
    if c.opt.hydrostatic:
        pn1, pk1 = col(S["peln"]), col(S["pk"])
        tv1 = col(S["pt"]) * np.diff(pk1, axis=1) / (c.opt.akap * np.diff(pn1, axis=1))
        worst = max(worst, cmp(tv1, pn1, col(got["pt"]) * col(got["pkz"]), col(got["peln"])))
    for d, nm, rk in ((0, "u", "U"), (1, "v", "V")):
        i0, i1, j0, j1 = R.R[rk]
        sh = (i0, i1, j0 - 1, j1 - 1) if d == 0 else (i0 - 1, i1 - 1, j0, j1)
        pa, pb = col(S["pe"], R.R[rk]), col(S["pe"], sh)
        pe0 = np.concatenate([pa[:, :1], 0.5 * (pa[:, 1:] + pb[:, 1:])], axis=1)
        pss = pa[:, -1] + pb[:, -1]
        pe3 = np.asarray(c.ak)[None] + 0.5 * np.asarray(c.bk)[None] * pss[:, None]
        if d == 1:
            pe3[:, 0] = c.ak[0]
        worst = max(worst, cmp(col(S[nm], R.R[rk]), pe0, col(got[nm], R.R[rk]), pe3))
    assert worst <= tol, worst
    return worst


def check_constant(c, S, tol=1e-13):
    """constant layer means map to the same constant (tracers, winds, T_v)"""
    S = dict(S)
    vals = dict(u=7.5, v=-3.25, q=2.0e-3, tv=250.0)
    pkz = np.diff(S["pk"], axis=0) / (c.opt.akap * np.diff(S["peln"], axis=0))
    S["pt"] = vals["tv"] / pkz
    S["u"], S["v"] = np.full_like(S["u"], vals["u"]), np.full_like(S["v"], vals["v"])
    for n in range(c.nq):
        S["q%d" % (n + 1)] = np.full_like(S["q1"], vals["q"])
    R = RO.Remap(c, 0)
    got = product(c, NL, 0, S)
    worst = 0.0
    for n, v_ in [("u", vals["u"]), ("v", vals["v"])] + [("q%d" % (n + 1), vals["q"]) for n in range(c.nq)]:
        worst = max(worst, float(np.max(np.abs(on_rect(R, n, got[n]) - v_))) / abs(v_))
    if c.opt.hydrostatic:
        tv2 = on_rect(R, "pt", got["pt"]) * on_rect(R, "pkz", got["pkz"])
        worst = max(worst, float(np.max(np.abs(tv2 - vals["tv"]))) / vals["tv"])
    assert worst <= tol, worst
    return worst


def check_identity(c, S, last=0, tol=1e-12):
    """source levels = target levels (column_state 'identity'): NL returns the inputs; with the pressures held (no pe / peln / pk tangent)
    the TL returns the input tangents; the adjoint of the mapped fields returns their seeds"""
    R = RO.Remap(c, last)
    mapped = ["pt", "u", "v"] + ["q%d" % (n + 1) for n in range(c.nq)] + ([] if c.opt.hydrostatic else ["w", "delz"])
    if last:
        mapped.remove("pt")
    got = product(c, NL, last, S)
    worst = 0.0
    for n in mapped:
        e = per_level(on_rect(R, n, got[n]), on_rect(R, n, S[n]))
        worst = max(worst, e)
        assert e <= tol, (n, "nl", e)
    P = perturbation(S, only=mapped)
    _, gt = product(c, TL, last, S, P)
    for n in mapped:
        e = per_level(on_rect(R, n, gt[n]), on_rect(R, n, P[n]))
        worst = max(worst, e)
        assert e <= tol, (n, "tl", e)
    seeds = {n: np.zeros(c.dy.shape(n)[1:]) for n, _ in R.outputs}
    full = make_seeds(c, R)
    for n in mapped:
        seeds[n] = full[n]
    ad = product(c, AD, last, S, seeds=seeds)
    for n in mapped:
        e = per_level(on_rect(R, n, ad[n]), on_rect(R, n, seeds[n]))
        worst = max(worst, e)
        assert e <= tol, (n, "ad", e)
    return worst


def check_nonnegative(c, S):
    """limited tracer profiles (scalar_profile, iv = 0) keep non-negative columns non-negative: every edge value is >= 0 after the
    constraints (the interior clamps, max(0, .) at both ends and where the interior edge test falls through), the monotone limiters of
    layers 1, 2, km-1, km then keep the parabola between its edges, and cs_limiters(iv = 0) clears the negative minimum of the others --
    whatever kord 8 .. 15 picked in between.  Asserted for every kord."""
    S = dict(S)
    for n in range(c.nq):
        q = np.abs(S["q%d" % (n + 1)])
        q[np.random.default_rng(n).uniform(size=q.shape) < 0.3] = 0.0
        S["q%d" % (n + 1)] = q
    R = RO.Remap(c, 0)
    got = product(c, NL, 0, S)
    for n in range(c.nq):
        nm = "q%d" % (n + 1)
        assert np.min(on_rect(R, nm, got[nm])) >= 0.0, (nm, float(np.min(on_rect(R, nm, got[nm]))))
    return True
