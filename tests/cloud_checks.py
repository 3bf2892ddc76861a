"""Checks of the linearised cloud scheme on the device (fv3lm_cloud_*; product csrc/cloud.h) shared by the host-emulation
(test_emul_cloud.py) and the MI355X (test_gpu_cloud.py) runs.

The yardstick is tests/golden/cloud_ref.npz: soundings at L40 and L72 (do_phy_mst = 2), L72 and L20 (do_phy_mst = 1) with what the
reference's own RASE0, CLOUD_DRIVER, CLOUD_DRIVER_D and CLOUD_DRIVER_B, compiled from their own source, returned for them
(tests/golden/make_cloud_golden.py); set_ltraj's split and fractions and the conversions of step_tl / step_ad are restated in numpy.  The
tolerance of an output is read from the fixture: (LM - 29) x the largest movement of that output, relative to its column maximum, when
the reference's inputs are perturbed by 1e-15 (errors pass down the column through the carried precipitation), floor 1e-12.  Every column
of the fixture is compared.  The forcing of the adjoint has no CF_con component in the levels of the loop: cloud_ad.F90:853-854 clears
that adjoint, which is not the transpose of anything in cloud_tl.F90, so only there is the reference's own pair adjoint (the generator
asserts it); the device's adjoint is the transpose of its tangent everywhere, which the dot-product checks hold it to."""
import os
import numpy as np
import turbulence_checks as TC
import convection_checks as CC
from fv3_jedi_linearmodel_amd._lib import Dycore, Fv3LmError

NL, TL, AD = 0, 1, 2
KTOP = 30
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cloud_ref.npz")
OUT8 = list(Dycore.CLOUD_NAMES)
FRAC = list(Dycore.FRAC_NAMES)
SRC = list(Dycore.SRC_NAMES)
IQI, IQL = 2, 3
LD = np.longdouble
_fix = {}
lev, pad, dealt, err, judge = CC.lev, CC.pad, CC.dealt, CC.err, CC.judge


def fixture(tag):
    if tag not in _fix:
        z = np.load(FIX)
        pre = tag + "_"
        f = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
        f["ref"] = {k[4:]: f.pop(k) for k in list(f) if k.startswith("ref_")}
        f["lm"] = f["T"].shape[0]; f["mst"] = int(tag.split("m")[1]); f["tag"] = tag
        m = max(f["lm"] - 29, 1)
        f["tol"] = {str(n): max(m * float(s), 1e-12) for n, s in zip(f.pop("spread_names"), f.pop("spread"))}
        f["dt"], f["ptop"], f["kappa"], f["p00"] = float(z["dt"]), float(z["ptop"]), float(z["kappa"]), float(z["p00"])
        f["X"] = f["X"].astype(np.float64); f["Y"] = f["Y"].astype(np.float64)
        f["ncol"] = f["T"].shape[1]
        _fix[tag] = f
    return _fix[tag]


def case_kw(fx):
    return dict(levels=(fx["ak"], fx["bk"]), ptop=fx["ptop"])


def placed(c, fx, col):
    """the fixture's columns on the case: the padded trajectory, the surface fields of the convection and the five arrays of the cloud set"""
    T, sfc, k = CC.placed(c, fx, col)
    cl = [lev(fx[n], k) for n in ("QLS", "QCN", "cfcn")] + [np.ascontiguousarray(fx[n][k]) for n in ("khl", "khu")]
    return T, sfc, cl, k


def ensure_created(c, fx, nslots=1):
    if getattr(c, "_conv_slots", 0) == 0:
        p = c.dy.ras_default_params(12)
        assert np.array_equal(np.array(p.r[:]), fx["rpar"])
        c.dy.convection_create(nslots, p, fx["mst"])
        c._conv_slots = nslots
        q = c.dy.cloud_default_params(12)
        assert np.array_equal(np.array(q.r[:]), fx["cpar"]), "cloud_default_params: the set of create :151-211"
        c.dy.cloud_create(q, IQI, IQL)
    assert c._conv_slots >= nslots


def set_fixture(c, tag, shift=0, slot=0, nslots=1):
    fx = fixture(tag)
    assert abs(c.dims.dt - fx["dt"]) == 0.0 and c.opt.ptop == fx["ptop"] and np.array_equal(c.ak, fx["ak"]) and c.nq >= 3
    T, sfc, cl, k = placed(c, fx, dealt(c, shift))
    ensure_created(c, fx, nslots)
    TC.put_all(c, T)
    c.dy.convection_set(slot, *sfc)
    c.dy.cloud_set(slot, *cl)
    return fx, T, sfc, cl, k


def tol_sum(fx, a, b):
    return max(fx["tol"][a], fx["tol"][b])


# ---- 1, 5: set against the reference
def check_set(c, tag):
    fx, T, sfc, cl, k = set_fixture(c, tag)
    lm = fx["lm"]
    assert set(np.unique(k)) == set(range(fx["ncol"])), "every column of the fixture is on the case"
    out, frac, pm = c.dy.cloud_get(0)
    e, tol = {}, dict(fx["tol"])
    for n in OUT8:
        e["out_" + n] = err(out[n], lev(fx["ref"]["out_" + n], k))
    for n in FRAC:
        e[n] = err(frac[n], lev(fx["ref"][n], k)); tol[n] = 1e-12
    # the split arrays are what the levels above the loop keep of the four condensates
    top = min(KTOP - 1, lm)
    for n, s in (("QI_ls", "QILST"), ("QL_ls", "QLLST"), ("QI_con", "QICNT"), ("QL_con", "QLCNT")):
        e[s] = err(out[n][:, :top], lev(fx["ref"][s], k)[:, :top]); tol[s] = 1e-12
    judge(e, tol, "%s set" % tag)
    ref_pm = lev(fx["ref"]["pertmod"], k)
    assert np.array_equal(pm, ref_pm), ("cloud_pertmod", int((pm != ref_pm).sum()))
    if fx["mst"] == 1:
        assert np.all(pm == 1)
    else:
        assert np.any(pm == 0) and np.any(pm[:, KTOP - 1:] == 1)
    assert np.all(out["CF_ls"][:, :top] == 0.0), "a level above KTOP was touched"
    return e


def host_fields(c, fx, k, pk, p00k, adjoint):
    """the fixture's drawn perturbation (theta, qv, qi, ql, cfcn, four sources) or adjoint forcing (theta, qv, qi, ql, cfcn) as the fields of
    the case, random elsewhere: the theta conversion restated"""
    Z = fx["Y"] if adjoint else fx["X"]
    rng = np.random.default_rng(7)
    shp = (c.dims.ntile, c.npz, c.ny + 7, c.nx + 7)
    P = {n: 1e-3 * rng.standard_normal(shp) for n in TC.all_names(c)}
    D = TC.dom(c)
    th = lev(Z[0], k)
    P["pt"][D] = th * p00k / pk if adjoint else th * pk / p00k
    P["q1"][D] = lev(Z[1], k); P["q%d" % IQI][D] = lev(Z[2], k); P["q%d" % IQL][D] = lev(Z[3], k)
    return P, lev(Z[4], k), ([lev(Z[5 + m], k) for m in range(4)] if not adjoint else None)


# ---- 2, 3, 4: the three modes against CLOUD_DRIVER_D, CLOUD_DRIVER_B and CLOUD_DRIVER
def check_modes(c, tag):
    fx, T, sfc, cl, k = set_fixture(c, tag)
    R = fx["ref"]
    D = TC.dom(c)
    pk, p00k = CC.pk_of(fx, TC.comp(c, T["delp"]))
    touched = ("pt", "q1", "q%d" % IQI, "q%d" % IQL)
    e, tol = {}, {}
    # tangent
    P, cf, src = host_fields(c, fx, k, pk, p00k, False)
    TC.put_all(c, T, P)
    c.dy.convection_sources(src)
    c.dy.cloud_cfcn(cf)
    c.dy.cloud(0, TL)
    got = {n: c.dy.get(n, 1) for n in TC.all_names(c)}
    want = dict(pt=lev(R["tl_th"], k), q1=lev(R["tl_q"], k), qi=lev(R["tl_QI_ls"] + R["tl_QI_con"], k), ql=lev(R["tl_QL_ls"] + R["tl_QL_con"], k), cfcn=lev(R["tl_CF_con"], k))
    e["tl_th"] = err(got["pt"][D] * p00k / pk, want["pt"]); tol["tl_th"] = fx["tol"]["tl_th"]
    e["tl_q"] = err(got["q1"][D], want["q1"]); tol["tl_q"] = fx["tol"]["tl_q"]
    e["tl_qi"] = err(got["q%d" % IQI][D], want["qi"]); tol["tl_qi"] = tol_sum(fx, "tl_QI_ls", "tl_QI_con")
    e["tl_ql"] = err(got["q%d" % IQL][D], want["ql"]); tol["tl_ql"] = tol_sum(fx, "tl_QL_ls", "tl_QL_con")
    e["tl_cfcn"] = err(c.dy.cloud_cfcn(), want["cfcn"]); tol["tl_cfcn"] = fx["tol"]["tl_CF_con"]
    for n in TC.all_names(c):
        keep = got[n].copy(); keep[D] = P[n][D]
        assert np.array_equal(keep, P[n]) and (n in touched or np.array_equal(got[n], P[n])), (n, "moved outside is..ie x js..je, or a field the cloud scheme does not touch")
        assert np.array_equal(c.dy.get(n, 0), T[n]), (n, "the trajectory moved in the tangent run")
    after = c.dy.convection_sources()
    assert all(np.array_equal(after[n], src[m]) for m, n in enumerate(SRC)), "the tangent run reads the sources and leaves them"
    # adjoint
    P, cf, _ = host_fields(c, fx, k, pk, p00k, True)
    TC.put_all(c, T, P)
    c.dy.cloud_cfcn(cf)
    c.dy.cloud(0, AD)
    got = {n: c.dy.get(n, 1) for n in TC.all_names(c)}
    F = {n: lev(R[n], k) for n in FRAC}
    e["ad_th"] = err(got["pt"][D] * pk / p00k, lev(R["ad_th"], k)); tol["ad_th"] = fx["tol"]["ad_th"]
    e["ad_q"] = err(got["q1"][D], lev(R["ad_q"], k)); tol["ad_q"] = fx["tol"]["ad_q"]
    e["ad_qi"] = err(got["q%d" % IQI][D], lev(R["ad_QI_ls"], k) * F["ILSF"] + lev(R["ad_QI_con"], k) * F["ICNF"]); tol["ad_qi"] = tol_sum(fx, "ad_QI_ls", "ad_QI_con")
    e["ad_ql"] = err(got["q%d" % IQL][D], lev(R["ad_QL_ls"], k) * F["LLSF"] + lev(R["ad_QL_con"], k) * F["LCNF"]); tol["ad_ql"] = tol_sum(fx, "ad_QL_ls", "ad_QL_con")
    e["ad_cfcn"] = err(c.dy.cloud_cfcn(), lev(R["ad_CF_con"], k)); tol["ad_cfcn"] = fx["tol"]["ad_CF_con"]
    sb = c.dy.convection_sources()
    for n in SRC:
        e["ad_" + n] = err(sb[n], lev(R["ad_" + n], k)); tol["ad_" + n] = fx["tol"]["ad_" + n]
    for n in TC.all_names(c):
        keep = got[n].copy(); keep[D] = P[n][D]
        assert np.array_equal(keep, P[n]) and (n in touched or np.array_equal(got[n], P[n])), (n, "moved outside is..ie x js..je, or a field the cloud scheme does not touch")
    # nonlinear: qi, ql of the trajectory from CLOUD_DRIVER in values; T, qv and everything else as they were
    TC.put_all(c, T, P)
    c.dy.cloud(0, NL)
    for n in TC.all_names(c):
        g = c.dy.get(n, 0)
        if n in ("q%d" % IQI, "q%d" % IQL):
            keep = g.copy(); keep[D] = T[n][D]
            assert np.array_equal(keep, T[n]), (n, "trajectory moved outside is..ie x js..je")
            a, b = ("QI_ls", "QI_con") if n == "q%d" % IQI else ("QL_ls", "QL_con")
            e["nl_" + a[:2]] = err(g[D], lev(R["out_" + a] + R["out_" + b], k)); tol["nl_" + a[:2]] = tol_sum(fx, "out_" + a, "out_" + b)
        else:
            assert np.array_equal(g, T[n]), (n, "the nonlinear run moved a field that is not qi or ql")
        assert np.array_equal(c.dy.get(n, 1), P[n]), (n, "the perturbation moved in the nonlinear run")
    out, _, _ = c.dy.cloud_get(0, frac=False, pertmod=False)
    e["nl_CF_con"] = err(out["CF_con"], lev(R["out_CF_con"], k)); tol["nl_CF_con"] = fx["tol"]["out_CF_con"]
    judge(e, tol, "%s modes" % tag)
    return e


# ---- 6: dot product
def dot_product(c, T, slot=0, chain=False):
    """<TL x, y> against <x, AD y>: x over T qv qi ql cfcn and the four sources, y over T qv qi ql cfcn, on is..ie x js..je.  chain:
    convection(1) ; cloud(1) against cloud(2) ; convection(2), x over u v T qv qi ql cfcn (the sources are inside), y over the same"""
    rng = np.random.default_rng(13)
    shp = (c.dims.ntile, c.npz, c.ny + 7, c.nx + 7)
    amp = dict(u=1.0, v=1.0, pt=0.5, q1=1e-4); amp["q%d" % IQI] = 1e-5; amp["q%d" % IQL] = 1e-5
    names = ["pt", "q1", "q%d" % IQI, "q%d" % IQL] + (["u", "v"] if chain else [])
    X = {n: amp.get(n, 1e-3) * rng.standard_normal(shp) for n in TC.all_names(c)}
    Y = {n: rng.standard_normal(shp) / amp.get(n, 1e-3) for n in TC.all_names(c)}
    XC, YC = 0.05 * rng.standard_normal(TC.cshape(c)), rng.standard_normal(TC.cshape(c))
    XS = [s * rng.standard_normal(TC.cshape(c)) for s in (1e-8, 1e-3, 1e-8, 1e-1)]
    D = TC.dom(c)
    TC.put_all(c, T, X)
    c.dy.cloud_cfcn(XC)
    if chain:
        c.dy.convection(slot, TL)
    else:
        c.dy.convection_sources(XS)
    c.dy.cloud(slot, TL)
    lhs = sum(float(np.sum(c.dy.get(n, 1)[D] * Y[n][D])) for n in names) + float(np.sum(c.dy.cloud_cfcn() * YC))
    TC.put_all(c, T, Y)
    c.dy.cloud_cfcn(YC)
    c.dy.cloud(slot, AD)
    if chain:
        c.dy.convection(slot, AD)
    rhs = sum(float(np.sum(c.dy.get(n, 1)[D] * X[n][D])) for n in names) + float(np.sum(c.dy.cloud_cfcn() * XC))
    if not chain:
        sb = c.dy.convection_sources()
        rhs += sum(float(np.sum(sb[n] * XS[m])) for m, n in enumerate(SRC))
    return lhs, rhs


def check_dot_product(c, tag, chain=False, tol=1e-12):
    fx, T, sfc, cl, k = set_fixture(c, tag)
    lhs, rhs = dot_product(c, T, 0, chain)
    res = abs(lhs - rhs) / abs(lhs)
    print("%s dot product%s: %.16e %.16e residual %.1e" % (tag, " of the chain" if chain else "", lhs, rhs, res))
    assert res <= tol, (lhs, rhs)
    return res


# ---- 7: position independence
FIELDS = ("pt", "q1", "q%d" % IQI, "q%d" % IQL)


def forcing(c, fx, k):
    """the fixture's drawn perturbation (fields, cfcn, four sources) and its adjoint forcing (fields, cfcn) as the fields of the case"""
    pk, p00k = CC.pk_of(fx, lev(fx["delp"], k))
    return host_fields(c, fx, k, pk, p00k, False), host_fields(c, fx, k, pk, p00k, True)[:2]


def run_slot(c, slot, T, F, nonlinear=True):
    """what a set slot returns and what its three runs leave on is..ie x js..je: the eight values, the fractions and the switch; the
    tangent's fields and cfcn; the adjoint's fields, cfcn and the four source adjoints it leaves; the qi, ql the nonlinear run wrote back to
    the trajectory and the CF_con it leaves in the slot"""
    (P, cf, src), (PA, cfa) = F
    D = TC.dom(c)
    out, frac, pm = c.dy.cloud_get(slot)
    TC.put_all(c, T, P)
    c.dy.convection_sources(src)
    c.dy.cloud_cfcn(cf)
    c.dy.cloud(slot, TL)
    r = [out[n] for n in OUT8] + [frac[n] for n in FRAC] + [pm.astype(np.float64)] + [c.dy.get(n, 1)[D] for n in FIELDS] + [c.dy.cloud_cfcn()]
    TC.put_all(c, T, PA)
    c.dy.cloud_cfcn(cfa)
    c.dy.cloud(slot, AD)
    r += [c.dy.get(n, 1)[D] for n in FIELDS] + [c.dy.cloud_cfcn()] + [v for v in c.dy.convection_sources().values()]
    if nonlinear:
        TC.put_all(c, T, P)
        c.dy.cloud(slot, NL)
        r += [c.dy.get(n, 0)[D] for n in FIELDS[2:]] + [c.dy.cloud_get(slot, frac=False, pertmod=False)[0]["CF_con"]]
    return r


def results(c, fx, T, sfc, cl, F):
    ensure_created(c, fx)
    TC.put_all(c, T, F[0][0])
    c.dy.convection_set(0, *sfc)
    c.dy.cloud_set(0, *cl)
    return run_slot(c, 0, T, F)


_small = {}


def small_tile(make_small, tag, key):
    """the results of the small tile, which checks 1 to 5 tie to the reference: computed once for a backend and left unchanged"""
    if (key, tag) not in _small:
        fx = fixture(tag)
        small = make_small()
        Ts, ss, cs, ks = placed(small, fx, dealt(small, 0))
        assert set(np.unique(ks)) == set(range(fx["ncol"])), "every column of the fixture is on the small tile"
        rs = results(small, fx, Ts, ss, cs, forcing(small, fx, ks))
        first = np.zeros(fx["ncol"], dtype=np.int64)
        first[ks.ravel()[::-1]] = np.arange(ks.size)[::-1]
        for a in rs:
            a.setflags(write=False)
        _small[(key, tag)] = (rs, first)
    return _small[(key, tag)]


def check_position(make_small, make_cube, tag, layout=2, key=None):
    """a column's set outputs and the results of its tangent, adjoint and nonlinear runs on the six faces, and on their sub-face layout,
    equal those on the small tile: bitwise"""
    fx = fixture(tag)
    lm = fx["lm"]
    rs, first = small_tile(make_small, tag, key)
    c1, c2 = make_cube(1), make_cube(layout)
    T1, s1, cl1, k1 = placed(c1, fx, dealt(c1, 5))
    F1 = forcing(c1, fx, k1)
    r1 = results(c1, fx, T1, s1, cl1, F1)
    win = lambda a: np.ascontiguousarray(np.stack([a[f, ..., j0 - 1:j0 - 1 + c2.nt, i0 - 1:i0 - 1 + c2.nt] for (f, i0, j0) in c2.tiles]))
    wpad = lambda P: {n: pad(c2, win(TC.comp(c1, P[n]))) for n in P}
    (P1, cf1, src1), (PA1, cfa1) = F1
    F2 = ((wpad(P1), win(cf1), [win(v) for v in src1]), (wpad(PA1), win(cfa1)))
    r2 = results(c2, fx, wpad(T1), [win(v) for v in s1], [win(v) for v in cl1], F2)
    assert len(r1) == len(rs) == 8 + 4 + 1 + 5 + 9 + 3
    for m, a in enumerate(r1):
        want = CC.as_on_small(rs, first, k1, lm, m)
        assert np.array_equal(a, want), (m, "a column's result depends on where it lies")
        g = np.zeros_like(a)
        for t, (f, i0, j0) in enumerate(c2.tiles):
            g[f, ..., j0 - 1:j0 - 1 + c2.nt, i0 - 1:i0 - 1 + c2.nt] = r2[m][t]
        assert np.array_equal(g, a), (m, "sub-face tiles gathered != six faces")
    assert all(np.any(rs[m]) for m in range(23, 27)), "the adjoint leaves source adjoints"
    return k1.size


# ---- 7b: columns beyond the first batch
def check_batches(make_small, make_big, tag, read_err, shift=5, full=False, key=None):
    """every column of a case of more columns than a batch holds -- read_err() returns what the library wrote under FV3LM_VERBOSE -- has
    the results of the same fixture column on the small tile, bitwise, in every mode.  full: the case is whole batches exactly (the loop
    bounds); otherwise its last batch is a partial one"""
    fx = fixture(tag)
    rs, first = small_tile(make_small, tag, key)
    read_err()
    c = make_big()
    T, sfc, cl, k = placed(c, fx, dealt(c, shift))
    r = results(c, fx, T, sfc, cl, forcing(c, fx, k))
    nb = CC.batch_size(read_err(), "cloud")
    print("%s %d columns, batch of %d" % (tag, k.size, nb))
    if full:
        assert k.size >= nb and k.size % nb == 0, (k.size, nb)
    else:
        assert nb < k.size and k.size % nb != 0, (k.size, nb)
    for m, a in enumerate(r):
        assert np.array_equal(a, CC.as_on_small(rs, first, k, fx["lm"], m)), (m, "a column's result depends on its batch")
    return k.size, nb


# ---- 7c: a slot set again, two slots in turn
def check_reset_and_slots(make, tag):
    """slot 0 from deal A, slot 1 from deal B (shift 5); run slot 1, then slot 0; the convection slot 0 set again from deal B: a cloud run
    on it is refused until the cloud slot follows; then every result equals that of a fresh single-slot handle given the same deal,
    bitwise, and slot 0 equals slot 1"""
    import pytest
    fx = fixture(tag)
    c = make()
    deals = {}
    for name, shift in (("A", 0), ("B", 5)):
        T, sfc, cl, k = placed(c, fx, dealt(c, shift))
        deals[name] = (T, sfc, cl, forcing(c, fx, k))
    fresh = {}
    for name, (T, sfc, cl, F) in deals.items():
        f = make()
        ensure_created(f, fx, 1)
        TC.put_all(f, T)
        f.dy.convection_set(0, *sfc)
        f.dy.cloud_set(0, *cl)
        fresh[name] = (run_slot(f, 0, T, F, nonlinear=False), f.dy.convection_get(0)[1])
    assert not np.array_equal(fresh["A"][1], fresh["B"][1]), "deal B has to change which columns are active"
    assert not np.array_equal(fresh["A"][0][12], fresh["B"][0][12]), "deal B has to change the switch"

    def same(got, name, what):
        for m, (a, b) in enumerate(zip(got, fresh[name][0])):
            assert np.array_equal(a, b), (what, m)

    def run(slot, name):
        return run_slot(c, slot, deals[name][0], deals[name][3], nonlinear=False)
    ensure_created(c, fx, 2)
    for slot, name in ((0, "A"), (1, "B")):
        TC.put_all(c, deals[name][0])
        c.dy.convection_set(slot, *deals[name][1])
        c.dy.cloud_set(slot, *deals[name][2])
    r1 = run(1, "B")
    same(r1, "B", "slot 1, deal B")
    same(run(0, "A"), "A", "slot 0, deal A, after slot 1 ran")
    TC.put_all(c, deals["B"][0])
    c.dy.convection_set(0, *deals["B"][1])
    for mode in (TL, AD, NL):
        with pytest.raises(Fv3LmError, match="never set"):
            c.dy.cloud(0, mode)
    same(run(1, "B"), "B", "slot 1 after the convection re-set of slot 0")
    c.dy.cloud_set(0, *deals["B"][2])
    assert np.array_equal(c.dy.convection_get(0)[1], fresh["B"][1]), "DOCONVEC of the slot set again"
    r0 = run(0, "B")
    same(r0, "B", "slot 0 set again from deal B")
    for a, b in zip(r0, r1):
        assert np.array_equal(a, b), "after the re-set, slot 0 equals slot 1"


# ---- 8: nothing else moves; the slot keeps what set saw
def check_nothing_else_moves(c, tag):
    fx = fixture(tag)
    T, sfc, cl, k = placed(c, fx, dealt(c))
    rng = np.random.default_rng(23)
    D = TC.dom(c)
    T = {n: a + 0.0 for n, a in T.items()}
    for n in T:      # the halo and the far edge rows carry values of their own
        h = 1e-3 * rng.standard_normal(T[n].shape) * np.abs(T[n]).max(); keep = T[n][D].copy(); T[n] = T[n] + h; T[n][D] = keep
    pk, p00k = CC.pk_of(fx, TC.comp(c, T["delp"]))
    P, cf, src = host_fields(c, fx, k, pk, p00k, False)
    ensure_created(c, fx, 2)
    TC.ensure_created(c, 1)
    TC.put_all(c, T, P)
    c.dy.turbulence_set_diagonals(0, TC.generated(c))
    turb = c.dy.turbulence_get(0)
    c.dy.convection_set(1, *[np.roll(a, 3, axis=-1) for a in sfc])
    c.dy.cloud_set(1, *[np.roll(a, 3, axis=-1) for a in cl])
    other, conv_other = c.dy.cloud_get(1), c.dy.convection_get(1)
    c.dy.convection_set(0, *sfc)
    conv0 = c.dy.convection_get(0)
    before = {(n, w): c.dy.get(n, w) for n in TC.all_names(c) for w in (0, 1)}
    host_in = [a.copy() for a in cl]
    c.dy.cloud_set(0, *cl)
    for (n, w), a in before.items():
        assert np.array_equal(c.dy.get(n, w), a), (n, w, "changed by cloud_set")
    for a, b in zip(cl, host_in):
        assert np.array_equal(a, b), "the host's array was written"
    touched = ("pt", "q1", "q%d" % IQI, "q%d" % IQL)

    def run():
        for n in TC.all_names(c):
            c.dy.put(n, P[n], 1)
        c.dy.convection_sources(src)
        c.dy.cloud_cfcn(cf)
        c.dy.cloud(0, TL)
        return {n: c.dy.get(n, 1) for n in TC.all_names(c)}, c.dy.cloud_cfcn()
    first, cf1 = run()
    for n in TC.all_names(c):
        keep = first[n].copy(); keep[D] = P[n][D]
        assert np.array_equal(keep, P[n]), (n, "halo or far edge rows moved")
        if n not in touched:
            assert np.array_equal(first[n], P[n]), (n, "a field the cloud scheme does not touch")
        assert np.array_equal(c.dy.get(n, 0), T[n])
    def flat(x):
        return [a for y in x for a in (flat(list(y.values())) if isinstance(y, dict) else [y])]
    same = lambda a, b: all(np.array_equal(x, y) for x, y in zip(flat(a), flat(b)))
    assert same(c.dy.cloud_get(1), other), "the other cloud slot changed"
    assert same(c.dy.convection_get(1), conv_other) and same(c.dy.convection_get(0), conv0), "a convection slot changed"
    assert np.array_equal(c.dy.turbulence_get(0), turb), "the turbulence slot changed"
    assert TC.relerr(first["pt"][D], P["pt"][D]) > 1e-6
    # set, step, run: the slot keeps what set saw
    T2, P2 = TC.unit_state(c)
    TC.put_all(c, T2, P2)
    c.dy.step_tl()
    assert not np.array_equal(c.dy.get("delp", 0), T["delp"])
    second, cf2 = run()
    for n in touched:
        assert np.array_equal(second[n], first[n]), (n, "slot 0 followed the resident trajectory")
    assert np.array_equal(cf1, cf2)


def check_untouched_handle(make, tag):
    """a handle that never created the cloud feature steps bitwise like one that created, set and ran it on another state"""
    a, b = make(), make()
    fx = fixture(tag)
    T, P = TC.unit_state(a)
    Tb, sfc, cl, k = placed(b, fx, dealt(b))
    ensure_created(b, fx)
    TC.put_all(b, Tb)
    b.dy.convection_set(0, *sfc)
    b.dy.cloud_set(0, *cl)
    b.dy.cloud(0, TL)
    for c in (a, b):
        TC.put_all(c, T, P)
        c.dy.step_tl()
    for n in TC.all_names(a):
        for w in (0, 1):
            assert np.array_equal(a.dy.get(n, w), b.dy.get(n, w)), (n, w)


# ---- 9: refusals, by message
def check_refusals(make):
    import pytest
    fx = fixture("L20m1")
    c = make(nq=3, npz=20, **case_kw(fx))
    T, sfc, cl, k = placed(c, fx, dealt(c))
    TC.put_all(c, T)
    p, q = c.dy.ras_default_params(12), c.dy.cloud_default_params(12)
    R = lambda m: pytest.raises(Fv3LmError, match=m)
    with R("fv3lm_convection_create first"):
        c.dy.cloud_create(q, IQI, IQL)
    for fn in (lambda: c.dy.cloud_set(0, *cl), lambda: c.dy.cloud(0, TL), lambda: c.dy.cloud_get(0), lambda: c.dy.cloud_cfcn()):
        with R("fv3lm_cloud_create first"):
            fn()
    c.dy.convection_create(2, p, 1); c._conv_slots = 2
    with R("null parameters"):
        c.dy.cloud_create(None, IQI, IQL)
    for i, l in ((1, 3), (2, 4), (0, 2), (3, 1)):
        with R("outside 2..nq"):
            c.dy.cloud_create(q, i, l)
    with R("iqi = iql"):
        c.dy.cloud_create(q, 2, 2)
    bad = c.dy.cloud_default_params(12); bad.r[12] = float("nan")
    with R("not finite"):
        c.dy.cloud_create(bad, IQI, IQL)
    bad = c.dy.cloud_default_params(12); bad.r[56] = 2.0
    with R("only the top-hat PDF is built"):
        c.dy.cloud_create(bad, IQI, IQL)
    c.dy.step_tl()                                    # the handle is not poisoned
    TC.put_all(c, T)
    c.dy.cloud_create(q, IQI, IQL)
    with R("already created"):
        c.dy.cloud_create(q, IQI, IQL)
    with R("convection slot 0 was never set"):
        c.dy.cloud_set(0, *cl)
    c.dy.convection_set(0, *sfc)
    for slot in (-1, 2):
        with R("out of range"):
            c.dy.cloud_set(slot, *cl)
        with R("out of range"):
            c.dy.cloud(slot, TL)
        with R("out of range"):
            c.dy.cloud_get(slot)

    def unset(slot=0):
        for fn in (lambda: c.dy.cloud(slot, TL), lambda: c.dy.cloud_get(slot)):
            with R("never set"):
                fn()
    unset()
    for n in range(5):
        s = list(cl); s[n] = None
        with R("null array"):
            c.dy.cloud_set(0, *s)
    for n in (3, 4):
        for v in (0, 21):
            s = [a.copy() for a in cl]; s[n][0, 1, 2] = v
            with R("outside 1..npz"):
                c.dy.cloud_set(0, *s)
    for n in range(5):
        for v in (float("nan"), float("inf")):
            s = [a.copy() for a in cl]; s[n][(0, 3, 2, 1) if n < 3 else (0, 2, 1)] = v
            with R("not finite"):
                c.dy.cloud_set(0, *s)
    unset()
    c.dy.cloud_set(0, *cl)                    # a good set works ...
    c.dy.cloud(0, TL)
    for mode in (-1, 3):
        with R("bad mode"):
            c.dy.cloud(0, mode)
    s = [a.copy() for a in cl]; s[3][0, 0, 0] = 25
    with R("outside 1..npz"):                # ... and a refusal of the arguments leaves that slot as it was
        c.dy.cloud_set(0, *s)
    c.dy.cloud(0, TL)
    unset(1)
    with R("null array"):
        c.dy.cloud_cfcn(null=True)
    cf = c.dy.cloud_cfcn(); cf[0, 1, 1, 1] = float("nan")
    with R("not finite"):
        c.dy.cloud_cfcn(cf)
    c.dy.convection_set(0, *sfc)              # the convection slot set again: the cloud slot has to follow
    unset()
    c.dy.cloud_set(0, *cl)
    c.dy.cloud(0, AD)
    c.dy.step_tl()                            # nothing above has poisoned the handle


def check_failed_allocation(make):
    """the failed allocation: the feature's arena follows the convection's slot count, and that create is refused before this one can be
    asked; a cloud create after it finds no convection feature"""
    import pytest
    fx = fixture("L20m1")
    c = make(nq=3, npz=20, **case_kw(fx))
    p, q = c.dy.ras_default_params(12), c.dy.cloud_default_params(12)
    with pytest.raises(Fv3LmError, match="allocation of [0-9]+ bytes failed"):
        c.dy.convection_create(2 ** 31 - 1, p, 1)
    with pytest.raises(Fv3LmError, match="fv3lm_convection_create first"):
        c.dy.cloud_create(q, IQI, IQL)
    c.dy.convection_create(1, p, 1)
    c.dy.cloud_create(q, IQI, IQL)


# ---- 10: at size
def check_at_size(c, repeats=3, tol=1e-12):
    T, P = TC.unit_state(c)
    t, j, i = np.meshgrid(np.arange(c.dims.ntile), np.arange(c.ny), np.arange(c.nx), indexing="ij")
    h = i + 2 * j + 3 * t
    pref = c.ak + c.bk * 1.0e5
    icmin = max(1, int(np.count_nonzero(pref < 3000.0)))
    kcbl = np.maximum(icmin + 1, c.npz - 3 - h % 3).astype(np.float64)
    tbot = TC.comp(c, T["pt"])[:, -1]
    sfc = [tbot + 1.5 + 0.1 * (h % 7), np.where(h % 4 == 3, 1.0, 0.0), kcbl]
    delp = TC.comp(c, T["delp"])
    pm = c.opt.ptop + np.cumsum(delp, axis=1) - 0.5 * delp
    tt = TC.comp(c, T["pt"])
    es = 611.2 * np.exp(17.67 * (tt - 273.15) / (tt - 29.65))
    rh = 0.35 + 0.5 * (pm / 1.0e5) ** 2 + 0.05 * (h % 3)[:, None]
    qv = np.where(pm > 1.0e4, rh * 0.622 * es / (pm - 0.378 * es), 3e-6)
    T = dict(T); T["q1"] = pad(c, np.ascontiguousarray(qv))
    w = np.clip((rh - 0.5) / 0.4, 0.0, 1.0) ** 2 * (pm > 1.5e4)
    s = ((h[:, None] + np.arange(c.npz)[None, :, None, None]) % 5) / 5.0
    cl = [6e-4 * w * s, 4e-4 * w * (1.0 - s), 0.6 * w * (1.0 - s), (c.npz - 3 - h % 4).astype(np.float64), (c.npz - 12 + h % 5).astype(np.float64)]
    c.dy.convection_create(1, c.dy.ras_default_params(c.nx), 1)
    c.dy.cloud_create(c.dy.cloud_default_params(c.nx), IQI, IQL)
    TC.put_all(c, T, P)
    c.dy.convection_set(0, *sfc)
    times = []
    for n in range(repeats):
        rec = {}
        for name, fn in (("set", lambda: c.dy.cloud_set(0, *cl)), ("tl", lambda: c.dy.cloud(0, TL)), ("ad", lambda: c.dy.cloud(0, AD))):
            c.dy.profile_begin()
            fn()
            rec[name] = sum(v[1] for v in c.dy.profile_end().values())
        times.append(rec)
    out, frac, pmod = c.dy.cloud_get(0)
    assert all(np.all(np.isfinite(out[n])) for n in OUT8) and all(np.all(np.isfinite(frac[n])) for n in FRAC)
    assert np.any((out["CF_ls"] > 0) & (out["CF_ls"] < 1)) and np.any(out["CF_con"] > 0), "no cloud: the check is empty"
    TC.put_all(c, T, P)
    c.dy.cloud(0, TL)
    assert all(np.all(np.isfinite(c.dy.get(n, 1))) for n in ("pt", "q1", "q%d" % IQI, "q%d" % IQL)) and np.all(np.isfinite(c.dy.cloud_cfcn()))
    lhs, rhs = dot_product(c, T)
    assert abs(lhs - rhs) <= tol * abs(lhs), (lhs, rhs)
    return times, abs(lhs - rhs) / abs(lhs)
