"""Checks of the linearised RAS convection on the device (fv3lm_convection_*; product csrc/convection.h) shared by the host-emulation
(test_emul_convection.py) and the MI355X (test_gpu_convection.py) runs.

The yardstick is tests/golden/convection_ref.npz: soundings at L40, L72 (do_phy_mst = 2) and L20 (do_phy_mst = 1) with what the
reference's own RASE0, RASE0_D, RASE_D and RASE_B, compiled from their own source, returned for them
(tests/golden/make_convection_golden.py); set_ltraj's filters are restated in numpy around those outputs.  The tolerance of an output is
read from the fixture: m x the largest movement of that output, relative to its column maximum, when the reference's THO, QHO are
perturbed by 1e-15, where m is the largest number of cloud types that fired in a column of the set (the device's exp / sqrt / pow may
differ from the host's by an ulp once per cloud type), floor 1e-12.  Every column of the fixture is compared."""
import os
import numpy as np
import turbulence_checks as TC
from fv3_jedi_linearmodel_amd._lib import Dycore, Fv3LmError

NL, TL, AD = 0, 1, 2
FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "convection_ref.npz")
SETN = list(Dycore.SET_NAMES)
SRC = list(Dycore.SRC_NAMES)
FOUR = ["pt", "q1", "u", "v"]
LD = np.longdouble
_fix = {}


def fixture(lm):
    if lm not in _fix:
        z = np.load(FIX)
        pre = "L%d_" % lm
        f = {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}
        f["ref"] = {k[4:]: f.pop(k) for k in list(f) if k.startswith("ref_")}
        m = int(f["ref"]["fired"].max())
        f["tol"] = {str(n): max(m * float(s), 1e-12) for n, s in zip(f.pop("spread_names"), f.pop("spread"))}
        f["m"], f["mst"], f["icmin"] = m, int(f["mst"]), int(f["icmin"])
        f["dt"], f["ptop"], f["kappa"], f["p00"] = float(z["dt"]), float(z["ptop"]), float(z["kappa"]), float(z["p00"])
        f["X"] = f["X"].astype(np.float64); f["Y"] = f["Y"].astype(np.float64)
        f["ncol"] = f["T"].shape[1]
        f["table"] = z["table_every_100th"]
        assert list(z["constant_names"]) == ["CP", "ALHL", "GRAV", "RGAS", "H2OMW", "AIRMW", "VIREPS", "P00", "KAPPA"]
        f["constants"] = z["constants"]
        _fix[lm] = f
    return _fix[lm]


def case_kw(fx):
    """how a case is built for the fixture: its levels and ptop"""
    return dict(levels=(fx["ak"], fx["bk"]), ptop=fx["ptop"])


def dealt(c, shift=0):
    n = c.dims.ntile * c.ny * c.nx
    return (np.arange(n) + shift).reshape(c.dims.ntile, c.ny, c.nx)


def pad(c, a):
    w = [(0, 0)] * (a.ndim - 2) + [(TC.NG, 4), (TC.NG, 4)]
    return np.ascontiguousarray(np.pad(a, w, mode="edge"))


def lev(a, k):
    """[lm, ncol] -> [ntile, lm, ny, nx]"""
    return np.ascontiguousarray(np.moveaxis(a[:, k], 0, 1))


def pk_of(fx, delp):
    """compute_pressures' pk of compact delp [ntile, lm, ny, nx], in extended precision, and p00^kappa"""
    pe = np.concatenate([np.full_like(delp[:, :1], fx["ptop"], dtype=LD), LD(fx["ptop"]) + np.cumsum(delp.astype(LD), axis=1)], axis=1)
    k = LD(fx["kappa"])
    pk = (pe[:, 1:] ** k - pe[:, :-1] ** k) / (k * (np.log(pe[:, 1:]) - np.log(pe[:, :-1])))
    return np.asarray(pk, dtype=np.float64), float(LD(fx["p00"]) ** k)


def placed(c, fx, col):
    """the fixture's columns on the case: padded trajectory (pt = temperature, q1 = qv, q2.. small) and the compact surface fields"""
    k = col % fx["ncol"]
    T = dict(u=pad(c, lev(fx["u"], k)), v=pad(c, lev(fx["v"], k)), pt=pad(c, lev(fx["T"], k)), delp=pad(c, lev(fx["delp"], k)), q1=pad(c, lev(fx["qv"], k)))
    rng = np.random.default_rng(41)
    for n in range(1, c.nq):
        T["q%d" % (n + 1)] = 1e-4 * (n + rng.random(T["u"].shape))
    sfc = [np.ascontiguousarray(fx[n][k]) for n in ("ts", "frland", "kcbl")]
    return T, sfc, k


def ensure_created(c, fx, nslots=1):
    if getattr(c, "_conv_slots", 0) == 0:
        p = c.dy.ras_default_params(12)
        assert np.array_equal(np.array(p.r[:]), fx["rpar"]), "ras_default_params: the set of create :120-148"
        c.dy.convection_create(nslots, p, fx["mst"])
        c._conv_slots = nslots
    assert c._conv_slots >= nslots


def set_fixture(c, lm, shift=0, slot=0, nslots=1):
    fx = fixture(lm)
    assert abs(c.dims.dt - fx["dt"]) == 0.0 and c.opt.ptop == fx["ptop"] and np.array_equal(c.ak, fx["ak"])
    T, sfc, k = placed(c, fx, dealt(c, shift))
    ensure_created(c, fx, nslots)
    TC.put_all(c, T)
    c.dy.convection_set(slot, *sfc)
    return fx, T, sfc, k


def colmax(a):
    s = np.abs(a).max(axis=1)
    return np.where(s > 0, s, 1.0)


def err(got, ref):
    """largest error over all points relative to the column maximum of the reference"""
    return float(np.max(np.abs(got - ref).max(axis=1) / colmax(ref)))


def judge(e, tol, what, verbose=True):
    if verbose:
        print(what + ": " + " ".join("%s %.1e/%.1e" % (n, e[n], tol[n]) for n in e))
    bad = {n: (e[n], tol[n]) for n in e if not e[n] <= tol[n]}
    assert not bad, (what, bad)


# ---- 1: set against the reference
def check_set(c, lm):
    fx, T, sfc, k = set_fixture(c, lm)
    assert set(np.unique(k)) == set(range(fx["ncol"])), "every column of the fixture is on the case"
    out, dc, jac = c.dy.convection_get(0)
    e = {"set_" + n: err(out[n], lev(fx["ref"]["set_" + n], k)) for n in SETN}
    ok = fx["ref"]["heat_ok"][k] == 1      # the Jacobian column exists where the heating-rate filter let the column through
    for m, n in enumerate(("jac_H_pert", "jac_M_pert")):
        ref = lev(fx["ref"][n], k) * ok[:, None]
        e[n] = err(jac[m], ref)
    judge(e, fx["tol"], "L%d set" % lm)
    assert np.array_equal(dc, fx["ref"]["doconvec"][k]), "DOCONVEC"
    tbl, cst = c.dy.convection_table()
    assert np.array_equal(tbl[::100], fx["table"]), "the device's table against every 100th entry of qsat_util.F90's ESINIT"
    assert np.array_equal(cst, fx["constants"]), ("the MAPL8 constants as the reference's wrapper saw them", cst, fx["constants"])
    assert 0 < dc.sum() < dc.size
    return e


# ---- 2, 4: the three modes against RASE_D, RASE_B and RASE
def perturbation(c, fx, k, pk, p00k, adjoint):
    """the fixture's drawn perturbation (of theta, qv, u, v) or adjoint forcing as the fields of the case: the theta conversion restated"""
    Z = fx["Y"] if adjoint else fx["X"]
    rng = np.random.default_rng(7)
    shp = (c.dims.ntile, c.npz, c.ny + 7, c.nx + 7)
    P = {n: 1e-3 * rng.standard_normal(shp) for n in TC.all_names(c)}
    D = TC.dom(c)
    th = lev(Z[0], k)
    P["pt"][D] = th * p00k / pk if adjoint else th * pk / p00k
    P["q1"][D] = lev(Z[1], k); P["u"][D] = lev(Z[2], k); P["v"][D] = lev(Z[3], k)
    return P


def check_modes(c, lm):
    fx, T, sfc, k = set_fixture(c, lm)
    D = TC.dom(c)
    pk, p00k = pk_of(fx, TC.comp(c, T["delp"]))
    act = fx["ref"]["doconvec"][k] == 1
    stable = ~act
    e = {}
    # tangent
    P = perturbation(c, fx, k, pk, p00k, False)
    TC.put_all(c, T, P)
    c.dy.convection(0, TL)
    got = {n: c.dy.get(n, 1) for n in TC.all_names(c)}
    src = c.dy.convection_sources()
    for n in FOUR:
        g = got[n][D] * (p00k / pk if n == "pt" else 1.0)
        ref = lev(fx["ref"]["tl_" + n], k)
        e["tl_" + n] = err(g * act[:, None], ref * act[:, None])
        assert np.array_equal(np.where(stable[:, None], got[n][D], 0.0), np.where(stable[:, None], P[n][D], 0.0)), (n, "a stable column moved")
    for n in SRC:
        e["tl_" + n] = err(src[n], lev(fx["ref"]["tl_" + n], k) * act[:, None])
        assert not np.any(np.where(stable[:, None], src[n], 0.0)), (n, "a source in a stable column")
    for n in TC.all_names(c):
        keep = got[n].copy(); keep[D] = P[n][D]
        assert np.array_equal(keep, P[n]) and (n in FOUR or np.array_equal(got[n], P[n])), (n, "moved outside is..ie x js..je, or a field convection does not touch")
        assert np.array_equal(c.dy.get(n, 0), T[n]), (n, "the trajectory moved in the tangent run")
    # adjoint
    P = perturbation(c, fx, k, pk, p00k, True)
    TC.put_all(c, T, P)
    c.dy.convection_sources([lev(fx["Y"][4 + m], k) for m in range(4)])
    c.dy.convection(0, AD)
    got = {n: c.dy.get(n, 1) for n in TC.all_names(c)}
    for n in FOUR:
        g = got[n][D] * (pk / p00k if n == "pt" else 1.0)
        e["ad_" + n] = err(g * act[:, None], lev(fx["ref"]["ad_" + n], k) * act[:, None])
        assert np.array_equal(np.where(stable[:, None], got[n][D], 0.0), np.where(stable[:, None], P[n][D], 0.0)), (n, "a stable column moved")
    after = c.dy.convection_sources()
    assert not any(np.any(after[n]) for n in SRC), "the incoming adjoints of the sources are consumed and cleared"
    # nonlinear: RASE on the trajectory, written back
    TC.put_all(c, T, P)
    c.dy.convection(0, NL)
    for n in FOUR:
        g = c.dy.get(n, 0)
        keep = g.copy(); keep[D] = T[n][D]
        assert np.array_equal(keep, T[n]), (n, "trajectory moved outside is..ie x js..je")
        x = g[D] * (p00k / pk if n == "pt" else 1.0)
        ref = lev(fx["ref"]["nl_" + n], k)
        e["nl_" + n] = err(x * act[:, None], ref * act[:, None])
        assert np.array_equal(np.where(stable[:, None], g[D], 0.0), np.where(stable[:, None], T[n][D], 0.0)), (n, "a stable column moved")
        assert np.array_equal(c.dy.get(n, 1), P[n]), (n, "the perturbation moved in the nonlinear run")
    assert np.array_equal(c.dy.get("delp", 0), T["delp"])
    judge(e, fx["tol"], "L%d modes" % lm)
    return e


# ---- 3: dot product
def dot_product(c, T, sfc, slot=0):
    """<TL x, y> against <x, AD y> over the eight fields (u v pt q1 and the four sources) on is..ie x js..je"""
    rng = np.random.default_rng(13)
    shp = (c.dims.ntile, c.npz, c.ny + 7, c.nx + 7)
    amp = dict(u=1.0, v=1.0, pt=0.5, q1=1e-4)
    X = {n: amp.get(n, 1e-3) * rng.standard_normal(shp) for n in TC.all_names(c)}
    Y = {n: rng.standard_normal(shp) / amp.get(n, 1e-3) for n in TC.all_names(c)}
    YS = [s * rng.standard_normal(TC.cshape(c)) for s in (1e4, 1e1, 1e4, 1.0)]
    D = TC.dom(c)
    TC.put_all(c, T, X)
    c.dy.convection(slot, TL)
    src = c.dy.convection_sources()
    lhs = sum(float(np.sum(c.dy.get(n, 1)[D] * Y[n][D])) for n in FOUR) + sum(float(np.sum(src[n] * YS[m])) for m, n in enumerate(SRC))
    TC.put_all(c, T, Y)
    c.dy.convection_sources(YS)
    c.dy.convection(slot, AD)
    rhs = sum(float(np.sum(c.dy.get(n, 1)[D] * X[n][D])) for n in FOUR)
    return lhs, rhs


def check_dot_product(c, lm, tol=1e-12):
    fx, T, sfc, k = set_fixture(c, lm)
    lhs, rhs = dot_product(c, T, sfc)
    res = abs(lhs - rhs) / abs(lhs)
    print("L%d dot product: %.16e %.16e residual %.1e" % (lm, lhs, rhs, res))
    assert res <= tol, (lhs, rhs)
    return res


# ---- 5: position independence
def forcing(c, fx, k):
    """the fixture's drawn perturbation, its adjoint forcing and the four source adjoints (Y[4:8]) as the fields of the case"""
    pk, p00k = pk_of(fx, lev(fx["delp"], k))
    return perturbation(c, fx, k, pk, p00k, False), perturbation(c, fx, k, pk, p00k, True), [lev(fx["Y"][4 + m], k) for m in range(4)]


def run_slot(c, slot, T, F, nonlinear=True):
    """what a set slot returns and what its three runs leave on is..ie x js..je: the set outputs and the Jacobian column; the tangent's
    fields and sources; the adjoint's fields and the consumed sources; the trajectory the nonlinear run wrote back.  -> (list, doconvec)"""
    P, PA, YS = F
    D = TC.dom(c)
    out, dc, jac = c.dy.convection_get(slot)
    TC.put_all(c, T, P)
    c.dy.convection(slot, TL)
    r = [out[n] for n in SETN] + [jac[0], jac[1]] + [c.dy.get(n, 1)[D] for n in FOUR] + [v for v in c.dy.convection_sources().values()]
    TC.put_all(c, T, PA)
    c.dy.convection_sources(YS)
    c.dy.convection(slot, AD)
    r += [c.dy.get(n, 1)[D] for n in FOUR] + [v for v in c.dy.convection_sources().values()]
    if nonlinear:
        TC.put_all(c, T, P)
        c.dy.convection(slot, NL)
        r += [c.dy.get(n, 0)[D] for n in FOUR]
    return r, dc


def results(c, fx, T, sfc, F):
    ensure_created(c, fx)
    TC.put_all(c, T, F[0])
    c.dy.convection_set(0, *sfc)
    return run_slot(c, 0, T, F)


_small = {}


def small_tile(make_small, lm, key):
    """the results of the small tile, which checks 1, 2 and 4 tie to the reference: computed once for a backend and left unchanged"""
    if (key, lm) not in _small:
        fx = fixture(lm)
        small = make_small()
        Ts, ss, ks = placed(small, fx, dealt(small, 0))
        assert set(np.unique(ks)) == set(range(fx["ncol"])), "every column of the fixture is on the small tile"
        rs, ds = results(small, fx, Ts, ss, forcing(small, fx, ks))
        first = np.zeros(fx["ncol"], dtype=np.int64)
        first[ks.ravel()[::-1]] = np.arange(ks.size)[::-1]
        for a in rs:
            a.setflags(write=False)
        _small[(key, lm)] = (rs, ds, first)
    return _small[(key, lm)]


def as_on_small(rs, first, k, lm, m):
    """result m of the small tile at the columns k of another case"""
    return np.moveaxis(np.moveaxis(rs[m], 1, -1).reshape(-1, lm)[first[k]], -1, 1)


def check_position(make_small, make_cube, lm, layout=2, key=None):
    """a column's set outputs and the results of its tangent, adjoint and nonlinear runs on the six faces, and on their sub-face layout,
    equal those on the small tile: bitwise"""
    fx = fixture(lm)
    rs, ds, first = small_tile(make_small, lm, key)
    c1, c2 = make_cube(1), make_cube(layout)
    T1, s1, k1 = placed(c1, fx, dealt(c1, 5))
    F1 = forcing(c1, fx, k1)
    r1, d1 = results(c1, fx, T1, s1, F1)
    win = lambda a: np.ascontiguousarray(np.stack([a[f, ..., j0 - 1:j0 - 1 + c2.nt, i0 - 1:i0 - 1 + c2.nt] for (f, i0, j0) in c2.tiles]))
    T2 = {n: pad(c2, win(TC.comp(c1, T1[n]))) for n in T1}
    F2 = tuple({n: pad(c2, win(TC.comp(c1, P[n]))) for n in P} for P in F1[:2]) + ([win(v) for v in F1[2]],)
    r2, d2 = results(c2, fx, T2, [win(v) for v in s1], F2)
    assert len(r1) == len(rs) == 6 + 2 + 8 + 8 + 4
    for m, a in enumerate(r1):
        want = as_on_small(rs, first, k1, lm, m)
        assert np.array_equal(a, want), (m, "a column's result depends on where it lies")
        g = np.zeros_like(a)
        for t, (f, i0, j0) in enumerate(c2.tiles):
            g[f, ..., j0 - 1:j0 - 1 + c2.nt, i0 - 1:i0 - 1 + c2.nt] = r2[m][t]
        assert np.array_equal(g, a), (m, "sub-face tiles gathered != six faces")
    assert np.array_equal(d1, ds.ravel()[first[k1]])
    assert not any(np.any(rs[m]) for m in range(20, 24)), "the adjoint consumes and clears its sources"
    return d1.size


def batch_size(err, scheme):
    """the columns of a batch as the library reports them at create under FV3LM_VERBOSE"""
    import re
    m = re.findall(r"fv3lm: %s arena .* batch of (\d+) columns" % scheme, err)
    assert m, ("no 'batch of %d columns' line of the " + scheme + " arena: is FV3LM_VERBOSE set?", err[-500:])
    return int(m[-1])


# ---- 5b: columns beyond the first batch
def check_batches(make_small, make_big, lm, read_err, shift=5, full=False, key=None):
    """every column of a case of more columns than a batch holds -- read_err() returns what the library wrote under FV3LM_VERBOSE -- has
    the results of the same fixture column on the small tile, bitwise, in every mode.  full: the case is whole batches exactly (the loop
    bounds); otherwise the active list itself has to need a second, partial batch"""
    fx = fixture(lm)
    rs, ds, first = small_tile(make_small, lm, key)
    read_err()
    c = make_big()
    T, sfc, k = placed(c, fx, dealt(c, shift))
    r, dc = results(c, fx, T, sfc, forcing(c, fx, k))
    nb = batch_size(read_err(), "convection")
    nactive = int(dc.sum())
    print("L%d %d columns, %d active, batch of %d" % (lm, dc.size, nactive, nb))
    if full:
        assert dc.size >= nb and dc.size % nb == 0, (dc.size, nb)
    else:
        assert nb < dc.size and dc.size % nb != 0, (dc.size, nb)
        assert nactive > nb and nactive % nb != 0, (nactive, nb, "the active list fits one batch, or fills whole batches: the case tests no later batch")
    for m, a in enumerate(r):
        assert np.array_equal(a, as_on_small(rs, first, k, lm, m)), (m, "a column's result depends on its batch")
    assert np.array_equal(dc, ds.ravel()[first[k]])
    return dc.size, nactive, nb


# ---- 5c: a slot set again, two slots in turn
def check_reset_and_slots(make, lm):
    """slot 0 from deal A, slot 1 from deal B (shift 5: other columns active, as many); run slot 1, then slot 0; slot 0 set again from deal
    B and run, and once more from deal C (shift 24: one more active): every result -- the set outputs, DOCONVEC, the Jacobian column,
    tangent and adjoint -- equals that of a fresh single-slot handle given the same deal, bitwise"""
    fx = fixture(lm)
    c = make()
    deals = {}
    for name, shift in (("A", 0), ("B", 5), ("C", 24)):
        T, sfc, k = placed(c, fx, dealt(c, shift))
        deals[name] = (T, sfc, forcing(c, fx, k))
    fresh = {}
    for name, (T, sfc, F) in deals.items():
        f = make()
        ensure_created(f, fx, 1)
        TC.put_all(f, T)
        f.dy.convection_set(0, *sfc)
        fresh[name] = run_slot(f, 0, T, F, nonlinear=False)
    dA, dB = fresh["A"][1], fresh["B"][1]
    assert not np.array_equal(dA, dB) and 0 < dB.sum() < dB.size, "deal B has to change which columns are active"
    assert fresh["C"][1].sum() != dB.sum(), "deal C has to change how many are"
    assert np.any((fresh["A"][0][6] != 0) & (dB == 0)[:, None]), "deal A leaves a Jacobian column where deal B has none: what a re-set has to clear"

    def same(got, name, what):
        for m, (a, b) in enumerate(zip(got[0], fresh[name][0])):
            assert np.array_equal(a, b), (what, m)
        assert np.array_equal(got[1], fresh[name][1]), (what, "DOCONVEC")
    ensure_created(c, fx, 2)
    for slot, name in ((0, "A"), (1, "B")):
        TC.put_all(c, deals[name][0])
        c.dy.convection_set(slot, *deals[name][1])
    r1 = run_slot(c, 1, deals["B"][0], deals["B"][2], nonlinear=False)
    same(r1, "B", "slot 1, deal B")
    same(run_slot(c, 0, deals["A"][0], deals["A"][2], nonlinear=False), "A", "slot 0, deal A, after slot 1 ran")
    TC.put_all(c, deals["B"][0])
    c.dy.convection_set(0, *deals["B"][1])
    r0 = run_slot(c, 0, deals["B"][0], deals["B"][2], nonlinear=False)
    same(r0, "B", "slot 0 set again from deal B")
    same(run_slot(c, 1, deals["B"][0], deals["B"][2], nonlinear=False), "B", "slot 1 after the re-set of slot 0")
    for a, b in zip(r0[0], r1[0]):
        assert np.array_equal(a, b), "after the re-set, slot 0 equals slot 1"
    TC.put_all(c, deals["C"][0])
    c.dy.convection_set(0, *deals["C"][1])
    same(run_slot(c, 0, deals["C"][0], deals["C"][2], nonlinear=False), "C", "slot 0 set a third time, from deal C with another count of active columns")


# ---- 6: nothing else moves; the slot keeps what set saw
def check_nothing_else_moves(c, lm):
    fx = fixture(lm)
    T, sfc, k = placed(c, fx, dealt(c))
    rng = np.random.default_rng(23)
    D = TC.dom(c)
    T = {n: a + 0.0 for n, a in T.items()}
    for n in T:      # the halo and the far edge rows carry values of their own
        h = 1e-3 * rng.standard_normal(T[n].shape) * np.abs(T[n]).max(); keep = T[n][D].copy(); T[n] = T[n] + h; T[n][D] = keep
    pk, p00k = pk_of(fx, TC.comp(c, T["delp"]))
    P = perturbation(c, fx, k, pk, p00k, False)
    ensure_created(c, fx, 2)
    TC.ensure_created(c, 1)
    TC.put_all(c, T, P)
    c.dy.turbulence_set_diagonals(0, TC.generated(c))
    turb = c.dy.turbulence_get(0)
    shifted = [np.roll(a, 3, axis=-1) for a in sfc]
    c.dy.convection_set(1, *shifted)
    other = c.dy.convection_get(1)
    before = {(n, w): c.dy.get(n, w) for n in TC.all_names(c) for w in (0, 1)}
    sfc_in = [a.copy() for a in sfc]
    c.dy.convection_set(0, *sfc)
    for (n, w), a in before.items():
        assert np.array_equal(c.dy.get(n, w), a), (n, w, "changed by convection_set")
    for a, b in zip(sfc, sfc_in):
        assert np.array_equal(a, b), "the host's array was written"
    c.dy.convection(0, TL)
    first = {n: c.dy.get(n, 1) for n in TC.all_names(c)}
    src1 = c.dy.convection_sources()
    for n in TC.all_names(c):
        keep = first[n].copy(); keep[D] = P[n][D]
        assert np.array_equal(keep, P[n]), (n, "halo or far edge rows moved")
        if n not in FOUR:
            assert np.array_equal(first[n], P[n]), (n, "a field convection does not touch")
        assert np.array_equal(c.dy.get(n, 0), T[n])
    o1 = c.dy.convection_get(1)
    assert all(np.array_equal(o1[0][n], other[0][n]) for n in SETN) and np.array_equal(o1[1], other[1]) and np.array_equal(o1[2], other[2]), "the other slot changed"
    assert np.array_equal(c.dy.turbulence_get(0), turb), "the turbulence slot changed"
    # set, step, run: the slot keeps what set saw
    T2, P2 = TC.unit_state(c)
    TC.put_all(c, T2, P2)
    c.dy.step_tl()
    assert not np.array_equal(c.dy.get("delp", 0), T["delp"])
    for n in TC.all_names(c):
        c.dy.put(n, P[n], 1)
    c.dy.convection(0, TL)
    src2 = c.dy.convection_sources()
    for n in FOUR:
        assert np.array_equal(c.dy.get(n, 1), first[n]), (n, "slot 0 followed the resident trajectory")
    assert all(np.array_equal(src1[n], src2[n]) for n in SRC)
    assert TC.relerr(first["pt"][D], P["pt"][D]) > 1e-6


def check_untouched_handle(make):
    """a handle that never called fv3lm_convection_create steps bitwise like one that created, set and ran convection on another state"""
    a, b = make(), make()
    fx = fixture(b.npz)
    T, P = TC.unit_state(a)
    Tb, sfc, k = placed(b, fx, dealt(b))
    ensure_created(b, fx)
    TC.put_all(b, Tb)
    b.dy.convection_set(0, *sfc)
    b.dy.convection(0, TL)
    for c in (a, b):
        TC.put_all(c, T, P)
        c.dy.step_tl()
    for n in TC.all_names(a):
        for w in (0, 1):
            assert np.array_equal(a.dy.get(n, w), b.dy.get(n, w)), (n, w)


# ---- 7: refusals, by message
def check_refusals(make):
    import pytest
    fx = fixture(20)
    c = make(nq=2, npz=20, **case_kw(fx))
    T, sfc, k = placed(c, fx, dealt(c))
    TC.put_all(c, T)
    p = c.dy.ras_default_params(12)
    R = lambda m: pytest.raises(Fv3LmError, match=m)
    with R("fv3lm_convection_create first"):
        c.dy.convection_set(0, *sfc)
    with R("fv3lm_convection_create first"):
        c.dy.convection(0, TL)
    with R("fv3lm_convection_create first"):
        c.dy.convection_sources()
    for ns in (0, -1):
        with R("nslots < 1"):
            c.dy.convection_create(ns, p, 1)
    for mst in (0, 3):
        with R("do_phy_mst outside 1..2"):
            c.dy.convection_create(1, p, mst)
    with R("null parameters"):
        c.dy.convection_create(1, None, 1)
    bad = c.dy.ras_default_params(12); bad.r[4] = float("inf")
    with R("not finite"):
        c.dy.convection_create(1, bad, 1)
    c0 = make(nq=0, npz=20, **case_kw(fx))
    with R("nq < 1"):
        c0.dy.convection_create(1, p, 1)
    with R("fv3lm_convection_create first"):
        c.dy.convection_table()
    with R("allocation of [0-9]+ bytes failed"):      # a request no machine can meet: refused, what was allocated goes back ...
        c.dy.convection_create(2 ** 31 - 1, p, 1)
    with R("fv3lm_convection_create first"):         # ... nothing is left created ...
        c.dy.convection_set(0, *sfc)
    c.dy.step_tl()                                    # ... and the handle is not poisoned: it steps, and the good create below works
    TC.put_all(c, T)
    c.dy.convection_create(2, p, 1); c._conv_slots = 2
    with R("already created"):
        c.dy.convection_create(1, p, 1)

    def unset(slot=0):
        for fn in (lambda: c.dy.convection(slot, TL), lambda: c.dy.convection_get(slot)):
            with R("never set"):
                fn()
    for slot in (-1, 2):
        with R("out of range"):
            c.dy.convection_set(slot, *sfc)
        with R("out of range"):
            c.dy.convection(slot, TL)
    for n in range(3):
        s = list(sfc); s[n] = None
        with R("null array"):
            c.dy.convection_set(0, *s)
    for kc in (fx["icmin"], 21, 0):
        s = [a.copy() for a in sfc]; s[2][0, 1, 2] = kc
        with R("kcbl = .* outside ICMIN\\+1 .. npz"):
            c.dy.convection_set(0, *s)
    for n in range(3):
        for v in (float("nan"), float("inf")):
            s = [a.copy() for a in sfc]; s[n][0, 2, 1] = v
            with R("not finite"):
                c.dy.convection_set(0, *s)
    Tn = dict(T)
    q = T["q1"].copy(); q[0, 3, TC.NG + 2, TC.NG + 1] = float("nan"); Tn["q1"] = q
    TC.put_all(c, Tn)
    with R("not finite in the resident trajectory"):
        c.dy.convection_set(0, *sfc)
    TC.put_all(c, T)
    unset()
    c.dy.convection_set(0, *sfc)             # a good set works ...
    c.dy.convection(0, TL)
    for mode in (-1, 3):
        with R("bad mode"):
            c.dy.convection(0, mode)
    s = [a.copy() for a in sfc]; s[2][0, 0, 0] = 25
    with R("outside ICMIN"):                 # ... and a refusal of the arguments leaves that slot as it was
        c.dy.convection_set(0, *s)
    c.dy.convection(0, TL)
    unset(1)
    with R("null array"):
        c.dy.convection_sources([None] * 4)
    src = c.dy.convection_sources()
    src["CNV_MFD"][0, 1, 1, 1] = float("nan")
    with R("not finite"):
        c.dy.convection_sources(src)
    # a handle without ak, bk
    from fv3_jedi_linearmodel_amd._lib import Dycore as D_
    import ctypes as C
    h = C.c_void_p()
    mp = (C.POINTER(C.c_double) * len(c.dy._keep))(*[a.ctypes.data_as(C.POINTER(C.c_double)) for a in c.dy._keep])
    phis = np.ascontiguousarray(c.phis, dtype=np.float64)
    rc = c.lib.L.fv3lm_create(C.byref(h), C.byref(c.dims), C.byref(c.opt), mp, c.da_min, c.da_min_c, phis.ctypes.data_as(C.POINTER(C.c_double)), None, None)
    assert rc == 0, c.lib.err()
    c.lib.L.fv3lm_convection_create.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    assert c.lib.L.fv3lm_convection_create(h, 1, C.byref(p), 1) != 0 and "no ak, bk" in c.lib.err()
    c.lib.L.fv3lm_destroy(h)
    c.dy.step_tl()                           # nothing above has poisoned the handle


# ---- 8: at size
def check_at_size(c, repeats=3, tol=1e-12):
    T, P = TC.unit_state(c)
    t, j, i = np.meshgrid(np.arange(c.dims.ntile), np.arange(c.ny), np.arange(c.nx), indexing="ij")
    h = i + 2 * j + 3 * t
    pref = c.ak + c.bk * 1.0e5
    icmin = max(1, int(np.count_nonzero(pref < 3000.0)))
    kcbl = np.maximum(icmin + 1, c.npz - 3 - h % 3).astype(np.float64)
    tbot = TC.comp(c, T["pt"])[:, -1]
    sfc = [tbot + 1.5 + 0.1 * (h % 7), np.where(h % 4 == 3, 1.0, 0.0), kcbl]
    # a moist, conditionally unstable lower troposphere on the harness state: qv from a relative humidity profile of the state's own T, p
    delp = TC.comp(c, T["delp"])
    pm = c.opt.ptop + np.cumsum(delp, axis=1) - 0.5 * delp
    tt = TC.comp(c, T["pt"])
    es = 611.2 * np.exp(17.67 * (tt - 273.15) / (tt - 29.65))
    qv = np.where(pm > 1.0e4, (0.35 + 0.5 * (pm / 1.0e5) ** 2 + 0.05 * (h % 3)[:, None]) * 0.622 * es / (pm - 0.378 * es), 3e-6)
    T = dict(T); T["q1"] = pad(c, np.ascontiguousarray(qv))
    p = c.dy.ras_default_params(c.nx)
    c.dy.convection_create(1, p, 1)
    TC.put_all(c, T, P)
    times = []
    for n in range(repeats):
        rec = {}
        for name, fn in (("set", lambda: c.dy.convection_set(0, *sfc)), ("tl", lambda: c.dy.convection(0, TL)), ("ad", lambda: c.dy.convection(0, AD))):
            c.dy.profile_begin()
            fn()
            rec[name] = sum(v[1] for v in c.dy.profile_end().values())
        times.append(rec)
    out, dc, jac = c.dy.convection_get(0)
    assert all(np.all(np.isfinite(out[n])) for n in SETN) and np.all(np.isfinite(jac))
    TC.put_all(c, T, P)
    c.dy.convection(0, TL)
    assert all(np.all(np.isfinite(c.dy.get(n, 1))) for n in FOUR) and all(np.all(np.isfinite(v)) for v in c.dy.convection_sources().values())
    assert dc.sum() > 0, "no column convects: the check is empty"
    lhs, rhs = dot_product(c, T, sfc)
    assert abs(lhs - rhs) <= tol * abs(lhs), (lhs, rhs)
    return times, int(dc.sum()), dc.size, abs(lhs - rhs) / abs(lhs)
