"""Checks of BL_DRIVER on the device (fv3lm_turbulence_set_driver; product csrc/bldriver.h) shared by the host-emulation
(test_emul_bl_driver.py) and the MI355X (test_gpu_bl_driver.py) runs.

The yardstick is tests/golden/bl_driver_ref.npz: columns at L72, L127 and L20 with what the reference's own BL_DRIVER, compiled from its
own source, returned for them (tests/golden/make_bl_driver_golden.py).  The tolerance of an output is read from the fixture: 4 x the
largest movement of that output, relative to its column maximum, when the reference's inputs are perturbed by 1e-15 (a few ulp, what
the device's pow / exp / log / sqrt may differ by from the host's; the factor 4 because such differences enter at each of the four or
five chained intrinsic evaluations, not once at the input), floor 1e-12.  Every column of the fixture is compared."""
import os
import numpy as np
import turbulence_checks as TC
import turbulence_oracle as TO
from turbulence_oracle import NL, TL, AD
from fv3_jedi_linearmodel_amd._lib import Dycore, Fv3LmError

FIX = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bl_driver_ref.npz")
RAW = list(Dycore.RAW_NAMES)
SFC = list(Dycore.SFC_NAMES)
_fix = {}


def fixture(lm):
    if lm not in _fix:
        z = np.load(FIX)
        assert list(z["outputs"]) == RAW and list(z["sfc"]) == SFC
        f = {k: z["L%d_%s" % (lm, k)] for k in ["delp", "T", "u", "v", "qv", "qi", "ql"] + SFC}
        f["out"] = {k: z["L%d_out_%s" % (lm, k)] for k in RAW}
        f["tol"] = {k: max(4.0 * float(s), 1e-12) for k, s in zip(RAW, z["L%d_spread" % lm])}
        f["rpar"], f["ipar"], f["dt"] = z["L%d_rpar" % lm], z["L%d_ipar" % lm], float(z["dt"])
        f["ncol"] = f["delp"].shape[1]
        assert abs(float(z["kappa"]) - 2.0 / 7.0) == 0.0 and float(z["ptop"]) == 1.0
        _fix[lm] = f
    return _fix[lm]


def params(c, fx):
    p = c.dy.bl_default_params(int(fx["ipar"][0]))
    assert np.array_equal(np.array(p.r[:]), fx["rpar"]) and np.array_equal(np.array(p.i[:]), fx["ipar"]), "the documented default set"
    return p


def dealt(c, shift=0):
    """column of the fixture at every compact point [ntile, ny, nx]: dealt cyclically"""
    n = c.dims.ntile * c.ny * c.nx
    return (np.arange(n) + shift).reshape(c.dims.ntile, c.ny, c.nx)


def pad(c, a):
    """compact [ntile, (nk,) ny, nx] -> padded plane, the halo filled with the nearest column (finite, never read by the unit)"""
    w = [(0, 0)] * (a.ndim - 2) + [(TC.NG, 4), (TC.NG, 4)]
    return np.ascontiguousarray(np.pad(a, w, mode="edge"))


def placed(c, fx, col):
    """the fixture's columns on the case: padded trajectory T (pt = temperature, q1 = qv, q2.. small), compact surface fields, QI, QL"""
    k = col % fx["ncol"]
    lev = lambda a: np.ascontiguousarray(np.moveaxis(a[:, k], 0, 1))      # [lm, ncol] -> [ntile, lm, ny, nx]
    T = dict(u=pad(c, lev(fx["u"])), v=pad(c, lev(fx["v"])), pt=pad(c, lev(fx["T"])), delp=pad(c, lev(fx["delp"])), q1=pad(c, lev(fx["qv"])))
    rng = np.random.default_rng(41)
    for n in range(1, c.nq):
        T["q%d" % (n + 1)] = 1e-4 * (n + rng.random(T["u"].shape))
    if not c.opt.hydrostatic:
        T["w"] = np.zeros_like(T["u"]); T["delz"] = -100.0 * np.ones_like(T["u"])
    sfc = {n: np.ascontiguousarray(fx[n][k]) for n in SFC}
    return T, sfc, lev(fx["qi"]), lev(fx["ql"]), k


def perturbation(c, seed=3):
    rng = np.random.default_rng(seed)
    shp = (c.dims.ntile, c.npz, c.ny + 7, c.nx + 7)
    amp = dict(u=1.0, v=1.0, pt=0.5, delp=10.0, w=0.1, delz=1.0)
    return {n: amp.get(n, 1e-4) * rng.standard_normal(shp) for n in TC.all_names(c)}


def colmax(a):
    """[ntile, (lm,) ny, nx] -> the column maximum of |a| at every point"""
    s = np.abs(a).max(axis=1) if a.ndim == 4 else np.abs(a)
    return np.where(s > 0, s, 1.0)


def errors(raw, fx, k):
    """per output: the largest error over all points relative to the output's column maximum in the fixture"""
    e = {}
    for n in RAW:
        ref = fx["out"][n]
        ref = np.moveaxis(ref[:, k], 0, 1) if ref.ndim == 2 else ref[k]
        d = np.abs(raw[n] - ref)
        d = d.max(axis=1) if d.ndim == 4 else d
        e[n] = float(np.max(d / colmax(ref)))
    return e


def set_fixture(c, lm, shift=0, cloud_mode=0, qa=None, qb=None, raw=True, slot=0):
    fx = fixture(lm)
    T, sfc, qi, ql, k = placed(c, fx, dealt(c, shift))
    TC.ensure_created(c)
    TC.put_all(c, T)
    out = c.dy.turbulence_set_driver(slot, params(c, fx), fx["dt"], sfc, qi if qa is None else qa, ql if qb is None else qb, cloud_mode, raw)
    return fx, T, sfc, qi, ql, k, out


# ---- 1: against the reference
def check_reference(c, lm, verbose=True):
    fx, T, sfc, qi, ql, k, raw = set_fixture(c, lm)
    assert set(np.unique(k)) == set(range(fx["ncol"])), "every column of the fixture is on the case"
    e = errors(raw, fx, k)
    if verbose:
        print("L%d %s: " % (lm, "face" if c.face is not None else "tile") + " ".join("%s %.1e/%.1e" % (n, e[n], fx["tol"][n]) for n in RAW))
    bad = {n: (e[n], fx["tol"][n]) for n in RAW if not e[n] <= fx["tol"][n]}
    assert not bad, bad
    # cloud_mode 1 with QLS = q, QCN = 0 against cloud_mode 0 fed the IceFraction split of q computed here
    q = np.ascontiguousarray(qi + ql)
    t = TC.comp(c, T["pt"])
    f = np.where(t <= 233.16, 1.0, np.where(t <= 273.16, 1.0 - (t - 233.16) / (273.16 - 233.16), 0.0))
    f = np.minimum(f, 1.0); f = np.maximum(f, 0.0); f = (f * f) * (f * f)
    r1 = c.dy.turbulence_set_driver(0, params(c, fx), fx["dt"], sfc, q, np.zeros_like(q), 1, True)
    r0 = c.dy.turbulence_set_driver(0, params(c, fx), fx["dt"], sfc, q * f, q * (1 - f), 0, True)
    rn = c.dy.turbulence_set_driver(0, params(c, fx), fx["dt"], sfc, q, None, 1, True)      # NULL = zero
    for n in RAW:
        d = np.abs(r1[n] - r0[n]); d = d.max(axis=1) if d.ndim == 4 else d
        assert float(np.max(d / colmax(r0[n]))) <= 1e-15, (n, "cloud_mode 1")
        assert np.array_equal(rn[n], r1[n]), (n, "NULL is zero")
    return e


# ---- 2: the slot holds the raw diagonals factorised
def check_slot_is_raw_factorised(c, lm):
    fx, T, sfc, qi, ql, k, raw = set_fixture(c, lm)
    got = c.dy.turbulence_get(0)
    c.dy.turbulence_set_diagonals(0, [raw[n] for n in RAW[:9]])
    want = c.dy.turbulence_get(0)
    for n in range(10):
        assert np.array_equal(got[n], want[n]), (n, "slot after set_driver != set_diagonals of its own raw_out")
    assert np.all(np.isfinite(got))
    # without raw_out: the same slot
    c.dy.turbulence_set_driver(0, params(c, fx), fx["dt"], sfc, qi, ql, 0, False)
    assert np.array_equal(c.dy.turbulence_get(0), got)


# ---- 3: through the solve
def check_solve(c, lm, tol_dot=1e-12):
    fx, T, sfc, qi, ql, k, raw = set_fixture(c, lm)
    P = perturbation(c)
    diag = [np.ascontiguousarray(np.moveaxis(fx["out"][n][:, k], 0, 1)) for n in RAW[:9]]
    rng = np.random.default_rng(19)
    sgn = [np.where(rng.random(d.shape) < 0.5, -1.0, 1.0) for d in diag]
    pert = [[d + s * g * fx["tol"][n] * colmax(d)[:, None] for d, g, n in zip(diag, sgn, RAW[:9])] for s in (1.0, -1.0)]
    D = TC.dom(c)
    worst = {}
    for mode in (NL, TL, AD):
        TC.put_all(c, T, P)
        c.dy.turbulence(0, mode)
        X = T if mode == NL else P
        ref = TC.restated(c, mode, diag, T, X)
        moved = [TC.restated(c, mode, pd, T, X) for pd in pert]
        for n in TC.seven(c):
            e = TC.relerr(c.dy.get(n, 0 if mode == NL else 1)[D], ref[n])
            bound = 1e-12 + max(TC.relerr(m[n], ref[n]) for m in moved)
            worst[(n, mode)] = (e, bound)
            assert e <= bound, (n, mode, e, bound)
            assert TC.relerr(ref[n], TC.comp(c, X[n])) > 1e-3, (n, mode, "the solve does nothing")
    lhs, rhs = TC.unit_dot_product(c, diag, T)
    assert abs(lhs - rhs) <= tol_dot * abs(lhs), (lhs, rhs)
    return worst, abs(lhs - rhs) / abs(lhs)


# ---- 4: position independence
def check_position(make_small, make_cube, lm=72, layout=2):
    """every column's raw outputs on the six faces equal those of the same column on the small tile, bitwise; the 24 sub-face tiles, fed
    the windows of the six-face fields, give the six-face result again, bitwise"""
    small = make_small()
    fx, _, _, _, _, ks, rs = set_fixture(small, lm)
    first = np.zeros(fx["ncol"], dtype=np.int64)      # a point of the small tile for every column
    first[ks.ravel()[::-1]] = np.arange(ks.size)[::-1]
    c1, c2 = make_cube(1), make_cube(layout)
    T1, sfc1, qi1, ql1, k1 = placed(c1, fx, dealt(c1, 5))
    win = lambda a: np.ascontiguousarray(np.stack([a[f, ..., j0 - 1:j0 - 1 + c2.nt, i0 - 1:i0 - 1 + c2.nt] for (f, i0, j0) in c2.tiles]))
    T2 = {n: pad(c2, win(TC.comp(c1, T1[n]))) for n in T1}
    outs = []
    for c, T, sfc, qi, ql in ((c1, T1, sfc1, qi1, ql1), (c2, T2, {n: win(v) for n, v in sfc1.items()}, win(qi1), win(ql1))):
        TC.ensure_created(c)
        TC.put_all(c, T)
        outs.append(c.dy.turbulence_set_driver(0, params(c, fx), fx["dt"], sfc, qi, ql, 0, True))
    for n in RAW:
        a = outs[0][n]
        if a.ndim == 4:
            want = np.moveaxis(np.moveaxis(rs[n], 1, -1).reshape(-1, lm)[first[k1]], -1, 1)
        else:
            want = rs[n].ravel()[first[k1]]
        assert np.array_equal(a, want), (n, "a column's result depends on where it lies")
        g = np.zeros_like(a)
        for t, (f, i0, j0) in enumerate(c2.tiles):
            g[f, ..., j0 - 1:j0 - 1 + c2.nt, i0 - 1:i0 - 1 + c2.nt] = outs[1][n][t]
        assert np.array_equal(g, a), (n, "24 tiles gathered != six faces")
    return c1.dims.ntile * c1.ny * c1.nx


# ---- 5: nothing else moves; the slot keeps what set saw
def check_nothing_else_moves(c, lm):
    fx = fixture(lm)
    T, sfc, qi, ql, k = placed(c, fx, dealt(c))
    rng = np.random.default_rng(23)
    T = {n: a + 0.0 for n, a in T.items()}
    D = TC.dom(c)
    for n in T:      # the halo and the far edge rows carry values of their own, so that a store outside is..ie x js..je shows
        h = 1e-3 * rng.standard_normal(T[n].shape) * np.abs(T[n]).max(); keep = T[n][D].copy(); T[n] = T[n] + h; T[n][D] = keep
    P = perturbation(c)
    TC.ensure_created(c, 2)
    TC.put_all(c, T, P)
    gen = TC.generated(c)
    c.dy.turbulence_set_diagonals(1, gen)
    other = c.dy.turbulence_get(1)
    before = {(n, w): c.dy.get(n, w) for n in TC.all_names(c) for w in (0, 1)}
    sfc_in = {n: v.copy() for n, v in sfc.items()}
    c.dy.turbulence_set_driver(0, params(c, fx), fx["dt"], sfc, qi, ql, 0, True)
    for (n, w), a in before.items():
        assert np.array_equal(c.dy.get(n, w), a), (n, w, "changed by set_driver")
    assert np.array_equal(c.dy.turbulence_get(1), other), "the other slot changed"
    for n in SFC:
        assert np.array_equal(sfc[n], sfc_in[n]), (n, "the host's surface array was written")
    # set, step, solve: the slot keeps what set saw (the rule of turbulence_checks.check_slots)
    c.dy.turbulence(0, TL)
    first = {n: c.dy.get(n, 1) for n in TC.seven(c)}
    T2, P2 = TC.unit_state(c)      # the resident trajectory moves on: the harness state and a whole step
    TC.put_all(c, T2, P2)
    c.dy.step_tl()
    assert not np.array_equal(c.dy.get("delp", 0), T["delp"])
    for n in TC.all_names(c):
        c.dy.put(n, P[n], 1)
    c.dy.turbulence(0, TL)
    for n in TC.seven(c):
        assert np.array_equal(c.dy.get(n, 1), first[n]), (n, "slot 0 followed the resident trajectory")
        assert TC.relerr(first[n][D], P[n][D]) > 1e-3, n


# ---- 6: refusals, by message
def neutral_column_case(make):
    """a shallow column (ptop = 700 hPa, 8 levels of 375 m) whose potential temperature -- the routine's temperature argument TH -- is
    the same at every level, dry, with BSTAR > 0: the parcel of mpbl_depth starts warmer than its surroundings, cools along the same
    adiabat and is only diluted towards them, so it is never colder; the layers are thinner than the 660 m at which the entrainment
    fraction reaches its exit threshold 0.9899.  The search never exits and the reference would go on with ipbl = -1."""
    c = make(nq=1, npz=8, ptop=70000.0)
    shp = (c.dims.ntile, c.npz, c.ny, c.nx)
    delp = np.full(shp, 30000.0 / 8)
    _, pk = TO.pressures(delp, c.opt.ptop, c.opt.akap)
    T = dict(u=pad(c, np.full(shp, 5.0)), v=pad(c, np.zeros(shp)), pt=pad(c, 300.0 * pk / 1.0e5 ** c.opt.akap), delp=pad(c, delp), q1=pad(c, np.full(shp, 1e-6)))
    one = np.ones(shp[:1] + shp[2:])
    sfc = dict(FRLAND=one, FROCEAN=0 * one, VARFLT=0 * one, ZPBL=500.0 * one, CM=0.01 * one, CT=0.01 * one, CQ=0.01 * one, USTAR=0.3 * one, BSTAR=0.02 * one)
    return c, T, sfc


def check_refusals(make):
    import pytest
    c = make(nq=4, npz=20)
    fx = fixture(20)
    T, sfc, qi, ql, k = placed(c, fx, dealt(c))
    TC.put_all(c, T)
    p = lambda: params(c, fx)
    call = lambda **kw: c.dy.turbulence_set_driver(kw.get("slot", 0), kw.get("p", p()), kw.get("dt", fx["dt"]), kw.get("sfc", sfc), qi, ql, kw.get("mode", 0), kw.get("raw", True))
    with pytest.raises(Fv3LmError, match="fv3lm_turbulence_create first"):
        call()
    c.dy.turbulence_create(2); c._turb_slots = 2

    def unset(slot=0):
        with pytest.raises(Fv3LmError, match="never set"):
            c.dy.turbulence(slot, TL)
    for slot in (-1, 2):
        with pytest.raises(Fv3LmError, match="out of range"):
            call(slot=slot)
    for kp in (0, -1, 21):
        bad = p(); bad.i[0] = kp
        with pytest.raises(Fv3LmError, match="KPBLMIN"):
            call(p=bad)
    bad = p(); bad.i[3] = 1
    with pytest.raises(Fv3LmError, match="RADLW_DEP"):
        call(p=bad)
    with pytest.raises(Fv3LmError, match="null parameters"):
        c.dy.turbulence_set_driver(0, None, fx["dt"], sfc, qi, ql, 0, True)
    for dt in (0.0, -1800.0, float("nan")):
        with pytest.raises(Fv3LmError, match="dt <= 0"):
            call(dt=dt)
    for n in (0, 4, 8):
        s = [sfc[m] for m in SFC]; s[n] = None
        with pytest.raises(Fv3LmError, match="null array"):
            call(sfc=s)
    with pytest.raises(Fv3LmError, match="null array"):
        c.dy.turbulence_set_driver(0, p(), fx["dt"], None, qi, ql, 0, True)
    for mode in (-1, 2):
        with pytest.raises(Fv3LmError, match="cloud_mode"):
            call(mode=mode)
    unset()
    call()                                   # a good set works ...
    c.dy.turbulence(0, TL)
    with pytest.raises(Fv3LmError, match="RADLW_DEP"):      # ... and a refusal of the arguments leaves that slot as it was
        call(p=bad)
    c.dy.turbulence(0, TL)
    unset(1)
    # npz < 7
    c6 = make(nq=1, npz=6)
    c6.dy.turbulence_create(1)
    one = np.ones((c6.dims.ntile, c6.ny, c6.nx))
    with pytest.raises(Fv3LmError, match="npz < 7"):
        c6.dy.turbulence_set_driver(0, c6.dy.bl_default_params(3), 1800.0, [one] * 9, None, None, 0, False)
    # the parcel that never stops: refused on every backend, the slot left unset, nothing read out of bounds; the same column made
    # stable (BSTAR <= 0 takes no parcel) is accepted
    cn, Tn, sn = neutral_column_case(make)
    cn.dy.turbulence_create(1)
    TC.put_all(cn, Tn)
    pn = cn.dy.bl_default_params(4)
    for raw in (True, False):
        with pytest.raises(Fv3LmError, match="never reaches its level of neutral buoyancy"):
            cn.dy.turbulence_set_driver(0, pn, 1800.0, sn, None, None, 0, raw)
        with pytest.raises(Fv3LmError, match="never set"):
            cn.dy.turbulence(0, TL)
    only_one = dict(sn); b = -0.01 * np.ones_like(sn["BSTAR"]); b[0, 1, 2] = 0.02; only_one["BSTAR"] = b      # one such column is enough
    with pytest.raises(Fv3LmError, match="never reaches its level of neutral buoyancy"):
        cn.dy.turbulence_set_driver(0, pn, 1800.0, only_one, None, None, 0, True)
    stable = dict(sn); stable["BSTAR"] = -0.01 * np.ones_like(sn["BSTAR"])
    out = cn.dy.turbulence_set_driver(0, pn, 1800.0, stable, None, None, 0, True)
    assert all(np.all(np.isfinite(out[n])) for n in RAW)
    cn.dy.turbulence(0, TL)
    cn.dy.step_tl()                          # nothing above has poisoned the handle


# ---- 7: at size
def synthetic_surface(c, T):
    """smooth-state surface fields: land / sea in turn, BSTAR of both signs"""
    t, j, i = np.meshgrid(np.arange(c.dims.ntile), np.arange(c.ny), np.arange(c.nx), indexing="ij")
    h = (i + 2 * j + 3 * t)
    frl = np.array([0.0, 0.3, 0.7, 1.0])[h % 4]
    return dict(FRLAND=frl, FROCEAN=1.0 - frl, VARFLT=np.where(h % 3 == 0, 0.0, 50.0 + 10.0 * (h % 17)), ZPBL=300.0 + 100.0 * (h % 13),
                CM=0.01 + 0.002 * (h % 11), CT=0.01 + 0.002 * (h % 7), CQ=0.01 + 0.002 * (h % 5), USTAR=0.1 + 0.03 * (h % 9),
                BSTAR=np.where(h % 5 < 2, -0.005, 0.002 + 0.002 * (h % 5)))


def check_at_size(c, repeats=5, tol=1e-12):
    T, P = TC.unit_state(c)
    sfc = synthetic_surface(c, T)
    kp = int(np.count_nonzero(0.5 * (c.ak[1:] + c.ak[:-1] + 1.0e5 * (c.bk[1:] + c.bk[:-1])) < 50000.0))
    p = c.dy.bl_default_params(max(1, kp))
    TC.ensure_created(c)
    TC.put_all(c, T, P)
    qi = TC.comp(c, T["q3"]) * 0.01; ql = TC.comp(c, T["q2"]) * 0.01
    c.dy.turbulence_set_driver(0, p, c.dims.dt, sfc, qi, ql, 0, False)      # warm-up (allocates the surface planes and the table)
    times = []
    for n in range(repeats):
        c.dy.profile_begin()
        c.dy.turbulence_set_driver(0, p, c.dims.dt, sfc, qi, ql, 0, False)
        times.append({k: v[1] for k, v in c.dy.profile_end().items()})
    fac = c.dy.turbulence_get(0)
    assert np.all(np.isfinite(fac))
    assert float(np.abs(fac[3]).max()) > 0.1, "the diagonals are not the identity"
    lhs, rhs = TC.unit_dot_product(c, None, T)
    assert abs(lhs - rhs) <= tol * abs(lhs), (lhs, rhs)
    return times, abs(lhs - rhs) / abs(lhs)
