"""Checks of the linearised boundary-layer turbulence (fv3lm_turbulence_*; product csrc/turbulence.h) shared by the host-emulation
(test_emul_turbulence.py) and the MI355X (test_gpu_turbulence.py) runs, against the numpy restatement tests/turbulence_oracle.py.

Where the diagonals come from: (i) the restated BL_simp on the case's own state at L127 -- at L12 the same state leaves KH at its floor
everywhere, a near-identity matrix that tests no solver; (ii) turbulence_oracle.diffusion_systems, diffusion-shaped and diagonally
dominant with |a| well above 1.  A check that uses (i) asserts |a| > 0.1 at >= 5 % of the points, one that uses (ii) max|a| >= 5.

Tolerances: a unit against its restatement 1e-12 of the field's max, dot products 1e-12 on one tile and 1e-11 on six faces (the
project's own, tests/test_gpu_split_damp.py); the restatement itself sits at <= 5e-15 on these measures (check 0)."""
import numpy as np
import turbulence_oracle as TO
from turbulence_oracle import NL, TL, AD
from fv3_jedi_linearmodel_amd import harness as H

NG = 3


def relerr(a, b):
    s = float(np.max(np.abs(b)))
    return float(np.max(np.abs(a - b))) / (s if s > 0 else 1.0)


def is_cube(c):
    return isinstance(c, H.CubeCase)


def qnames(c):
    return ["q%d" % (n + 1) for n in range(c.nq)]


def seven(c):
    return ["u", "v", "pt"] + qnames(c)


def all_names(c):
    return ["u", "v", "pt", "delp"] + ([] if c.opt.hydrostatic else ["w", "delz"]) + qnames(c)


def dom(c):
    """is..ie x js..je of the padded planes [ntile, nk, ny+7, nx+7]"""
    return (Ellipsis, slice(NG, NG + c.ny), slice(NG, NG + c.nx))


def comp(c, a):
    return np.ascontiguousarray(a[dom(c)])


def cshape(c):
    return (c.dims.ntile, c.npz, c.ny, c.nx)


def ensure_created(c, nslots=1):
    if getattr(c, "_turb_slots", 0) == 0:
        c.dy.turbulence_create(nslots)
        c._turb_slots = nslots
    assert c._turb_slots >= nslots


def frocean(c):
    """1.0 (sea), 0.0 and 0.5 (not sea) in turn over the columns"""
    t, j, i = np.meshgrid(np.arange(c.dims.ntile), np.arange(c.ny), np.arange(c.nx), indexing="ij")
    f = np.array([1.0, 0.0, 0.5])[(i + 2 * j + t) % 3]
    assert np.mean(f == 1.0) >= 0.10 and np.mean(f != 1.0) >= 0.10
    return np.ascontiguousarray(f)


def unit_state(c, seed=3):
    """padded trajectory (pt = temperature, as the host hands it over) and a random perturbation -- random on the WHOLE padded plane, so
    that a store outside is..ie x js..je shows -- of every prognostic field of the case"""
    T0, _ = H.cube_step_state(c) if is_cube(c) else H.step_state(c)
    lift = (lambda a: a) if is_cube(c) else (lambda a: a[None])
    T = {n: np.array(lift(T0[n]), dtype=np.float64) for n in ["u", "v", "pt", "delp"] + qnames(c)}
    rng = np.random.default_rng(seed)
    shp = T["u"].shape
    if not c.opt.hydrostatic:
        T["w"] = 2.0 * rng.standard_normal(shp)
        T["delz"] = -(100.0 + 50.0 * rng.random(shp))
    amp = dict(u=1.0, v=1.0, pt=0.5, delp=10.0, w=0.1, delz=1.0)
    P = {n: amp.get(n, 1e-4) * rng.standard_normal(shp) for n in all_names(c)}
    return T, P


def put_all(c, T, P=None):
    for n in all_names(c):
        c.dy.put(n, T[n], 0)
        if P is not None:
            c.dy.put(n, P[n], 1)


def generated(c, seed=29, strength=8.0, shape=None):
    d = TO.diffusion_systems(np.random.default_rng(seed), shape or cshape(c), strength)
    assert max(float(np.abs(d[n]).max()) for n in (0, 3, 6)) >= 5.0
    return d


def simple(c, T):
    """(i): restated BL_simp on the compact trajectory; -> diagonals, intermediates, frocean"""
    assert c.nq >= 3
    fro = frocean(c)
    diag, mid, _ = TO.bl_simp_of_state(c.opt, c.dims.dt, {n: comp(c, T[n]) for n in T}, fro)
    a = np.abs(diag[3][:, 1:])
    assert np.mean(a > 0.1) >= 0.05, np.mean(a > 0.1)
    return diag, mid, fro


def diagonals(c, T, kind):
    return simple(c, T)[0] if kind == "simple" else generated(c)


def restated(c, mode, diag, T, X):
    _, pk = TO.pressures(comp(c, T["delp"]), c.opt.ptop, c.opt.akap)
    return TO.turbulence(mode, TO.factorise(diag), pk, c.opt.akap, {n: comp(c, X[n]) for n in seven(c)})


# ---- 0: the restatement against independent algebra (no product)
def check_restatement(diag, tol=1e-13):
    """diag: nine arrays [lm, 1, ncol].  Phase 1 / ygswitch 1 against numpy.linalg.solve of the assembled matrix; the matrix of phase 2
    against the transpose of the matrix of phase 1, both switches."""
    lm, ncol = diag[0].shape[0], diag[0].shape[-1]
    rng = np.random.default_rng(5)
    worst = dict(solve=0.0, t1=0.0, t0=0.0)
    for s in range(3):
        a0, b0, c0 = diag[3 * s:3 * s + 3]
        a, b = TO.vtrilupert(a0, b0, c0)
        y = rng.standard_normal((lm, 1, ncol))
        x = TO.vtrisolvepert(a, b, c0, y, 1, 1)
        for n in range(ncol):
            M = TO.tridiagonal_matrix(a0[:, 0, n], b0[:, 0, n], c0[:, 0, n])
            ref = np.linalg.solve(M, y[:, 0, n])
            worst["solve"] = max(worst["solve"], float(np.abs(x[:, 0, n] - ref).max() / np.abs(ref).max()))
        eye = np.zeros((lm, lm, ncol))                   # [level, unit vector, column]: the matrix of every column at once
        eye[np.arange(lm), np.arange(lm), :] = 1.0
        for yg in (1, 0):
            M1 = TO.vtrisolvepert(a, b, c0, eye, 1, yg)      # M1[i, j, n] = (phase 1 e_j)_i
            M2 = TO.vtrisolvepert(a, b, c0, eye, 2, yg)
            e = float(np.max(np.abs(M2 - np.swapaxes(M1, 0, 1))) / np.max(np.abs(M1)))
            worst["t%d" % yg] = max(worst["t%d" % yg], e)
    assert worst["solve"] <= tol and worst["t1"] <= tol and worst["t0"] <= tol, worst
    return worst


# ---- 1: the unit in the three modes, and what it must leave alone
def check_unit(c, kind, tol=1e-12):
    T, P = unit_state(c)
    diag = diagonals(c, T, kind)
    ensure_created(c)
    put_all(c, T, P)
    c.dy.turbulence_set_diagonals(0, diag)
    fac = TO.factorise(diag)
    _, pk = TO.pressures(comp(c, T["delp"]), c.opt.ptop, c.opt.akap)
    got = c.dy.turbulence_get(0)
    worst = 0.0
    for n in range(9):
        e = relerr(got[n], fac[n]); worst = max(worst, e)
        assert e <= tol, ("factor", n, e)
    e = relerr(got[9], pk); worst = max(worst, e)
    assert e <= tol, ("pk", e)
    D = dom(c)
    for mode in (NL, TL, AD):
        put_all(c, T, P)
        c.dy.turbulence(0, mode)
        which = 0 if mode == NL else 1
        ref = restated(c, mode, diag, T, T if mode == NL else P)
        for n in all_names(c):
            for w, orig in ((0, T[n]), (1, P[n])):
                g = c.dy.get(n, w)
                if w == which and n in seven(c):
                    e = relerr(g[D], ref[n]); worst = max(worst, e)
                    assert e <= tol, (n, mode, e)
                    assert relerr(g[D], orig[D]) > 1e-3, (n, mode, "the unit did nothing")
                    want = orig.copy(); want[D] = g[D]
                    assert np.array_equal(g, want), (n, mode, "changed outside is..ie x js..je (halo or far edge row)")
                else:
                    assert np.array_equal(g, orig), (n, mode, w, "must be bitwise unchanged")
    return worst


# ---- 2: adjoint identity of the unit
def unit_dot_product(c, diag, T, seed=17):
    rng = np.random.default_rng(seed)
    D = dom(c)
    shp = T["u"].shape
    x = {n: np.zeros(shp) for n in all_names(c)}; y = {n: np.zeros(shp) for n in all_names(c)}
    for n in seven(c):
        x[n][D] = rng.standard_normal(x[n][D].shape); y[n][D] = rng.standard_normal(y[n][D].shape)
    put_all(c, T, x)
    c.dy.turbulence(0, TL)
    lhs = sum(float(np.sum(c.dy.get(n, 1)[D] * y[n][D])) for n in seven(c))
    put_all(c, T, y)
    c.dy.turbulence(0, AD)
    rhs = sum(float(np.sum(c.dy.get(n, 1)[D] * x[n][D])) for n in seven(c))
    return lhs, rhs


def check_unit_dot_product(c, kind, tol=1e-12):
    T, _ = unit_state(c)
    diag = diagonals(c, T, kind)
    ensure_created(c)
    put_all(c, T)
    c.dy.turbulence_set_diagonals(0, diag)
    lhs, rhs = unit_dot_product(c, diag, T)
    assert abs(lhs - rhs) <= tol * abs(lhs), (lhs, rhs)
    return abs(lhs - rhs) / abs(lhs)


# ---- 3: BL_simp on the device
def check_simple(c, tol=1e-12):
    T, _ = unit_state(c)
    diag, mid, fro = simple(c, T)
    ri, kh = mid["ri"], mid["kh"]
    frac = dict(ri_neg=np.mean(ri < 0), ri_pos=np.mean(ri > 0), kh_floor=np.mean(kh == 0.01), kh_above=np.mean(kh > 0.01),
                sea=np.mean(fro == 1.0), not_sea=np.mean(fro != 1.0))
    for k in ("ri_neg", "ri_pos", "kh_floor", "kh_above"):
        assert frac[k] >= 0.05, frac
    assert frac["sea"] >= 0.10 and frac["not_sea"] >= 0.10, frac
    ensure_created(c)
    put_all(c, T)
    c.dy.turbulence_set_simple(0, fro)
    got = c.dy.turbulence_get(0)
    fac = TO.factorise(diag)
    _, pk = TO.pressures(comp(c, T["delp"]), c.opt.ptop, c.opt.akap)
    worst = 0.0
    for n, ref in enumerate(fac + [pk]):
        e = relerr(got[n], ref); worst = max(worst, e)
        assert e <= tol, (n, e, frac)
    # the surface terms reached the right system: b(lm) of V, S, Q differ as frocean says
    bv, bs, bq = (got[n][:, -1] for n in (1, 4, 7))
    assert np.all((bs == bq)[fro != 1.0]) and np.all((bs == bv)[fro == 1.0]) and np.all(bv != bq)
    return worst, frac


# ---- 4: a slot keeps what its set call saw
def check_slots(c, tol=1e-12):
    T, P = unit_state(c)
    d = [generated(c, seed=29, strength=8.0), generated(c, seed=31, strength=3.0)]
    ensure_created(c, 2)
    put_all(c, T, P)
    c.dy.turbulence_set_diagonals(0, d[0]); c.dy.turbulence_set_diagonals(1, d[1])
    c.dy.turbulence(0, TL)
    first = {n: c.dy.get(n, 1) for n in seven(c)}
    # the resident trajectory moves on: delp overwritten, then a whole step
    T2 = dict(T); T2["delp"] = 1.05 * T["delp"]
    put_all(c, T2, P)
    c.dy.step_tl()
    assert not np.array_equal(c.dy.get("delp", 0), T["delp"])
    for n in all_names(c):
        c.dy.put(n, P[n], 1)
    c.dy.turbulence(0, TL)
    for n in seven(c):
        assert np.array_equal(c.dy.get(n, 1), first[n]), (n, "slot 0 followed the resident trajectory")
    # two slots used alternately
    D = dom(c)
    worst = 0.0
    for k in (1, 0, 1, 0):
        for n in all_names(c):
            c.dy.put(n, P[n], 1)
        c.dy.turbulence(k, TL)
        ref = restated(c, TL, d[k], T, P)
        for n in seven(c):
            e = relerr(c.dy.get(n, 1)[D], ref[n]); worst = max(worst, e)
            assert e <= tol, (k, n, e)
    return worst


# ---- 5: M = turbulence_TL o step_tl, M^T = step_ad o turbulence_AD
def step_state(c):
    """names, padded trajectory and perturbation of the whole step (hydrostatic: u v pt delp q*; non-hydrostatic: + w delz)"""
    lift = (lambda a: a) if is_cube(c) else (lambda a: a[None])
    if c.opt.hydrostatic:
        T0, P0 = H.cube_step_state(c) if is_cube(c) else H.step_state(c)
        names = ["u", "v", "pt", "delp"] + qnames(c)
        return names, {n: lift(T0[n]) for n in names}, {n: lift(P0[n]) for n in names}
    from nh_checks import fv_names
    if is_cube(c):
        Tl, Pl = H.cube_nh_state(c)
    else:
        from test_oracle_nh import nh_state_fv
        Tl, Pl = nh_state_fv(c)
    names = fv_names(c)
    return names, {n: lift(t) for n, t in zip(names, Tl)}, {n: lift(p) for n, p in zip(names, Pl)}


def sdom(c, n):
    return c.rect(1, c.nx, 1, c.ny + 1) if n == "u" else c.rect(1, c.nx + 1, 1, c.ny) if n == "v" else c.rect(1, c.nx, 1, c.ny)


def _masked(c, n, a):
    out = np.zeros_like(a); r = sdom(c, n); out[r] = a[r]
    return out


def check_composite(c, tol, tol_tl=1e-12):
    names, T, P = step_state(c)
    dx = {n: _masked(c, n, P[n]) for n in names}
    diag = generated(c)
    ensure_created(c)
    for n in names:
        c.dy.put(n, T[n], 0); c.dy.put(n, dx[n], 1)
    c.dy.turbulence_set_diagonals(0, diag)         # the trajectory at the START of the step
    c.dy.step_tl()
    S = {n: c.dy.get(n, 1) for n in names}
    c.dy.turbulence(0, TL)
    Mdx = {n: c.dy.get(n, 1) for n in names}
    ref = restated(c, TL, diag, T, S)
    D = dom(c)
    for n in names:
        if n in seven(c):
            e = relerr(Mdx[n][D], ref[n])
            assert e <= tol_tl, (n, "composite TL", e)
            assert relerr(Mdx[n][D], S[n][D]) > 1e-3, n
        else:
            assert np.array_equal(Mdx[n], S[n]), n
    rng = np.random.default_rng(13)
    dy = {n: _masked(c, n, rng.standard_normal(Mdx[n].shape) / max(1e-30, float(np.abs(Mdx[n]).max()))) for n in names}
    lhs = sum(float(np.sum(_masked(c, n, Mdx[n]) * dy[n])) for n in names)
    for n in names:
        c.dy.put(n, T[n], 0)
    c.dy.step_nl()
    for n in names:
        c.dy.put(n, dy[n], 1)
    c.dy.turbulence(0, AD)
    c.dy.step_ad()
    rhs = sum(float(np.sum(c.dy.get(n, 1) * dx[n])) for n in names)
    assert abs(lhs - rhs) <= tol * abs(lhs), (lhs, rhs)
    return abs(lhs - rhs) / abs(lhs)


# ---- 6: sub-face tiles against whole faces, bitwise
def check_layout(make, layout=2):
    from fv3_jedi_linearmodel_amd import cube
    c1, c2 = make(1), make(layout)
    n, nt = c1.n, c2.nt
    T1, _ = unit_state(c1); T2, _ = unit_state(c2)
    rng = np.random.default_rng(7)
    P1 = {k: rng.standard_normal(T1["u"].shape) for k in all_names(c1)}
    P2 = {k: cube.tile_window(v, c2.tiles, nt) for k, v in P1.items()}
    d1 = generated(c1)
    d2 = [np.ascontiguousarray(np.stack([a[f, :, j0 - 1:j0 - 1 + nt, i0 - 1:i0 - 1 + nt] for (f, i0, j0) in c2.tiles])) for a in d1]
    D = dom(c1)
    for c, T, P, d in ((c1, T1, P1, d1), (c2, T2, P2, d2)):
        ensure_created(c)
        put_all(c, T, P)
        c.dy.turbulence_set_diagonals(0, d)
    for mode in (NL, TL, AD):
        res = []
        for c, T, P in ((c1, T1, P1), (c2, T2, P2)):
            put_all(c, T, P)
            c.dy.turbulence(0, mode)
            res.append({k: c.gather(c.dy.get(k, 0 if mode == NL else 1)) for k in seven(c)})
        for k in seven(c1):
            assert relerr(res[0][k][D], (T1 if mode == NL else P1)[k][D]) > 1e-3
            assert np.array_equal(res[0][k][D], res[1][k][D]), (k, mode)


# ---- 7: refusals, by message
def check_refusals(make):
    import pytest
    from fv3_jedi_linearmodel_amd._lib import Fv3LmError
    c = make(nq=4, npz=6)
    T, P = unit_state(c)
    put_all(c, T, P)
    d = generated(c)
    fro = frocean(c)
    for call in (lambda: c.dy.turbulence_set_diagonals(0, d), lambda: c.dy.turbulence_set_simple(0, fro), lambda: c.dy.turbulence(0, TL),
                 lambda: c.dy.turbulence_get(0)):
        with pytest.raises(Fv3LmError, match="fv3lm_turbulence_create first"):
            call()
    for bad in (0, -3):
        with pytest.raises(Fv3LmError, match="nslots < 1"):
            c.dy.turbulence_create(bad)
    c.dy.turbulence_create(2)
    with pytest.raises(Fv3LmError, match="already created"):
        c.dy.turbulence_create(1)
    for slot in (-1, 2):
        for call in (lambda: c.dy.turbulence_set_diagonals(slot, d), lambda: c.dy.turbulence_set_simple(slot, fro),
                     lambda: c.dy.turbulence(slot, TL), lambda: c.dy.turbulence_get(slot)):
            with pytest.raises(Fv3LmError, match="out of range"):
                call()
    with pytest.raises(Fv3LmError, match="never set"):
        c.dy.turbulence(1, TL)
    with pytest.raises(Fv3LmError, match="never set"):
        c.dy.turbulence_get(1)
    with pytest.raises(Fv3LmError, match="null array"):
        c.dy.turbulence_set_diagonals(0, d[:4] + [None] + d[5:])
    with pytest.raises(Fv3LmError, match="null array"):
        c.dy.turbulence_set_simple(0, None)
    with pytest.raises(Fv3LmError, match="bad mode"):
        c.dy.turbulence(0, 3)
    # a main diagonal that cannot be factorised: reported by set_diagonals, and the slot stays unset
    for what in ("zero", "nan"):
        bad = [a.copy() for a in d]
        if what == "zero":
            bad[4][0, 0, 1, 2] = 0.0                         # b(1) = 0 in one column of S
        else:
            bad[7][0, 3, 2, 1] = np.nan                      # a NaN half way down one column of Q
        with pytest.raises(Fv3LmError, match="zero or non-finite pivot"):
            c.dy.turbulence_set_diagonals(0, bad)
        with pytest.raises(Fv3LmError, match="never set"):
            c.dy.turbulence(0, TL)
    c.dy.turbulence_set_diagonals(0, d)                      # and a good set afterwards works
    c.dy.turbulence(0, TL)
    assert np.all(np.isfinite(c.dy.get("pt", 1)))
    # nothing above has poisoned the handle
    c.dy.step_tl()
    c3 = make(nq=2, npz=6)
    c3.dy.turbulence_create(1)
    with pytest.raises(Fv3LmError, match="nq < 3"):
        c3.dy.turbulence_set_simple(0, frocean(c3))
    # npz < 2: no tridiagonal system.  fv3lm_create itself refuses such a handle today (the remap needs two levels); should it ever
    # accept one, fv3lm_turbulence_create must refuse it
    try:
        c1 = make(nq=0, npz=1)
    except Fv3LmError as e:
        assert "npz >= 2" in str(e), e
    else:
        with pytest.raises(Fv3LmError, match="npz < 2"):
            c1.dy.turbulence_create(1)


# ---- 8: at size (six faces C192 L127 on the MI355X): set_simple, TL and AD against the restatement, the unit's dot product
def check_at_size(c, tol=1e-12):
    T, P = unit_state(c)
    diag, mid, fro = simple(c, T)
    ensure_created(c)
    put_all(c, T, P)
    c.dy.turbulence_set_simple(0, fro)
    D = dom(c)
    worst = 0.0
    for mode in (TL, AD):
        for n in all_names(c):
            c.dy.put(n, P[n], 1)
        c.dy.turbulence(0, mode)
        ref = restated(c, mode, diag, T, P)
        for n in seven(c):
            e = relerr(c.dy.get(n, 1)[D], ref[n]); worst = max(worst, e)
            assert e <= tol, (n, mode, e)
    lhs, rhs = unit_dot_product(c, diag, T)
    assert abs(lhs - rhs) <= tol * abs(lhs), (lhs, rhs)
    return worst, abs(lhs - rhs) / abs(lhs)
