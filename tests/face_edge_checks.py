"""The face-edge operators of the product, point by point, against tests/face_oracle.py: the restatement of d2a2c_vect, divergence_corner,
the area-flux scaling of c_sw, the first loops of d_sw, a2b_ord4 / one_grad_p and p_grad_c written from the reference's nonlinear
Fortran (whole faces: check; six faces cut into tiles: check_layout).  The library receives
the RESTATEMENT's metrics (harness metrics_hook), with 1e30 in every entry the reference leaves undefined, so product and reference share
the corner points and nothing else.  Values and tangent through put / run_group(TL) / get; the adjoint with seeds on the compared outputs
only, against the transpose of the restated statements (their Jacobian, column by column, by complex step on the trajectory's branches).

Error of a point: relative to the largest reference value of the same output, level and region, the regions being the bulk, the four
edge strips and the four corner blocks (3 cells wide, halo included), so that an edge error is never divided by a bulk maximum.  Bound per
output, region and mode: 8 x the movement of the restatement itself -- float64 on inputs moved by <= 1 ulp (three draws) against
longdouble on the unmoved ones -- and at least 1e-12.  Every point of the rects of groups.py is compared, except those the reference
itself forms from poisoned entries (poison_checks.drop_undefined).  Measured figures: DESIGN.md section 5."""
import numpy as np
from oracle import NL, TL, AD
import groups as G
import face_oracle as fo
import poison_checks as PC

FLOOR, H = 1.0e-12, 1.0e-30
_REST = {}


def restatement(n, dtype):
    if (n, dtype) not in _REST:
        from fv3_jedi_linearmodel_amd import cube
        _REST[(n, dtype)] = fo.face_metrics(cube.cube_corner_points(n), dtype=dtype)
    return _REST[(n, dtype)]


def face_metrics_of(n, face, dtype):
    m, poison, edge, ecorner, _ = restatement(n, dtype)
    M = {k: np.where(poison[k][face], np.nan, v[face]) for k, v in m.items()}       # poison as NaN: a read shows in the reference too
    npx = n + 1
    for r in ((1, npx, 1, 1), (1, npx, npx, npx), (1, 1, 1, npx), (npx, npx, 1, npx)):
        fo.V(M["rsina"], *r)[...] = fo.BIG
    return M, edge[face], ecorner[face]


def restatement_hook(n, face=None, value=1.0e30):
    """metrics_hook: the library gets the float64 restatement, `value` where it is undefined"""
    m, poison, edge, ecorner, _ = restatement(n, np.float64)
    ok = fo.defined(m, poison)
    sel = slice(None) if face is None else slice(face, face + 1)

    def hook(metrics, e, ec):
        assert set(metrics) == set(m)
        return ({k: np.where(ok[k][sel], m[k][sel], value) for k in metrics}, np.where(np.isfinite(edge[sel]), edge[sel], value), ecorner[sel].copy())
    return hook


regions, region_errors = G.regions, G.region_errors


def compared_mask(c, name, rk):
    one = np.ones((1, c.ny + 7, c.nx + 7))
    return PC.drop_undefined(c, name, G.masked(c, one, rk))[0] != 0


def ulp_move(rng, a):
    return a + rng.integers(-1, 2, size=a.shape) * np.spacing(np.abs(a))


def noise(rng, shape, amp):
    return amp * rng.standard_normal(shape)


def both_signs(vals):
    big = np.max(np.abs(vals))
    return bool((vals > 0).any() and (vals < 0).any() and np.all(np.abs(vals) > 1e-6 * big))


# ------------------------------------------------------------------------------------------------------------ the three operators
class CSw:
    level_local = True
    group, ins = "c_sw", ["u", "v"]
    outs = [("ua", "Ah"), ("va", "Ah"), ("utf", "UTF"), ("vtf", "VTF"), ("divgd", "B")]

    def __init__(self, c):
        self.n, self.dt2 = c.nx, 0.5 * c.dt_ac

    def fixed(self, c):
        return {"delp": c.traj["delp"][0], "pt": c.traj["pt"][0]}

    def draw(self, c, rng):
        shp = (c.npz, c.ny + 7, c.nx + 7)
        return {k: noise(rng, shp, 10.0) for k in self.ins}, {k: noise(rng, shp, 1.0) for k in self.ins}

    def apply(self, x, M, edge, ecorner):
        return fo.c_sw_winds(x["u"], x["v"], M, self.n, self.dt2)

    def signs_ok(self, x, M, edge, ecorner):
        """both signs of ut, vt on every edge row and in every corner-halo block, none near zero"""
        o, n = self.apply(x, M, edge, ecorner), self.n
        npx = n + 1
        rows = [fo.V(o["ut"], i, i, 0, n + 1) for i in (1, npx)] + [fo.V(o["vt"], 0, n + 1, j, j) for j in (1, npx)]
        for (i0, j0) in ((1, 0), (npx - 1, 0), (1, n + 1), (npx - 1, n + 1)):        # (ut(0|npx+1, 0|n+1) itself holds no value)
            rows.append(fo.V(o["ut"], i0, i0 + 1, j0, j0))
        for (i0, j0) in ((0, 1), (n + 1, 1), (0, npx - 1), (n + 1, npx - 1)):
            rows.append(fo.V(o["vt"], i0, i0, j0, j0 + 1))
        return all(both_signs(np.real(r)) for r in rows)


class OneGradP:
    group, ins = "one_grad_p", ["u_m", "v_m", "pk", "gzd"]
    outs = [("u_o", "U"), ("v_o", "V")]

    def __init__(self, c):
        self.n, self.dt, self.ptk = c.nx, c.dt_ac, c.opt.ptop ** c.opt.akap

    def fixed(self, c):
        return {}

    def draw(self, c, rng):
        npz, shp = c.npz, (c.npz, c.ny + 7, c.nx + 7)
        shp1 = (npz + 1,) + shp[1:]
        base = (c.opt.ptop + np.arange(npz + 1) * 1.0e5 / npz) ** c.opt.akap
        T = dict(u_m=noise(rng, shp, 10.0), v_m=noise(rng, shp, 10.0), pk=base[:, None, None] * (1 + noise(rng, shp1, 0.01)),
                 gzd=1.0e4 * (npz + 1 - np.arange(npz + 1))[:, None, None] * (1 + noise(rng, shp1, 0.01)))
        P = dict(u_m=noise(rng, shp, 1.0), v_m=noise(rng, shp, 1.0), pk=noise(rng, shp1, 1e-2), gzd=noise(rng, shp1, 10.0))
        return T, P

    def apply(self, x, M, edge, ecorner):
        return fo.one_grad_p(x["u_m"], x["v_m"], x["pk"], x["gzd"], M, edge, ecorner, self.n, self.dt, self.ptk)

    def signs_ok(self, *a):
        return True


class PGradC:
    group, ins = "p_grad_c", ["pkc", "gz", "uc1", "vc1"]
    outs = [("uc", "V"), ("vc", "U")]

    def __init__(self, c):
        self.n, self.dt2 = c.nx, 0.5 * c.dt_ac

    fixed = OneGradP.fixed

    def draw(self, c, rng):
        T, P = OneGradP.draw(self, c, rng)
        ren = dict(u_m="uc1", v_m="vc1", pk="pkc", gzd="gz")
        return {ren[k]: v for k, v in T.items()}, {ren[k]: v for k, v in P.items()}

    def apply(self, x, M, edge, ecorner):
        return fo.p_grad_c(x["pkc"], x["gz"], x["uc1"], x["vc1"], M, self.n, self.dt2)

    def signs_ok(self, *a):
        return True


class DSw:
    """the first loops of d_sw: uc, vc -> crx, cry, xfx, yfx; the other inputs of the group are given plausible data and no seed"""
    level_local = True
    group, ins = "d_sw", ["uc", "vc"]
    outs = [("crx", "CX"), ("cry", "CY"), ("xfx", "CX"), ("yfx", "CY")]

    def __init__(self, c):
        self.n, self.dt = c.nx, c.dt_ac

    def fixed(self, c):
        rng = np.random.default_rng(5)
        shp = (c.npz, c.ny + 7, c.nx + 7)
        out = {"delp": c.traj["delp"][0], "pt": c.traj["pt"][0]}
        out.update({k: noise(rng, shp, 5.0) for k in ("u", "v", "ua", "va")})
        out.update({k: noise(rng, shp, 1e-6) for k in ("divgd",)})
        out.update({k: np.zeros(shp) for k in ("mfx", "mfy", "cx", "cy")})
        return out

    def draw(self, c, rng):
        shp = (c.npz, c.ny + 7, c.nx + 7)
        return {k: noise(rng, shp, 10.0) for k in self.ins}, {k: noise(rng, shp, 1.0) for k in self.ins}

    def apply(self, x, M, edge, ecorner):
        return fo.d_sw_courant(x["uc"], x["vc"], M, self.n, self.dt)

    def signs_ok(self, x, M, edge, ecorner):
        """both signs of the Courant numbers on every edge row and in every corner-halo block (rows j <= 0, j >= npy of crx, columns
        i <= 0, i >= npx of cry, next to the face edges), none near zero"""
        o, n = self.apply(x, M, edge, ecorner), self.n
        npx = n + 1
        rows = [fo.V(o["crx"], i, i, 1, n) for i in (1, npx)] + [fo.V(o["cry"], 1, n, j, j) for j in (1, npx)]
        for i in (1, 2, npx - 1, npx):
            rows += [fo.V(o["crx"], i, i, -2, 0), fo.V(o["crx"], i, i, npx, n + 3)]
        for j in (1, 2, npx - 1, npx):
            rows += [fo.V(o["cry"], -2, 0, j, j), fo.V(o["cry"], npx, n + 3, j, j)]
        return all(both_signs(np.real(r)) for r in rows)


OPERATORS = {"c_sw": CSw, "one_grad_p": OneGradP, "p_grad_c": PGradC, "d_sw": DSw}
GHOST_FREE = ("pk", "gzd", "pkc", "gz")     # geopk outputs: the corner-halo columns hold no data; NaN for the restatement, 1e30 for the library


def _ghost_fill(c, x, value):
    g = fo._ghost(c.nx)
    out = {}
    for k, v in x.items():
        out[k] = v.copy()
        if k in GHOST_FREE:
            out[k][:, g] = value
    return out


def _tangent(op, T, P, M, edge, ecorner, dtype):
    ct = np.clongdouble if dtype == np.longdouble else np.complex128
    z = {k: T[k].astype(ct) + 1j * ct(H) * P[k].astype(ct) for k in T}
    o = op.apply(z, M, edge, ecorner)
    return {k: (np.real(v).astype(dtype), (np.imag(v) / dtype(H)).astype(dtype)) for k, v in o.items()}


SPACING, REACH = 14, 6


def _adjoint(op, T, seeds, M, edge, ecorner, dtype, points, chunk=192, coloured=False):
    """J^T s at the listed input points {input: boolean [nlev, pj, pj]}: one unit perturbation per column, complex step.
    coloured: the statements are local -- an input point reaches no output further than REACH cells away, the corner rotations of
    d2a2c_vect and the replace of a2b_ord4 included -- so one column perturbs a whole lattice of points SPACING apart on one level and
    every point collects the seeds in its own window.  test_emul_face_edges.py::test_coloured_adjoint_is_the_exact_one holds this
    to the one-point-per-column form."""
    ct = np.clongdouble if dtype == np.longdouble else np.complex128
    if getattr(op, "level_local", False) and next(iter(T.values())).shape[0] > 1:      # no statement couples two levels: one at a time
        parts = [_adjoint(op, {k: v[l:l + 1] for k, v in T.items()}, {k: v[l:l + 1] for k, v in seeds.items()}, M, edge, ecorner, dtype,
                          {k: v[l:l + 1] for k, v in points.items()}, chunk, coloured) for l in range(next(iter(T.values())).shape[0])]
        return {k: np.concatenate([p_[k] for p_ in parts], axis=0) for k in T}
    res = {k: np.zeros(T[k].shape, dtype=dtype) for k in T}

    def seeded(o):
        out = {}
        for on, s in seeds.items():
            d = np.where(s != 0, np.imag(o[on]) / dtype(H), 0)
            assert np.all(np.isfinite(d.astype(np.float64))), ("the restatement read an undefined entry", on)
            out[on] = d * s
        return out
    for name in T:
        if coloured:
            nlev, pj = T[name].shape[0], T[name].shape[-1]
            cols = [(l, a, b) for l in range(nlev) for a in range(SPACING) for b in range(SPACING) if points[name][l, a::SPACING, b::SPACING].any()]
            for c0 in range(0, len(cols), chunk):
                sub = cols[c0:c0 + chunk]
                z = {k: np.broadcast_to(T[k].astype(ct), (len(sub),) + T[k].shape) for k in T}
                zz = z[name].copy()
                for q, (l, a, b) in enumerate(sub):
                    zz[q, l, a::SPACING, b::SPACING] += 1j * ct(H)
                z[name] = zz
                ds = seeded(op.apply(z, M, edge, ecorner))
                tot = sum(v.sum(axis=1) for v in ds.values())          # over the output levels: [ncol, pj, pj]
                pad = np.zeros((len(sub), pj + 2 * REACH, pj + 2 * REACH), dtype=dtype)
                pad[:, REACH:-REACH, REACH:-REACH] = tot
                csum = np.cumsum(np.cumsum(pad, axis=1), axis=2)
                csum = np.pad(csum, ((0, 0), (1, 0), (1, 0)))
                w = 2 * REACH + 1                                       # window sums centred on every point
                win = csum[:, w:, w:] - csum[:, :-w, w:] - csum[:, w:, :-w] + csum[:, :-w, :-w]
                for q, (l, a, b) in enumerate(sub):
                    res[name][l, a::SPACING, b::SPACING] = win[q, a::SPACING, b::SPACING]
            res[name] = np.where(points[name], res[name], 0)
            continue
        idx = np.argwhere(points[name])
        for c0 in range(0, len(idx), chunk):
            sub = idx[c0:c0 + chunk]
            z = {k: np.broadcast_to(T[k].astype(ct), (len(sub),) + T[k].shape) for k in T}
            zz = z[name].copy()
            zz[np.arange(len(sub)), sub[:, 0], sub[:, 1], sub[:, 2]] += 1j * ct(H)
            z[name] = zz
            ds = seeded(op.apply(z, M, edge, ecorner))
            res[name][sub[:, 0], sub[:, 1], sub[:, 2]] = sum(v.reshape(len(sub), -1).sum(axis=1) for v in ds.values())
    return res


def near_edge(n, cells=4):
    pj = n + 7
    J, I = np.meshgrid(np.arange(pj) - 2, np.arange(pj) - 2, indexing="ij")
    return (I <= cells + 1) | (I >= n + 1 - cells) | (J <= cells + 1) | (J >= n + 1 - cells)


def check(backend, group, n, face, npz=3, adjoint_all=True, seed=0, report=None, coloured=False, adjoint_levels=None, env=None):
    """values, tangent and adjoint of one operator on one whole face; returns [(mode, output, region, movement, bound, error)].
    adjoint_all: J^T s entry by entry at every input point; otherwise at the points within four cells of a face edge on the first
    adjoint_levels levels (None: all), and four random dot products <s, J dx> = <J^T s, dx> for all the other points."""
    import os
    from common import Case
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})                              # switches the library reads when an instance is created
    try:
        c = Case(nx=n, ny=n, npz=npz, n_split=2, dt=1800.0, backend=backend, face=face, oracle=False, metrics_hook=restatement_hook(n, face))
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    op = OPERATORS[group](c)
    M64, e64, ec64 = face_metrics_of(n, face, np.float64)
    ML, eL, ecL = face_metrics_of(n, face, np.longdouble)
    rng = np.random.default_rng(1000 * n + 10 * face + seed)
    for _ in range(50):                                      # redraw until the trajectory takes both branches everywhere, clear of zero
        T, P = op.draw(c, rng)
        if op.signs_ok(T, M64, e64, ec64):
            break
    else:
        raise AssertionError("no trajectory with both signs on every edge row")
    Tn, Pn = _ghost_fill(c, T, np.nan), _ghost_fill(c, P, np.nan)
    rects, rows = G.rects(c), []
    masks = {o: compared_mask(c, o, rk) for o, rk in op.outs}
    L = lambda d: {k: v.astype(np.longdouble) for k, v in d.items()}
    ref = _tangent(op, L(Tn), L(Pn), ML, eL, ecL, np.longdouble)
    # ---- values and tangent
    fixed = op.fixed(c)
    for k, v in fixed.items():
        c.dy.put(k, v[None], 0); c.dy.put(k, np.zeros_like(v)[None], 1)
    Tg, Pg = _ghost_fill(c, T, 1.0e30), _ghost_fill(c, P, 1.0e30)
    for k in op.ins:
        c.dy.put(k, Tg[k][None], 0); c.dy.put(k, Pg[k][None], 1)
    c.dy.run_group(group, TL)
    got = {o: (c.dy.get(o, 0)[0], c.dy.get(o, 1)[0]) for o, _ in op.outs}
    move = {}
    for d in range(3):
        Td, Pd = {k: ulp_move(rng, v) for k, v in Tn.items()}, {k: ulp_move(rng, v) for k, v in Pn.items()}
        r64 = _tangent(op, Td, Pd, M64, e64, ec64, np.float64)
        for o, rk in op.outs:
            for w, tag in ((0, "values"), (1, "tangent")):
                for reg, e in region_errors(r64[o][w], ref[o][w], masks[o], n, rects[rk]).items():
                    move[(tag, o, reg)] = max(move.get((tag, o, reg), 0.0), e)
    for o, rk in op.outs:
        for w, tag in ((0, "values"), (1, "tangent")):
            for reg, e in region_errors(got[o][w], ref[o][w], masks[o], n, rects[rk]).items():
                mv = move[(tag, o, reg)]
                rows.append((tag, o, reg, mv, max(8 * mv, FLOOR), e))
    # ---- adjoint: seeds on the compared outputs only
    seeds = {o: np.where(masks[o], rng.standard_normal((c.dy.levels(o), n + 7, n + 7)), 0.0) for o, _ in op.outs}
    for k, v in fixed.items():
        c.dy.put(k, v[None], 0)
    for k in op.ins:
        c.dy.put(k, Tg[k][None], 0)
    c.dy.run_group(group, NL)
    c.dy.zero_work_adjoint()
    _, _, gins, gouts = G.table(c)[group]
    for k in set(gins) | {o for o, _ in gouts if o}:
        c.dy.put(k, np.zeros(c.dy.shape(k)), 1)
    for o, s in seeds.items():
        c.dy.put(o, s[None], 1)
    c.dy.run_group(group, AD)
    gota = {k: c.dy.get(k, 1)[0] for k in op.ins}
    ne = near_edge(n)
    pts = {k: np.broadcast_to(ne if not adjoint_all else np.ones_like(ne), T[k].shape).copy() for k in op.ins}
    for k in op.ins:
        if k in GHOST_FREE:
            pts[k][:, fo._ghost(n)] = False                   # no data there: nothing to differentiate with respect to
        if not adjoint_all and adjoint_levels is not None:
            pts[k][adjoint_levels:] = False
    nl = {k: (T[k].shape[0] if adjoint_all or adjoint_levels is None else adjoint_levels) for k in op.ins}      # levels compared entry by entry
    refa = _adjoint(op, L(Tn), L(seeds), ML, eL, ecL, np.longdouble, pts, coloured=coloured)
    mva = {}
    for d in range(3):
        r64 = _adjoint(op, {k: ulp_move(rng, v) for k, v in Tn.items()}, seeds, M64, e64, ec64, np.float64, pts, coloured=coloured)
        for k in op.ins:
            for reg, e in (region_errors(r64[k][:nl[k]], refa[k][:nl[k]], pts[k][0], n, rects["full"]).items() if nl[k] else ()):
                mva[(k, reg)] = max(mva.get((k, reg), 0.0), e)
    for k in op.ins:
        for reg, e in (region_errors(gota[k][:nl[k]], refa[k][:nl[k]], pts[k][0], n, rects["full"]).items() if nl[k] else ()):
            rows.append(("adjoint", k, reg, mva[(k, reg)], max(8 * mva[(k, reg)], FLOOR), e))
    if not adjoint_all:                                        # the rest of the plane: four random dot products <s, J dx> = <J^T s, dx>
        for d in range(4):
            dx = {k: np.where(pts[k], 0.0, noise(rng, T[k].shape, 1.0)) for k in op.ins}
            for k in GHOST_FREE:
                if k in dx:
                    dx[k][:, fo._ghost(n)] = 0.0
            jdx = _tangent(op, L(Tn), L(dx), ML, eL, ecL, np.longdouble)
            lhs = sum(float(np.sum(np.where(seeds[o] != 0, jdx[o][1], 0) * seeds[o])) for o, _ in op.outs)
            rhs = sum(float(np.sum(gota[k] * dx[k])) for k in op.ins)
            scale = sum(float(np.sum(np.abs(np.where(seeds[o] != 0, jdx[o][1], 0) * seeds[o]))) for o, _ in op.outs)
            rows.append(("adjoint", "dot%d" % d, "rest", 0.0, FLOOR, abs(lhs - rhs) / scale))
    if report is not None:
        report.extend((group, n, face) + r for r in rows)
    bad = [r for r in rows if not r[5] <= r[4]]
    assert not bad, (group, n, face, bad[:8])
    return rows


# ------------------------------------------------------------------------------------------------------------ faces cut into tiles
class _FaceShape:
    """what the operator classes and groups.py read of a case, for a whole face of the cube behind a tiled CubeCase"""
    def __init__(self, c):
        self.nx = self.ny = c.n
        self.npz, self.dt_ac, self.opt, self.face = c.npz, c.dt_ac, c.opt, "cube"

    def rect(self, i0, i1, j0, j1):
        return (Ellipsis, slice(j0 + 2, j1 + 3), slice(i0 + 2, i1 + 3))


def check_layout(backend, group, n=16, layout=2, npz=3, report=None):
    """Six faces of C<n> cut layout x layout (the tile offset into edge[] and the clipped strip rects of the a2b builders): every tile's
    outputs on its own rects against the windows of the whole-face restatement, values and tangent per point and region (regions of the
    tile), and the adjoint through four dot products <s, J dx> = <J^T s, dx> summed over the tiles, dx and J dx from the restatement."""
    from common import CubeCase
    from fv3_jedi_linearmodel_amd import cube
    c = CubeCase(n=n, npz=npz, n_split=2, backend=backend, layout=layout, oracle=False, metrics_hook=restatement_hook(n))
    fc = _FaceShape(c)
    op = OPERATORS[group](fc)
    nt, tl = c.nt, c.tiles
    W = lambda a: cube.tile_window(a, tl, nt)                    # [6, ..., pj, pj] -> [ntile, ..., nt+7, nt+7]
    rng = np.random.default_rng(7 * n + layout)
    Ms = [face_metrics_of(n, f, np.float64) for f in range(6)]
    MLs = [face_metrics_of(n, f, np.longdouble) for f in range(6)]
    T6, P6 = [], []
    for f in range(6):
        for _ in range(50):
            T, P = op.draw(fc, rng)
            if op.signs_ok(T, *Ms[f]):
                break
        else:
            raise AssertionError("no trajectory with both signs on every edge row")
        T6.append(T); P6.append(P)
    stack = lambda d6, fill: {k: np.stack([_ghost_fill(fc, d, fill)[k] for d in d6]) for k in d6[0]}
    L = lambda d: {k: v.astype(np.longdouble) for k, v in d.items()}
    Tn, Pn = [_ghost_fill(fc, d, np.nan) for d in T6], [_ghost_fill(fc, d, np.nan) for d in P6]
    ref = [_tangent(op, L(Tn[f]), L(Pn[f]), *MLs[f], np.longdouble) for f in range(6)]
    refw = {o: [W(np.stack([ref[f][o][w] for f in range(6)])) for w in (0, 1)] for o, _ in op.outs}
    # masks per tile: the tile's own rect minus the windows of the points that hold no value on the face
    rects = G.rects(c)
    one = np.ones((6, 1, n + 7, n + 7))
    masks = {}
    for o, rk in op.outs:
        dropped = W(np.stack([G.drop_face_corners(fc, o, one[f]) for f in range(6)]))[:, 0] == 0
        masks[o] = (G.masked(c, np.ones((len(tl), 1, nt + 7, nt + 7)), rk)[:, 0] != 0) & ~dropped
    if group == "c_sw":
        for k in ("delp", "pt"):
            c.dy.put(k, c.traj[k], 0); c.dy.put(k, np.zeros_like(c.traj[k]), 1)
    Tg = {k: W(v) for k, v in stack(T6, 1.0e30).items()}; Pg = {k: W(v) for k, v in stack(P6, 1.0e30).items()}
    for k in op.ins:
        c.dy.put(k, Tg[k], 0); c.dy.put(k, Pg[k], 1)
    c.dy.run_group(group, TL)
    got = {o: (c.dy.get(o, 0), c.dy.get(o, 1)) for o, _ in op.outs}
    move, rows = {}, []
    for d in range(3):
        r64 = [_tangent(op, {k: ulp_move(rng, v) for k, v in Tn[f].items()}, {k: ulp_move(rng, v) for k, v in Pn[f].items()}, *Ms[f], np.float64)
               for f in range(6)]
        for o, rk in op.outs:
            for w, tag in ((0, "values"), (1, "tangent")):
                rw = W(np.stack([r64[f][o][w] for f in range(6)]))
                for t in range(len(tl)):
                    for reg, e in region_errors(rw[t], refw[o][w][t], masks[o][t], nt, rects[rk]).items():
                        move[(tag, o, reg)] = max(move.get((tag, o, reg), 0.0), e)
    err = {}
    for o, rk in op.outs:
        for w, tag in ((0, "values"), (1, "tangent")):
            for t in range(len(tl)):
                for reg, e in region_errors(got[o][w][t], refw[o][w][t], masks[o][t], nt, rects[rk]).items():
                    err[(tag, o, reg)] = max(err.get((tag, o, reg), 0.0), e)
    for k, e in sorted(err.items()):
        rows.append(k + (move[k], max(8 * move[k], FLOOR), e))
    # ---- adjoint: seeds on the compared outputs of every tile
    seeds = {o: np.where(masks[o][:, None], rng.standard_normal(got[o][0].shape), 0.0) for o, _ in op.outs}
    if group == "c_sw":
        for k in ("delp", "pt"):
            c.dy.put(k, c.traj[k], 0)
    for k in op.ins:
        c.dy.put(k, Tg[k], 0)
    c.dy.run_group(group, NL)
    c.dy.zero_work_adjoint()
    _, _, gins, gouts = G.table(c)[group]
    for k in set(gins) | {o for o, _ in gouts if o}:
        c.dy.put(k, np.zeros(c.dy.shape(k)), 1)
    for o, s in seeds.items():
        c.dy.put(o, s, 1)
    c.dy.run_group(group, AD)
    gota = {k: c.dy.get(k, 1) for k in op.ins}
    g6 = fo._ghost(n)
    for d in range(4):
        dx6 = []
        for f in range(6):
            dx = {k: noise(rng, T6[f][k].shape, 1.0) for k in op.ins}
            for k in GHOST_FREE:
                if k in dx:
                    dx[k][:, g6] = 0.0
            dx6.append(dx)
        jdx = [_tangent(op, L(Tn[f]), L(dx6[f]), *MLs[f], np.longdouble) for f in range(6)]
        lhs = scale = 0.0
        for o, _ in op.outs:
            jw = W(np.stack([jdx[f][o][1] for f in range(6)]))
            term = np.where(seeds[o] != 0, jw, 0) * seeds[o]
            lhs += float(np.sum(term)); scale += float(np.sum(np.abs(term)))
        rhs = sum(float(np.sum(gota[k] * W(np.stack([dx6[f][k] for f in range(6)])))) for k in op.ins)
        rows.append(("adjoint", "dot%d" % d, "tiles", 0.0, FLOOR, abs(lhs - rhs) / scale))
    if report is not None:
        report.extend((group, n, "2x2") + r for r in rows)
    bad = [r for r in rows if not r[5] <= r[4]]
    assert not bad, (group, n, layout, bad[:8])
    return rows
