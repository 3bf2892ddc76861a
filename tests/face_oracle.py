"""TEST INFRASTRUCTURE -- a second restatement of the cube-edge metric terms, written from the reference's nonlinear Fortran and from
nothing else: not from csrc/, not from oracle/*.hpp, not from fv3_jedi_linearmodel_amd/cube.py.

Shared input, declared: the cell-corner unit vectors cube.cube_corner_points(n) (what a host hands over as grid(:,:,1:2) after
mpp_update_domains and fill_corners(FILL=XDir, BGRID), tools/fv_grid_tools_nlm.F90:648-650), the radius and omega.  Nothing else is
imported from the package.  The data motion of mpp_update_domains is taken from oracle/cube_topology.py, which derives it from the
reference's contact list by index arithmetic and is itself independent of the package.

Everything is numpy, generic in the dtype (float64, longdouble), on all six faces at once: arrays [6, pj, pj] (pj = n + 7) hold Fortran
element (i, j), i, j = isd .. ied + 1, at [.., j + 2, i + 2]; R(i0, i1, j0, j1) is the one helper that turns Fortran ranges into slices and
sh(a, di, dj) reads a(i + di, j + dj).  Each block cites the lines it follows (paths relative to src/dynamics/atmos_cubed_sphere/).

Three kinds of entries come out:
  defined    a finite number: the value the reference holds there.
  poisoned   the reference leaves tiny_number / big_number there (fill_ghost, initial fills) or the element lies outside its array:
             `poison[name]` is True.  "This will cause NAN if used" (model/fv_grid_utils_nlm.F90:563).
  degenerate NaN here.  The reference holds a number there that is neither tiny nor big but carries no geometry: it was computed
             from the cell centre of a corner-halo cell, whose longitude fill_corners takes from one cell and whose latitude from
             another (tools/fv_grid_tools_nlm.F90:712-713: XDir for lon, YDir for lat), or from sin_sg / cos_sg values of corner-halo
             cells that the reference goes on to poison (:561-566).  They are treated like poison: never compared, and overwritten in
             the poison runs, which is the stricter reading.
"""
import os
import sys
import numpy as np

NG = 3
BIG, TINY = 1.0e8, 1.0e-8            # model/fv_grid_utils_nlm.F90:49-50
_ORACLE_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle")


def R(i0, i1, j0, j1):
    """slices of a padded plane [6, pj, pj(, 3)] for the Fortran ranges i0..i1, j0..j1"""
    return (slice(None), slice(j0 + NG - 1, j1 + NG), slice(i0 + NG - 1, i1 + NG))


def at(i, j):
    return (slice(None), j + NG - 1, i + NG - 1)


def sh(a, di, dj):
    """b(i, j) = a(i + di, j + dj); NaN where that leaves the plane"""
    b = np.full_like(a, np.nan)
    pj = a.shape[1]
    d0, d1 = max(0, -dj), min(pj, pj - dj)
    e0, e1 = max(0, -di), min(pj, pj - di)
    b[:, d0:d1, e0:e1] = a[:, d0 + dj:d1 + dj, e0 + di:e1 + di]
    return b


# ------------------------------------------------------------------------------------------------------- vector algebra on [..., 3]
def _dot(a, b):
    return a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]


def _cross(a, b):                                    # vect_cross, model/fv_grid_utils_nlm.F90:1708-1718
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1)


def _unit(a):                                        # normalize_vect :1807
    with np.errstate(invalid="ignore", divide="ignore"):
        return a / np.sqrt(_dot(a, a))[..., None]


def _mid(a, b):                                      # mid_pt3_cart :1923-1949
    return _unit(a + b)


def _lonlat(p):                                      # cart_to_latlon :1666-1704
    p = _unit(p)
    return np.arctan2(p[..., 1], p[..., 0]), np.arcsin(p[..., 2])


def _gcd(p, q):                                      # great_circle_dist :1967-1989, on the longitudes / latitudes the reference stores
    (l1, t1), (l2, t2) = _lonlat(p), _lonlat(q)
    return 2 * np.arcsin(np.sqrt(np.sin((t1 - t2) / 2) ** 2 + np.cos(t1) * np.cos(t2) * np.sin((l1 - l2) / 2) ** 2))


def _pq(p1, p2, p3):
    P, Q = _cross(p1, p2), _cross(p1, p3)
    return _dot(P, Q), _dot(P, P) * _dot(Q, Q)


def _cos_angle(p1, p2, p3):                          # cos_angle :2825-2869: cos of the angle at p1 between p2 and p3; 1 where degenerate
    num, dd = _pq(p1, p2, p3)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(dd > 0, num / np.sqrt(dd), np.where(np.isnan(dd), np.nan, 1.0)).astype(p1.dtype)


def _sph_angle(p1, p2, p3):                          # spherical_angle :2765-2822
    num, dd = _pq(p1, p2, p3)
    with np.errstate(invalid="ignore", divide="ignore"):
        c = num / np.sqrt(dd)
    c = np.where(dd > 0, np.clip(c, -1, 1), 1.0)
    return np.where(np.isnan(dd), np.nan, np.arccos(c)).astype(p1.dtype)


def _quad_area(q1, q2, q3, q4):                      # get_area :2676-2717 (q1..q4 in cyclic order): spherical excess
    pi = np.arccos(np.array(-1, dtype=q1.dtype))
    return _sph_angle(q1, q2, q4) + _sph_angle(q2, q3, q1) + _sph_angle(q3, q4, q2) + _sph_angle(q4, q3, q1) - 2 * pi


# ------------------------------------------------------------------------------------------------------- data motion
_TABLES = {}


def _tables(n):
    if n not in _TABLES:
        if _ORACLE_DIR not in sys.path:
            sys.path.insert(0, _ORACLE_DIR)
        import cube_topology as ct
        _TABLES[n] = {k: ct.exchange_table(n, k) for k in ("cell", "dvec", "cvec", "corner")}
    return _TABLES[n]


def _update_domains(n, kind, *fields):
    """mpp_update_domains of a scalar or of a SCALAR_PAIR (no sign change, components swapped across rotated contacts)"""
    tab = _tables(n)[kind]
    flat = [f.reshape(6, f.shape[1] * f.shape[2], *f.shape[3:]) for f in fields]
    src = [flat[r[3]][r[4], r[5]].copy() for r in tab]
    for r, v in zip(tab, src):
        flat[r[0]][r[1], r[2]] = v


def _fill_corners(n, kind, x, y=None):
    """fill_corners of tools/fv_mp_nlm_mod.F90, the variants grid_init uses: 'B' = BGRID, FILL=XDir (:1057-1064); 'D' = DGRID pair (x on
    the u points, y on the v points, :1278-1301); 'A' = AGRID pair (:1454-1469); 'C' = CGRID pair (x on the uc points, y on the vc
    points, :1390-1405)"""
    npx = npy = n + 1
    for j in range(1, NG + 1):
        for i in range(1, NG + 1):
            if kind == "B":
                x[at(1 - i, 1 - j)] = x[at(1 - j, i + 1)]; x[at(1 - i, npy + j)] = x[at(1 - j, npy - i)]
                x[at(npx + i, 1 - j)] = x[at(npx + j, i + 1)]; x[at(npx + i, npy + j)] = x[at(npx + j, npy - i)]
            elif kind == "D":
                x[at(1 - i, 1 - j)] = y[at(1 - j, i)]; x[at(1 - i, npy + j)] = y[at(1 - j, npy - i)]
                x[at(npx - 1 + i, 1 - j)] = y[at(npx + j, i)]; x[at(npx - 1 + i, npy + j)] = y[at(npx + j, npy - i)]
            elif kind == "A":
                x[at(1 - i, 1 - j)] = y[at(1 - j, i)]; x[at(1 - i, npy - 1 + j)] = y[at(1 - j, npy - i)]
                x[at(npx - 1 + i, 1 - j)] = y[at(npx - 1 + j, i)]; x[at(npx - 1 + i, npy - 1 + j)] = y[at(npx - 1 + j, npy - i)]
            elif kind == "C":
                x[at(1 - i, 1 - j)] = y[at(j, 1 - i)]; x[at(1 - i, npy - 1 + j)] = y[at(j, npy + i)]
                x[at(npx + i, 1 - j)] = y[at(npx - j, 1 - i)]; x[at(npx + i, npy - 1 + j)] = y[at(npx - j, npy + i)]
    if kind == "B":
        return
    for j in range(1, NG + 1):
        for i in range(1, NG + 1):
            if kind == "D":
                y[at(1 - i, 1 - j)] = x[at(j, 1 - i)]; y[at(1 - i, npy - 1 + j)] = x[at(j, npy + i)]
                y[at(npx + i, 1 - j)] = x[at(npx - j, 1 - i)]; y[at(npx + i, npy - 1 + j)] = x[at(npx - j, npy + i)]
            elif kind == "A":
                y[at(1 - j, 1 - i)] = x[at(i, 1 - j)]; y[at(1 - j, npy - 1 + i)] = x[at(i, npy - 1 + j)]
                y[at(npx - 1 + j, 1 - i)] = x[at(npx - i, 1 - j)]; y[at(npx - 1 + j, npy - 1 + i)] = x[at(npx - i, npy - 1 + j)]
            elif kind == "C":
                y[at(1 - i, 1 - j)] = x[at(1 - j, i)]; y[at(1 - i, npy + j)] = x[at(1 - j, npy - i)]
                y[at(npx - 1 + i, 1 - j)] = x[at(npx + j, i)]; y[at(npx - 1 + i, npy + j)] = x[at(npx + j, npy - i)]


def _ghost(n, staggered=False):
    """the cells fill_ghost writes (model/fv_grid_utils_nlm.F90:3017-3032) as a mask [pj, pj]"""
    pj = n + 2 * NG + 1
    J, I = np.meshgrid(np.arange(pj) - NG + 1, np.arange(pj) - NG + 1, indexing="ij")
    npx = npy = n + 1
    return ((I < 1) & (J < 1)) | ((I > npx - 1) & (J < 1)) | ((I > npx - 1) & (J > npy - 1)) | ((I < 1) & (J > npy - 1))


# ------------------------------------------------------------------------------------------------------- grid_init + grid_utils_init
DIMENSIONAL = "area,rarea,rarea_c,dx,dy,dxa,dya,dxc,dyc,rdx,rdy,rdxa,rdya,rdxc,rdyc,f0,fC".split(",")
METRIC_PLANES = ("area,rarea,rarea_c,dx,dy,dxa,dya,dxc,dyc,rdx,rdy,rdxa,rdya,rdxc,rdyc,cosa,sina,rsina,cosa_u,cosa_v,cosa_s,sina_u,sina_v,"
                 "rsin_u,rsin_v,rsin2,f0,fC,del6_u,del6_v,divg_u,divg_v").split(",") + ["sin_sg%d" % k for k in range(1, 10)] + \
                ["cos_sg%d" % k for k in range(1, 10)]


def face_metrics(corners, radius=6371.0e3, omega=7.292e-5, dtype=np.float64, literal_se_corner=False):
    """grid_init (tools/fv_grid_tools_nlm.F90:648-937) and grid_utils_init (model/fv_grid_utils_nlm.F90:78-838) for a non-nested,
    non-stretched cubed sphere with one tile per face (sw/se/ne/nw_corner all true), from the corner points [6, pj, pj, 3].
    Returns (m, poison, edge, ecorner, c2l): m[name] [6, pj, pj] with the reference's values (tiny / big where it leaves them, NaN where
    degenerate or outside its array), poison[name] boolean, edge [6, 4, pj] (w, e, s, n by plane position; NaN outside 2..npx-1),
    ecorner [6, 4, 3] (sw, se, ne, nw; the three extrap_corner calls in the reference's order), c2l [6, 4, pj, pj] (a11 a12 a21 a22).

    literal_se_corner: area_c(npx, 1).  The reference closes that corner kite with agrid(npx, 1), the centre of the NEIGHBOUR's cell
    (tools/fv_grid_tools_nlm.F90:841), where the other three corners take the cell inside the face (:832, :846, :855); the spherical
    excess of the resulting self-crossing quadrilateral is negative (about -300 times the area of its three sisters).  By default
    the restatement takes agrid(npx - 1, 1), which makes the four corners alike; True gives the reference's own number."""
    g = np.asarray(corners, dtype=dtype)
    pj = g.shape[1]; n = pj - 2 * NG - 1
    npx = npy = n + 1
    isd, ied, jsd, jed = 1 - NG, n + NG, 1 - NG, n + NG
    nan = lambda: np.full((6, pj, pj), np.nan, dtype=dtype)
    ghost = _ghost(n)
    g10, g01, g11 = sh(g, 1, 0), sh(g, 0, 1), sh(g, 1, 1)              # grid3(i+1,j), (i,j+1), (i+1,j+1)
    m = {}

    # ---- dx, dy: tools/fv_grid_tools_nlm.F90:653-688 (the symmetric branch gives the same lengths by another route)
    dx, dy = nan(), nan()
    dx[R(1, n, 1, n + 1)] = (radius * _gcd(g10, g))[R(1, n, 1, n + 1)]
    dy[R(1, n + 1, 1, n)] = (radius * _gcd(g01, g))[R(1, n + 1, 1, n)]
    _update_domains(n, "dvec", dx, dy)
    _fill_corners(n, "D", dx, dy)
    # ---- agrid: :693-713.  Corner halo: lon by XDir, lat by YDir from two different cells -> degenerate (NaN)
    a = np.full((6, pj, pj, 3), np.nan, dtype=dtype)
    a[R(1, n, 1, n)] = _unit(g + g10 + g01 + g11)[R(1, n, 1, n)]       # cell_center2, model/fv_grid_utils_nlm.F90:2627-2652
    _update_domains(n, "cell", a)
    # ---- dxa, dya: :715-727
    dxa, dya = nan(), nan()
    dxa[R(isd, ied, jsd, jed)] = (radius * _gcd(_mid(g10, g11), _mid(g, g01)))[R(isd, ied, jsd, jed)]
    dya[R(isd, ied, jsd, jed)] = (radius * _gcd(_mid(g01, g11), _mid(g, g10)))[R(isd, ied, jsd, jed)]
    _fill_corners(n, "A", dxa, dya)
    # ---- dxc, dyc: :734-752, face edges :776-826, exchange and corners :863-865
    dxc, dyc = nan(), nan()
    dxc[R(isd + 1, ied, jsd, jed)] = (radius * _gcd(a, sh(a, -1, 0)))[R(isd + 1, ied, jsd, jed)]
    dxc[R(isd, isd, jsd, jed)] = dxc[R(isd + 1, isd + 1, jsd, jed)]; dxc[R(ied + 1, ied + 1, jsd, jed)] = dxc[R(ied, ied, jsd, jed)]
    dyc[R(isd, ied, jsd + 1, jed)] = (radius * _gcd(a, sh(a, 0, -1)))[R(isd, ied, jsd + 1, jed)]
    dyc[R(isd, ied, jsd, jsd)] = dyc[R(isd, ied, jsd + 1, jsd + 1)]; dyc[R(isd, ied, jed + 1, jed + 1)] = dyc[R(isd, ied, jed, jed)]
    mx, my = _mid(g, g01), _mid(g, g10)                               # mid-points of the west / south edge of cell (i, j)
    dxc[R(1, 1, 1, n)] = (2 * radius * _gcd(mx, a))[R(1, 1, 1, n)]
    dxc[R(npx, npx, 1, n)] = (2 * radius * _gcd(sh(a, -1, 0), mx))[R(npx, npx, 1, n)]
    dyc[R(1, n, 1, 1)] = (2 * radius * _gcd(my, a))[R(1, n, 1, 1)]
    dyc[R(1, n, npy, npy)] = (2 * radius * _gcd(sh(a, 0, -1), my))[R(1, n, npy, npy)]
    _update_domains(n, "cvec", dxc, dyc)
    _fill_corners(n, "C", dxc, dyc)
    # ---- area: grid_area :1987-2009, exchange :867, fill_ghost(-big) :902
    area = nan()
    area[R(1, n, 1, n)] = (radius ** 2 * _quad_area(g, g10, g11, g01))[R(1, n, 1, n)]
    _update_domains(n, "cell", area)
    area[:, ghost] = -BIG
    # ---- area_c: grid_area :2051-2069 (the corner triangles of :2071-2139 are overwritten below), face edges :767-826, corners :828-859,
    #      exchange :898, fill_corners(XDir, BGRID) :903
    area_c = nan()
    amm, a0m, am0 = sh(a, -1, -1), sh(a, 0, -1), sh(a, -1, 0)
    area_c[R(1, npx, 1, npy)] = (radius ** 2 * _quad_area(amm, a0m, a, am0))[R(1, npx, 1, npy)]
    mxm, mym = sh(mx, 0, -1), sh(my, -1, 0)                           # mid(grid(i,j-1), grid(i,j)), mid(grid(i-1,j), grid(i,j))
    area_c[R(1, 1, 1, npy)] = (2 * radius ** 2 * _quad_area(mxm, a0m, a, mx))[R(1, 1, 1, npy)]
    area_c[R(npx, npx, 1, npy)] = (2 * radius ** 2 * _quad_area(amm, mxm, mx, am0))[R(npx, npx, 1, npy)]
    area_c[R(1, npx, 1, 1)] = (2 * radius ** 2 * _quad_area(mym, my, a, am0))[R(1, npx, 1, 1)]
    area_c[R(1, npx, npy, npy)] = (2 * radius ** 2 * _quad_area(amm, a0m, my, mym))[R(1, npx, npy, npy)]
    for (i, j, q) in ((1, 1, (g, my, a, mx)), (npx, 1, (mym, g, mx, a if literal_se_corner else am0)), (npx, npy, (amm, mxm, g, mym)), (1, npy, (mxm, a0m, my, g))):
        area_c[at(i, j)] = 3 * radius ** 2 * _quad_area(*[v[at(i, j)] for v in q])
    _update_domains(n, "corner", area_c)
    _fill_corners(n, "B", area_c)
    m.update(dx=dx, dy=dy, dxa=dxa, dya=dya, dxc=dxc, dyc=dyc, area=area)
    with np.errstate(divide="ignore", invalid="ignore"):               # :906-937
        for k in ("dx", "dy", "dxa", "dya", "dxc", "dyc", "area"):
            m["r" + k] = 1 / m[k]
        m["rarea_c"] = 1 / area_c
    m["rarea"][:, ghost] = -1 / BIG

    # ============================== grid_utils_init, model/fv_grid_utils_nlm.F90
    cells = R(isd, ied, jsd, jed)
    # ---- get_center_vect :1722-1772 (zero in the corner halo)
    pc = _unit(g + g10 + g01 + g11)
    ec1 = _unit(_cross(pc, _cross(_mid(g10, g11), _mid(g, g01))))
    ec2 = _unit(_cross(pc, _cross(_mid(g01, g11), _mid(g, g10))))
    ec1[:, ghost] = 0; ec2[:, ghost] = 0
    # ---- cos_sg, sin_sg :211-212, :318-357
    cs = [None] + [np.full((6, pj, pj), BIG, dtype=dtype) for _ in range(9)]
    sn = [None] + [np.full((6, pj, pj), TINY, dtype=dtype) for _ in range(9)]
    raw = {6: _cos_angle(g, g10, g01), 7: -_cos_angle(g10, g, g11), 8: _cos_angle(g11, g10, g01), 9: -_cos_angle(g01, g, g11),
           1: _cos_angle(_mid(g, g01), a, g01), 2: _cos_angle(_mid(g, g10), g10, a), 3: _cos_angle(_mid(g10, g11), a, g10),
           4: _cos_angle(_mid(g01, g11), g01, a), 5: _dot(ec1, ec2)}
    one, zero = np.array(1, dtype=dtype), np.array(0, dtype=dtype)
    for k in range(1, 10):
        cs[k][cells] = raw[k][cells]
        sn[k][cells] = np.minimum(one, np.sqrt(np.maximum(zero, 1 - cs[k] ** 2)))[cells]
    for a_ in cs[1:] + sn[1:]:                                        # outside the reference's arrays (isd:ied, jsd:jed)
        a_[:, -1, :] = np.nan; a_[:, :, -1] = np.nan

    def transport_overrides(both):
        """:363-391 (sin_sg only, before the edge sines are formed) and :571-627 (sin_sg and cos_sg, after fill_ghost)"""
        for arr in ([sn, cs] if both else [sn]):
            for i in (0, -1, -2):                                      # sw
                arr[3][at(0, i)] = arr[2][at(i, 1)]; arr[4][at(i, 0)] = arr[1][at(1, i)]
            for i in (npy, npy + 1, npy + 2):                          # nw
                arr[3][at(0, i)] = arr[4][at(npy - i, npy - 1)]
            for i in (0, -1, -2):                                      # the first pass reads (1, npx + i), the second (1, npy - i)
                arr[2][at(i, npy)] = arr[1][at(1, npy - i if both else npx + i)]
            for j in (0, -1, -2):                                      # se
                arr[1][at(npx, j)] = arr[2][at(npx - j, 1)]
            for i in (npx, npx + 1, npx + 2):
                arr[4][at(i, 0)] = arr[3][at(npx - 1, npx - i)]
            for i in (0, 1, 2):                                        # ne
                arr[1][at(npx, npy + i)] = arr[4][at(npx + i, npy - 1)]; arr[2][at(npx + i, npy)] = arr[3][at(npx - 1, npy + i)]
    transport_overrides(False)
    # ---- cosa, sina :454-491 (big outside is..ie+1)
    cosa, sina = np.full((6, pj, pj), BIG, dtype=dtype), np.full((6, pj, pj), BIG, dtype=dtype)
    B = R(1, npx, 1, npy)
    cosa[B] = (0.5 * (sh(cs[8], -1, -1) + cs[6]))[B]; sina[B] = (0.5 * (sh(sn[8], -1, -1) + sn[6]))[B]
    for (i, j) in ((1, 1), (npx, 1), (npx, npy), (1, npy)):            # degenerate: one of the two angles is that of the corner-halo
        cosa[at(i, j)] = np.nan; sina[at(i, j)] = np.nan               # cell at the vertex, two of whose corners are one point
    # ---- cosa_u, sina_u, rsin_u, cosa_v, sina_v, rsin_v, cosa_s, rsin2 :445-453, :498-525
    big = lambda: np.full((6, pj, pj), BIG, dtype=dtype)
    cosa_u, sina_u, rsin_u, cosa_v, sina_v, rsin_v, cosa_s, rsin2, rsina = (big() for _ in range(9))
    tiny = np.array(TINY, dtype=dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        U = R(isd + 1, ied, jsd, jed)
        cosa_u[U] = (0.5 * (sh(cs[3], -1, 0) + cs[1]))[U]; sina_u[U] = (0.5 * (sh(sn[3], -1, 0) + sn[1]))[U]
        rsin_u[U] = (1 / np.maximum(tiny, sina_u ** 2))[U]
        V = R(isd, ied, jsd + 1, jed)
        cosa_v[V] = (0.5 * (sh(cs[4], 0, -1) + cs[2]))[V]; sina_v[V] = (0.5 * (sh(sn[4], 0, -1) + sn[2]))[V]
        rsin_v[V] = (1 / np.maximum(tiny, sina_v ** 2))[V]
        cosa_s[cells] = cs[5][cells]; rsin2[cells] = (1 / np.maximum(tiny, sn[5] ** 2))[cells]
        cosa_s[:, ghost] = BIG
        rsin2[:, ghost] = np.nan                                       # degenerate: sin_sg5 = 1 there from ec1 = ec2 = 0 (:1743-1744)
        # ---- edge forms :529-557
        inner = R(2, npx - 1, 2, npy - 1)
        rsina[inner] = (1 / np.maximum(tiny, sina ** 2))[inner]
        for i in (1, npx):
            rsin_u[R(i, i, jsd, jed)] = (1 / (np.sign(sina_u) * np.maximum(tiny, np.abs(sina_u))))[R(i, i, jsd, jed)]
        for j in (1, npy):
            rsin_v[R(isd, ied, j, j)] = (1 / (np.sign(sina_v) * np.maximum(tiny, np.abs(sina_v))))[R(isd, ied, j, j)]
    for a_ in (cosa_u, sina_u, rsin_u):                                # arrays (isd:ied+1, jsd:jed)
        a_[:, -1, :] = np.nan
    for a_ in (cosa_v, sina_v, rsin_v):                                # arrays (isd:ied, jsd:jed+1)
        a_[:, :, -1] = np.nan
    for a_ in (cosa_s, rsin2):
        a_[:, -1, :] = np.nan; a_[:, :, -1] = np.nan
    # ---- the poisoning of the corner halo and the values put back for transport :561-627
    for k in range(1, 10):
        sn[k][:, ghost] = TINY; cs[k][:, ghost] = BIG
    transport_overrides(True)
    # ---- divg_u/v, del6_u/v :700-726, exchange :743-746
    divg_u, del6_u, divg_v, del6_v = nan(), nan(), nan(), nan()
    with np.errstate(divide="ignore", invalid="ignore"):
        Ur = R(isd, ied, jsd, jed + 1)
        divg_u[Ur] = (sina_v * dyc / dx)[Ur]; del6_u[Ur] = (sina_v * dx / dyc)[Ur]
        for j in (1, npy):
            f = 0.5 * (sn[2] + sh(sn[4], 0, -1)); r = R(isd, ied, j, j)
            divg_u[r] = (f * dyc / dx)[r]; del6_u[r] = (f * dx / dyc)[r]
        Vr = R(isd, ied + 1, jsd, jed)
        divg_v[Vr] = (sina_u * dxc / dy)[Vr]; del6_v[Vr] = (sina_u * dy / dxc)[Vr]
        for i in (1, npx):
            f = 0.5 * (sn[1] + sh(sn[3], -1, 0)); r = R(i, i, jsd, jed)
            divg_v[r] = (f * dxc / dy)[r]; del6_v[r] = (f * dy / dxc)[r]
    _update_domains(n, "cvec", divg_v, divg_u)
    _update_domains(n, "cvec", del6_v, del6_u)
    # ---- Coriolis parameters (tools/fv_restart_nlm.F90:347 with alpha = 0, tools/test_cases_nlm.F90:1006-1011)
    f0, fC = nan(), 2 * omega * np.sin(_lonlat(g)[1])
    f0[cells] = (2 * omega * np.sin(_lonlat(a)[1]))[cells]
    m.update(cosa=cosa, sina=sina, rsina=rsina, cosa_u=cosa_u, cosa_v=cosa_v, cosa_s=cosa_s, sina_u=sina_u, sina_v=sina_v, rsin_u=rsin_u,
             rsin_v=rsin_v, rsin2=rsin2, f0=f0, fC=fC, del6_u=del6_u, del6_v=del6_v, divg_u=divg_u, divg_v=divg_v)
    for k in range(1, 10):
        m["sin_sg%d" % k] = sn[k]; m["cos_sg%d" % k] = cs[k]
    poison = {}
    for k, v in m.items():
        with np.errstate(invalid="ignore"):
            if k in ("area", "rarea"):                                 # lengths and areas exceed big_number legitimately
                poison[k] = np.broadcast_to(ghost, v.shape) & np.isfinite(v)
            elif k in DIMENSIONAL:
                poison[k] = np.zeros(v.shape, bool)
            else:
                poison[k] = (np.abs(v) >= BIG) | (np.abs(v) == TINY)
    # rsina = big_number along the face edges (:531-533) is a value the reference reads on purpose (it multiplies a difference that
    # is zero in exact arithmetic): not poison.  The vertex (npx, npy) keeps the initial fill, which is the same number.
    for r in (R(1, npx, 1, 1), R(1, npx, npy, npy), R(1, 1, 1, npy), R(npx, npx, 1, npy)):
        poison["rsina"][r] = False
    # a value formed from a poisoned one: 1 / max(tiny, sin^2) of a tiny sine etc. cannot occur above (the sines are formed first), but
    # divg / del6 at the outermost rows take dyc / dxc copies and the edge sines of poisoned cells only through sina_u/v = big
    for k in ("divg_u", "divg_v", "del6_u", "del6_v"):
        with np.errstate(invalid="ignore"):
            poison[k] |= np.abs(m[k]) >= 1.0e3                         # these ratios are O(1): anything larger carries a big_number
    # ---- edge_factors :1105-1214
    edge = np.full((6, 4, pj), np.nan, dtype=dtype)
    for e, (i, j) in enumerate(((1, None), (npx, None), (None, 1), (None, npy))):
        if j is None:
            pm = _mid(sh(a, -1, 0), a)[:, :, i + NG - 1]              # py(j) = mid(agrid(i-1,j), agrid(i,j)) along j
            gg = g[:, :, i + NG - 1]
        else:
            pm = _mid(sh(a, 0, -1), a)[:, j + NG - 1, :]
            gg = g[:, j + NG - 1, :]
        d1, d2 = _gcd(np.roll(pm, 1, axis=1), gg), _gcd(pm, gg)
        edge[:, e, 2 + NG - 1:npx - 1 + NG] = (d2 / (d1 + d2))[:, 2 + NG - 1:npx - 1 + NG]
    # ---- the extrap_corner coefficients of a2b_ord4 (model/a2b_edge_nlm.F90:108-132, :800-810): x1 / (x2 - x1)
    ecorner = np.zeros((6, 4, 3), dtype=dtype)
    A, G = (lambda i, j: a[at(i, j)]), (lambda i, j: g[at(i, j)])
    calls = [((1, 1), [((1, 1), (2, 2)), ((0, 1), (-1, 2)), ((1, 0), (2, -1))]),
             ((npx, 1), [((npx - 1, 1), (npx - 2, 2)), ((npx - 1, 0), (npx - 2, -1)), ((npx, 1), (npx + 1, 2))]),
             ((npx, npy), [((npx - 1, npy - 1), (npx - 2, npy - 2)), ((npx, npy - 1), (npx + 1, npy - 2)), ((npx - 1, npy), (npx - 2, npy + 1))]),
             ((1, npy), [((1, npy - 1), (2, npy - 2)), ((0, npy - 1), (-1, npy - 2)), ((1, npy), (2, npy + 1))])]
    for c, (p0, trip) in enumerate(calls):
        for q, (p1, p2) in enumerate(trip):
            x1, x2 = _gcd(A(*p1), G(*p0)), _gcd(A(*p2), G(*p0))
            ecorner[:, c, q] = x1 / (x2 - x1)
    # ---- init_cubed_to_latlon :2287-2307 (is-1..ie+1)
    lon, lat = _lonlat(a)
    vlon = np.stack([-np.sin(lon), np.cos(lon), np.zeros_like(lon)], axis=-1)
    vlat = np.stack([-np.sin(lat) * np.cos(lon), -np.sin(lat) * np.sin(lon), np.cos(lat)], axis=-1)
    z11, z12, z21, z22 = _dot(ec1, vlon), _dot(ec1, vlat), _dot(ec2, vlon), _dot(ec2, vlat)
    c2l = np.full((6, 4, pj, pj), np.nan, dtype=dtype)
    H = R(0, n + 1, 0, n + 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        for q, z in enumerate((0.5 * z22 / sn[5], -0.5 * z12 / sn[5], -0.5 * z21 / sn[5], 0.5 * z11 / sn[5])):
            c2l[:, q][H] = z[H]
    c2l[:, :, ghost] = np.nan                                           # 0 / tiny there
    return m, poison, edge, ecorner, c2l


def defined(m, poison):
    """{name: boolean [6, pj, pj]}: the entries that hold the reference's value"""
    return {k: np.isfinite(v) & ~poison[k] for k, v in m.items()}


# =========================================================================================================== operators on one face
# Restated from the nonlinear routines, with their in-place corner fills, on one padded face: fields [..., pj, pj] (any leading axes:
# levels, or a batch of perturbed copies), metrics M[name] [pj, pj] of that face as face_metrics gives them -- poison and NaN included,
# so that a statement that read an undefined entry would show up as a huge or NaN output.  Generic in the dtype, complex included: every
# branch is taken on the real part, so f(x + i h dx).imag / h is the tangent with the trajectory's branch choices (all these routines
# are linear once the signs are fixed, and one_grad_p / p_grad_c are rational), and a batch of unit perturbations gives the Jacobian
# whose transpose is the adjoint reference.
def V(a, i0, i1, j0, j1, di=0, dj=0):
    """a(i0+di : i1+di, j0+dj : j1+dj) of a field [..., pj, pj] as a view (empty where i1 < i0 or j1 < j0)"""
    return a[..., max(j0 + dj + NG - 1, 0):max(j1 + dj + NG, 0), max(i0 + di + NG - 1, 0):max(i1 + di + NG, 0)]


def _pos(x):
    return np.real(x) > 0


A1, A2 = 0.5625, -0.0625                           # 4-pt Lagrange interpolation (sw_core_nlm.F90:51-52, a2b_edge_nlm.F90:35-36)
C1, C2, C3 = -2.0 / 14.0, 11.0 / 14.0, 5.0 / 14.0    # sw_core_nlm.F90:55-57
B1, B2 = 7.0 / 12.0, -1.0 / 12.0                   # a2b_edge_nlm.F90:40-41


def _edge_interpolate4(u1, u2, u3, u4, d1, d2, d3, d4):        # sw_core_nlm.F90:3088-3099
    t1, t2 = d1 + d2, d3 + d4
    return 0.5 * (((t1 + d2) * u2 - d2 * u1) / t1 + ((t2 + d3) * u3 - d3 * u4) / t2)


def d2a2c_vect(u, v, M, n):
    """sw_core_nlm.F90:2746-3085 for a whole face (is = js = 1, ie = je = n, not nested, grid_type < 3, dord4): returns
    ua, va, uc, vc, ut, vt with every element the routine does not write left NaN"""
    npx = npy = n + 1
    isd, ied, jsd, jed = 1 - NG, n + NG, 1 - NG, n + NG
    is_, ie, js, je = 1, n, 1, n
    npt = 4
    new = lambda: np.full(np.broadcast(u, v).shape, np.nan, dtype=np.result_type(u, v))
    utmp, vtmp, ua, va, uc, vc, ut, vt = (new() for _ in range(8))
    sg = lambda k: M["sin_sg%d" % k]
    # interior :2839-2848
    r = (max(npt, isd), min(npx - npt, ied), max(npt, js - 1), min(npy - npt, je + 1))
    V(utmp, *r)[...] = A2 * (V(u, *r, dj=-1) + V(u, *r, dj=2)) + A1 * (V(u, *r) + V(u, *r, dj=1))
    r = (max(npt, is_ - 1), min(npx - npt, ie + 1), max(npt, jsd), min(npy - npt, jed))
    V(vtmp, *r)[...] = A2 * (V(v, *r, di=-1) + V(v, *r, di=2)) + A1 * (V(v, *r) + V(v, *r, di=1))
    # edges :2855-2887
    for r in ((isd, ied, jsd, npt - 1), (isd, ied, npy - npt + 1, jed), (isd, npt - 1, max(npt, jsd), min(npy - npt, jed)),
              (npx - npt + 1, ied, max(npt, jsd), min(npy - npt, jed))):
        V(utmp, *r)[...] = 0.5 * (V(u, *r) + V(u, *r, dj=1)); V(vtmp, *r)[...] = 0.5 * (V(v, *r) + V(v, *r, di=1))
    # contravariant components at the cell centres :2892-2897
    r = (is_ - 2, ie + 2, js - 2, je + 2)
    V(ua, *r)[...] = (V(utmp, *r) - V(vtmp, *r) * V(M["cosa_s"], *r)) * V(M["rsin2"], *r)
    V(va, *r)[...] = (V(vtmp, *r) - V(utmp, *r) * V(M["cosa_s"], *r)) * V(M["rsin2"], *r)
    P = lambda a, i, j: a[..., j + NG - 1, i + NG - 1]
    def put(a, i, j, val):
        a[..., j + NG - 1, i + NG - 1] = val
    # X direction: corner rows of utmp :2906-2925
    for i in (-2, -1, 0):
        put(utmp, i, 0, -P(vtmp, 0, 1 - i)); put(utmp, i, npy, P(vtmp, 0, je + i))
    for i in (0, 1, 2):
        put(utmp, npx + i, 0, P(vtmp, npx, i + 1)); put(utmp, npx + i, npy, -P(vtmp, npx, je - i))
    r = (3, npx - 2, js - 1, je + 1)                                 # :2937-2942
    V(uc, *r)[...] = A2 * (V(utmp, *r, di=-2) + V(utmp, *r, di=1)) + A1 * (V(utmp, *r, di=-1) + V(utmp, *r))
    V(ut, *r)[...] = (V(uc, *r) - V(v, *r) * V(M["cosa_u"], *r)) * V(M["rsin_u"], *r)
    put(ua, -1, 0, -P(va, 0, 2)); put(ua, 0, 0, -P(va, 0, 1))                              # :2946-2961
    put(ua, npx, 0, P(va, npx, 1)); put(ua, npx + 1, 0, P(va, npx, 2))
    put(ua, npx, npy, -P(va, npx, npy - 1)); put(ua, npx + 1, npy, -P(va, npx, npy - 2))
    put(ua, -1, npy, P(va, 0, npy - 2)); put(ua, 0, npy, P(va, 0, npy - 1))
    col = lambda a, i: V(a, i, i, js - 1, je + 1)
    mcol = lambda k, i: V(M[k], i, i, js - 1, je + 1)
    def ucut(i):
        col(ut, i)[...] = (col(uc, i) - col(v, i) * mcol("cosa_u", i)) * mcol("rsin_u", i)
    # west edge :2963-2977
    col(uc, 0)[...] = C1 * col(utmp, -2) + C2 * col(utmp, -1) + C3 * col(utmp, 0)
    col(ut, 1)[...] = _edge_interpolate4(col(ua, -1), col(ua, 0), col(ua, 1), col(ua, 2), *[mcol("dxa", i) for i in (-1, 0, 1, 2)])
    col(uc, 1)[...] = col(ut, 1) * np.where(_pos(col(ut, 1)), mcol("sin_sg3", 0), mcol("sin_sg1", 1))
    col(uc, 2)[...] = C1 * col(utmp, 3) + C2 * col(utmp, 2) + C3 * col(utmp, 1)
    ucut(0); ucut(2)
    # east edge :2979-2992
    col(uc, npx - 1)[...] = C1 * col(utmp, npx - 3) + C2 * col(utmp, npx - 2) + C3 * col(utmp, npx - 1)
    col(ut, npx)[...] = _edge_interpolate4(*[col(ua, npx + d) for d in (-2, -1, 0, 1)], *[mcol("dxa", npx + d) for d in (-2, -1, 0, 1)])
    col(uc, npx)[...] = col(ut, npx) * np.where(_pos(col(ut, npx)), mcol("sin_sg3", npx - 1), mcol("sin_sg1", npx))
    col(uc, npx + 1)[...] = C3 * col(utmp, npx) + C2 * col(utmp, npx + 1) + C1 * col(utmp, npx + 2)
    ucut(npx - 1); ucut(npx + 1)
    # Y direction: corner columns of vtmp :2999-3018, corner values of va :3019-3034
    for j in (-2, -1, 0):
        put(vtmp, 0, j, -P(utmp, 1 - j, 0)); put(vtmp, npx, j, P(utmp, ie + j, 0))
    for j in (0, 1, 2):
        put(vtmp, 0, npy + j, P(utmp, j + 1, npy)); put(vtmp, npx, npy + j, -P(utmp, ie - j, npy))
    put(va, 0, -1, -P(ua, 2, 0)); put(va, 0, 0, -P(ua, 1, 0))
    put(va, npx, 0, P(ua, npx - 1, 0)); put(va, npx, -1, P(ua, npx - 2, 0))
    put(va, npx, npy, -P(ua, npx - 1, npy)); put(va, npx, npy + 1, -P(ua, npx - 2, npy))
    put(va, 0, npy, P(ua, 1, npy)); put(va, 0, npy + 1, P(ua, 2, npy))
    row = lambda a, j: V(a, is_ - 1, ie + 1, j, j)
    mrow = lambda k, j: V(M[k], is_ - 1, ie + 1, j, j)
    for j in range(js - 1, je + 3):                                   # :3038-3074
        if j in (1, npy):
            row(vt, j)[...] = _edge_interpolate4(*[row(va, j + d) for d in (-2, -1, 0, 1)], *[mrow("dya", j + d) for d in (-2, -1, 0, 1)])
            row(vc, j)[...] = row(vt, j) * np.where(_pos(row(vt, j)), mrow("sin_sg4", j - 1), mrow("sin_sg2", j))
            continue
        if j in (0, npy - 1):
            row(vc, j)[...] = C1 * row(vtmp, j - 2) + C2 * row(vtmp, j - 1) + C3 * row(vtmp, j)
        elif j in (2, npy + 1):
            row(vc, j)[...] = C1 * row(vtmp, j + 1) + C2 * row(vtmp, j) + C3 * row(vtmp, j - 1)
        else:
            row(vc, j)[...] = A2 * (row(vtmp, j - 2) + row(vtmp, j + 1)) + A1 * (row(vtmp, j - 1) + row(vtmp, j))
        row(vt, j)[...] = (row(vc, j) - row(u, j) * mrow("cosa_v", j)) * mrow("rsin_v", j)
    return ua, va, uc, vc, ut, vt


def c_sw_fluxes(ut, vt, M, n, dt2):
    """the scaling of ut, vt to area fluxes with the sign-selected sin_sg, sw_core_nlm.F90:157-174"""
    utf, vtf = np.full_like(ut, np.nan), np.full_like(vt, np.nan)
    r = (0, n + 2, 0, n + 1)
    V(utf, *r)[...] = dt2 * V(ut, *r) * V(M["dy"], *r) * np.where(_pos(V(ut, *r)), V(M["sin_sg3"], *r, di=-1), V(M["sin_sg1"], *r))
    r = (0, n + 1, 0, n + 2)
    V(vtf, *r)[...] = dt2 * V(vt, *r) * V(M["dx"], *r) * np.where(_pos(V(vt, *r)), V(M["sin_sg4"], *r, dj=-1), V(M["sin_sg2"], *r))
    return utf, vtf


def divergence_corner(u, v, ua, va, M, n):
    """sw_core_nlm.F90:1719-1762 (grid_type < 4, not nested, whole face)"""
    npx = npy = n + 1
    uf, vf, dv = np.full_like(ua, np.nan), np.full_like(ua, np.nan), np.full_like(ua, np.nan)
    sg = lambda k: M["sin_sg%d" % k]
    cg = lambda k: M["cos_sg%d" % k]
    r = (0, n + 1, 1, npy)
    s = 0.5 * (V(sg(4), *r, dj=-1) + V(sg(2), *r))
    V(uf, *r)[...] = (V(u, *r) - 0.25 * (V(va, *r, dj=-1) + V(va, *r)) * (V(cg(4), *r, dj=-1) + V(cg(2), *r))) * V(M["dyc"], *r) * s
    for j in (1, npy):
        r = (0, n + 1, j, j)
        V(uf, *r)[...] = V(u, *r) * V(M["dyc"], *r) * 0.5 * (V(sg(4), *r, dj=-1) + V(sg(2), *r))
    r = (2, npx - 1, 0, n + 1)
    V(vf, *r)[...] = (V(v, *r) - 0.25 * (V(ua, *r, di=-1) + V(ua, *r)) * (V(cg(3), *r, di=-1) + V(cg(1), *r))) * V(M["dxc"], *r) * \
        0.5 * (V(sg(3), *r, di=-1) + V(sg(1), *r))
    for i in (1, npx):
        r = (i, i, 0, n + 1)
        V(vf, *r)[...] = V(v, *r) * V(M["dxc"], *r) * 0.5 * (V(sg(3), *r, di=-1) + V(sg(1), *r))
    r = (1, npx, 1, npy)
    V(dv, *r)[...] = (V(vf, *r, dj=-1) - V(vf, *r)) + (V(uf, *r, di=-1) - V(uf, *r))
    P = lambda a, i, j: a[..., j + NG - 1, i + NG - 1]
    dv[..., 1 + NG - 1, 1 + NG - 1] = P(dv, 1, 1) - P(vf, 1, 0)
    dv[..., 1 + NG - 1, npx + NG - 1] = P(dv, npx, 1) - P(vf, npx, 0)
    dv[..., npy + NG - 1, npx + NG - 1] = P(dv, npx, npy) + P(vf, npx, npy)
    dv[..., npy + NG - 1, 1 + NG - 1] = P(dv, 1, npy) + P(vf, 1, npy)
    V(dv, *r)[...] = V(M["rarea_c"], *r) * V(dv, *r)
    return dv


def c_sw_winds(u, v, M, n, dt2):
    """the statements of c_sw (sw_core_nlm.F90:146-174) behind the product fields ua, va, utf, vtf, divgd"""
    ua, va, uc, vc, ut, vt = d2a2c_vect(u, v, M, n)
    dv = divergence_corner(u, v, ua, va, M, n)
    utf, vtf = c_sw_fluxes(ut, vt, M, n, dt2)
    return dict(ua=ua, va=va, utf=utf, vtf=vtf, divgd=dv, ut=ut, vt=vt)


def a2b_ord4(qin, M, edge, ecorner, n, replace=False):
    """a2b_edge_nlm.F90:49-329 (the default algorithm) on a whole face; edge [4, pj] (w, e, s, n), ecorner [4, 3] of that face.
    Returns qout (NaN outside 1..npx, 1..npy); replace=True: a copy of qin with that range overwritten (:319-327)."""
    npx = npy = n + 1
    c1, c2, r3 = 2.0 / 3.0, -1.0 / 6.0, 1.0 / 3.0
    new = lambda: np.full(qin.shape, np.nan, dtype=qin.dtype)
    qout, qx, qy, qxx, qyy = (new() for _ in range(5))
    P = lambda i, j: qin[..., j + NG - 1, i + NG - 1]
    dxa, dya = M["dxa"], M["dya"]
    ext = lambda c, k, p1, p2: P(*p1) + ecorner[c, k] * (P(*p1) - P(*p2))          # extrap_corner :800-810
    corners = [((1, 1), [((1, 1), (2, 2)), ((0, 1), (-1, 2)), ((1, 0), (2, -1))]),
               ((npx, 1), [((npx - 1, 1), (npx - 2, 2)), ((npx - 1, 0), (npx - 2, -1)), ((npx, 1), (npx + 1, 2))]),
               ((npx, npy), [((npx - 1, npy - 1), (npx - 2, npy - 2)), ((npx, npy - 1), (npx + 1, npy - 2)), ((npx - 1, npy), (npx - 2, npy + 1))]),
               ((1, npy), [((1, npy - 1), (2, npy - 2)), ((0, npy - 1), (-1, npy - 2)), ((1, npy), (2, npy + 1))])]
    for c, ((i, j), trip) in enumerate(corners):                       # :108-132
        qout[..., j + NG - 1, i + NG - 1] = (ext(c, 0, *trip[0]) + ext(c, 1, *trip[1]) + ext(c, 2, *trip[2])) * r3
    # X: interior :137-141, west :144-159, east :162-177
    r = (3, npx - 2, 1, npy - 1)
    V(qx, *r)[...] = B2 * (V(qin, *r, di=-2) + V(qin, *r, di=1)) + B1 * (V(qin, *r, di=-1) + V(qin, *r))
    col = lambda a, i, j0=1, j1=npy - 1, dj=0: V(a, i, i, j0, j1, dj=dj)
    ew = lambda e, j0, j1: edge[e][j0 + NG - 1:j1 + NG][:, None]
    for (e, io, ii, s) in ((0, 0, 1, 1), (1, npx, npx - 1, -1)):       # io: the halo column next to the edge, ii: the one inside, s: inward
        q2 = (col(qin, io) * col(dxa, ii) + col(qin, ii) * col(dxa, io)) / (col(dxa, io) + col(dxa, ii))
        ie_ = 1 if e == 0 else npx
        w = ew(e, 2, npy - 1)
        V(qout, ie_, ie_, 2, npy - 1)[...] = w * q2[..., :-1, :] + (1 - w) * q2[..., 1:, :]
        g_in, g_ou = col(dxa, ii + s) / col(dxa, ii), col(dxa, io - s) / col(dxa, io)
        col(qx, ie_)[...] = 0.5 * (((2 + g_in) * col(qin, ii) - col(qin, ii + s)) / (1 + g_in) + ((2 + g_ou) * col(qin, io) - col(qin, io - s)) / (1 + g_ou))
        i2 = ie_ + s
        if e == 0:
            col(qx, 2)[...] = (3 * (g_in * col(qin, 1) + col(qin, 2)) - (g_in * col(qx, 1) + col(qx, 3))) / (2 + 2 * g_in)
        else:
            col(qx, npx - 1)[...] = (3 * (col(qin, npx - 2) + g_in * col(qin, npx - 1)) - (g_in * col(qx, npx) + col(qx, npx - 2))) / (2 + 2 * g_in)
    # Y: interior :195-199, south :202-217, north :220-235
    r = (1, npx - 1, 3, npy - 2)
    V(qy, *r)[...] = B2 * (V(qin, *r, dj=-2) + V(qin, *r, dj=1)) + B1 * (V(qin, *r, dj=-1) + V(qin, *r))
    row = lambda a, j, i0=1, i1=npx - 1: V(a, i0, i1, j, j)
    ewr = lambda e, i0, i1: edge[e][i0 + NG - 1:i1 + NG][None, :]
    for (e, jo, ji, s) in ((2, 0, 1, 1), (3, npy, npy - 1, -1)):
        q1 = (row(qin, jo) * row(dya, ji) + row(qin, ji) * row(dya, jo)) / (row(dya, jo) + row(dya, ji))
        je_ = 1 if e == 2 else npy
        w = ewr(e, 2, npx - 1)
        V(qout, 2, npx - 1, je_, je_)[...] = w * q1[..., :, :-1] + (1 - w) * q1[..., :, 1:]
        g_in, g_ou = row(dya, ji + s) / row(dya, ji), row(dya, jo - s) / row(dya, jo)
        row(qy, je_)[...] = 0.5 * (((2 + g_in) * row(qin, ji) - row(qin, ji + s)) / (1 + g_in) + ((2 + g_ou) * row(qin, jo) - row(qin, jo - s)) / (1 + g_ou))
        if e == 2:
            row(qy, 2)[...] = (3 * (g_in * row(qin, 1) + row(qin, 2)) - (g_in * row(qy, 1) + row(qy, 3))) / (2 + 2 * g_in)
        else:
            row(qy, npy - 1)[...] = (3 * (row(qin, npy - 2) + g_in * row(qin, npy - 1)) - (g_in * row(qy, npy) + row(qy, npy - 2))) / (2 + 2 * g_in)
    # :262-290
    r = (2, npx - 1, 3, npy - 2)
    V(qxx, *r)[...] = A2 * (V(qx, *r, dj=-2) + V(qx, *r, dj=1)) + A1 * (V(qx, *r, dj=-1) + V(qx, *r))
    rw = lambda a, j: V(a, 2, npx - 1, j, j)
    rw(qxx, 2)[...] = c1 * (rw(qx, 1) + rw(qx, 2)) + c2 * (rw(qout, 1) + rw(qxx, 3))
    rw(qxx, npy - 1)[...] = c1 * (rw(qx, npy - 2) + rw(qx, npy - 1)) + c2 * (rw(qout, npy) + rw(qxx, npy - 2))
    r = (3, npx - 2, 2, npy - 1)
    V(qyy, *r)[...] = A2 * (V(qy, *r, di=-2) + V(qy, *r, di=1)) + A1 * (V(qy, *r, di=-1) + V(qy, *r))
    cl = lambda a, i: V(a, i, i, 2, npy - 1)
    cl(qyy, 2)[...] = c1 * (cl(qy, 1) + cl(qy, 2)) + c2 * (cl(qout, 1) + cl(qyy, 3))
    cl(qyy, npx - 1)[...] = c1 * (cl(qy, npx - 2) + cl(qy, npx - 1)) + c2 * (cl(qout, npx) + cl(qyy, npx - 2))
    r = (2, npx - 1, 2, npy - 1)
    V(qout, *r)[...] = 0.5 * (V(qxx, *r) + V(qyy, *r))
    if not replace:
        return qout
    out = qin.copy()
    r = (1, npx, 1, npy)
    V(out, *r)[...] = V(qout, *r)
    return out


def one_grad_p(u, v, pk, gz, M, edge, ecorner, n, dt, ptk):
    """dyn_core_nlm.F90:1645-1778, hydrostatic, a2b_ord = 4, d_ext = 0: u, v [..., npz, pj, pj], pk, gz [..., npz+1, pj, pj]"""
    npx = npy = n + 1
    pk = pk.copy()
    V(pk[..., 0, :, :], 1, npx, 1, npy)[...] = ptk                     # :1687-1691
    pkb = np.concatenate([pk[..., :1, :, :], a2b_ord4(pk[..., 1:, :, :], M, edge, ecorner, n, True)], axis=-3)     # :1695-1701
    gzb = a2b_ord4(gz, M, edge, ecorner, n, True)                      # :1705-1711
    wk = pkb[..., 1:, :, :] - pkb[..., :-1, :, :]                      # :1749-1753
    p0, p1, g0, g1 = pkb[..., :-1, :, :], pkb[..., 1:, :, :], gzb[..., :-1, :, :], gzb[..., 1:, :, :]
    uo, vo = np.full_like(wk, np.nan), np.full_like(wk, np.nan)
    r = (1, n, 1, npy)                                                 # :1762-1768
    V(uo, *r)[...] = V(M["rdx"], *r) * (V(u, *r) + dt / (V(wk, *r) + V(wk, *r, di=1)) *
                                        ((V(g1, *r) - V(g0, *r, di=1)) * (V(p1, *r, di=1) - V(p0, *r)) + (V(g0, *r) - V(g1, *r, di=1)) * (V(p1, *r) - V(p0, *r, di=1))))
    r = (1, npx, 1, n)                                                 # :1769-1775
    V(vo, *r)[...] = V(M["rdy"], *r) * (V(v, *r) + dt / (V(wk, *r) + V(wk, *r, dj=1)) *
                                        ((V(g1, *r) - V(g0, *r, dj=1)) * (V(p1, *r, dj=1) - V(p0, *r)) + (V(g0, *r) - V(g1, *r, dj=1)) * (V(p1, *r) - V(p0, *r, dj=1))))
    return dict(u_o=uo, v_o=vo)


def p_grad_c(pkc, gz, uc, vc, M, n, dt2):
    """dyn_core_nlm.F90:1369-1428, hydrostatic: the C-grid pressure gradient with rdxc, rdyc and their face-edge forms"""
    npx = npy = n + 1
    wk = pkc[..., 1:, :, :] - pkc[..., :-1, :, :]
    p0, p1, g0, g1 = pkc[..., :-1, :, :], pkc[..., 1:, :, :], gz[..., :-1, :, :], gz[..., 1:, :, :]
    uo, vo = np.full_like(wk, np.nan), np.full_like(wk, np.nan)
    r = (1, npx, 1, n)
    V(uo, *r)[...] = V(uc, *r) + dt2 * V(M["rdxc"], *r) / (V(wk, *r, di=-1) + V(wk, *r)) * \
        ((V(g1, *r, di=-1) - V(g0, *r)) * (V(p1, *r) - V(p0, *r, di=-1)) + (V(g0, *r, di=-1) - V(g1, *r)) * (V(p1, *r, di=-1) - V(p0, *r)))
    r = (1, n, 1, npy)
    V(vo, *r)[...] = V(vc, *r) + dt2 * V(M["rdyc"], *r) / (V(wk, *r, dj=-1) + V(wk, *r)) * \
        ((V(g1, *r, dj=-1) - V(g0, *r)) * (V(p1, *r) - V(p0, *r, dj=-1)) + (V(g0, *r, dj=-1) - V(g1, *r)) * (V(p1, *r, dj=-1) - V(p0, *r)))
    return dict(uc=uo, vc=vo)


def d_sw_courant(uc, vc, M, n, dt):
    """The first loops of d_sw (sw_core_nlm.F90:660-892, grid_type < 3, not nested, whole face): the contravariant winds ut, vt with
    their face-edge and corner forms, then xfx, yfx, crx, cry on jsd..jed / isd..ied with the sign-selected sin_sg -- the rows that read
    sin_sg(0, j <= 0, 3) and their kin.  Elements the routine does not write stay NaN."""
    npx = npy = n + 1
    isd, ied, jsd, jed = 1 - NG, n + NG, 1 - NG, n + NG
    ut, vt = np.full_like(uc, np.nan), np.full_like(uc, np.nan)
    cu, cv, ru, rv = M["cosa_u"], M["cosa_v"], M["rsin_u"], M["rsin_v"]
    sg = lambda k: M["sin_sg%d" % k]
    for j in range(jsd, jed + 1):                                      # :660-667
        if j not in (0, 1, npy - 1, npy):
            r = (0, n + 2, j, j)
            V(ut, *r)[...] = (V(uc, *r) - 0.25 * V(cu, *r) * (V(vc, *r, di=-1) + V(vc, *r) + V(vc, *r, di=-1, dj=1) + V(vc, *r, dj=1))) * V(ru, *r)
    for j in range(0, n + 3):                                          # :668-677
        if j not in (1, npy):
            r = (isd, ied, j, j)
            V(vt, *r)[...] = (V(vc, *r) - 0.25 * V(cv, *r) * (V(uc, *r, dj=-1) + V(uc, *r, di=1, dj=-1) + V(uc, *r) + V(uc, *r, di=1))) * V(rv, *r)
    for (i, ia, ib) in ((1, 0, 1), (npx, npx - 1, npx)):                # west :682-696, east :699-714
        r = (i, i, jsd, jed)
        V(ut, *r)[...] = V(uc, *r) / np.where(_pos(V(uc, *r) * dt), V(sg(3), *r, di=-1), V(sg(1), *r))
        for iv in (ia, ib):
            r = (iv, iv, 3, npy - 2)
            V(vt, *r)[...] = V(vc, *r) - 0.25 * V(cv, *r) * (V(ut, *r, dj=-1) + V(ut, *r, di=1, dj=-1) + V(ut, *r) + V(ut, *r, di=1))
    for (j, ja, jb) in ((1, 0, 1), (npy, npy - 1, npy)):                # south :717-733, north :736-750
        r = (isd, ied, j, j)
        V(vt, *r)[...] = V(vc, *r) / np.where(_pos(V(vc, *r) * dt), V(sg(4), *r, dj=-1), V(sg(2), *r))
        for ju in (ja, jb):
            r = (3, npx - 2, ju, ju)
            V(ut, *r)[...] = V(uc, *r) - 0.25 * V(cu, *r) * (V(vt, *r, di=-1) + V(vt, *r) + V(vt, *r, di=-1, dj=1) + V(vt, *r, dj=1))
    P = lambda a, i, j: a[..., j + NG - 1, i + NG - 1]
    CU, CV = (lambda i, j: cu[j + NG - 1, i + NG - 1]), (lambda i, j: cv[j + NG - 1, i + NG - 1])
    UT, VT, UC, VC = (lambda i, j: P(ut, i, j)), (lambda i, j: P(vt, i, j)), (lambda i, j: P(uc, i, j)), (lambda i, j: P(vc, i, j))

    def set_ut(i, j, val):
        ut[..., j + NG - 1, i + NG - 1] = val

    def set_vt(i, j, val):
        vt[..., j + NG - 1, i + NG - 1] = val

    def solve_u(iu, ju, iv, jv, vts, uts):
        """ut(iu,ju) = (uc - 0.25 cosa_u (sum of three vt + vc(iv,jv) - 0.25 cosa_v(iv,jv) (sum of three ut))) * damp"""
        damp = 1.0 / (1.0 - 0.0625 * CU(iu, ju) * CV(iv, jv))
        set_ut(iu, ju, (UC(iu, ju) - 0.25 * CU(iu, ju) * (sum(VT(*p) for p in vts) + VC(iv, jv) - 0.25 * CV(iv, jv) * sum(UT(*p) for p in uts))) * damp)

    def solve_v(iv, jv, iu, ju, uts, vts):
        damp = 1.0 / (1.0 - 0.0625 * CU(iu, ju) * CV(iv, jv))
        set_vt(iv, jv, (VC(iv, jv) - 0.25 * CV(iv, jv) * (sum(UT(*p) for p in uts) + UC(iu, ju) - 0.25 * CU(iu, ju) * sum(VT(*p) for p in vts))) * damp)
    x, y = npx, npy
    # sw :762-776
    solve_u(2, 0, 1, 0, [(1, 1), (2, 1), (2, 0)], [(1, 0), (1, -1), (2, -1)])
    solve_v(0, 2, 0, 1, [(1, 1), (1, 2), (0, 2)], [(0, 1), (-1, 1), (-1, 2)])
    u21 = [(1, 1), (2, 1), (2, 2)], [(1, 1), (1, 2), (2, 2)]
    solve_u(2, 1, 1, 2, u21[0], u21[1])
    solve_v(1, 2, 2, 1, u21[1], u21[0])
    # se :778-795
    solve_u(x - 1, 0, x - 1, 0, [(x - 1, 1), (x - 2, 1), (x - 2, 0)], [(x, 0), (x, -1), (x - 1, -1)])
    solve_v(x, 2, x + 1, 1, [(x, 1), (x, 2), (x + 1, 2)], [(x, 1), (x + 1, 1), (x + 1, 2)])
    a_, b_ = [(x - 1, 1), (x - 2, 1), (x - 2, 2)], [(x, 1), (x, 2), (x - 1, 2)]
    solve_u(x - 1, 1, x - 1, 2, a_, b_)
    solve_v(x - 1, 2, x - 1, 1, b_, a_)
    # ne :797-814
    solve_u(x - 1, y, x - 1, y + 1, [(x - 1, y), (x - 2, y), (x - 2, y + 1)], [(x, y), (x, y + 1), (x - 1, y + 1)])
    solve_v(x, y - 1, x + 1, y - 1, [(x, y - 1), (x, y - 2), (x + 1, y - 2)], [(x, y), (x + 1, y), (x + 1, y - 1)])
    a_, b_ = [(x - 1, y), (x - 2, y), (x - 2, y - 1)], [(x, y - 1), (x, y - 2), (x - 1, y - 2)]
    solve_u(x - 1, y - 1, x - 1, y - 1, a_, b_)
    solve_v(x - 1, y - 1, x - 1, y - 1, b_, a_)
    # nw :816-834
    solve_u(2, y, 1, y + 1, [(1, y), (2, y), (2, y + 1)], [(1, y), (1, y + 1), (2, y + 1)])
    solve_v(0, y - 1, 0, y - 1, [(1, y - 1), (1, y - 2), (0, y - 2)], [(0, y), (-1, y), (-1, y - 1)])
    a_, b_ = [(1, y), (2, y), (2, y - 1)], [(1, y - 1), (1, y - 2), (2, y - 2)]
    solve_u(2, y - 1, 1, y - 1, a_, b_)
    solve_v(1, y - 1, 2, y - 1, b_, a_)
    # :853-892
    xfx, crx, yfx, cry = (np.full_like(uc, np.nan) for _ in range(4))
    r = (1, npx, jsd, jed)
    xa = dt * V(ut, *r)
    V(crx, *r)[...] = xa * np.where(_pos(xa), V(M["rdxa"], *r, di=-1), V(M["rdxa"], *r))
    V(xfx, *r)[...] = V(M["dy"], *r) * xa * np.where(_pos(xa), V(sg(3), *r, di=-1), V(sg(1), *r))
    r = (isd, ied, 1, npy)
    ya = dt * V(vt, *r)
    V(cry, *r)[...] = ya * np.where(_pos(ya), V(M["rdya"], *r, dj=-1), V(M["rdya"], *r))
    V(yfx, *r)[...] = V(M["dx"], *r) * ya * np.where(_pos(ya), V(sg(4), *r, dj=-1), V(sg(2), *r))
    return dict(crx=crx, cry=cry, xfx=xfx, yfx=yfx, ut=ut, vt=vt)
