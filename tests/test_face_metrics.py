"""CPU (-m "not gpu"): every metric plane cube.cubed_sphere_metrics(edge_forms="reference") hands to the library in the tests, the a2b_ord4 edge weights and corner
coefficients and the c2l matrices, against tests/face_oracle.py -- the restatement of grid_init / grid_utils_init written from the
reference's Fortran, which shares the corner points with the package and nothing else.  All six faces, n = 6, 8, 12, 48, entry by entry
wherever the restatement says the reference holds a value; the error of an entry is relative to the largest value of that plane on that
face.

Bound, per plane and size: 8 x the movement of the restatement itself -- float64 on corner points moved by <= 1 ulp (three draws)
against longdouble on the unmoved ones -- at least 8 eps (a float64 plane cannot be pinned tighter than its own rounding) and at most
the 1e-9 of test_cube.py::test_metrics_match_lonlat_formulas.  Measured movements and errors: DESIGN.md section 5."""
import numpy as np
import pytest
from fv3_jedi_linearmodel_amd import cube
import face_oracle as fo

EPS = np.finfo(np.float64).eps
SIZES = [6, 8, 12, 48]


def _planes(m, edge, ecorner, c2l):
    """everything as {name: [6, ...]}"""
    out = dict(m)
    for e, nm in enumerate("wesn"):
        out["edge_" + nm] = edge[:, e]
    for c, nm in enumerate(("sw", "se", "ne", "nw")):
        out["ecorner_" + nm] = ecorner[:, c]
    for q, nm in enumerate(("a11", "a12", "a21", "a22")):
        out["c2l_" + nm] = c2l[:, q]
    return out


def _rel(a, ref, ok):
    """per face: largest |a - ref| over the entries ok, relative to the largest |ref| there"""
    worst = 0.0
    for f in range(6):
        if not ok[f].any():
            continue
        r = np.asarray(ref[f][ok[f]], dtype=np.longdouble)
        worst = max(worst, float(np.max(np.abs(np.asarray(a[f][ok[f]], dtype=np.longdouble) - r)) / np.max(np.abs(r))))
    return worst


def measure(n):
    """{plane: (movement of the restatement, error of the package, number of entries compared)}"""
    pm, _, _, pedge, pecorner, geo = cube.cubed_sphere_metrics(n, edge_forms="reference")
    P = geo["corners"]
    m, poison, edge, ecorner, c2l = fo.face_metrics(P, dtype=np.longdouble)
    ok = fo.defined(m, poison)
    ref = _planes(m, edge, ecorner, c2l)
    okp = {k: ok[k] if k in ok else np.isfinite(v) for k, v in ref.items()}
    npx = n + 1
    for r in (fo.R(1, npx, 1, 1), fo.R(1, npx, npx, npx), fo.R(1, 1, 1, npx), fo.R(npx, npx, 1, npx)):
        okp["rsina"][r] = False          # big_number by design (checked apart: any huge number serves)
    rng = np.random.default_rng(n)
    move = {k: 0.0 for k in ref}
    for _ in range(3):
        Pd = P + rng.integers(-1, 2, size=P.shape) * np.spacing(P)
        md, pod, ed, ecd, cd = fo.face_metrics(Pd, dtype=np.float64)
        assert all(np.array_equal(pod[k], poison[k]) for k in poison)
        got = _planes(md, ed, ecd, cd)
        for k in ref:
            move[k] = max(move[k], _rel(got[k], ref[k], okp[k]))
    mine = _planes(pm, pedge, pecorner, geo["c2l"])
    return {k: (move[k], _rel(mine[k], ref[k], okp[k]), int(okp[k].sum())) for k in ref}, (pm, okp)


@pytest.mark.parametrize("n", SIZES)
def test_every_plane_matches_the_restatement(n):
    res, (pm, okp) = measure(n)
    assert set(fo.METRIC_PLANES) <= set(res) and set(fo.METRIC_PLANES) == set(pm)
    bad = []
    for k, (mv, err, cnt) in sorted(res.items()):
        bound = min(1e-9, max(8 * mv, 8 * EPS))
        print("C%-3d %-10s entries %6d  movement %.2e  bound %.2e  error %.2e" % (n, k, cnt, mv, bound, err))
        assert cnt > 0, k
        if not err <= bound:
            bad.append((k, err, bound))
    assert not bad, bad
    # rsina on the face edges: the reference's big_number (model/fv_grid_utils_nlm.F90:531-533) or anything as large
    npx = n + 1
    for r in (fo.R(1, npx, 1, 1), fo.R(1, npx, npx, npx), fo.R(1, 1, 1, npx), fo.R(npx, npx, 1, npx)):
        assert np.all(pm["rsina"][r] >= fo.BIG)


def test_defined_set_covers_the_compute_domain():
    """Sanity of the mask: on the cells, edges and corners of the face itself every plane is defined, except cosa / sina at the four
    vertices (the coincident-corner cell) and rsina along the edges."""
    n = 8
    P = cube.cube_corner_points(n)
    m, poison, _, _, _ = fo.face_metrics(P)
    ok = fo.defined(m, poison)
    cells, npx = fo.R(1, n, 1, n), n + 1
    for k in fo.METRIC_PLANES:
        assert ok[k][cells].all() or k in ("rsina", "cosa", "sina"), k
    assert ok["rsina"][fo.R(2, n, 2, n)].all()
    for k in ("cosa", "sina"):
        assert ok[k][fo.R(1, npx, 1, npx)].sum() == 6 * (npx * npx - 4)


def test_reference_se_corner_area_is_negative():
    """The finding recorded in DESIGN.md section 5: area_c(npx, 1) as the reference writes it (tools/fv_grid_tools_nlm.F90:836-843)."""
    n = 8
    P = cube.cube_corner_points(n)
    lit = fo.face_metrics(P, literal_se_corner=True)[0]["rarea_c"]
    sym = fo.face_metrics(P)[0]["rarea_c"]
    assert np.all(lit[fo.at(n + 1, 1)] < 0) and np.all(sym[fo.at(n + 1, 1)] > 0)
    assert np.allclose(sym[fo.at(n + 1, 1)], sym[fo.at(1, 1)], rtol=1e-12)


def test_extended_form_departs_only_where_recorded():
    """The default form of cube.cubed_sphere_metrics ("extended": what the benchmark runs on, kept bit for bit so that its results
    stay comparable with earlier ones) against the pinned "reference" form: identical away from the face edges (points 2 .. n-1 of
    every plane) and in every plane outside the recorded list, identical extrap_corner coefficients; the planes of the list, the a2b
    edge weights and da_min_c differ along the edges and in the halo as DESIGN.md section 5 describes."""
    recorded = set("area rarea rarea_c dx dy dxa dya dxc dyc rdx rdy rdxa rdya rdxc rdyc del6_u del6_v divg_u divg_v sina_u sina_v rsin_u rsin_v "
                   "sin_sg1 sin_sg2 sin_sg3 sin_sg4 cos_sg1 cos_sg2 cos_sg3 cos_sg4".split())
    for n in (8, 12):
        a, b = cube.cubed_sphere_metrics(n), cube.cubed_sphere_metrics(n, edge_forms="reference")
        inner = (slice(None), slice(4, n + 2), slice(4, n + 2))
        for k in a[0]:
            assert np.array_equal(a[0][k][inner], b[0][k][inner]), k
            assert k in recorded or np.array_equal(a[0][k], b[0][k]), k
        assert np.array_equal(a[4], b[4]) and a[1] == b[1]
        assert np.max(np.abs(a[3] - b[3])) > 0.1          # the edge weights: 0.47 .. 0.53 against 0.27 .. 0.73 at C8
