"""CPU (-m "not gpu"): face_edge_checks.py through the host-emulation build of the stage code -- c_sw (ua, va, utf, vtf, divgd), the first
loops of d_sw (crx, cry, xfx, yfx), one_grad_p
(u_o, v_o through a2b_ord4 with replace) and p_grad_c (uc, vc) on whole faces n = 8 and 12, all six faces, values, tangent and adjoint,
point by point and region by region against the restatement, with the restatement's metrics (poisoned) in the library.  n = 6, which
the issue behind these tests also names, is refused by fv3lm_create (nx, ny >= 8): test_c6_is_refused keeps that on record.
The rest of both shallow-water routines -- c_sw after the area fluxes, d_sw after its first loops, u_m / v_m by composition -- the same
way (test_c_sw_after_the_area_fluxes, test_d_sw_after_the_first_loops, ..._cap, test_rest_operators_c70), the 2 x 2 layout for every
operator, and one case per operator on metrics whose sin_sg / cos_sg planes are scaled apart (the cube holds equal sines across an edge)."""
import pytest
import face_edge_checks as F


@pytest.mark.parametrize("face", range(6))
@pytest.mark.parametrize("n", [8, 12])
@pytest.mark.parametrize("group", ["c_sw", "one_grad_p", "p_grad_c"])
def test_face_edge_operator(group, n, face):
    F.check("emul", group, n, face)


@pytest.mark.parametrize("group,levels", [("c_sw", 1), ("one_grad_p", 0), ("d_sw", 1)])
def test_face_edge_operator_c70(group, levels):
    """edge strips longer than one 64-column block: values and tangent at every point and level; the adjoint entry by entry within four
    cells of the edges on `levels` levels (lattice columns), everything else through four dot products"""
    F.check("emul", group, 70, 2, npz=2, adjoint_all=False, coloured=True, adjoint_levels=levels)


@pytest.mark.parametrize("group", ["c_sw", "one_grad_p"])
def test_face_edge_operator_c16_cut_2x2(group):
    """six faces of C16 in 24 tiles: the tile offset into edge[] and the clipped strip rects under the reference"""
    F.check_layout("emul", group)


@pytest.mark.parametrize("group", ["d_sw", "p_grad_c", "c_sw_rest", "d_sw_rest"])
def test_face_edge_operator_c16_cut_2x2_more(group):
    """the 2 x 2 layout for the first loops of d_sw, p_grad_c and the two operators that follow the area fluxes / the first loops
    (d_sw_rest on its three levels; u_m, v_m by composition are left to the whole-face tests)"""
    kw = dict(npz=F.DSW_REST["npz"], opt=F.DSW_REST["opt"]) if group == "d_sw_rest" else {}
    F.check_layout("emul", group, **kw)


@pytest.mark.parametrize("group,face", [("c_sw_rest", 0), ("d_sw_rest", 5), ("c_sw", 3), ("d_sw", 4)])
def test_sin_sg_selection_on_detuned_metrics(group, face):
    """C8 with every sin_sg / cos_sg plane scaled by a factor of its own, in library and restatement alike: across a face edge the true
    cube holds sin_sg(i, j-1, 4) = sin_sg(i, j, 2), so only this shows which of the two a branch takes"""
    if group == "d_sw_rest":
        F.check_d_sw_rest("emul", 8, face, coloured=True, adjoint_on=[1], detune=True)
    else:
        F.check("emul", group, 8, face, detune=True)


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("face", range(6))
@pytest.mark.parametrize("n", [8, 12])
def test_d_sw_first_loops(n, face, fused):
    """crx, cry, xfx, yfx from uc, vc (the rows that read sin_sg(0, j <= 0, 3) and their kin), under both forms of fv_tp_2d: the staged
    stages (fused = "0": FV3LM_TP_FUSED=0) and the tiled launches of the default environment (fused = "1")"""
    F.check("emul", "d_sw", n, face, env={"FV3LM_TP_FUSED": "0"} if fused == "0" else None)


@pytest.mark.parametrize("face", range(6))
@pytest.mark.parametrize("n", [8, 12])
def test_c_sw_after_the_area_fluxes(n, face):
    """delpc, ptc, ke_c, vort_c, uc1, vc1, uc0, vc0 from delp, pt, u, v (sw_core_nlm.F90:177-486): the upwind transport through
    fill2_4corners, the sin_sg / cos_sg forms of the kinetic energy, the three-sided corner vorticity, the wind update"""
    F.check("emul", "c_sw_rest", n, face)


@pytest.mark.parametrize("face", range(6))
@pytest.mark.parametrize("n", [8, 12])
def test_d_sw_after_the_first_loops(n, face):
    """ra_x, ra_y, vb, ub, ke, wk, vort_abs, vort_b, dd_c, ke2, del6_d2 and, by composition, u_m, v_m on three levels that run
    (nord, iord, nord_v) = (0, 1, 0), (0, 2, 0), (1, 2, 1); the adjoint entry by entry on every level at one in three of the lattice
    offsets, the other points through four dot products"""
    F.check_d_sw_rest("emul", n, face, coloured=True, adjoint_on=[0, 1, 2], adjoint_thin=3)


@pytest.mark.parametrize("n,face", [(8, 1), (12, 4)])
def test_d_sw_divergence_damping_cap(n, face):
    """one more draw with the winds amplified until min(0.20, dddmp x) takes the cap at >= 10 % of the bulk and in every strip and corner
    block (a single evaluation of the operator: stability is no concern)"""
    F.check_d_sw_rest("emul", n, face, coloured=True, adjoint_on=[2], amplify=2.0)


@pytest.mark.parametrize("group", ["c_sw_rest", "d_sw_rest"])
def test_rest_operators_c70(group):
    """strips longer than one 64-column block, npz = 2: values and tangent everywhere; the adjoint entry by entry within four cells of
    the edges on the first level at one in four (c_sw) / eight (d_sw) of the lattice offsets, everything else through four dot products"""
    if group == "c_sw_rest":
        F.check("emul", group, 70, 2, npz=2, adjoint_all=False, coloured=True, adjoint_levels=1, adjoint_thin=4)
    else:
        F.check_d_sw_rest("emul", 70, 2, case=F.DSW_REST_C70, adjoint_all=False, coloured=True, adjoint_levels=1, adjoint_thin=8)


def test_coloured_adjoint_is_the_exact_one_rest():
    """test_coloured_adjoint_is_the_exact_one for the two operators that follow the area fluxes / the first loops (C16, two levels that run
    nord = 0 and nord = 1)"""
    import numpy as np
    from common import Case
    n, face = 16, 3
    for g, kw in (("c_sw_rest", {}), ("d_sw_rest", F.DSW_REST_C70["opt"])):
        c = Case(nx=n, ny=n, npz=2, backend="none", face=face, oracle=False, **kw)
        op = F.OPERATORS[g](c)
        M, e, ec = F.face_metrics_of(n, face, np.float64)
        rng = np.random.default_rng(1)
        T = F._ghost_fill(c, op.draw(c, rng)[0], np.nan)
        seeds = {}
        for o, rk in op.outs:
            lv = op.levels_of(o) if hasattr(op, "levels_of") and op.levels_of(o) is not None else [0, 1]
            on = np.zeros((c.npz, 1, 1), bool); on[lv] = True
            seeds[o] = np.where(F.compared_mask(c, o, rk) & on, rng.standard_normal((c.npz, n + 7, n + 7)), 0.0)
        pts = {k: np.ones(T[k].shape, bool) for k in op.ins}
        for k in op.ins:
            if k in F.GHOST_FREE:
                pts[k][:, F.fo._ghost(n)] = False
        a = F._adjoint(op, T, seeds, M, e, ec, np.float64, pts)
        b = F._adjoint(op, T, seeds, M, e, ec, np.float64, pts, coloured=True)
        for k in a:
            assert np.max(np.abs(a[k] - b[k])) <= 1e-13 * np.max(np.abs(a[k])), (g, k)


def test_coloured_adjoint_is_the_exact_one():
    """the lattice form of the adjoint reference against one perturbed point per column, C16 (two lattice points per direction)"""
    import numpy as np
    from common import Case
    n, face = 16, 3
    c = Case(nx=n, ny=n, npz=2, backend="none", face=face, oracle=False)
    for g in ("c_sw", "one_grad_p", "d_sw"):
        op = F.OPERATORS[g](c)
        M, e, ec = F.face_metrics_of(n, face, np.float64)
        rng = np.random.default_rng(1)
        T = F._ghost_fill(c, op.draw(c, rng)[0], np.nan)
        seeds = {o: np.where(F.compared_mask(c, o, rk), rng.standard_normal((c.npz, n + 7, n + 7)), 0.0) for o, rk in op.outs}
        pts = {k: np.ones(T[k].shape, bool) for k in op.ins}
        for k in op.ins:
            if k in F.GHOST_FREE:
                pts[k][:, F.fo._ghost(n)] = False
        a = F._adjoint(op, T, seeds, M, e, ec, np.float64, pts)
        b = F._adjoint(op, T, seeds, M, e, ec, np.float64, pts, coloured=True)
        for k in a:
            assert np.max(np.abs(a[k] - b[k])) <= 1e-13 * np.max(np.abs(a[k])), (g, k)


def test_c6_is_refused():
    from common import Case
    from fv3_jedi_linearmodel_amd._lib import Fv3LmError
    with pytest.raises(Fv3LmError, match="tile too small"):
        Case(nx=6, ny=6, npz=3, backend="emul", face=0, oracle=False)


@pytest.mark.parametrize("face", range(6))
@pytest.mark.parametrize("n", [8, 12])
def test_c_sw_non_hydrostatic_w(n, face):
    """c_sw_rest on a non-hydrostatic case: w through fill_4corners and the upwind fluxes into wc (sw_core_nlm.F90:210-284), beside the
    other outputs"""
    F.check("emul", "c_sw_rest_nh", n, face, opt=dict(hydrostatic=0), coloured=True, adjoint_on=[0, 1, 2], adjoint_thin=2)


@pytest.mark.parametrize("face", range(6))
@pytest.mark.parametrize("n", [8, 12])
@pytest.mark.parametrize("nord", [2, 3])
def test_d_sw_split_damp_trajectory_nord(nord, n, face):
    """split_damp with the trajectory's nord = 2, 3 over the perturbation's nord = 1 on level 2: the VALUES of ke2 (and of u_m, v_m) from
    the trajectory's damping -- the higher-order loop with fill_corners in its B-grid scalar and D-grid vector forms, nord_v = 2 --
    the tangent and the adjoint with the perturbation's coefficients"""
    F.check_d_sw_rest("emul", n, face, case=F.DSW_SPLIT[nord], coloured=True, adjoint_on=[0, 1], adjoint_thin=3)
