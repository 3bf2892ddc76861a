"""-m gpu: face_edge_checks.py through the C-ABI of the HIP library: c_sw, one_grad_p and p_grad_c on whole faces n = 8 and 12, all six
faces, and C70 on one face (strips beyond one 64-column block), values, tangent and adjoint per point and region against the
restatement of the reference's nonlinear Fortran; the rest of c_sw and d_sw (c_sw_rest, d_sw_rest with u_m, v_m by composition), the 2 x 2
layout and the detuned sin_sg / cos_sg planes as in tests/test_emul_face_edges.py."""
import pytest
import face_edge_checks as F

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("face", range(6))
@pytest.mark.parametrize("n", [8, 12])
@pytest.mark.parametrize("group", ["c_sw", "one_grad_p", "p_grad_c"])
def test_face_edge_operator(group, n, face):
    F.check("hip", group, n, face)


@pytest.mark.parametrize("group,levels", [("c_sw", 1), ("one_grad_p", 0), ("d_sw", 1)])
def test_face_edge_operator_c70(group, levels):
    F.check("hip", group, 70, 2, npz=2, adjoint_all=False, coloured=True, adjoint_levels=levels)


@pytest.mark.parametrize("group", ["c_sw", "one_grad_p"])
def test_face_edge_operator_c16_cut_2x2(group):
    """six faces of C16 in 24 tiles: the tile offset into edge[] and the clipped strip rects under the reference"""
    F.check_layout("hip", group)


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("face", range(6))
@pytest.mark.parametrize("n", [8, 12])
def test_d_sw_first_loops(n, face, fused):
    """crx, cry, xfx, yfx from uc, vc (the rows that read sin_sg(0, j <= 0, 3) and their kin), under both forms of fv_tp_2d: the staged
    stages (fused = "0": FV3LM_TP_FUSED=0) and the tiled launches of the default environment (fused = "1")"""
    F.check("hip", "d_sw", n, face, env={"FV3LM_TP_FUSED": "0"} if fused == "0" else None)


@pytest.mark.parametrize("face", range(6))
@pytest.mark.parametrize("n", [8, 12])
def test_c_sw_after_the_area_fluxes(n, face):
    """delpc, ptc, ke_c, vort_c, uc1, vc1, uc0, vc0 from delp, pt, u, v (sw_core_nlm.F90:177-486)"""
    F.check("hip", "c_sw_rest", n, face)


@pytest.mark.parametrize("face", range(6))
@pytest.mark.parametrize("n", [8, 12])
def test_d_sw_after_the_first_loops(n, face):
    """ra_x, ra_y, vb, ub, ke, wk, vort_abs, vort_b, dd_c, ke2, del6_d2 and, by composition, u_m, v_m on three levels that run
    (nord, iord, nord_v) = (0, 1, 0), (0, 2, 0), (1, 2, 1); the adjoint entry by entry at one in three of the lattice offsets"""
    F.check_d_sw_rest("hip", n, face, coloured=True, adjoint_on=[0, 1, 2], adjoint_thin=3)


@pytest.mark.parametrize("n,face", [(8, 1), (12, 4)])
def test_d_sw_divergence_damping_cap(n, face):
    F.check_d_sw_rest("hip", n, face, coloured=True, adjoint_on=[2], amplify=2.0)


@pytest.mark.parametrize("group", ["c_sw_rest", "d_sw_rest"])
def test_rest_operators_c70(group):
    if group == "c_sw_rest":
        F.check("hip", group, 70, 2, npz=2, adjoint_all=False, coloured=True, adjoint_levels=1, adjoint_thin=4)
    else:
        F.check_d_sw_rest("hip", 70, 2, case=F.DSW_REST_C70, adjoint_all=False, coloured=True, adjoint_levels=1, adjoint_thin=8)


@pytest.mark.parametrize("group", ["d_sw", "p_grad_c", "c_sw_rest", "d_sw_rest"])
def test_face_edge_operator_c16_cut_2x2_more(group):
    """the 2 x 2 layout for the first loops of d_sw, p_grad_c and the two operators that follow the area fluxes / the first loops
    (d_sw_rest on its three levels; u_m, v_m by composition are left to the whole-face tests)"""
    kw = dict(npz=F.DSW_REST["npz"], opt=F.DSW_REST["opt"]) if group == "d_sw_rest" else {}
    F.check_layout("hip", group, **kw)


@pytest.mark.parametrize("group,face", [("c_sw_rest", 0), ("d_sw_rest", 5), ("c_sw", 3), ("d_sw", 4)])
def test_sin_sg_selection_on_detuned_metrics(group, face):
    """C8 with every sin_sg / cos_sg plane scaled by a factor of its own, in library and restatement alike: across a face edge the true
    cube holds sin_sg(i, j-1, 4) = sin_sg(i, j, 2), so only this shows which of the two a branch takes"""
    if group == "d_sw_rest":
        F.check_d_sw_rest("hip", 8, face, coloured=True, adjoint_on=[1], detune=True)
    else:
        F.check("hip", group, 8, face, detune=True)


@pytest.mark.parametrize("face", range(6))
@pytest.mark.parametrize("n", [8, 12])
def test_c_sw_non_hydrostatic_w(n, face):
    """c_sw_rest on a non-hydrostatic case: w through fill_4corners and the upwind fluxes into wc (sw_core_nlm.F90:210-284), beside the
    other outputs"""
    F.check("hip", "c_sw_rest_nh", n, face, opt=dict(hydrostatic=0), coloured=True, adjoint_on=[0, 1, 2], adjoint_thin=2)


@pytest.mark.parametrize("face", range(6))
@pytest.mark.parametrize("n", [8, 12])
@pytest.mark.parametrize("nord", [2, 3])
def test_d_sw_split_damp_trajectory_nord(nord, n, face):
    """split_damp with the trajectory's nord = 2, 3 over the perturbation's nord = 1 on level 2: the VALUES of ke2 (and of u_m, v_m) from
    the trajectory's damping -- the higher-order loop with fill_corners in its B-grid scalar and D-grid vector forms, nord_v = 2 --
    the tangent and the adjoint with the perturbation's coefficients"""
    F.check_d_sw_rest("hip", n, face, case=F.DSW_SPLIT[nord], coloured=True, adjoint_on=[0, 1], adjoint_thin=3)
