"""-m gpu: face_edge_checks.py through the C-ABI of the HIP library: c_sw, one_grad_p and p_grad_c on whole faces n = 8 and 12, all six
faces, and C70 on one face (strips beyond one 64-column block), values, tangent and adjoint per point and region against the
restatement of the reference's nonlinear Fortran."""
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
    """crx, cry, xfx, yfx from uc, vc (the rows that read sin_sg(0, j <= 0, 3) and their kin), the adjoint under both
    FV3LM_TP_AD_FUSED settings"""
    F.check("hip", "d_sw", n, face, env={"FV3LM_TP_AD_FUSED": fused})
