"""CPU (-m "not gpu"): face_edge_checks.py through the host-emulation build of the stage code -- c_sw (ua, va, utf, vtf, divgd), the first
loops of d_sw (crx, cry, xfx, yfx), one_grad_p
(u_o, v_o through a2b_ord4 with replace) and p_grad_c (uc, vc) on whole faces n = 8 and 12, all six faces, values, tangent and adjoint,
point by point and region by region against the restatement, with the restatement's metrics (poisoned) in the library.  n = 6, which
the issue behind these tests also names, is refused by fv3lm_create (nx, ny >= 8): test_c6_is_refused keeps that on record."""
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


@pytest.mark.parametrize("fused", ["0", "1"])
@pytest.mark.parametrize("face", range(6))
@pytest.mark.parametrize("n", [8, 12])
def test_d_sw_first_loops(n, face, fused):
    """crx, cry, xfx, yfx from uc, vc (the rows that read sin_sg(0, j <= 0, 3) and their kin), the adjoint under both
    FV3LM_TP_AD_FUSED settings"""
    F.check("emul", "d_sw", n, face, env={"FV3LM_TP_AD_FUSED": fused})


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
