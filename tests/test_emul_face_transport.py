"""CPU (-m "not gpu"): fv_tp_2d on whole faces through the host-emulation build -- the transports of d_sw (delp, pt, absolute vorticity)
with every trajectory scheme 1 .. 13 over the perturbation scheme, their fluxes, delp_o, pt_o and u_m, v_m, point by point and region by
region against tests/face_oracle.py (xppm, yppm, pert_ppm, deln_flux, fv_tp_2d restated from the nonlinear routines of
model_tlmadm/tp_core_tlm.F90), face_edge_checks.DSwTransport: values, tangent and adjoint, the restatement's branch census holding every
branch of the scheme taken both ways and no discontinuous selector near its switch."""
import pytest
import face_edge_checks as F

PERT = {6: 333, 3: 1}


@pytest.mark.parametrize("h", range(1, 14))
def test_every_trajectory_scheme(h):
    """C12, face h % 6, perturbation scheme 2 (333 under h = 6, 1 under h = 3)"""
    F.check_transport("emul", 12, h % 6, h, PERT.get(h, 2))


@pytest.mark.parametrize("face", range(6))
@pytest.mark.parametrize("n", [8, 12])
@pytest.mark.parametrize("h", [2, 10])
def test_all_six_faces(h, n, face):
    """h = 2 unsplit (the single fused pass) and the operational pairing 10 over 2"""
    F.check_transport("emul", n, face, h)


@pytest.mark.parametrize("switch", ["FV3LM_TP_FUSED"])
@pytest.mark.parametrize("h", [5, 10])
def test_kernel_forms(h, switch):
    """the other device form of the same arithmetic.  The staged stages (FV3LM_TP_FUSED=0) hold no trajectory pass: the library refuses a
    split scheme under them, which is kept on record here, and test_staged_forward_unsplit runs them"""
    from fv3_jedi_linearmodel_amd._lib import Fv3LmError
    with pytest.raises(Fv3LmError, match="need the fused fv_tp_2d"):
        F.check_transport("emul", 12, 3, h, env={switch: "0"})


@pytest.mark.parametrize("h", [1, 2, 333])
def test_staged_forward_unsplit(h):
    """the staged stages of fv_tp_2d (FV3LM_TP_FUSED=0) with the schemes they hold: trajectory and perturbation share 1, 2 or 333"""
    F.check_transport("emul", 12, 3, h, h, env={"FV3LM_TP_FUSED": "0"})


@pytest.mark.parametrize("h", [6, 10])
def test_block_cutting_c70(h):
    """edge strips and corners beside a bulk of several 64 x 16 blocks"""
    F.check_transport("emul", 70, 2, h, PERT.get(h, 2), adjoint_thin=64)


@pytest.mark.parametrize("h", [2, 10])
def test_damped_fluxes(h):
    """DELN_FLUX with nord = 1 on level 2, without the mass (delp) and with it (pt), beside the nord = 0 form of level 1"""
    F.check_transport("emul", 12, 4, h, more=F.TRANSPORT_DAMPED)


@pytest.mark.parametrize("h,face", [(2, 1), (8, 5)])
def test_edge_value_on_detuned_lengths(h, face):
    """C8 with dxa, dya scaled by 1 + 0.01 i - 0.007 j (and the sin_sg / cos_sg planes apart): on the cube dxa(0, j) = dxa(1, j), so only
    this shows which length the two-sided edge value of xppm / yppm takes where"""
    F.check_transport("emul", 8, face, h, detune=True)


@pytest.mark.parametrize("h,face", [(6, 0), (10, 4)])
def test_non_hydrostatic_w(h, face):
    """w beside the others: its damping increment (damp_w is on: del6_vt_flux of w runs), its transport with hord_vt = h and the mass fluxes, w_m"""
    F.check_transport("emul", 12, face, h, PERT.get(h, 2), more=dict(hydrostatic=0))


def test_c16_cut_2x2():
    """six faces of C16 in 24 tiles under the operational pairing 10 over 2: every tile's fluxes, delp_o, pt_o and u_m, v_m on its own rects
    against the windows of the whole-face restatement"""
    F.check_layout("emul", "d_sw_transport", npz=2, opt=F.transport_opt(10))
