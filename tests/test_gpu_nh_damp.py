"""-m gpu: the non-hydrostatic step with a trajectory nord of 2 and 3 through fv3lm_set_trajectory_damping_order of the HIP library on an
MI355X (checks and tolerances in nh_damp_checks.py): against the oracle on the periodic tile and on six faces, sub-face tiles against
whole faces, the differentiated del-6 of w alone against the numpy restatement del6_oracle.py with its adjoint dot products, the
hydrostatic set-equals-create identity, the LDS-tiled launch of the chain against the staged chain (1e-12), and the HIP-event times of
the order-2 chain, tiled and staged (printed, no threshold)."""
import numpy as np
import pytest
import nh_checks as N
import nh_damp_checks as K
from oracle import NL, TL, AD

BACKEND = "hip"
pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[2, 3])
def tile(request):
    return K.tile_case(BACKEND, request.param)


def test_dyn_core_tangent(tile):
    lw, lv = K.level_orders(tile)
    assert {n for n, _ in lw} == {0, 2} and {n for n, _ in lv} == {0, 2}
    N.check_nh_tangent(tile)


def test_dyn_core_adjoint(tile):
    N.check_nh_adjoint(tile)


def test_dyn_core_dot_product(tile):
    N.check_nh_dot_product(tile)


@pytest.fixture(scope="module", params=[2, 3])
def tile_fv(request):
    return K.tile_case_fv(BACKEND, request.param)


def test_fv_dynamics_tangent(tile_fv):
    N.check_nh_fv_tangent(tile_fv)


def test_fv_dynamics_adjoint(tile_fv):
    N.check_nh_fv_adjoint(tile_fv)


def test_fv_dynamics_dot_product(tile_fv):
    N.check_nh_fv_dot_product(tile_fv)


@pytest.fixture(scope="module", params=[2, 3])
def cube(request):
    return K.cube_case(BACKEND, request.param)


@pytest.mark.parametrize("mode", [TL, AD])
def test_cube_fv_dynamics(cube, mode):
    N.cube_check_nh_fv(cube, mode)


def test_cube_dot_product(cube):
    N.cube_check_nh_dot_product(cube)


def test_sub_face_tiles_equal_whole_faces():
    from layout_checks import check_layout_equals_whole_faces
    check_layout_equals_whole_faces(lambda L: K.layout_case(BACKEND, 2, L), 2, tol=1e-11)


@pytest.fixture(scope="module", params=[(1, None), (2, None), (1, 2), (2, 2)], ids=["nord1-tile", "nord2-tile", "nord1-face", "nord2-face"])
def dsw(request):
    nord, face = request.param
    return nord, K.dsw_case(BACKEND, nord, face)


def test_dw_against_restatement(dsw):
    nord, c = dsw
    _, orders = K.check_dw_against_restatement(c)
    assert orders == [0, nord]


def test_dw_adjoint_dot_product(dsw):
    _, c = dsw
    lhs, rhs, w_ad = K.dw_dot_product(c)
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)
    halo = w_ad.copy(); halo[c.rect(1, c.nx, 1, c.ny)] = 0.0
    assert np.abs(halo).max() > 0


@pytest.mark.parametrize("face", [None, 2])
def test_dw_adjoint_dot_product_seeded_on_dw(monkeypatch, face):
    monkeypatch.setenv("FV3LM_NO_AD_WRITE_MODE", "1")
    c = K.dsw_case(BACKEND, 2, face)
    lhs, rhs, _ = K.dw_dot_product(c, through="dw")
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)


# ---- the chain as one LDS-tiled launch (FV3LM_DEL6_FUSED=1) against the staged chain (0, the default): 1e-12 on the device, both directions
@pytest.mark.parametrize("nord,face", [(1, None), (2, None), (1, 2), (2, 2)], ids=["nord1-tile", "nord2-tile", "nord1-face", "nord2-face"])
def test_tiled_equals_staged_dsw(monkeypatch, nord, face):
    K.check_tiled_equals_staged_dsw(monkeypatch, BACKEND, nord, face, 1e-12, 1e-12)


def test_tiled_equals_staged_dyn_core(monkeypatch):
    K.check_tiled_equals_staged_dyn_core(monkeypatch, BACKEND, 1e-12, 1e-12)


def test_tiled_against_the_oracle(monkeypatch):
    monkeypatch.setenv("FV3LM_DEL6_FUSED", "1")
    c = K.tile_case(BACKEND, 2)
    N.check_nh_tangent(c); N.check_nh_adjoint(c); N.check_nh_dot_product(c)
    c = K.cube_case(BACKEND, 2)
    N.cube_check_nh_fv(c, TL); N.cube_check_nh_fv(c, AD)


def test_tiled_adjoint_on_tiles_without_a_corner(monkeypatch):
    from layout_checks import check_layout_equals_whole_faces
    monkeypatch.setenv("FV3LM_DEL6_FUSED", "1")
    check_layout_equals_whole_faces(lambda L: K.edge_tile_case(BACKEND, L), 3, tol=1e-11)


@pytest.mark.parametrize("start,target", [(1, 2), (3, 1)])
def test_hydrostatic_set_equals_create(start, target):
    K.check_set_equals_create(BACKEND, start, target)


def test_measure_order_two_chain_48x48x72(monkeypatch):
    """no threshold: the figures go to DESIGN.md (non-hydrostatic nord 2, measured cost).  HIP-event times, median of 3 profiled calls after
    one warm-up, of the launches of the del-6 chain -- tiled (Del6) and staged (Del6A, Del6B and the two consumers) -- and of the whole
    fv3lm_dyn_core, order 1 and order 2"""
    from common import Case
    from test_oracle_nh import nh_state
    chain = ("Del6", "DswDw", "UpdateDzD")
    for nord, fused in ((1, "0"), (2, "1"), (2, "0")):
        monkeypatch.setenv("FV3LM_DEL6_FUSED", fused)
        c = Case(nx=48, ny=48, npz=72, n_split=2, dt=300.0, backend=BACKEND, oracle=False, nord=nord, **K.NH)
        T, P = nh_state(c)
        label = "nord %d %s" % (nord, "tiled" if fused == "1" else "staged")
        for mode in (NL, TL, AD):
            tot, per = [], []
            for r in range(4):
                N.put(c, T, P)
                if mode == AD:
                    c.dy.dyn_core(NL)
                c.dy.sync(); c.dy.profile_begin()
                c.dy.dyn_core(mode)
                prof = c.dy.profile_end()
                tot.append(sum(v[1] for v in prof.values()))
                per.append({k: (v[0], v[1]) for k, v in prof.items() if k.startswith(chain)})
            med = float(np.median(tot[1:]))
            assert med > 0.
            print("fv3lm_dyn_core 48x48x72 non-hydrostatic, %s, mode %d: %.3f ms (runs %s)" % (label, mode, med, " ".join("%.3f" % t for t in tot[1:])))
            for k in sorted(per[-1]):
                ms = float(np.median([p[k][1] for p in per[1:]]))
                print("    %-16s %3d launches  %.4f ms  (%.4f ms per launch)" % (k, per[-1][k][0], ms, ms / max(1, per[-1][k][0])))
