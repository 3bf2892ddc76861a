"""CPU (-m "not gpu"): the non-hydrostatic step with a trajectory nord of 2 and 3, reached through fv3lm_set_trajectory_damping_order, on
the host-emulation build (checks and tolerances in nh_damp_checks.py): against the oracle on the periodic tile and on six faces, the
differentiated del-6 of w alone against the numpy restatement del6_oracle.py, sub-face tiles against whole faces, and the setter itself.
The Fortran binding of the setter and of the getter is called by fortran/shim_driver.F90 (with the order the handle has, so that the
driver's results, which tests/shim_checks.py holds against ctypes bit for bit, stay what they were); a change of the order through Fortran
would need a new input of that driver and is covered by the ctypes calls of the same symbol here."""
import numpy as np
import pytest
import nh_checks as N
import nh_damp_checks as K
from common import Case
from oracle import TL, AD

BACKEND = "emul"


# ---- 1. against the oracle, periodic tile
@pytest.fixture(scope="module", params=[2, 3])
def tile(request):
    return K.tile_case(BACKEND, request.param)


def test_orders_of_the_tile(tile):
    lw, lv = K.level_orders(tile)
    assert {n for n, _ in lw} == {0, 2} and {n for n, _ in lv} == {0, 2}      # sponge and regular levels both present
    assert tile.dy.trajectory_damping_order() == tile.opt.nord


def test_dyn_core_tangent(tile):
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


def test_order_two_is_not_order_one():
    """the tangent of a step with the trajectory's nord = 2 differs from the one with nord = 1 far beyond the tolerances above: a product
    that stayed at order 1 would not pass them"""
    out = []
    for nord in (1, 2):
        c = K.tile_case(BACKEND, nord, oracle=False)
        from test_oracle_nh import nh_state
        T, P = nh_state(c)
        N.put(c, T, P)
        c.dy.dyn_core(TL)
        out.append(c.dy.get("w", 1)[0][c.rect(1, c.nx, 1, c.ny)].copy())
    assert K.relerr(out[0], out[1]) > 1e-7


# ---- 2. six faces
@pytest.fixture(scope="module", params=[2, 3])
def cube(request):
    return K.cube_case(BACKEND, request.param)


@pytest.mark.parametrize("mode", [TL, AD])
def test_cube_fv_dynamics(cube, mode):
    N.cube_check_nh_fv(cube, mode)


def test_cube_dot_product(cube):
    N.cube_check_nh_dot_product(cube)


def test_sub_face_tiles_equal_whole_faces():
    """8-wide tiles of C16 (windowed kernels, at most one cube corner per tile) against the six whole faces; six levels (three of the
    sponge, three of order 2) and one remap step keep the two C16 runs of the host emulation to a few seconds"""
    from layout_checks import check_layout_equals_whole_faces
    check_layout_equals_whole_faces(lambda L: K.layout_case(BACKEND, 2, L, small=True), 2, tol=1e-11)


# ---- 3. the operator alone
@pytest.fixture(scope="module", params=[(1, None), (2, None), (1, 2), (2, 2)], ids=["nord1-tile", "nord2-tile", "nord1-face", "nord2-face"])
def dsw(request):
    nord, face = request.param
    return nord, K.dsw_case(BACKEND, nord, face)


def test_dw_against_restatement(dsw):
    nord, c = dsw
    _, orders = K.check_dw_against_restatement(c)
    assert orders == [0, nord]          # over the four cases: orders 0, 1 and 2


def test_dw_adjoint_dot_product(dsw):
    _, c = dsw
    lhs, rhs, w_ad = K.dw_dot_product(c)
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)
    halo = w_ad.copy(); halo[c.rect(1, c.nx, 1, c.ny)] = 0.0
    assert np.abs(halo).max() > 0          # the adjoint does reach the halo rows


@pytest.mark.parametrize("face", [None, 2])
def test_dw_adjoint_dot_product_seeded_on_dw(monkeypatch, face):
    """the same identity with the adjoint of the increment itself as seed, on a handle whose backward sweep clears and accumulates"""
    monkeypatch.setenv("FV3LM_NO_AD_WRITE_MODE", "1")
    c = K.dsw_case(BACKEND, 2, face)
    lhs, rhs, _ = K.dw_dot_product(c, through="dw")
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)


# ---- 4. the chain as one LDS-tiled launch (FV3LM_DEL6_FUSED=1) against the staged chain (FV3LM_DEL6_FUSED=0; unset: the same)
@pytest.mark.parametrize("nord,face", [(1, None), (2, None), (1, 2), (2, 2)], ids=["nord1-tile", "nord2-tile", "nord1-face", "nord2-face"])
def test_tiled_equals_staged_dsw(monkeypatch, nord, face):
    """forward modes bit for bit (the block keeps the staged expressions in their order), adjoint 1e-13 (on the face the staged adjoint
    runs in both: the tiled adjoint leaves tiles with a cube corner to it)"""
    K.check_tiled_equals_staged_dsw(monkeypatch, BACKEND, nord, face, 0, 1e-13)


def test_tiled_equals_staged_dyn_core_and_lds_guard(monkeypatch):
    """the periodic case of the oracle checks; the run also passes the LDS guard of the host emulation (csrc/tiled.h run_tiled): a block of
    the new launch that wrote past its declared LDS would fail the call"""
    K.check_tiled_equals_staged_dyn_core(monkeypatch, BACKEND, 0, 1e-13)


def test_tiled_adjoint_on_tiles_without_a_corner(monkeypatch):
    """sub-face tiles, five of nine per face without a cube corner (tiled adjoint) against whole faces (staged adjoint)"""
    from layout_checks import check_layout_equals_whole_faces
    monkeypatch.setenv("FV3LM_DEL6_FUSED", "1")
    check_layout_equals_whole_faces(lambda L: K.edge_tile_case(BACKEND, L), 3, tol=1e-11)


def test_tiled_against_the_oracle(monkeypatch):
    """the tiled launch in the oracle checks themselves: periodic tile (tiled in every mode) and six faces (tiled forward, staged adjoint)"""
    monkeypatch.setenv("FV3LM_DEL6_FUSED", "1")
    c = K.tile_case(BACKEND, 2)
    N.check_nh_tangent(c); N.check_nh_adjoint(c); N.check_nh_dot_product(c)
    c = K.cube_case(BACKEND, 2)
    N.cube_check_nh_fv(c, TL); N.cube_check_nh_fv(c, AD)


def test_the_switch_is_off_by_default(monkeypatch):
    """unset and 0 build the same program: the staged chain"""
    n = []
    for v in (None, "0", "1"):
        monkeypatch.delenv("FV3LM_DEL6_FUSED", raising=False)
        if v is not None:
            monkeypatch.setenv("FV3LM_DEL6_FUSED", v)
        n.append(K.dsw_fields(K.dsw_case(BACKEND, 2))[1])
    assert n[0] == n[1] == n[2] + 2


# ---- 5. the setter
@pytest.mark.parametrize("start,target", [(1, 2), (3, 1), (2, 3)])
def test_hydrostatic_set_equals_create(start, target):
    K.check_set_equals_create(BACKEND, start, target)


def test_setter_order_with_external_damping():
    a = K.hydro_case(BACKEND, 1); a.dy.set_external_damping(0.02); a.dy.set_trajectory_damping_order(2)
    b = K.hydro_case(BACKEND, 1); b.dy.set_trajectory_damping_order(2); b.dy.set_external_damping(0.02)
    K.assert_same_bits(K.step_bits(a), K.step_bits(b))
    K.assert_same_bits(K.step_bits(b), K.step_bits(K.hydro_case(BACKEND, 2, d_ext=0.02)))


def test_setting_the_current_order_changes_nothing():
    a, b = K.hydro_case(BACKEND, 2), K.hydro_case(BACKEND, 2)
    ref = K.step_bits(b)
    n0 = a.dy.launch_count()
    first = K.step_bits(a)
    per_sweep = a.dy.launch_count() - n0
    a.dy.set_trajectory_damping_order(2)
    n1 = a.dy.launch_count()
    again = K.step_bits(a)
    assert a.dy.launch_count() - n1 == per_sweep
    K.assert_same_bits(first, ref); K.assert_same_bits(again, ref)


def test_handles_that_never_call_the_setter_launch_what_they_did():
    """an order-1 non-hydrostatic handle created directly and one that went 1 -> 2 -> 1 run the same number of launches and give the same bits"""
    from test_oracle_nh import nh_state
    res = []
    for back_and_forth in (False, True):
        c = Case(nx=12, ny=10, npz=12, n_split=2, dt=600.0, backend=BACKEND, oracle=False, nord=1, **{k: v for k, v in K.NH.items() if k != "late_nord"})
        if back_and_forth:
            c.dy.set_trajectory_damping_order(2); c.dy.set_trajectory_damping_order(1)
        T, P = nh_state(c)
        N.put(c, T, P)
        n0 = c.dy.launch_count()
        c.dy.dyn_core(TL)
        res.append((c.dy.launch_count() - n0, c.dy.get("w", 1).copy(), c.dy.get("delz", 1).copy()))
    assert res[0][0] == res[1][0]
    assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][2], res[1][2])


def test_order_set_after_the_rayleigh_damping_equals_before():
    """non-hydrostatic handle with the Rayleigh damping on: its form of pt_in writes into the work arena the rebuild moves"""
    from test_oracle_nh import nh_state_fv
    kw = dict(nx=12, ny=10, npz=12, n_split=2, k_split=2, nq=1, dt=1200.0, backend=BACKEND, oracle=False, tau=0.2, rf_cutoff=3.0e4)
    nh = {k: v for k, v in K.NH.items() if k != "late_nord"}
    a = Case(nord=1, **kw, **nh); a.dy.set_trajectory_damping_order(2)          # Rayleigh first, then the order
    b = Case(nord=2, late_nord=True, **kw, **nh)                               # the order first (harness), then Rayleigh
    assert a.dy.rayleigh_profile()[1] > 0
    out = []
    for c in (a, b):
        T, P = nh_state_fv(c)
        N.fv_put(c, T, P)
        c.dy.fv_dynamics(TL)
        out.append({(n, w): c.dy.get(n, w).copy() for n in N.fv_names(c) for w in (0, 1)})
    K.assert_same_bits(out[0], out[1])


REFUSALS = [("hydro", 4, "nord in 0..3"), ("hydro", -1, "nord in 0..3"), ("hydro", 0, "nord = 0 with nord_pert > 0"), ("nosplit", 2, "split_damp = 0")]


@pytest.mark.parametrize("kind,nord,msg", REFUSALS)
def test_refusals_leave_the_handle_as_it_was(kind, nord, msg):
    if kind == "hydro":
        c, ref = K.hydro_case(BACKEND, 2), K.hydro_case(BACKEND, 2)
    else:
        kw = dict(nx=12, ny=10, npz=12, n_split=2, k_split=1, dt=1800.0, backend=BACKEND, oracle=False)
        c, ref = Case(**kw), Case(**kw)
    before = c.dy.trajectory_damping_order()
    with pytest.raises(RuntimeError, match=msg):
        c.dy.set_trajectory_damping_order(nord)
    assert c.dy.trajectory_damping_order() == before
    K.assert_same_bits(K.step_bits(c), K.step_bits(ref))          # the handle still steps, as if nothing had been asked


def test_null_handle_is_refused():
    import ctypes as C
    c = K.hydro_case(BACKEND, 1)
    L = c.dy.lib.L
    L.fv3lm_set_trajectory_damping_order.argtypes = [C.c_void_p, C.c_int]
    L.fv3lm_trajectory_damping_order.argtypes = [C.c_void_p, C.POINTER(C.c_int)]
    assert L.fv3lm_set_trajectory_damping_order(None, 2) != 0 and "null handle" in c.dy.lib.err()
    n = C.c_int(7)
    assert L.fv3lm_trajectory_damping_order(None, C.byref(n)) != 0 and n.value == 7
    assert L.fv3lm_trajectory_damping_order(c.dy.h, None) != 0
    assert c.dy.trajectory_damping_order() == 1


def test_create_still_refuses_the_non_hydrostatic_order_two():
    with pytest.raises(RuntimeError, match="non-hydrostatic with a trajectory nord > 1: the w / height damping would need the tangent of del6_vt_flux with nord 2"):
        Case(nx=12, ny=10, npz=6, backend=BACKEND, oracle=False, split_damp=1, nord=2, hydrostatic=0)
