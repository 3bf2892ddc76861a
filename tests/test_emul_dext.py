"""CPU (-m "not gpu") tests of the external-mode divergence damping of the acoustic step (flagstruct%d_ext; fv3lm_set_external_damping,
csrc/dext.h) on the host-emulation build of the product's stage code, against the numpy restatement of dext_oracle.py composed with the
C++ oracle's pieces (dext_checks.py): the unit on the periodic tile and on faces, its place in one acoustic step in the three modes, two
acoustic steps, the dot-product identity (tile, face data on six faces, sub-face tiles), the off state, the non-hydrostatic handle, a
repeated adjoint, the refusals, and the Fortran binding."""
import os
import numpy as np
import pytest
from oracle import NL, TL, AD
import dext_checks as DC

BACKEND = "emul"


def case(**kw):
    from common import Case
    return Case(backend=BACKEND, **kw)


def cube(**kw):
    from common import CubeCase
    return CubeCase(backend=BACKEND, **kw)


# ---- 1. units against the restatement
@pytest.mark.parametrize("cfg", list(DC.SPONGE))
def test_unit_periodic_tile(cfg):
    DC.check_unit(case(**DC.TILE, n_split=1, d_ext=DC.D_EXT, **DC.SPONGE[cfg]))


def test_unit_periodic_tile_split_damp():
    DC.check_unit(case(**DC.TILE, n_split=1, d_ext=DC.D_EXT, **DC.SPLIT))


@pytest.mark.parametrize("face", [0, 3])
@pytest.mark.parametrize("cfg", list(DC.SPONGE))
def test_unit_face(face, cfg):
    """one whole face, all four edges and corners with the metrics of the restatement, 1e30 where the reference leaves them undefined"""
    import face_edge_checks as FE
    n = DC.FACE["nx"]
    DC.check_unit(case(**DC.FACE, n_split=1, face=face, metrics_hook=FE.restatement_hook(n, face), d_ext=DC.D_EXT, **DC.SPONGE[cfg]))


# ---- 2. place in the step
@pytest.mark.parametrize("mode", [NL, TL, AD])
@pytest.mark.parametrize("cfg", list(DC.SPONGE))
def test_step(cfg, mode):
    kw = dict(**DC.TILE, n_split=1, dt=900.0, **DC.SPONGE[cfg])
    DC.check_step(case(d_ext=DC.D_EXT, **kw), mode, off=case(**kw))


@pytest.mark.parametrize("mode", [NL, TL])
def test_step_split_damp(mode):
    kw = dict(**DC.TILE, n_split=1, dt=900.0, **DC.SPLIT)
    c = case(d_ext=DC.D_EXT, **kw)
    val, tan = DC.nords(c)
    assert any(a != b and (a == 0 or b == 0) for a, b in zip(val, tan)), (val, tan)      # a level whose value and tangent branches differ
    DC.check_step(c, mode, off=case(**kw))


# ---- 3. more than one acoustic step
@pytest.mark.parametrize("mode", [TL, AD])
def test_two_steps(mode):
    DC.check_two_steps(case(**DC.TILE, n_split=2, dt=1800.0, d_ext=DC.D_EXT), mode)


# ---- 4. dot-product identity
def _dot(lhs, rhs):
    print("dot product: %.3e" % (abs(lhs - rhs) / abs(lhs)))
    assert abs(lhs - rhs) <= DC.TOL_DOT * abs(lhs), (lhs, rhs)


def test_dot_product_dyn_core_tile():
    from groups import dot_product_test
    _dot(*dot_product_test(case(**DC.TILE, n_split=2, oracle=False, d_ext=DC.D_EXT)))


def test_dot_product_step_tile():
    from groups import dot_product_step
    _dot(*dot_product_step(case(**DC.TILE, n_split=2, k_split=2, nq=1, oracle=False, d_ext=DC.D_EXT)))


def test_dot_product_six_faces():
    from groups import cube_dot_product, cube_dot_product_step
    c = cube(n=12, npz=6, n_split=2, k_split=1, nq=1, d_ext=DC.D_EXT)
    _dot(*cube_dot_product(c))
    _dot(*cube_dot_product_step(c))


def test_dot_product_sub_face_tiles():
    """2 x 2 tiles per face: the adjoint of the ring of delp around a tile travels with the existing adjoint exchange"""
    from groups import cube_dot_product_step
    _dot(*cube_dot_product_step(cube(n=16, npz=6, n_split=2, k_split=1, nq=0, layout=2, d_ext=DC.D_EXT)))


def test_sub_face_tiles_equal_whole_faces():
    from layout_checks import check_layout_equals_whole_faces
    check_layout_equals_whole_faces(lambda L: cube(n=16, npz=6, n_split=2, k_split=1, dt=900.0, nq=0, layout=L, d_ext=DC.D_EXT), 2)


# ---- 5. off state
def test_off_state():
    kw = dict(**DC.TILE, n_split=2, k_split=2, nq=1, oracle=False)
    base = case(**kw)
    assert base.dy.external_damping() == 0.0
    zero = case(d_ext=0.0, **kw)
    back = case(d_ext=DC.D_EXT, **kw); back.dy.set_external_damping(0.0)
    assert back.dy.external_damping() == 0.0
    la = DC.check_same(base, zero)
    DC.check_same(base, back)
    on = case(d_ext=DC.D_EXT, **kw)
    lo = DC.run_all(on)[1]
    DC.check_added_launches(la, lo, BACKEND)
    assert on.dy.levels("divg2") == 1
    from fv3_jedi_linearmodel_amd._lib import Fv3LmError
    with pytest.raises(Fv3LmError, match="unknown field divg2"):
        base.dy.levels("divg2")


# ---- 6. non-hydrostatic
def test_non_hydrostatic_accepts_and_adds_nothing():
    kw = dict(nx=12, ny=10, npz=6, n_split=2, k_split=1, nq=0, oracle=False, hydrostatic=0)
    on = case(d_ext=DC.D_EXT, **kw)
    assert on.dy.external_damping() == DC.D_EXT
    DC.check_same(case(**kw), on)


# ---- 7. repeated adjoint
def test_repeated_adjoint():
    from groups import repeated_adjoint
    e = repeated_adjoint(case(**DC.TILE, n_split=2, k_split=2, nq=1, oracle=False, d_ext=DC.D_EXT))
    assert e == 0.0, e


# ---- the backward sweep without trajectory slots: every step recomputes its intermediates, divg2 and W among them
def test_without_trajectory_slots(monkeypatch):
    monkeypatch.setenv("FV3LM_TRAJ_SLOTS", "0")
    c = case(**DC.TILE, n_split=2, dt=1800.0, d_ext=DC.D_EXT)
    assert c.dy.lib.L.fv3lm_traj_slots(c.dy.h) == 0
    DC.check_two_steps(c, AD)


# ---- 8. refusals
def test_refusals():
    DC.check_refusals(case(**DC.TILE, n_split=2, nq=0, oracle=False, d_ext=DC.D_EXT))
    DC.check_refusals(case(**DC.TILE, n_split=2, nq=0, oracle=False))


# ---- the setter between complete steps
def test_switching_on_between_steps_equals_a_fresh_handle():
    kw = dict(**DC.TILE, n_split=2, k_split=2, nq=1, oracle=False)
    a = case(**kw)
    DC.run_all(a)
    a.dy.set_external_damping(DC.D_EXT)
    b = case(d_ext=DC.D_EXT, **kw)
    (oa, la), (ob, lb) = DC.run_all(a), DC.run_all(b)
    assert la == lb and all(np.array_equal(x, y) for x, y in zip(oa, ob))
    a.dy.set_external_damping(0.5 * DC.D_EXT)          # the coefficient alone: no rebuild, felt by the next step
    oc = DC.run_all(a)[0]
    assert not np.array_equal(oc[0], oa[0])


# ---- 9. Fortran
def test_fortran_binding_is_declared_and_called():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    mod = open(os.path.join(root, "fortran", "fv3lm_hip_mod.F90")).read()
    for name in ("fv3lm_set_external_damping", "fv3lm_external_damping"):
        assert 'bind(C, name="%s")' % name in mod, name
    drv = open(os.path.join(root, "fortran", "shim_driver.F90")).read()
    assert "call fv3lm_hip_set_external_damping(dyn, 0.0_c_double)" in drv and "call fv3lm_hip_external_damping(dyn, d_ext)" in drv
