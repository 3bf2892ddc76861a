"""Host emulation (CPU): the tracer damping of tracer_2d -- nord_tr, trdm2, nord_tr_pert, trdm2_pert, split_damp_tr through
fv3lm_set_tracer_damping -- against the oracle's per-level fv_tp_2d composed by the rules of the reference's call site
(tracer_damp_oracle.py): the unit in the tangent and adjoint modes on the periodic tile, sub-cycled, on one whole face and over
several fused blocks; the whole step (dot products, sub-face tiles, the trajectory of step_tl); the off state; the refusals."""
import pytest
from oracle import TL, AD
import tracer_damp_checks as TC

BACKEND = "emul"
UNIT = dict(nx=12, ny=10, npz=6, n_split=2, nq=2)


def case(name=None, **kw):
    from common import Case
    optkw, dmp, _ = TC.SETS[name] if name else ({}, {}, False)
    return Case(backend=BACKEND, **{**UNIT, **optkw, **dmp, **kw})


@pytest.fixture(scope="module")
def plain():
    """no damping: the composition's own check, and the inputs every unit case shares"""
    return case()


@pytest.mark.parametrize("scale", [1.0, 10.0])
def test_composition_is_the_oracle_without_damping(plain, scale):
    nsplt = TC.check_composition(plain, scale)
    assert (nsplt > 1) == (scale > 1.0)


@pytest.mark.parametrize("mode", [TL, AD])
@pytest.mark.parametrize("name", ["equal_nord0", "equal_nord1", "split_nord2", "split_pert_off"])
def test_unit(name, mode):
    TC.check_unit(case(name), TC.SETS[name][1], mode)


@pytest.mark.parametrize("mode", [TL, AD])
def test_unit_trajectory_below_threshold_is_the_off_state(mode):
    c = case("traj_off")
    assert c.dy.tracer_damping() == ((1, 5e-5), (1, 0.1))
    TC.check_unit(c, TC.SETS["traj_off"][1], mode, damped=False)
    TC.check_same_as(c, case(**TC.SPLIT), mode)


@pytest.mark.parametrize("mode", [TL, AD])
def test_unit_without_split_damp_tr(mode):
    c = case("no_split_damp")
    assert c.dy.tracer_damping() == ((1, 0.15), (1, 0.15))
    TC.check_unit(c, TC.SETS["no_split_damp"][1], mode)
    TC.check_same_as(c, case(nord_tr=1, trdm2=0.15, nord_tr_pert=1, trdm2_pert=0.15, split_damp_tr=1), mode)


@pytest.mark.parametrize("mode", [TL, AD])
@pytest.mark.parametrize("name", ["equal_nord1", "split_nord2"])
def test_unit_subcycled(name, mode):
    TC.check_unit(case(name), TC.SETS[name][1], mode, scale=10.0, want_nsplt=2)


@pytest.mark.parametrize("mode", [TL, AD])
@pytest.mark.parametrize("name", ["equal_nord0", "equal_nord1"])
def test_unit_one_face(name, mode):
    TC.check_unit(case(name, nx=8, ny=8, face=2), TC.SETS[name][1], mode)


@pytest.mark.parametrize("mode", [TL, AD])
def test_unit_several_fused_blocks(mode):
    TC.check_unit(case("equal_nord1", nx=72, ny=24, npz=3), TC.SETS["equal_nord1"][1], mode)


STEP = dict(nord_tr=1, trdm2=0.15, nord_tr_pert=0, trdm2_pert=0.0, split_damp_tr=1)


def test_step_dot_product():
    from common import Case
    from groups import dot_product_step
    c = Case(nx=12, ny=10, npz=8, n_split=2, k_split=2, nq=2, backend=BACKEND, oracle=False, **STEP)
    lhs, rhs = dot_product_step(c)
    assert abs(lhs - rhs) <= TC.TOL_DOT * abs(lhs), (lhs, rhs)


def test_step_dot_product_six_faces():
    from common import CubeCase
    from groups import cube_dot_product_step
    c = CubeCase(n=16, npz=6, n_split=2, k_split=1, nq=1, backend=BACKEND, **STEP)
    lhs, rhs = cube_dot_product_step(c)
    assert abs(lhs - rhs) <= TC.TOL_DOT * abs(lhs), (lhs, rhs)


def test_step_layout_equals_whole_faces():
    from common import CubeCase
    from layout_checks import check_layout_equals_whole_faces
    check_layout_equals_whole_faces(lambda L: CubeCase(n=16, npz=6, n_split=2, k_split=1, dt=900.0, nq=1, backend=BACKEND, layout=L, **STEP), 2)


def test_step_trajectory_of_step_tl():
    from common import Case
    kw = dict(nx=12, ny=10, npz=8, n_split=2, k_split=2, nq=2, backend=BACKEND, oracle=False)
    TC.check_step_traj(Case(**kw, **STEP), Case(**kw))


def test_off_state():
    from common import Case
    TC.check_off_state(lambda: Case(nx=12, ny=10, npz=8, n_split=2, k_split=2, nq=2, backend=BACKEND))


def test_refusals():
    c = case(nord_tr=1, trdm2=0.15, nord_tr_pert=0, trdm2_pert=0.05, split_damp_tr=1)
    TC.check_refusals(c)


def test_no_tracers_is_accepted():
    from common import Case
    c = Case(nx=8, ny=8, npz=6, n_split=2, nq=0, backend=BACKEND, oracle=False, **STEP)
    assert c.dy.tracer_damping() == ((1, 0.15), (0, 0.0))
    c.put_state(pert=c.pert); c.dy.step_tl()


def test_later_substeps_launch_nothing_extra():
    TC.check_later_substeps_launch_nothing(lambda **kw: case(**kw))
