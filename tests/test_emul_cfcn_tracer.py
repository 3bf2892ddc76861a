"""CPU (-m "not gpu"): the convective cloud fraction as a tracer of the dycore (fv3lm_cloud_bind_cfcn) on the host-emulation build:
the bound composed step against the parts routed through the host, bit for bit, the coupling it adds, its dot product, the trajectory
side, the refusals and the six faces (cfcn_tracer_checks.py).  test_gpu_cfcn_tracer.py runs them on the MI355X."""
import pytest
import cfcn_tracer_checks as CT

BACKEND = "emul"


def tile(**kw):
    from common import Case
    return Case(backend=BACKEND, **CT.tile_kw(**kw))


def cube():
    from common import CubeCase
    return CubeCase(backend=BACKEND, **CT.cube_kw())


def world(where="tile"):
    if where == "tile, non-hydrostatic":
        return CT.World.get(lambda: tile(hydrostatic=0), (BACKEND, where), parts=False)
    return CT.World.get(cube if where == "cube" else tile, (BACKEND, where))


@pytest.mark.parametrize("mode", [CT.TL, CT.AD])
@pytest.mark.parametrize("slot", [0, 1])
def test_the_bound_composed_step_equals_the_parts_through_the_host(slot, mode):
    """1: lm_step on a bound handle against a handle that never binds and moves cfcn between tracer 4 and fv3lm_cloud_cfcn by hand, in
    the reference's order, bit for bit; tracer 4 and fv3lm_cloud_cfcn read back zero after the step"""
    CT.check_composed_equals_host(world(), slot, mode)


def test_the_state_lets_cfcn_act():
    """2, the condition, from the unbound parts alone: step_tl turns a zero cfcn' into a non-zero one, and the cloud tangent given only
    that cfcn' moves T' or qv' in at least four columns (the L40m2 fixture meets it)"""
    CT.check_condition(world())


@pytest.mark.parametrize("mode", [CT.TL, CT.AD])
def test_the_coupling_is_there(mode):
    """2: the bound composed tangent differs from the unbound one in T qv qi ql, the adjoint in u v delp, by a tenth of what the host
    emulation measured"""
    CT.check_coupling(world(), mode)


@pytest.mark.parametrize("where", ["tile", "tile, non-hydrostatic"])
def test_the_bound_step_is_adjoint(where):
    """3: <L x, y> = <x, L' y> of the bound composed step over u v T delp q1..q3 (w delz), the draw, residual and bound of lm_checks"""
    CT.check_dot_product(world(where))


def test_a_window_of_two_times_is_adjoint():
    """3: tangent at 0 then 1, adjoint at 1 then 0"""
    CT.check_dot_product(world(), (0, 1))


def test_the_trajectory_side():
    """4: cloud_set with cfcn = NULL equals the array passed; mode 0 writes CF_con to the trajectory of tracer 4 inside is..ie x js..je
    only, and unbound leaves it alone; fv3lm_cloud_cfcn moves the tracer's perturbation"""
    CT.check_trajectory_side(tile)


@pytest.mark.parametrize("mode", [CT.TL, CT.AD])
def test_six_faces_equal_the_parts_through_the_host(mode):
    """6: check 1 on CubeCase(n = 8): the tile index of the padded planes"""
    CT.check_composed_equals_host(world("cube"), 0, mode)


def test_six_faces_are_adjoint():
    """6: check 3 on CubeCase(n = 8)"""
    CT.check_dot_product(world("cube"))


def test_refusals():
    """5: every refusal of fv3lm_cloud_bind_cfcn by its message; the perturbation unchanged after each, and the handle still steps"""
    CT.check_refusals(tile)
