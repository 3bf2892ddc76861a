"""-m gpu: the physics and Rayleigh wrappers of the ISO_C_BINDING shim driven by a Fortran program (fortran/shim_physics_driver, built
by __graft_entry__.build() against libfv3lm_hip.so) on the MI355X, against the same calls through ctypes, bit for bit
(physics_shim_checks.py).  The program runs once a leg as a fresh child under a time limit; its exit status is asserted first."""
import os
import pytest
import physics_shim_checks as PS

pytestmark = pytest.mark.gpu
BACKEND = "hip"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case(leg):
    """the smallest cases on which the schemes act, all on the periodic 12 x 10 tile"""
    from common import Case
    import cloud_checks as KC
    if leg == PS.MOIST:
        fx = KC.fixture("L40m2")
        return Case(nx=12, ny=10, npz=fx["lm"], n_split=2, dt=1800.0, nq=3, backend=BACKEND, oracle=False, **KC.case_kw(fx))
    if leg == PS.BL:
        return Case(nx=12, ny=10, npz=20, n_split=2, dt=1800.0, nq=4, backend=BACKEND, oracle=False)
    return Case(nx=12, ny=10, npz=8, n_split=2, k_split=1, dt=900.0, nq=2, backend=BACKEND, oracle=False)


def driver():
    drv = os.path.join(ROOT, "fortran", "shim_physics_driver")
    assert os.path.exists(drv), "fortran/shim_physics_driver missing: run __graft_entry__.build()"
    return drv


@pytest.mark.parametrize("leg", list(PS.LEGS))
def test_physics_through_the_shim_on_the_gpu(leg, tmp_path):
    """moist: convection and cloud scheme on Fortran slot 2 (set, three gets, tangent chain, adjoint chain, both nonlinear runs);
    boundary layer: set_driver on slot 2, the three solves, set_diagonals and set_simple on slot 1; rayleigh: set_rayleigh, the profile,
    step_tl and step_ad.  Every array the program writes equals the ctypes caller's, bitwise; finite; not zero where the scheme acts"""
    PS.run_physics_shim_check(lambda: case(PS.LEGS[leg]), PS.LEGS[leg], driver(), str(tmp_path))


def test_a_refused_physics_call_ends_the_fortran_host_on_the_gpu(tmp_path):
    """convection on a slot that was never set: exit status 1, FATAL and the library's message"""
    PS.run_physics_shim_refusal(lambda: case(PS.MOIST), PS.MOIST, driver(), str(tmp_path))
