"""CPU (-m "not gpu"): the physics and Rayleigh wrappers of the ISO_C_BINDING shim driven by a Fortran program
(fortran/shim_physics_driver.F90) linked against the host-emulation build of the library, against the same calls through ctypes, bit
for bit (physics_shim_checks.py); and, without a compiler, that every public procedure of the module is called by one of the two Fortran
drivers.  test_gpu_physics_shim.py runs the legs against libfv3lm_hip.so on the MI355X."""
import os
import shutil
import pytest
import physics_shim_checks as PS

BACKEND = "emul"
needs_fortran = pytest.mark.skipif(shutil.which("amdflang") is None, reason="no Fortran compiler")


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
    from common import build_emul
    from shim_checks import build_driver
    so = build_emul()
    return build_driver(os.path.dirname(so), "fv3lm_emul", os.path.join(os.path.dirname(so), "shim_physics_driver_emul"), "shim_physics_driver.F90")


def test_every_public_procedure_of_the_shim_is_called_by_a_driver():
    """the public :: list of fortran/fv3lm_hip_mod.F90 against the call statements of the two drivers: all 24 physics and Rayleigh wrappers
    (with their three parameter types, the 27 names of that part of the list) in shim_physics_driver.F90, the rest in shim_driver.F90; a binding added later without a call fails here"""
    procs, physics = PS.check_completeness()
    print("%d public procedures, %d of them physics: %s" % (len(procs), len(physics), " ".join(physics)))


@needs_fortran
@pytest.mark.parametrize("leg", list(PS.LEGS))
def test_physics_through_the_shim(leg, tmp_path):
    """moist: convection and cloud scheme on Fortran slot 2 (set, three gets, tangent chain, adjoint chain, both nonlinear runs);
    boundary layer: set_driver on slot 2, the three solves, set_diagonals and set_simple on slot 1; rayleigh: set_rayleigh, the profile,
    step_tl and step_ad.  Every array the program writes equals the ctypes caller's, bitwise; finite; not zero where the scheme acts"""
    PS.run_physics_shim_check(lambda: case(PS.LEGS[leg]), PS.LEGS[leg], driver(), str(tmp_path))


@needs_fortran
@pytest.mark.parametrize("leg", list(PS.LEGS))
def test_a_refused_physics_call_ends_the_fortran_host(leg, tmp_path):
    """convection / turbulence on a slot that was never set, set_rayleigh with tau < 0: exit status 1, FATAL and the library's message"""
    PS.run_physics_shim_refusal(lambda: case(PS.LEGS[leg]), PS.LEGS[leg], driver(), str(tmp_path))
