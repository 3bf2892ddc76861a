"""-m gpu: the composed model step through the Fortran host (fortran/shim_lm_driver, built by __graft_entry__.build() from
fortran/fv3lm_hip_lm_mod.F90 against libfv3lm_hip.so) on the MI355X: a window of two times through fv3lm_hip_lm_step only, against the
same window through ctypes, bit for bit (lm_checks.py).  The program runs as a fresh child under a time limit; its exit status is
asserted first."""
import os
import pytest
import lm_checks as LM

pytestmark = pytest.mark.gpu
BACKEND = "hip"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make(**kw):
    from common import Case
    return Case(backend=BACKEND, **kw)


def driver():
    drv = os.path.join(ROOT, "fortran", "shim_lm_driver")
    assert os.path.exists(drv), "fortran/shim_lm_driver missing: run __graft_entry__.build()"
    return drv


def test_the_window_through_the_fortran_host_on_the_gpu(tmp_path):
    """9: fortran/shim_lm_driver sets and saves two times and runs the window through fv3lm_hip_lm_step only: bitwise the ctypes caller"""
    LM.run_shim(make, driver(), str(tmp_path))


def test_a_refused_step_ends_the_fortran_host_on_the_gpu(tmp_path):
    """9: a step at a slot never saved: exit status 1, FATAL and the library's message"""
    LM.run_shim_refusal(make, driver(), str(tmp_path))
