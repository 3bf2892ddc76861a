"""CPU (-m "not gpu"): the composed model step (fv3lm_lm_*; csrc/model.h) on the host-emulation build: the trajectory store against the
upload path, the composed tangent and adjoint against their parts in the reference's order, bit for bit, the dot product of the whole
step and of a window of two times, the subsets of the flags, more than one batch of columns, every refusal by its message, and the
Fortran host of fortran/shim_lm_driver.F90 (lm_checks.py).  test_gpu_lm.py and test_gpu_lm_shim.py run them on the MI355X."""
import os
import shutil
import pytest
import lm_checks as LM

BACKEND = "emul"
needs_fortran = pytest.mark.skipif(shutil.which("amdflang") is None, reason="no Fortran compiler")


def make(**kw):
    from common import Case
    return Case(backend=BACKEND, **kw)


def world(**kw):
    return LM.World.get(make, BACKEND, **kw)


CASES = {
    "tile": lambda: make(**LM.tile_kw()),
    "tile, non-hydrostatic": lambda: make(nx=10, ny=8, npz=12, n_split=2, k_split=2, dt=1200.0, nq=2, oracle=False, hydrostatic=0),
    "cube": lambda: __import__("common").CubeCase(n=8, npz=6, n_split=2, k_split=2, nq=2, backend=BACKEND),
    "cube, non-hydrostatic": lambda: __import__("common").CubeCase(n=8, npz=6, n_split=2, k_split=2, nq=2, backend=BACKEND, hydrostatic=0),
}


@pytest.mark.parametrize("where", list(CASES))
def test_a_loaded_slot_equals_the_upload(where):
    """1: save two times, step, load: prognostics with halos, phis and the pressures bit for bit what traj_to_fv3 leaves on a fresh handle"""
    LM.check_load_equals_upload(CASES[where])


def test_the_composed_tangent_equals_its_parts_in_the_reference_order():
    """2: lm_step(s, 1) against traj_to_fv3 ; cfcn = 0 ; step_tl ; convection ; cloud ; turbulence, bitwise; cfcn reads back zero; the
    sequence with turbulence before convection differs by more than 1e-6 of a field's largest value"""
    LM.check_tangent(world(), 0)


def test_the_composed_adjoint_equals_its_parts():
    """3: lm_step(s, 2) against cfcn = 0 ; turbulence ; cloud ; convection ; traj_to_fv3 ; step_ad, bitwise"""
    LM.check_adjoint(world(), 0)


def test_the_whole_step_is_adjoint():
    """4: <L x, y> = <x, L' y> over one lm_step with all three flags"""
    LM.check_dot_product(world(), (0,))


def test_two_times_of_one_window():
    """5: tangent at 0 then 1, adjoint at 1 then 0 through lm_step only: the dot product, and the tangent against uploads and per-part calls"""
    LM.check_window(world())


@pytest.mark.parametrize("flags", [(1, 0, 0), (0, 1, 1)])
def test_a_subset_of_the_flags(flags):
    """6: the dynamics only equals traj_to_fv3 ; step_tl / step_ad; the physics only equals the parts and leaves the resident trajectory"""
    LM.check_subset(make, BACKEND, flags)


def test_more_than_one_batch_of_columns():
    """7: check 2 on 72 x 48 columns: the convection's active columns and the cloud scheme's columns run two batches each, the second partial"""
    LM.check_tangent(world(size=(72, 48)), 0, batches=True)


def test_refusals():
    """8: every refusal of the four calls by its message; the perturbation and cfcn unchanged after each, and the handle still steps"""
    LM.check_refusals(make)


def driver():
    from common import build_emul
    so = build_emul()
    return LM.build_driver(os.path.dirname(so), "fv3lm_emul", os.path.join(os.path.dirname(so), "shim_lm_driver_emul"))


@needs_fortran
def test_the_window_through_the_fortran_host(tmp_path):
    """9: fortran/shim_lm_driver.F90 sets and saves two times and runs the window through fv3lm_hip_lm_step only: bitwise the ctypes caller"""
    LM.run_shim(make, driver(), str(tmp_path))


@needs_fortran
def test_a_refused_step_ends_the_fortran_host(tmp_path):
    """9: a step at a slot never saved: exit status 1, FATAL and the library's message"""
    LM.run_shim_refusal(make, driver(), str(tmp_path))
