"""-m "not gpu": BL_DRIVER on the device (fv3lm_turbulence_set_driver; csrc/bldriver.h) in the host-emulation build of the product
sources, against the fixture recorded from the reference's own routine (tests/golden/bl_driver_ref.npz).  Checks: tests/bl_driver_checks.py."""
import pytest
import bl_driver_checks as BC

BACKEND = "emul"
LMS = [72, 127, 20]


def tile(face=None, hydro=1, npz=12, nq=4, **kw):
    """the periodic tile 12 x 10, or one 12 x 12 face of a C12 cube"""
    from common import Case
    nx, ny = (12, 10) if face is None else (12, 12)
    return Case(nx=nx, ny=ny, npz=npz, n_split=2, dt=1800.0, nq=nq, backend=BACKEND, oracle=False, face=face, hydrostatic=hydro, **kw)


def cube(n, npz, layout=1, nq=1):
    from common import CubeCase
    return CubeCase(n=n, npz=npz, n_split=1, k_split=1, dt=900.0, nq=nq, backend=BACKEND, layout=layout)


@pytest.mark.parametrize("lm", LMS)
@pytest.mark.parametrize("face", [None, 2])
def test_against_the_reference(face, lm):
    """check 1: the 13 outputs of every fixture column, relative to the output's column maximum, within the fixture's tolerance (4 x the
    reference's own movement under 1e-15 perturbations of its inputs, floor 1e-12); cloud_mode 1 equals cloud_mode 0 fed the same split
    to 1e-15"""
    BC.check_reference(tile(face, 1, lm), lm)


@pytest.mark.parametrize("lm", LMS)
def test_slot_equals_raw_diagonals_factorised(lm):
    """check 2: fv3lm_turbulence_get after set_driver equals it after set_diagonals fed the call's own raw_out, pk included: bitwise"""
    BC.check_slot_is_raw_factorised(tile(None, 1, lm), lm)


@pytest.mark.parametrize("lm", LMS)
@pytest.mark.parametrize("face", [None, 2])
def test_through_the_solve(face, lm):
    """check 3: fv3lm_turbulence modes 0, 1, 2 after set_driver against the restated solve fed the fixture's diagonals, within 1e-12 + the
    movement of that restated solve under +- the fixture's tolerance; <TL x, y> = <x, AD y> at 1e-12"""
    BC.check_solve(tile(face, 1, lm), lm)


def test_position_independence():
    """check 4: the L72 columns dealt over the six faces of a C96 cube and over its 2 x 2 sub-face layout: every column as on the small
    tile, the 24 tiles gathered as the six faces, bitwise"""
    BC.check_position(lambda: tile(None, 1, 72, 1), lambda L: cube(96, 72, L), 72, 2)


@pytest.mark.parametrize("where", ["tile", "six faces"])
def test_nothing_else_moves(where):
    """check 5: trajectory, perturbation, halos, far edge rows, the other slot and the host's arrays bitwise unchanged; set, step, solve:
    the slot keeps what set saw (the periodic tile, and the six faces of a C12 cube: a step on faces needs all six)"""
    BC.check_nothing_else_moves(tile(None, 1, 20) if where == "tile" else cube(12, 20, 1, 4), 20)


def test_refusals():
    """check 6: every item of the refusal list by its message, the slot left unset; the column whose parcel never stops"""
    BC.check_refusals(lambda nq, npz, **kw: tile(None, 1, npz, nq, **kw))
