"""-m "not gpu": the launches every call of the column physics makes, in the host-emulation build of the product sources, against the
table recorded before the host side moved to csrc/physics.h.  Checks: tests/physics_launch_checks.py."""
import pytest
import cloud_checks as KC
import physics_launch_checks as LC

BACKEND = "emul"


def tile(npz, nq, size=(12, 10), **kw):
    from common import Case
    return Case(nx=size[0], ny=size[1], npz=npz, n_split=2, dt=1800.0, nq=nq, backend=BACKEND, oracle=False, **kw)


def test_turbulence():
    """set_diagonals, get, the three modes and set_simple on the 12 x 10 x L12 tile"""
    c = tile(12, 4)
    LC.check("turbulence", c, LC.turbulence_calls(c))


def test_bl_driver():
    """set_driver with and without raw_out on the L20 fixture of BL_DRIVER"""
    c = tile(20, 4)
    LC.check("bl_driver", c, LC.bl_driver_calls(c))


@pytest.mark.parametrize("case,size", [("moist", (12, 10)), ("moist 64 x 40", (64, 40))])
def test_convection_and_cloud(case, size):
    """create, set, get, sources, table, cfcn and the three modes of both schemes: 120 columns (one batch) and 2,560 (two batches, the
    second partial)"""
    fx = KC.fixture(LC.TAG)
    c = tile(fx["lm"], 3, size, **KC.case_kw(fx))
    LC.check(case, c, LC.moist_calls(c))
