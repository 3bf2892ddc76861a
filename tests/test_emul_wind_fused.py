"""CPU (-m "not gpu"): the fused wind conversion of c_sw in the host-emulation build (csrc/d2a2c.h) against the staged launches
(fused_checks.py): step_tl bit for bit, step_ad to 1e-13.  The emulation checks every stage's reads against its declared stencil
box on the way (common.py).  The same cases run on the MI355X in test_gpu_wind_fused.py."""
import pytest
from common import Case, CubeCase
from fused_checks import check_fused_equals_staged

SWITCHES = ("FV3LM_D2A2C_FUSED",)


@pytest.mark.parametrize("switch", SWITCHES)
def test_fused_winds_periodic_tile_many_blocks(switch):
    # 70 x 20 cells: 2 x 2 blocks, a thin last block column and a second block row
    check_fused_equals_staged("emul/periodic", lambda: Case(nx=70, ny=20, npz=3, n_split=2, k_split=1, dt=900.0, backend="emul", oracle=False, nq=1), switch)


@pytest.mark.parametrize("switch", SWITCHES)
def test_fused_winds_cube_faces_bands_strips_corners(switch):
    # six C66 faces: bands, strips and corners beside a bulk of 2 x 5 blocks
    check_fused_equals_staged("emul/cube", lambda: CubeCase(n=66, npz=2, n_split=1, k_split=1, dt=225.0, backend="emul", nq=1), switch)


@pytest.mark.parametrize("switch", SWITCHES)
def test_fused_winds_nonhydrostatic(switch):
    # the non-hydrostatic program runs the same stages
    check_fused_equals_staged("emul/nh", lambda: Case(nx=66, ny=18, npz=3, n_split=1, k_split=1, dt=300.0, backend="emul", oracle=False, hydrostatic=0), switch)


@pytest.mark.parametrize("switch", SWITCHES)
def test_fused_winds_subface_windows(switch):
    # six C136 faces cut 2 x 2: 68-wide windows, each with one cube corner, two cube edges and two interior boundaries
    check_fused_equals_staged("emul/windows", lambda: CubeCase(n=136, npz=2, n_split=1, k_split=1, dt=100.0, backend="emul", nq=1, layout=2), switch)
