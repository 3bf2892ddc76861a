"""MI355X: the fused wind conversion of c_sw (csrc/d2a2c.h) against the staged launches, the four cases of test_emul_wind_fused.py at
rtol 1e-12 of the field maximum (two kernels for one arithmetic, hipcc contracts a*b+c per kernel), and the step_tl / step_ad
dot-product identity on the six faces that run the fused adjoint beside its strips."""
import pytest

pytestmark = pytest.mark.gpu

SWITCHES = ("FV3LM_D2A2C_FUSED",)


@pytest.mark.parametrize("switch", SWITCHES)
def test_fused_winds_equal_staged_periodic(switch):
    from common import Case
    from fused_checks import check_fused_equals_staged
    check_fused_equals_staged("hip/periodic", lambda: Case(nx=70, ny=20, npz=3, n_split=2, k_split=1, dt=900.0, backend="hip", oracle=False, nq=1), switch, rtol=1e-12)


@pytest.mark.parametrize("switch", SWITCHES)
def test_fused_winds_equal_staged_cube(switch):
    from common import CubeCase
    from fused_checks import check_fused_equals_staged
    check_fused_equals_staged("hip/cube", lambda: CubeCase(n=66, npz=2, n_split=1, k_split=1, dt=225.0, backend="hip", nq=1), switch, rtol=1e-12)


@pytest.mark.parametrize("switch", SWITCHES)
def test_fused_winds_equal_staged_nonhydrostatic(switch):
    from common import Case
    from fused_checks import check_fused_equals_staged
    check_fused_equals_staged("hip/nh", lambda: Case(nx=66, ny=18, npz=3, n_split=1, k_split=1, dt=300.0, backend="hip", oracle=False, hydrostatic=0), switch, rtol=1e-12)


@pytest.mark.parametrize("switch", SWITCHES)
def test_fused_winds_equal_staged_subface_windows(switch):
    from common import CubeCase
    from fused_checks import check_fused_equals_staged
    check_fused_equals_staged("hip/windows", lambda: CubeCase(n=136, npz=2, n_split=1, k_split=1, dt=100.0, backend="hip", nq=1, layout=2), switch, rtol=1e-12)


def test_fused_winds_cube_step_dot_product():
    from common import CubeCase
    from groups import cube_dot_product_step
    c = CubeCase(n=66, npz=2, n_split=1, k_split=1, dt=225.0, backend="hip", nq=1)
    lhs, rhs = cube_dot_product_step(c)
    print("step dot product: %.17e %.17e rel %.3e" % (lhs, rhs, abs(lhs - rhs) / abs(lhs)))
    assert abs(lhs - rhs) <= 1e-11 * abs(lhs), (lhs, rhs)
