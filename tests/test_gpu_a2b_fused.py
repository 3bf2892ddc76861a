"""MI355X: the fused a2b_ord4 launch (csrc/a2b.h) against the staged launches (FV3LM_A2B_FUSED=0), the four cases of
test_emul_a2b_fused.py at rtol 1e-12 of the field maximum (two kernels for one arithmetic, hipcc contracts a*b+c per kernel), and the
step_tl / step_ad dot-product identity on the six faces that run the fused adjoint with its rim."""
import pytest

pytestmark = pytest.mark.gpu


def test_fused_a2b_equals_staged_periodic():
    from common import Case
    from fused_checks import check_fused_equals_staged
    check_fused_equals_staged("hip/periodic", lambda: Case(nx=70, ny=20, npz=3, n_split=2, k_split=1, dt=900.0, backend="hip", oracle=False, nq=1), "FV3LM_A2B_FUSED", rtol=1e-12)


def test_fused_a2b_equals_staged_cube():
    from common import CubeCase
    from fused_checks import check_fused_equals_staged
    check_fused_equals_staged("hip/cube", lambda: CubeCase(n=66, npz=2, n_split=1, k_split=1, dt=225.0, backend="hip", nq=1), "FV3LM_A2B_FUSED", rtol=1e-12)


def test_fused_a2b_equals_staged_nonhydrostatic():
    from common import Case
    from fused_checks import check_fused_equals_staged
    check_fused_equals_staged("hip/nh", lambda: Case(nx=66, ny=18, npz=3, n_split=1, k_split=1, dt=300.0, backend="hip", oracle=False, hydrostatic=0), "FV3LM_A2B_FUSED", rtol=1e-12)


def test_fused_a2b_equals_staged_subface_windows():
    from common import CubeCase
    from fused_checks import check_fused_equals_staged
    check_fused_equals_staged("hip/windows", lambda: CubeCase(n=136, npz=2, n_split=1, k_split=1, dt=100.0, backend="hip", nq=1, layout=2), "FV3LM_A2B_FUSED", rtol=1e-12)


def test_fused_a2b_cube_step_dot_product():
    from common import CubeCase
    from groups import cube_dot_product_step
    c = CubeCase(n=66, npz=2, n_split=1, k_split=1, dt=225.0, backend="hip", nq=1)
    lhs, rhs = cube_dot_product_step(c)
    assert abs(lhs - rhs) <= 1e-11 * abs(lhs), (lhs, rhs)
