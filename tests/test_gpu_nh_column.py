"""The non-hydrostatic column operators (csrc/nh.h, nh_ad.h), column by column, through the C-ABI of the HIP library on an MI355X against the numpy
restatement tests/nh_column_oracle.py (checks, columns and tolerances in nh_column_checks.py, shared with test_emul_nh_column.py)."""
import pytest
import nh_column_checks as K

pytestmark = pytest.mark.gpu

NPZ = [3, 4, 8, 64, 65, 127, 129]
BACKEND = "hip"
# the whole cross product (solver setting x p_fac) up to 8 levels; deeper, every level count runs the three settings and p_fac alternates with
# level count and setting
CASES = [(n, s, p) for n in NPZ for i, s in enumerate(K.SETTINGS) for j, p in enumerate(K.P_FACS) if n <= 8 or (NPZ.index(n) + i) % 2 == j]


def _case(npz, setting, p_fac):
    from common import Case
    return Case(**K.case_kwargs(npz, setting, p_fac, BACKEND))


@pytest.mark.parametrize("npz,setting,p_fac", CASES)
def test_solvers(npz, setting, p_fac, monkeypatch):
    """values, tangent and the hand-written adjoint (csrc/nh_ad.h), then the taped adjoint of the generic column code (FV3LM_NH_TAPE=1, read when
    the handle is created) against the same references; a tape overflow surfaces as the library's error"""
    tag = "%s L%d %s p_fac %.2f" % (BACKEND, npz, setting, p_fac)
    monkeypatch.delenv("FV3LM_NH_TAPE", raising=False)
    K.run_solvers(_case(npz, setting, p_fac), tag + " hand", ("values", "adjoint"))
    monkeypatch.setenv("FV3LM_NH_TAPE", "1")
    K.run_solvers(_case(npz, setting, p_fac), tag + " tape", ("adjoint",))


@pytest.mark.parametrize("npz", NPZ)
def test_edge_profile_and_rings(npz, monkeypatch):
    monkeypatch.delenv("FV3LM_NH_TAPE", raising=False)
    K.run_small(_case(npz, "sim075", 0.05), "%s L%d" % (BACKEND, npz))
