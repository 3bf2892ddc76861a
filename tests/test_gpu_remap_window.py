"""-m gpu: the vertical remap with the source window (csrc/remap.h) on an MI355X, on the states of test_emul_remap_window.py: every column
draws its own warp, so the lanes of a wavefront move their windows by 0 to 8 and more layers per target, and the columns with tied
interfaces.  npz 12 and 20, hydrostatic, one non-hydrostatic case and one with a limited trajectory profile (kord 9); against the numpy
restatement with remap_checks' own tolerances (NL / TL 1e-12, adjoint dot products 1e-11), both values of last.  No goldens here: hipcc
contracts a * b + c and g++ -O2 does not."""
import pytest
import test_emul_remap_window as W

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", list(W.CASES))
def test_against_the_restatement(name):
    c = W.make_case(name, backend="hip")
    W.run_checks(c, W.make_state(c, name))
