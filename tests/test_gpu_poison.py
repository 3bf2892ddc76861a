"""-m gpu: the poison runs of poison_checks.py (metric entries the reference leaves undefined set to 1e30 / -3e33: no defined output may
move by a bit) through the C-ABI of the HIP library, on one C8 face and on six C8 faces."""
import pytest
import poison_checks as PC

pytestmark = pytest.mark.gpu


def test_face_ignores_poisoned_metric_entries():
    assert PC.check_face("hip") > 0


def test_cube_ignores_poisoned_metric_entries():
    assert PC.check_cube("hip") > 0
