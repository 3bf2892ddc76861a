"""slots_checks.py through the C-ABI of the HIP library on an MI355X: the whole step with the trajectory slots capped (the restore
from the checkpoint and the recompute of the backward sweep, which no other device test reaches: every case of the suite is small
enough for a slot per acoustic step) and the device snapshot of the prognostic state."""
import pytest
import slots_checks as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("slots", S.HYDRO_SLOTS)
def test_capped_slots_hydrostatic(slots, monkeypatch):
    S.check_capped_hydrostatic(monkeypatch, "hip", slots)


@pytest.mark.parametrize("slots", S.NONHYDRO_SLOTS)
def test_capped_slots_nonhydrostatic(slots, monkeypatch):
    S.check_capped_nonhydrostatic(monkeypatch, "hip", slots)


@pytest.mark.parametrize("hydrostatic", [1, 0])
def test_state_snapshot(hydrostatic):
    S.check_snapshot("hip", hydrostatic)
