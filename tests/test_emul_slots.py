"""CPU (-m "not gpu") runs of slots_checks.py on the host-emulation build, and the sizes of the checkpoint sets: what the library
reports under FV3LM_VERBOSE when a case is created against the closed forms of the layouts."""
import re
import pytest
import slots_checks as S
from common import Case, CubeCase


@pytest.mark.parametrize("slots", S.HYDRO_SLOTS)
def test_emul_capped_slots_hydrostatic(slots, monkeypatch):
    S.check_capped_hydrostatic(monkeypatch, "emul", slots)


@pytest.mark.parametrize("slots", S.NONHYDRO_SLOTS)
def test_emul_capped_slots_nonhydrostatic(slots, monkeypatch):
    S.check_capped_nonhydrostatic(monkeypatch, "emul", slots)


@pytest.mark.parametrize("hydrostatic", [1, 0])
def test_emul_state_snapshot(hydrostatic):
    S.check_snapshot("emul", hydrostatic)


@pytest.mark.parametrize("make", [lambda: Case(oracle=False, **S.HYDRO), lambda: Case(oracle=False, **S.NONHYDRO),
                                  lambda: CubeCase(n=8, npz=6, n_split=2, k_split=2, nq=2, hydrostatic=0)],
                         ids=["hydrostatic", "nonhydrostatic", "nonhydrostatic-six-faces"])
def test_checkpoint_memory(make, monkeypatch, capfd):
    """bytes per set at create: acoustic n_split*k_split*S, S = 4 n3 (non-hydrostatic 6 n3 + n3p); per k_split step (2 nq + 7) n3 + 3 n3p
    (non-hydrostatic + 3 n3 + P); entry 2 n3; 3 n3p + n3 per trajectory slot; nothing for the sub-steps and the snapshot until they are used"""
    monkeypatch.setenv("FV3LM_VERBOSE", "1")
    monkeypatch.setenv("FV3LM_TRAJ_SLOTS", "3")
    capfd.readouterr()
    c = make()
    err = capfd.readouterr().err
    sets = {m.group(1): (int(m.group(2)), int(m.group(3))) for m in re.finditer(r"fv3lm: checkpoint set (.+): (\d+) records, (\d+) bytes", err)}
    ntile, npz, ny, nx = c.dy.shape("delp")
    P = ntile * ny * nx
    n3, n3p, nq, nh = P * npz, P * (npz + 1), c.nq, not c.opt.hydrostatic
    n_split, k_split = c.dims.n_split, c.dims.k_split
    assert sorted(sets) == ["acoustic", "entry", "remap", "slot pressures", "tracer"], err
    assert sets["acoustic"] == (n_split * k_split, n_split * k_split * (6 * n3 + n3p if nh else 4 * n3) * 8)
    assert sets["tracer"][0] == sets["remap"][0] == k_split
    assert sets["tracer"][1] + sets["remap"][1] == k_split * ((2 * nq + 7) * n3 + 3 * n3p + (3 * n3 + P if nh else 0)) * 8
    assert sets["entry"] == (1, 2 * n3 * 8)
    assert sets["slot pressures"] == (3, 3 * (3 * n3p + n3) * 8)
    assert c.dy.lib.L.fv3lm_traj_slots(c.dy.h) == 3
