"""-m gpu: column tests of the vertical remap (fv3lm_remap; remap.h, nh.h) through the C-ABI of the HIP library on an MI355X, against the
numpy restatement tests/remap_oracle.py -- the checks of remap_checks.py at every shape the host-emulation file samples: the linear
profile at npz 2 .. 5, every limited kord 8 .. 15 at each of npz 6, 7, 8, the production sizes and wavefront-width boundaries npz 63, 64,
65, 127, 128, 129 (hydrostatic and non-hydrostatic), stretched L127 levels, extreme thickness ratios, the non-hydrostatic adjoint with and
without the tape, and the remap workspace outside the acoustic arena.  Tolerances and measured maxima: test_emul_remap_column.py."""
import numpy as np
import pytest
from oracle import NL
import remap_checks as RC

pytestmark = pytest.mark.gpu


def _case(npz, nq=1, hydro=1, nx=8, ny=9, **kw):
    from common import Case
    return Case(nx=nx, ny=ny, npz=npz, nq=nq, oracle=False, hydrostatic=hydro, backend="hip", **kw)


@pytest.mark.parametrize("npz", [2, 3, 4, 5])
@pytest.mark.parametrize("kind", ["small", "large", "identity"])
def test_linear_small_npz(npz, kind):
    c = _case(npz, nq=1, nx=8, ny=8)
    S = RC.column_state(c, kind, seed=npz, hard=True)
    for last in (0, 1):
        RC.check_nl_tl(c, S, last)
    RC.check_ad_jacobian(c, S, 1)


@pytest.mark.parametrize("npz", [3, 4, 5])
def test_linear_small_npz_nh(npz):
    c = _case(npz, nq=1, hydro=0, nx=8, ny=8)
    S = RC.column_state(c, "small", seed=npz, hard=True)
    RC.check_nl_tl(c, S, 1)
    RC.check_ad_jacobian(c, S, 0)


@pytest.mark.parametrize("npz", [6, 7, 8])
@pytest.mark.parametrize("kord", [8, 9, 10, 11, 12, 13, 14, 15])
def test_limited(kord, npz):
    c = _case(npz, nq=2, nx=10, ny=8, kord_tm=-kord, kord_tr=kord, kord_mt=kord)
    S = RC.column_state(c, "small" if (kord + npz) % 2 else "large", seed=kord, hard=True)
    for last in (0, 1):
        RC.check_nl_tl(c, S, last)
    RC.check_ad_jacobian(c, S, 0)


@pytest.mark.parametrize("kord", [8, 10, 11, 13, 15])
def test_limited_nh(kord):
    c = _case(8, nq=1, hydro=0, kord_tm=-kord, kord_tr=kord, kord_mt=kord, kord_wz=kord)
    S = RC.column_state(c, "small", seed=kord, hard=True)
    RC.check_nl_tl(c, S, 1)
    RC.check_ad_dot(c, S, 1)


@pytest.mark.parametrize("kord", [8, 9, 10, 11, 12, 13, 14, 15])
def test_limited_tracers_stay_nonnegative(kord):
    c = _case(8, nq=2, kord_tr=kord)
    RC.check_nonnegative(c, RC.column_state(c, "large", seed=kord))


@pytest.mark.parametrize("hydro", [1, 0])
@pytest.mark.parametrize("npz", [63, 64, 65, 127, 128, 129])
def test_large_npz(npz, hydro):
    c = _case(npz, nq=1, hydro=hydro, nx=8 + npz % 5, ny=8)
    S = RC.column_state(c, "large" if hydro else "small", seed=npz, hard=True)
    RC.check_nl_tl(c, S, npz % 2, conditioned=True)
    RC.check_ad_dot(c, S, 1 - npz % 2)


@pytest.mark.parametrize("kind", ["small", "large", "identity"])
def test_stretched_l127(kind):
    c = _case(127, nq=2, nx=12, ny=10, levels=RC.stretched_levels(127))
    S = RC.column_state(c, kind, seed=3, hard=True)
    RC.check_nl_tl(c, S, 1, conditioned=True)
    RC.check_ad_dot(c, S, 0)


@pytest.mark.parametrize("npz", [8, 64, 128])
def test_thickness_ratios(npz):
    c = _case(npz, nq=1, nx=8, ny=8)
    S = RC.column_state(c, "ratio", seed=npz)
    RC.check_nl_tl(c, S, 0, conditioned=True)
    RC.check_ad_dot(c, S, 0, tol=1e-10)


@pytest.mark.parametrize("tape", ["0", "1"])
def test_nh_adjoint(tape, monkeypatch):
    monkeypatch.setenv("FV3LM_NH_TAPE", tape)
    c = _case(7, nq=2, hydro=0, nx=9, ny=8)
    S = RC.column_state(c, "small", seed=11, hard=True)
    RC.check_ad_jacobian(c, S, 1)
    RC.check_ad_jacobian(c, S, 0)


def test_remap_workspace_outside_the_arena(capfd, monkeypatch):
    monkeypatch.setenv("FV3LM_VERBOSE", "1")
    c = _case(8, nq=3, nx=8, ny=8)
    err = capfd.readouterr().err
    assert "remap workspace" in err and "own allocation" in err, err
    S = RC.column_state(c, "large", seed=4, hard=True)
    RC.check_nl_tl(c, S, 1)
    RC.check_ad_jacobian(c, S, 1)


@pytest.mark.parametrize("hydro", [1, 0])
def test_properties(hydro):
    c = _case(64, nq=2, hydro=hydro, nx=10, ny=10)
    for kind in ("large", "small"):
        S = RC.column_state(c, kind, seed=9)
        RC.check_conservation(c, S)
        RC.check_constant(c, S)
    RC.check_identity(c, RC.column_state(c, "identity", seed=2, hard=True))


def test_nh_remap_maps_w_and_delz():
    c = _case(8, nq=1, hydro=0)
    S = RC.column_state(c, "small", seed=6)
    got = RC.product(c, NL, 0, S)
    R = RC.RO.Remap(c, 0)
    for n in ("w", "delz"):
        assert np.max(np.abs(RC.on_rect(R, n, got[n]) - RC.on_rect(R, n, S[n]))) > 1e-3 * np.max(np.abs(S[n]))
