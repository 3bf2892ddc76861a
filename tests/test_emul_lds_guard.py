"""CPU (-m "not gpu"): the LDS guard of the host emulation (csrc/tiled.h run_tiled).  Every LDS-tiled launch runs there over a buffer of
exactly the bytes its block descriptor declares, with guard words behind it that are checked after the launch; a block that wrote past
its declared LDS fails the call through the library's status.  With every switch at its default the three sweeps run every tiled
kernel of the step (fv_tp_2d nonlinear, tangent and adjoint, a2b_ord4, d2a2c_vect): each call must return 0 and leave no error (the last error stays what it was before the sweeps: empty when the test runs alone).  The
guard's message names the launch and "LDS".  No GPU test: the guard does not exist in the device build."""
from common import Case, CubeCase
from fused_checks import SWITCHES, _names_and_state


def _sweeps_are_clean(c):
    L, h = c.dy.lib.L, c.dy.h
    names, T, P = _names_and_state(c)
    for n in names:
        c.dy.put(n, T[n], 0); c.dy.put(n, P[n], 1)
    before = c.dy.lib.err()      # the library writes its last error only when a call fails: empty in a fresh process, else an earlier test's refusal
    for call in (L.fv3lm_step_tl, L.fv3lm_step_nl, L.fv3lm_step_ad):
        assert call(h) == 0, c.dy.lib.err()
        assert c.dy.lib.err() == before and "LDS" not in before
    assert c.dy.launch_count() > 0


def test_lds_guard_silent_periodic_tile(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    _sweeps_are_clean(Case(nx=70, ny=20, npz=3, n_split=2, k_split=1, dt=900.0, backend="emul", oracle=False, nq=1))


def test_lds_guard_silent_cube_faces(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    _sweeps_are_clean(CubeCase(n=66, npz=2, n_split=1, k_split=1, dt=225.0, backend="emul", nq=1))
