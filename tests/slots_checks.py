"""Checks of the trajectory saves of the backward sweep, shared by the host-emulation (test_emul_slots.py) and the MI355X
(test_gpu_slots.py) runs.

Capped slots: FV3LM_TRAJ_SLOTS, read when the case is created, caps the number of acoustic steps whose intermediates the forward sweep
keeps.  A step without a slot is restored from its checkpoint and recomputed by the backward sweep, so the whole step is checked with no
slot, with one, and with one per acoustic step: fv_dynamics' adjoint against the oracle and the dot-product identity of step_tl / step_ad,
at the tolerances the suite applies to the same checks without a cap (1e-10 / 1e-12 hydrostatic, nh_checks' 1e-11 non-hydrostatic).
Measured on an MI355X, hydrostatic case, the same with 0, 1 and 6 slots: adjoint relative error 1.2e-14, dot-product residual 8.0e-15;
the non-hydrostatic cases pass nh_checks' asserts; each case takes 0.2 - 0.3 s there.

Snapshot: fv3lm_state_save / fv3lm_state_restore bring back every prognostic field, trajectory and perturbation, bit for bit."""
import numpy as np
import pytest
from common import Case
from oracle import AD

HYDRO = dict(nx=12, ny=10, npz=10, n_split=3, k_split=2, dt=1800.0, nq=3)
NONHYDRO = dict(nx=10, ny=8, npz=12, n_split=2, k_split=2, dt=1200.0, nq=2, hydrostatic=0)
HYDRO_SLOTS = (0, 1, 6)
NONHYDRO_SLOTS = (0, 1, 4)


def capped_case(monkeypatch, backend, slots, **kw):
    monkeypatch.setenv("FV3LM_TRAJ_SLOTS", str(slots))
    c = Case(backend=backend, **kw)
    assert c.dy.lib.L.fv3lm_traj_slots(c.dy.h) == slots
    return c


def check_capped_hydrostatic(monkeypatch, backend, slots):
    from groups import check_fv_dynamics, dot_product_step
    c = capped_case(monkeypatch, backend, slots, **HYDRO)
    e = check_fv_dynamics(c, AD, 1e-10)
    lhs, rhs = dot_product_step(c)
    print("slots %d (%s): fv_dynamics AD rel err %.3e, step dot-product residual %.3e" % (slots, backend, e, abs(lhs - rhs) / abs(lhs)))
    assert abs(lhs - rhs) <= 1e-12 * abs(lhs), (lhs, rhs)


def check_capped_nonhydrostatic(monkeypatch, backend, slots):
    import nh_checks as N
    c = capped_case(monkeypatch, backend, slots, **NONHYDRO)
    N.check_nh_fv_adjoint(c)
    N.check_nh_fv_dot_product(c)


def check_snapshot(backend, hydrostatic):
    from fv3_jedi_linearmodel_amd._lib import Fv3LmError
    c = Case(backend=backend, **dict(NONHYDRO, hydrostatic=hydrostatic))
    with pytest.raises(Fv3LmError):
        c.dy.state_restore()        # no snapshot yet
    names = ["u", "v", "pt", "delp"] + ["q%d" % (n + 1) for n in range(c.nq)] + ([] if hydrostatic else ["w", "delz"])
    if hydrostatic:
        from groups import step_state
        T, P = step_state(c)
    else:
        from test_oracle_nh import nh_state_fv
        import nh_checks as N
        T, P = (dict(zip(N.fv_names(c), x)) for x in nh_state_fv(c))
    for n in names:
        c.dy.put(n, T[n][None], 0); c.dy.put(n, P[n][None], 1)
    saved = {(n, w): c.dy.get(n, w).copy() for n in names for w in (0, 1)}
    c.dy.state_save()
    c.dy.step_tl()
    assert any(not np.array_equal(c.dy.get(n, w), saved[n, w]) for n, w in saved)
    c.dy.state_restore()
    for (n, w), a in saved.items():
        assert np.array_equal(c.dy.get(n, w), a), (n, "pert" if w else "traj")
