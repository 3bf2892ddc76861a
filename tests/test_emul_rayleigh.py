"""CPU (-m "not gpu") tests of the Rayleigh damping of the upper layers (fv3lm_set_rayleigh; RAYLEIGH_SUPER, fv_dynamics_tlm.F90:1749-1899)
on the host-emulation build of the product, against the numpy restatement tests/rayleigh_oracle.py and, for its place in the step, the
oracle's fv_dynamics composed with it (rayleigh_checks.py)."""
import numpy as np
import pytest
from common import Case, CubeCase
from oracle import TL, AD
from fv3_jedi_linearmodel_amd._lib import Fv3LmError
import rayleigh_checks as RC

# dt = 1800 s: tau of a fraction of a day gives rf(1) ~ 0.1 .. 0.5, a damping the checks can see
PAIRS = [(0.2, 1.0e4), (0.5, 3.0e4)]         # kmax 2 and 4 of the 8 levels of the cases below (pm = 438, 6576, 15318, 26439, 39645 .. Pa)


@pytest.mark.parametrize("tau,cutoff", PAIRS)
def test_profile(tau, cutoff):
    c = Case(nx=8, ny=8, npz=8, n_split=2, oracle=False, tau=tau, rf_cutoff=cutoff)
    assert RC.check_profile(c) == {1.0e4: 2, 3.0e4: 4}[cutoff]


@pytest.mark.parametrize("hydro", [1, 0])
@pytest.mark.parametrize("face", [None, 2])
def test_unit(face, hydro):
    c = Case(nx=8, ny=8, npz=8, n_split=2, oracle=False, face=face, hydrostatic=hydro, tau=0.3, rf_cutoff=3.0e4)
    RC.check_unit(c)


@pytest.fixture(scope="module")
def hcase():
    return Case(nx=12, ny=10, npz=8, n_split=2, k_split=2, dt=1800.0, nq=2, tau=0.3, rf_cutoff=3.0e4)


@pytest.mark.parametrize("mode", [TL, AD])
def test_fv_dynamics_composition(hcase, mode):
    RC.check_composition(hcase, mode, 1e-10)


def test_fv_dynamics_composition_cube():
    c = CubeCase(n=8, npz=6, n_split=2, k_split=2, nq=1, oracle=True, tau=0.3, rf_cutoff=3.0e4)
    RC.check_composition(c, TL, 1e-10)
    RC.check_composition(c, AD, 1e-10)


def test_hydrostatic_step_dot_product(hcase):
    from groups import dot_product_step
    lhs, rhs = dot_product_step(hcase)
    assert abs(lhs - rhs) <= 1e-11 * abs(lhs), (lhs, rhs)


@pytest.fixture(scope="module")
def nhcase():
    return Case(nx=10, ny=8, npz=8, n_split=2, k_split=2, dt=1200.0, nq=2, hydrostatic=0, tau=0.2, rf_cutoff=3.0e4, oracle=False)


def test_nh_step_dot_product(nhcase):
    from nh_checks import check_nh_fv_dot_product
    check_nh_fv_dot_product(nhcase, tol=1e-11)


def test_nh_step_taylor():
    c = Case(nx=10, ny=8, npz=8, n_split=2, dt=600.0, hydrostatic=0, tau=0.1, rf_cutoff=3.0e4, oracle=False, do_vort_damp=0, do_vort_damp_pert=0)
    RC.check_nh_taylor(c)


def test_nh_pkz_from_temperature_before_heating():
    kw = dict(nx=8, ny=8, npz=4, n_split=2, dt=600.0, hydrostatic=0, oracle=False)
    RC.check_nh_pkz_before_heating(Case(tau=0.2, rf_cutoff=1.5e4, **kw), Case(**kw))


def _run(c):
    """step_tl, then step_nl + step_ad, on the case's state: every output of both"""
    from fv3_jedi_linearmodel_amd.harness import step_state
    T, P = step_state(c)
    names = ["u", "v", "pt", "delp"] + ["q%d" % (n + 1) for n in range(c.nq)]
    for n in names:
        c.dy.put(n, T[n][None], 0); c.dy.put(n, P[n][None], 1)
    c.dy.step_tl()
    out = [c.dy.get(n, w) for n in names for w in (0, 1)]
    for n in names:
        c.dy.put(n, T[n][None], 0)
    c.dy.step_nl()
    rng = np.random.default_rng(3)
    for n in names:
        c.dy.put(n, rng.standard_normal(c.dy.shape(n)), 1)
    c.dy.step_ad()
    return out + [c.dy.get(n, 1) for n in names]


def test_tau_zero_is_bit_identical():
    kw = dict(nx=8, ny=8, npz=8, n_split=2, k_split=2, nq=1, oracle=False)
    a = _run(Case(**kw))
    c = Case(**kw)
    c.dy.set_rayleigh(0.3, 3.0e4, c.c2l)
    c.dy.set_rayleigh(0.0, 0.0, None)
    assert c.dy.rayleigh_profile()[1] == 0
    b = _run(c)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_refusals():
    c = Case(nx=8, ny=8, npz=8, n_split=2, oracle=False)
    with pytest.raises(Fv3LmError, match="tau < 0"):
        c.dy.set_rayleigh(-1.0, 3.0e4, c.c2l)
    with pytest.raises(Fv3LmError, match="tau and rf_cutoff must be finite"):
        c.dy.set_rayleigh(float("nan"), 3.0e4, c.c2l)
    with pytest.raises(Fv3LmError, match="tau and rf_cutoff must be finite"):
        c.dy.set_rayleigh(1.0, float("inf"), c.c2l)
    with pytest.raises(Fv3LmError, match="rf_cutoff > ptop"):
        c.dy.set_rayleigh(1.0, c.opt.ptop, c.c2l)
    with pytest.raises(Fv3LmError, match="c2l is null"):
        c.dy.set_rayleigh(1.0, 3.0e4, None)
    assert c.dy.rayleigh_profile()[1] == 0        # a refused call leaves the damping off


def test_layout_equals_whole_faces():
    from layout_checks import check_layout_equals_whole_faces
    check_layout_equals_whole_faces(lambda L: CubeCase(n=16, npz=6, n_split=2, k_split=1, dt=900.0, nq=1, layout=L, tau=0.2, rf_cutoff=3.0e4), 2)
