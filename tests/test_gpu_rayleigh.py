"""-m gpu: the Rayleigh damping of the upper layers (fv3lm_set_rayleigh; RAYLEIGH_SUPER, fv_dynamics_tlm.F90:1749-1899) through the
C-ABI of the HIP library on an MI355X: the profile, the unit alone in the three modes (periodic tile, one face; hydrostatic and
non-hydrostatic), its place in fv_dynamics against the oracle composed with the numpy restatement (periodic tile, six faces at C24L16),
sub-face tiles against whole faces, and the non-hydrostatic step (dot product on one tile and six faces, finite differences, pkz)."""
import pytest
from oracle import TL, AD
import rayleigh_checks as RC

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("tau,cutoff", [(0.2, 1.0e4), (0.5, 3.0e4)])
def test_profile(tau, cutoff):
    from common import Case
    c = Case(nx=8, ny=8, npz=8, n_split=2, backend="hip", oracle=False, tau=tau, rf_cutoff=cutoff)
    assert RC.check_profile(c) == {1.0e4: 2, 3.0e4: 4}[cutoff]


@pytest.mark.parametrize("hydro", [1, 0])
@pytest.mark.parametrize("face", [None, 2])
def test_unit(face, hydro):
    from common import Case
    c = Case(nx=8, ny=8, npz=8, n_split=2, backend="hip", oracle=False, face=face, hydrostatic=hydro, tau=0.3, rf_cutoff=3.0e4)
    RC.check_unit(c)


@pytest.mark.parametrize("mode", [TL, AD])
def test_fv_dynamics_composition(mode):
    from common import Case
    c = Case(nx=12, ny=10, npz=8, n_split=2, k_split=2, dt=1800.0, nq=2, backend="hip", tau=0.3, rf_cutoff=3.0e4)
    RC.check_composition(c, mode, 1e-10)


@pytest.fixture(scope="module")
def cube24():
    from common import CubeCase
    return CubeCase(n=24, npz=16, n_split=2, k_split=2, dt=900.0, nq=1, backend="hip", oracle=True, tau=0.3, rf_cutoff=2.0e4)


@pytest.mark.parametrize("mode", [TL, AD])
def test_six_faces_composition_c24l16(cube24, mode):
    RC.check_composition(cube24, mode, 1e-10)


def test_six_faces_step_dot_product_c24l16(cube24):
    from groups import cube_dot_product_step
    lhs, rhs = cube_dot_product_step(cube24)
    assert abs(lhs - rhs) <= 1e-11 * abs(lhs), (lhs, rhs)


def test_layout_equals_whole_faces():
    from common import CubeCase
    from layout_checks import check_layout_equals_whole_faces
    check_layout_equals_whole_faces(lambda L: CubeCase(n=32, npz=8, n_split=2, k_split=2, dt=600.0, backend="hip", nq=1, layout=L,
                                                       tau=0.2, rf_cutoff=3.0e4), 2)


def test_layout_equals_whole_faces_nonhydrostatic():
    from common import CubeCase
    from layout_checks import check_layout_equals_whole_faces
    check_layout_equals_whole_faces(lambda L: CubeCase(n=32, npz=8, n_split=2, k_split=1, dt=150.0, backend="hip", nq=1, layout=L,
                                                       hydrostatic=0, tau=0.2, rf_cutoff=3.0e4), 2, tol=1e-11)


def test_nh_step_dot_product():
    from common import Case
    from nh_checks import check_nh_fv_dot_product
    c = Case(nx=10, ny=8, npz=8, n_split=2, k_split=2, dt=1200.0, nq=2, backend="hip", oracle=False, hydrostatic=0, tau=0.2, rf_cutoff=3.0e4)
    check_nh_fv_dot_product(c, tol=1e-11)


def test_nh_six_faces_dot_product():
    from common import CubeCase
    from nh_checks import cube_check_nh_dot_product
    c = CubeCase(n=16, npz=8, n_split=2, k_split=2, dt=300.0, nq=1, backend="hip", hydrostatic=0, tau=0.2, rf_cutoff=3.0e4)
    cube_check_nh_dot_product(c, tol=1e-11)


def test_nh_step_taylor():
    from common import Case
    c = Case(nx=10, ny=8, npz=8, n_split=2, dt=600.0, backend="hip", oracle=False, hydrostatic=0, tau=0.1, rf_cutoff=3.0e4,
             do_vort_damp=0, do_vort_damp_pert=0)
    RC.check_nh_taylor(c)


def test_nh_pkz_from_temperature_before_heating():
    from common import Case
    kw = dict(nx=8, ny=8, npz=4, n_split=2, dt=600.0, backend="hip", hydrostatic=0, oracle=False)
    RC.check_nh_pkz_before_heating(Case(tau=0.2, rf_cutoff=1.5e4, **kw), Case(**kw))


def test_refusals():
    from common import Case
    from fv3_jedi_linearmodel_amd._lib import Fv3LmError
    c = Case(nx=8, ny=8, npz=8, n_split=2, backend="hip", oracle=False)
    for tau, cut, c2l, msg in ((-1.0, 3.0e4, c.c2l, "tau < 0"), (float("nan"), 3.0e4, c.c2l, "finite"), (1.0, float("inf"), c.c2l, "finite"),
                               (1.0, c.opt.ptop, c.c2l, "rf_cutoff > ptop"), (1.0, 3.0e4, None, "c2l is null")):
        with pytest.raises(Fv3LmError, match=msg):
            c.dy.set_rayleigh(tau, cut, c2l)
    assert c.dy.rayleigh_profile()[1] == 0
