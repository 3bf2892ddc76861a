"""-m "not gpu": the linearised boundary-layer turbulence (fv3lm_turbulence_*; csrc/turbulence.h) in the host-emulation build of the
product sources, and the numpy restatement itself against independent algebra (check 0).  Checks: tests/turbulence_checks.py."""
import numpy as np
import pytest
import turbulence_checks as TC
import turbulence_oracle as TO

BACKEND = "emul"


def tile(face=None, hydro=1, npz=12, nq=4, **kw):
    """the periodic tile 12 x 10, or one 12 x 12 face of a C12 cube"""
    from common import Case
    nx, ny = (12, 10) if face is None else (12, 12)
    return Case(nx=nx, ny=ny, npz=npz, n_split=2, dt=1800.0, nq=nq, backend=BACKEND, oracle=False, face=face, hydrostatic=hydro, **kw)


@pytest.mark.parametrize("lm", [8, 72, 127])
def test_restatement_generated(lm):
    """check 0 (no product): the numpy restatement against numpy.linalg.solve and against its own transpose, 400 columns of (ii)"""
    diag = TO.diffusion_systems(np.random.default_rng(100 + lm), (lm, 1, 400), 8.0)
    assert max(float(np.abs(diag[n]).max()) for n in (0, 3, 6)) >= 5.0
    TC.check_restatement(diag, 1e-13)


def test_restatement_bl_simp_l127():
    """check 0 on the physically shaped diagonals (i): the restated BL_simp on the 12 x 10 x L127 tile"""
    from common import Case
    c = Case(nx=12, ny=10, npz=127, n_split=2, dt=1800.0, nq=4, backend="none", oracle=False)
    T, _ = TC.unit_state(c)
    diag = TC.simple(c, T)[0]
    TC.check_restatement([np.ascontiguousarray(a[0].reshape(127, 1, -1)) for a in diag], 1e-13)


@pytest.mark.parametrize("npz,kind", [(127, "simple"), (12, "generated")])
@pytest.mark.parametrize("hydro", [1, 0])
@pytest.mark.parametrize("face", [None, 2])
def test_unit_three_modes(face, hydro, npz, kind):
    """check 1: u v pt q1..q4 on is..ie x js..je against the restatement <= 1e-12 of the field's max for NL, TL, AD; every halo point,
    u(:, je+1), v(ie+1, :), delp, w, delz and (TL / AD) the whole trajectory bitwise unchanged; the factors and pk <= 1e-12"""
    TC.check_unit(tile(face, hydro, npz), kind, 1e-12)


@pytest.mark.parametrize("npz,kind", [(127, "simple"), (12, "generated")])
@pytest.mark.parametrize("face", [None, 2])
def test_unit_dot_product(face, npz, kind):
    """check 2: <TL x, y> = <x, AD y> over the seven fields, 1e-12 relative"""
    TC.check_unit_dot_product(tile(face, 1, npz), kind, 1e-12)


@pytest.mark.parametrize("face", [None, 2])
def test_bl_simp_on_the_device(face):
    """check 3: set_simple + get against the restated BL_simp + VTRILUPERT, 1e-12, on a state that exercises both branches of RI and KH"""
    TC.check_simple(tile(face, 1, 127), 1e-12)


def test_slot_keeps_what_set_saw():
    """check 4"""
    TC.check_slots(tile(None, 1, 12), 1e-12)


def test_composite_dot_product_tile():
    """check 5, periodic tile, hydrostatic (sizes and time step of tests/test_gpu_split_damp.py)"""
    from common import Case
    c = Case(nx=24, ny=20, npz=12, n_split=2, k_split=2, dt=1800.0, nq=4, backend=BACKEND, oracle=False)
    TC.check_composite(c, 1e-12)


def test_composite_dot_product_tile_nonhydrostatic():
    """check 5, periodic tile, non-hydrostatic (case of tests/test_gpu_rayleigh.py::test_nh_step_dot_product)"""
    from common import Case
    c = Case(nx=10, ny=8, npz=8, n_split=2, k_split=2, dt=1200.0, nq=2, backend=BACKEND, oracle=False, hydrostatic=0, tau=0.2, rf_cutoff=3.0e4)
    TC.check_composite(c, 1e-11)


def test_composite_dot_product_six_faces():
    """check 5, six faces, hydrostatic"""
    from common import CubeCase
    TC.check_composite(CubeCase(n=8, npz=6, n_split=2, k_split=2, nq=4, backend=BACKEND), 1e-11)


def test_composite_dot_product_six_faces_nonhydrostatic():
    """check 5, six faces, non-hydrostatic (CPU size; the MI355X run takes the case of tests/test_gpu_rayleigh.py)"""
    from common import CubeCase
    TC.check_composite(CubeCase(n=8, npz=6, n_split=2, k_split=2, dt=300.0, nq=1, backend=BACKEND, hydrostatic=0, tau=0.2, rf_cutoff=3.0e4), 1e-11)


def test_layout_equals_whole_faces():
    """check 6: 24 sub-face tiles gathered against six whole faces, same global fields and diagonals: bitwise"""
    from common import CubeCase
    TC.check_layout(lambda L: CubeCase(n=16, npz=6, n_split=2, k_split=1, dt=900.0, nq=4, backend=BACKEND, layout=L), 2)


def test_refusals():
    """check 7"""
    TC.check_refusals(lambda nq, npz: tile(None, 1, npz, nq))
