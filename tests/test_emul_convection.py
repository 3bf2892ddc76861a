"""-m "not gpu": the linearised RAS convection (fv3lm_convection_*; csrc/convection.h) in the host-emulation build of the product
sources, against the fixture recorded from the reference's own RASE0, RASE0_D, RASE_D, RASE_B (tests/golden/convection_ref.npz).
Checks: tests/convection_checks.py."""
import pytest
import convection_checks as CC

BACKEND = "emul"
LMS = [40, 72, 20]


def tile(lm, face=None, nq=2, size=None, **kw):
    """the periodic tile 12 x 10 (or size), or one 12 x 12 face of a C12 cube, on the fixture's levels"""
    from common import Case
    nx, ny = (size or (12, 10)) if face is None else (12, 12)
    kw = kw or CC.case_kw(CC.fixture(lm))
    return Case(nx=nx, ny=ny, npz=lm, n_split=2, dt=1800.0, nq=nq, backend=BACKEND, oracle=False, face=face, **kw)


def cube(lm, layout=1, nq=1, n=12):
    from common import CubeCase
    return CubeCase(n=n, npz=lm, n_split=1, k_split=1, dt=1800.0, nq=nq, backend=BACKEND, layout=layout, **CC.case_kw(CC.fixture(lm)))


@pytest.mark.parametrize("lm", LMS)
@pytest.mark.parametrize("face", [None, 2])
def test_set_against_the_reference(face, lm):
    """check 1: PTT_C QVT_C and the four _C sources of RASE0 and the Jacobian column of RASE0_D within the fixture's tolerance (m x the
    reference's own movement under 1e-15 perturbations, floor 1e-12), every column; DOCONVEC equal; ras_default_params, the device's table at the fixture's 184 samples and the kernels' constants equal"""
    CC.check_set(tile(lm, face), lm)


@pytest.mark.parametrize("lm", LMS)
@pytest.mark.parametrize("face", [None, 2])
def test_modes_against_the_reference(face, lm):
    """checks 2 and 4: tangent against RASE_D, adjoint against RASE_B (the theta conversion restated in numpy, the four sources
    compared), nonlinear against RASE's values; stable columns bitwise unchanged with zero sources"""
    CC.check_modes(tile(lm, face), lm)


@pytest.mark.parametrize("where", ["tile", "face", "six faces"])
@pytest.mark.parametrize("lm", [40, 20])
def test_dot_product(where, lm):
    """check 3: <TL x, y> = <x, AD y> over the eight fields at 1e-12"""
    CC.check_dot_product(tile(lm) if where == "tile" else tile(lm, 2) if where == "face" else cube(lm), lm)


def test_position_independence():
    """check 5: the L40 columns dealt over the six faces of a C16 cube and over its 2 x 2 sub-face layout (a tile needs 8 cells, so
    C12 cannot be cut): every column's set outputs, Jacobian column, tangent fields and sources, adjoint fields and consumed sources and
    the trajectory the nonlinear run writes back as on the small tile, bitwise"""
    CC.check_position(lambda: tile(40, None, 1), lambda L: cube(40, L, 1, 16), 40, 2, key=BACKEND)


@pytest.mark.parametrize("where", ["six faces C24 L40", "tile 64 x 32 L20", "tile 64 x 40 L40"])
def test_columns_beyond_one_batch(where, monkeypatch, capfd):
    """check 5b: 3,456, 2,048 and 2,560 columns against a batch whose size the library reports: set runs two batches on the first and the
    last case (on the cube the boundary falls inside a face) and exactly one full batch on the second; on the first and the last the
    active list needs a second, partial batch too, which the test asserts.  Every column, every mode, as on the small tile: bitwise"""
    monkeypatch.setenv("FV3LM_VERBOSE", "1")
    lm = 20 if "L20" in where else 40
    big = (lambda: cube(40, 1, 1, 24)) if "six" in where else (lambda: tile(lm, None, 1, (64, 32) if lm == 20 else (64, 40)))
    CC.check_batches(lambda: tile(lm, None, 1), big, lm, lambda: capfd.readouterr().err, full=lm == 20, key=BACKEND)


def test_reset_and_two_slots():
    """check 5c: two slots with different trajectories run in turn, and a slot set again: results, DOCONVEC and the Jacobian column
    as a fresh single-slot handle gives them for the same deal, bitwise"""
    CC.check_reset_and_slots(lambda: tile(40, None, 1), 40)


@pytest.mark.parametrize("where", ["tile", "six faces"])
def test_nothing_else_moves(where):
    """check 6: halos, far edge rows, delp, q2.., the other slot, the turbulence slot and the host's arrays bitwise unchanged; set,
    step_tl, run: the slot did not follow the resident trajectory"""
    CC.check_nothing_else_moves(tile(20, None, 3) if where == "tile" else cube(20, 1, 3), 20)


def test_a_handle_without_convection_steps_as_before():
    """check 6, last item"""
    CC.check_untouched_handle(lambda: tile(20, None, 2))


def test_refusals():
    """check 7: every item of the refusal list by its message, the slot left unset, a following good call works; the failed allocation by a slot count no machine can hold"""
    CC.check_refusals(lambda nq, npz, **kw: tile(npz, None, nq, **kw))
