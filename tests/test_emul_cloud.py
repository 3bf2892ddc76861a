"""-m "not gpu": the linearised cloud scheme (fv3lm_cloud_*; csrc/cloud.h) in the host-emulation build of the product sources, against
the fixture recorded from the reference's own RASE0, CLOUD_DRIVER, CLOUD_DRIVER_D, CLOUD_DRIVER_B (tests/golden/cloud_ref.npz).
Checks: tests/cloud_checks.py."""
import pytest
import cloud_checks as KC

BACKEND = "emul"
TAGS = ["L40m2", "L72m2", "L72m1", "L20m1"]


def tile(tag, face=None, nq=3, size=None, **kw):
    """the periodic tile 12 x 10 (or size), or one 12 x 12 face of a C12 cube, on the fixture's levels"""
    from common import Case
    nx, ny = (size or (12, 10)) if face is None else (12, 12)
    fx = KC.fixture(tag)
    kw = kw or KC.case_kw(fx)
    return Case(nx=nx, ny=ny, npz=fx["lm"], n_split=2, dt=1800.0, nq=nq, backend=BACKEND, oracle=False, face=face, **kw)


def cube(tag, layout=1, nq=3, n=12):
    from common import CubeCase
    fx = KC.fixture(tag)
    return CubeCase(n=n, npz=fx["lm"], n_split=1, k_split=1, dt=1800.0, nq=nq, backend=BACKEND, layout=layout, **KC.case_kw(fx))


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("face", [None, 2])
def test_set_against_the_reference(face, tag):
    """checks 1 and 5: the split arrays (in the levels the loop leaves alone), the fractions and the eight values of CLOUD_DRIVER within the
    fixture's tolerance ((LM - 29) x the reference's own movement under 1e-15 perturbations, floor 1e-12), every column; cloud_pertmod
    equal cell by cell (all 1 for do_phy_mst = 1); cloud_default_params equal; L20: nothing but the tail acts"""
    KC.check_set(tile(tag, face), tag)


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("face", [None, 2])
def test_modes_against_the_reference(face, tag):
    """checks 2, 3, 4 and 5: tangent against CLOUD_DRIVER_D, adjoint against CLOUD_DRIVER_B with the adjoints of the four sources (the theta
    conversion and the qi / ql splits restated in numpy), nonlinear against CLOUD_DRIVER's values; everything else bitwise unchanged"""
    KC.check_modes(tile(tag, face), tag)


@pytest.mark.parametrize("where", ["tile", "face", "six faces"])
@pytest.mark.parametrize("tag", ["L40m2", "L72m2", "L72m1"])
def test_dot_product(where, tag):
    """check 6: <TL x, y> = <x, AD y> over T, qv, qi, ql, cfcn and the four sources at 1e-12"""
    KC.check_dot_product(tile(tag) if where == "tile" else tile(tag, 2) if where == "face" else cube(tag), tag)


@pytest.mark.parametrize("tag", ["L40m2", "L72m1"])
def test_dot_product_of_the_chain(tag):
    """check 6: convection(1) ; cloud(1) against cloud(2) ; convection(2) on the tile at 1e-12"""
    KC.check_dot_product(tile(tag), tag, chain=True)


def test_position_independence():
    """check 7: the L40 columns dealt over the six faces of a C16 cube and over its 2 x 2 sub-face layout: every column's set outputs,
    fractions, switch and tangent results, adjoint results with cfcn and the source adjoints, and the qi, ql and CF_con of the nonlinear
    run as on the small tile, bitwise"""
    KC.check_position(lambda: tile("L40m2"), lambda L: cube("L40m2", L, 3, 16), "L40m2", 2, key=BACKEND)


@pytest.mark.parametrize("where", ["six faces C24 L40", "tile 64 x 32 L20", "tile 64 x 40 L40"])
def test_columns_beyond_one_batch(where, monkeypatch, capfd):
    """check 7b: 3,456, 2,048 and 2,560 columns against a batch whose size the library reports: two batches, the second partial, on the
    first and the last case (on the cube the boundary falls inside a face); exactly one full batch on the second.  Every column, every
    mode, as on the small tile: bitwise"""
    monkeypatch.setenv("FV3LM_VERBOSE", "1")
    tag = "L20m1" if "L20" in where else "L40m2"
    big = (lambda: cube(tag, 1, 3, 24)) if "six" in where else (lambda: tile(tag, None, 3, (64, 32) if tag == "L20m1" else (64, 40)))
    KC.check_batches(lambda: tile(tag), big, tag, lambda: capfd.readouterr().err, full=tag == "L20m1", key=BACKEND)


def test_reset_and_two_slots():
    """check 7c: two slots with different trajectories run in turn; a convection slot set again refuses the cloud run until the cloud
    slot is set again; then slot 0 equals slot 1 and a fresh single-slot handle, bitwise"""
    KC.check_reset_and_slots(lambda: tile("L40m2"), "L40m2")


@pytest.mark.parametrize("where", ["tile", "six faces"])
def test_nothing_else_moves(where):
    """check 8: halos, far edge rows, delp, u, v, the other tracers, the other slot, the convection and turbulence slots and the host's
    arrays bitwise unchanged; set, step_tl, run: the slot did not follow the resident trajectory"""
    KC.check_nothing_else_moves(tile("L40m2", None, 4) if where == "tile" else cube("L40m2", 1, 4), "L40m2")


def test_a_handle_without_the_cloud_scheme_steps_as_before():
    """check 8, last item"""
    KC.check_untouched_handle(lambda: tile("L20m1"), "L20m1")


def test_refusals():
    """check 9: every item of the refusal list by its message, the slot left unset, a following good call works"""
    KC.check_refusals(lambda nq, npz, **kw: tile("L20m1", None, nq, **kw))
    KC.check_failed_allocation(lambda nq, npz, **kw: tile("L20m1", None, nq, **kw))
