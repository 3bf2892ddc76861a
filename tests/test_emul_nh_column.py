"""The non-hydrostatic column operators (csrc/nh.h, nh_ad.h), column by column, on the host-emulation build against the numpy restatement
tests/nh_column_oracle.py (checks, columns and tolerances in nh_column_checks.py): riem_c_col and riem3_col with the dz_min fix and the
p_fac floor taken, in values, tangent and adjoint (hand-written and taped), both last_call states; edge_col, ring_col on their own."""
import numpy as np
import pytest
from common import Case
import nh_column_checks as K
import nh_column_oracle as O

NPZ = [3, 4, 5, 6, 7, 8, 16, 63, 64, 65, 127, 128, 129]
BACKEND = "emul"
# the whole cross product (solver setting x p_fac) up to 16 levels; deeper, where the longdouble reference costs seconds, every level count runs the
# three settings and p_fac alternates with level count and setting, so that each (setting, p_fac) pair still meets three deep level counts
CASES = [(n, s, p) for n in NPZ for i, s in enumerate(K.SETTINGS) for j, p in enumerate(K.P_FACS) if n <= 16 or (NPZ.index(n) + i) % 2 == j]


def _case(npz, setting, p_fac):
    return Case(**K.case_kwargs(npz, setting, p_fac, BACKEND))


@pytest.mark.parametrize("npz,setting,p_fac", CASES)
def test_solvers(npz, setting, p_fac, monkeypatch):
    """values, tangent and the hand-written adjoint (csrc/nh_ad.h), then the taped adjoint of the generic column code (FV3LM_NH_TAPE=1, read when
    the handle is created) against the same references; a tape overflow surfaces as the library's error"""
    tag = "%s L%d %s p_fac %.2f" % (BACKEND, npz, setting, p_fac)
    monkeypatch.delenv("FV3LM_NH_TAPE", raising=False)
    K.run_solvers(_case(npz, setting, p_fac), tag + " hand", ("values", "adjoint"))
    monkeypatch.setenv("FV3LM_NH_TAPE", "1")
    K.run_solvers(_case(npz, setting, p_fac), tag + " tape", ("adjoint",))


@pytest.mark.parametrize("npz", NPZ)
def test_edge_profile_and_rings(npz, monkeypatch):
    monkeypatch.delenv("FV3LM_NH_TAPE", raising=False)
    K.run_small(_case(npz, "sim075", 0.05), "%s L%d" % (BACKEND, npz))


# ---- the restatement against itself (no product)
def _bare(npz, setting):
    from fv3_jedi_linearmodel_amd import harness as H
    return H.Case(**K.case_kwargs(npz, setting, 0.05, "none"))


@pytest.mark.parametrize("setting", list(K.SETTINGS))
def test_restatement_complex_step_matches_finite_differences(setting):
    """the quiet columns, which sit away from both switches: complex step against centred differences in longdouble"""
    c = _bare(8, setting)
    D = K.draw(c)
    for name in ("riem_c", "riem3"):
        op = K.Op(c, name, 1 if name == "riem3" else 0)
        X = K.solver_inputs(op, D)
        info = {}
        op.f(K.as_ld(X), info=info)
        kinds = np.array([D["kinds"][n] for n in D["col_of_point"][op.pj, op.pi]])
        calm = ~np.any(info["lifted"] | info["floored"], axis=1) & (kinds == "quiet")
        assert calm.sum() >= 4
        cols = np.where(calm)[0]
        Xc = {n: a[cols] for n, a in X.items()}
        dX = K.perturbation(Xc)
        f = lambda Z: op.f(Z, cols)
        _, t = O.tangent(f, Xc, dX)
        eps = np.longdouble(1e-5)
        up = f({n: np.asarray(Xc[n], dtype=np.longdouble) + eps * dX[n] for n in Xc})
        dn = f({n: np.asarray(Xc[n], dtype=np.longdouble) - eps * dX[n] for n in Xc})
        for n in op.outs:
            fd = (up[n] - dn[n]) / (2 * eps)
            # truncation: the relative step is at most eps x 0.3 (w), squared 1e-11, times a curvature allowed up to 1e3: 1e-8;
            # rounding: 1e3 ulps of the longdouble values (the solves cancel that much) over the step, relative to the tangent
            bound = 1e-8 + 1e3 * float(np.finfo(np.longdouble).eps) * np.max(np.abs(up[n]), axis=1) / (float(eps) * np.max(np.abs(t[n]), axis=1))
            e = K.col_err(fd, t[n])
            assert np.all(e <= bound), (name, n, float(np.max(e / bound)))


def test_restatement_small_operators():
    """edge_profile returns a constant for constant layer means and a linear profile's interface values where the levels are uniform;
    the halo pressures are the running sums; the initial heights stack the thicknesses on the surface"""
    km = 9
    one = np.ones((2, km), dtype=np.longdouble)
    a, b = O.edge_profile(3.5 * one, -2.0 * one, np.linspace(1.0, 7.0, km))
    assert np.max(np.abs(a - 3.5)) < 1e-16 and np.max(np.abs(b + 2.0)) < 1e-16
    lin = (np.arange(km) + 0.5)[None] * one
    a, _ = O.edge_profile(lin, lin, np.ones(km))
    assert np.max(np.abs(a - np.arange(km + 1))) < 1e-15
    C = O.Consts(1.0, 2.0 / 7.0, 1.0, 287.04, 9.8, 0.75, 0.05, 0.0)
    dp = np.arange(1.0, km + 1)[None] * one
    assert np.array_equal(O.pe_halo(C, dp)[0], 1.0 + np.concatenate([[0.0], np.cumsum(np.arange(1.0, km + 1))]))
    assert np.max(np.abs(O.pk3_halo(C, dp) - O.pe_halo(C, dp) ** np.longdouble(2.0 / 7.0))) < 1e-15
    zh = O.zh_init(-dp, np.array([10.0, 20.0], dtype=np.longdouble))
    assert np.array_equal(zh[:, -1], [10.0, 20.0]) and np.allclose(np.diff(zh, axis=1), -dp)
