"""CPU (-m "not gpu") column tests of the vertical remap (fv3lm_remap; remap.h, nh.h) on the host-emulation build of the product, against
the numpy restatement tests/remap_oracle.py (remap_checks.py), plus the cross-check of that restatement with the C++ oracle's orc_remap.
Measured maxima (per-level relative errors) on this build:
  NL / TL, linear profile, npz 2 .. 129:              <= 5.1e-13 (large displacement at npz 6: 5.1e-13; others ~1e-13 .. 2.4e-13)
  NL / TL, limited kords 8 .. 15, npz 6 .. 8:         <= 2.4e-13
  ratio columns (thickness ratios 1e-3 .. 1e3):       as far as double rounding moves the reference itself (up to 1.9e-10 on pt)
  AD against J^T s entry by entry (npz <= 8):         <= 4.4e-13;  dot products <= 1.2e-15 (ratio columns 8e-12)
  conservation 2.4e-15, constant column 8e-16, identity 8.9e-14.  The MI355X build passes the same bounds (test_gpu_remap_column.py)."""
import numpy as np
import pytest
from common import Case
from oracle import NL, TL
import remap_checks as RC


def _case(npz, nq=1, hydro=1, nx=8, ny=9, **kw):
    return Case(nx=nx, ny=ny, npz=npz, nq=nq, oracle=False, hydrostatic=hydro, **kw)


# --------------------------------------------------------------------------- linear profile where the boundary formulas overlap
@pytest.mark.parametrize("npz", [2, 3, 4, 5])
@pytest.mark.parametrize("kind", ["small", "large"])
def test_linear_small_npz(npz, kind):
    c = _case(npz, nq=1, nx=8, ny=8)
    S = RC.column_state(c, kind, seed=npz, hard=True)
    for last in (0, 1):
        RC.check_nl_tl(c, S, last)
    RC.check_ad_jacobian(c, S, 1)


@pytest.mark.parametrize("npz", [3, 5])
def test_linear_small_npz_nh(npz):
    c = _case(npz, nq=1, hydro=0, nx=8, ny=8)
    S = RC.column_state(c, "small", seed=npz, hard=True)      # (the cubic warp of 'large' at npz < 5 overshoots -delz/delp below zero)
    RC.check_nl_tl(c, S, 0)
    RC.check_ad_jacobian(c, S, 1)


# --------------------------------------------------------------------------- limited trajectory profiles (split_kord)
LIM = [(8, 6), (9, 7), (10, 8), (11, 6), (12, 7), (13, 8), (14, 6), (15, 7)]


@pytest.mark.parametrize("kord,npz", LIM)
def test_limited(kord, npz):
    c = _case(npz, nq=2, nx=10, ny=8, kord_tm=-kord, kord_tr=kord, kord_mt=kord)
    S = RC.column_state(c, "small" if kord % 2 else "large", seed=kord, hard=True)
    for last in (0, 1):
        RC.check_nl_tl(c, S, last)
    RC.check_ad_jacobian(c, S, 0)


@pytest.mark.parametrize("kord,npz", [(9, 8), (13, 6)])
def test_limited_nh(kord, npz):
    c = _case(npz, nq=1, hydro=0, kord_tm=-kord, kord_tr=kord, kord_mt=kord, kord_wz=kord)
    S = RC.column_state(c, "small", seed=kord, hard=True)
    RC.check_nl_tl(c, S, 1)
    RC.check_ad_dot(c, S, 1)


@pytest.mark.parametrize("kord", [8, 9, 10, 11, 12, 13, 14, 15])
def test_limited_tracers_stay_nonnegative(kord):
    c = _case(8, nq=2, kord_tr=kord)
    RC.check_nonnegative(c, RC.column_state(c, "large", seed=kord))


# --------------------------------------------------------------------------- production sizes, stretched levels, extreme ratios
@pytest.mark.parametrize("npz,kind,hydro", [(64, "large", 1), (127, "small", 0), (128, "large", 1)])
def test_large_npz(npz, kind, hydro):
    c = _case(npz, nq=1, hydro=hydro, nx=8, ny=8)
    S = RC.column_state(c, kind, seed=npz, hard=True)
    RC.check_nl_tl(c, S, 0, conditioned=True)
    RC.check_ad_dot(c, S, 1)


@pytest.mark.parametrize("kind", ["small", "large"])
def test_stretched_l127(kind):
    c = _case(127, nq=1, nx=8, ny=8, levels=RC.stretched_levels(127))
    dp = np.diff(c.ak + c.bk * 1.0e5)
    assert dp[0] < 2.0 and dp.max() > 1400.0, (dp[0], dp.max())
    S = RC.column_state(c, kind, seed=3, hard=True)
    RC.check_nl_tl(c, S, 1, conditioned=True)
    RC.check_ad_dot(c, S, 0)


@pytest.mark.parametrize("npz", [8, 64])
def test_thickness_ratios(npz):
    c = _case(npz, nq=1, nx=8, ny=8)
    S = RC.column_state(c, "ratio", seed=npz)
    RC.check_nl_tl(c, S, 0, conditioned=True)
    RC.check_ad_dot(c, S, 0, tol=1e-10)      # ill-conditioned edge solve: measured 8e-12


# --------------------------------------------------------------------------- non-hydrostatic adjoint, with and without the tape
@pytest.mark.parametrize("tape", ["0", "1"])
def test_nh_adjoint(tape, monkeypatch):
    monkeypatch.setenv("FV3LM_NH_TAPE", tape)
    c = _case(7, nq=2, hydro=0, nx=9, ny=8)
    S = RC.column_state(c, "small", seed=11, hard=True)
    RC.check_ad_jacobian(c, S, 1)
    RC.check_ad_jacobian(c, S, 0)


def test_remap_workspace_outside_the_arena(capfd, monkeypatch):
    """nq = 3 at 8 levels: (22 + 8 (1 + nq)) (npz + 2) columns of workspace exceed the acoustic work arena, remap_ws_own is taken"""
    monkeypatch.setenv("FV3LM_VERBOSE", "1")
    c = _case(8, nq=3, nx=8, ny=8)
    err = capfd.readouterr().err
    assert "remap workspace" in err and "own allocation" in err, err
    S = RC.column_state(c, "large", seed=4, hard=True)
    RC.check_nl_tl(c, S, 1)
    RC.check_ad_jacobian(c, S, 1)


# --------------------------------------------------------------------------- properties (no restatement)
@pytest.mark.parametrize("hydro", [1, 0])
def test_conservation_and_constant(hydro):
    c = _case(16, nq=2, hydro=hydro)
    for kind in ("large", "small"):
        S = RC.column_state(c, kind, seed=9)
        RC.check_conservation(c, S)
        RC.check_constant(c, S)


@pytest.mark.parametrize("hydro", [1, 0])
def test_identity(hydro):
    c = _case(10, nq=1, hydro=hydro)
    S = RC.column_state(c, "identity", seed=2, hard=True)
    RC.check_identity(c, S)


# --------------------------------------------------------------------------- the two restatements agree
def test_numpy_reference_matches_the_cpp_oracle():
    """on today's case_q columns (state after the oracle's dyn_core), tests/remap_oracle.py and the C++ oracle's orc_remap agree"""
    import remap_oracle as RO
    from groups import _dyn_outputs, masked
    c = Case(nx=12, ny=10, npz=10, n_split=2, nq=2)
    T, P = _dyn_outputs(c)
    for n in range(c.nq):
        T["q%d" % (n + 1)], P["q%d" % (n + 1)] = c.qtraj[n][0], c.qpert[n][0]
    ins = ["pe", "peln", "pk", "pt", "delp", "u", "v"] + ["q%d" % (n + 1) for n in range(c.nq)]
    for d in (T, P):      # the oracle's pe is defined on 0..nx+1, peln / pk on the compute domain
        d["pe"] = masked(c, d["pe"], "Ah"); d["peln"] = masked(c, d["peln"], "A"); d["pk"] = masked(c, d["pk"], "A")
    T["pe"] = np.where(T["pe"] == 0, 1.0, T["pe"]); T["peln"] = np.where(T["peln"] == 0, 1.0, T["peln"])
    for last in (0, 1):
        ot, op = c.oracle.remap(TL, c.nq, last, [T[n] for n in ins], [P[n] for n in ins])
        R = RO.Remap(c, last)
        S = {n: T[n] for n in R.inputs}
        rv, rt = R.tl(S, {n: P[n] for n in R.inputs})
        names = ["pe", "peln", "pk", "pkz", "pt", "delp", "u", "v"] + ["q%d" % (n + 1) for n in range(c.nq)]
        for n, a, b in zip(names, ot, op):
            assert RC.per_level(RC.on_rect(R, n, a), rv[n]) <= 1e-12, (n, last)
            assert RC.per_level(RC.on_rect(R, n, b), rt[n]) <= 1e-12, (n, last, "tl")


# --------------------------------------------------------------------------- the C-ABI
def test_nh_remap_maps_w_and_delz():
    """fv3lm_remap on a non-hydrostatic handle runs the non-hydrostatic remap: w and delz change (and match the reference above)"""
    c = _case(8, nq=1, hydro=0)
    S = RC.column_state(c, "large", seed=6)
    got = RC.product(c, NL, 0, S)
    R = RC.RO.Remap(c, 0)
    for n in ("w", "delz"):
        assert np.max(np.abs(RC.on_rect(R, n, got[n]) - RC.on_rect(R, n, S[n]))) > 1e-3 * np.max(np.abs(S[n]))
