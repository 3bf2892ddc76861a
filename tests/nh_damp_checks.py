"""Checks of the non-hydrostatic step with a trajectory nord of 2 or 3 (fv3lm_set_trajectory_damping_order), shared by the host-emulation
(test_emul_nh_damp.py) and the MI355X (test_gpu_nh_damp.py) runs.

The damping of w in d_sw and of the interface heights in update_dz_d then runs del6_vt_flux with order min(2, nord) = 2, differentiated
(sw_core_tlm.F90:1712-1745, nh_utils_tlm.F90:489-520).  Three kinds of check:
  - against the oracle (nh_checks.py as it is: dyn_core_nh and fv_dynamics_nh on the periodic tile, fv_dynamics_nh on six faces), 1e-11;
  - the operator alone, the product's d_sw group against the numpy restatement del6_oracle.py, 1e-12 relative per level (the product
    multiplies the coefficient last, the reference first: no bit equality), and its adjoint by the dot product, 1e-12;
  - the setter: a hydrostatic handle set to an order equals, bit for bit, the one created with it.
The oracle for this path holds no reference fixtures: parity is unpinned, like the rest of the non-hydrostatic step."""
import numpy as np
import nh_checks as N      # noqa: F401  (the oracle checks are used as they are)
import del6_oracle as D6
from common import Case, CubeCase, relerr
from oracle import NL, TL, AD

# every trajectory coefficient differs from its perturbation counterpart (tests/test_emul_split_damp.py COEF)
COEF = dict(split_damp=1, dddmp=0.35, dddmp_pert=0.2, d4_bg=0.11, d4_bg_pert=0.15, d2_bg=0.02, d2_bg_pert=0.015, vtdm4=0.03, vtdm4_pert=0.0005,
            d2_bg_k1=0.18, d2_bg_k2=0.1)
NH = dict(COEF, hydrostatic=0, nord_pert=1, late_nord=True)


def tile_case(backend, nord, **kw):
    """two acoustic steps on the 12 x 10 x 12 periodic tile: sponge levels (order 0) and regular levels (order 2)"""
    return Case(nx=12, ny=10, npz=12, n_split=2, dt=600.0, backend=backend, nord=nord, **dict(NH, **kw))


def tile_case_fv(backend, nord, **kw):
    return Case(nx=12, ny=10, npz=12, n_split=2, k_split=2, nq=2, dt=1200.0, backend=backend, nord=nord, **dict(NH, **kw))


def cube_case(backend, nord, n=8, layout=1, oracle=True, **kw):
    return CubeCase(n=n, npz=12, n_split=2, k_split=2, dt=1200.0, nq=1, backend=backend, oracle=oracle, layout=layout, nord=nord, **dict(NH, **kw))


def layout_case(backend, nord, layout, small=False):
    """the six-face case on C16 in 8-wide tiles; small: six levels (three of the sponge, three of order 2) and one remap step, which keeps
    the two C16 runs of the host emulation to a few seconds"""
    if small:
        return CubeCase(n=16, npz=6, n_split=2, k_split=1, dt=600.0, nq=1, backend=backend, layout=layout, nord=nord, **NH)
    return cube_case(backend, nord, n=16, layout=layout, oracle=False)


# ---- the operator alone
def level_orders(c):
    """[(nord_w, damp_w)] and [(nord_v, damp_vt)] per level as the handle resolved them"""
    lw, lv = [], []
    for k in range(1, c.npz + 1):
        ip, rp = c.dy.level_params(k)
        lw.append((ip[7], rp[2])); lv.append((ip[6], rp[1]))
    return lw, lv


def dsw_case(backend, nord, face=None, **kw):
    """the d_sw group alone: 70 x 20 periodic tile (crosses a 64-column and a 16-row block boundary) or one whole face of C12 (all four
    corners); one acoustic step of 60 s keeps every Courant number small whatever the winds"""
    nx, ny = (70, 20) if face is None else (12, 12)
    return Case(nx=nx, ny=ny, npz=6, n_split=1, k_split=1, dt=60.0, backend=backend, oracle=False, face=face, nord=nord, n_sponge_pert=2, **dict(NH, **kw))


DSW_INS = ["delp", "pt", "u", "v", "uc", "vc", "ua", "va", "divgd", "mfx", "mfy", "cx", "cy", "w"]


def dsw_put(c, w, w_tl):
    """inputs of the d_sw group: the case's smooth state, C-grid and A-grid winds taken from the D-grid ones (any smooth field serves: dw
    depends on w alone), w and its tangent as given over the whole padded plane, every other tangent zero"""
    t = c.traj
    src = dict(delp=t["delp"], pt=t["pt"], u=t["u"], v=t["v"], uc=t["u"], vc=t["v"], ua=t["u"], va=t["v"])
    for n in DSW_INS:
        a = src.get(n)
        c.dy.put(n, a if a is not None else np.zeros(c.dy.shape(n)), 0)
        c.dy.put(n, np.zeros(c.dy.shape(n)), 1)
    c.dy.put("w", w[None], 0)
    c.dy.put("w", w_tl[None], 1)


def check_dw_against_restatement(c, tol=1e-12, verbose=True):
    """dw of the product's d_sw group, values (NL and TL run) and tangent, level by level against del6_oracle.py"""
    rng = np.random.default_rng(41)
    shp = (c.npz, c.ny + 7, c.nx + 7)
    w, w_tl = rng.standard_normal(shp), rng.standard_normal(shp)
    lw, _ = level_orders(c)
    m = {n: c.metrics[n][0] for n in ("del6_u", "del6_v", "rarea")}
    face = c.face is not None
    ref = D6.dw_levels(c.nx, c.ny, lw, c.da_min_c, w, m["del6_u"], m["del6_v"], m["rarea"], face)
    ref_tl = D6.dw_levels(c.nx, c.ny, lw, c.da_min_c, w_tl, m["del6_u"], m["del6_v"], m["rarea"], face)
    A = c.rect(1, c.nx, 1, c.ny)
    dsw_put(c, w, w_tl)
    c.dy.run_group("d_sw", NL)
    got_nl = c.dy.get("dw", 0)[0].copy()
    dsw_put(c, w, w_tl)
    c.dy.run_group("d_sw", TL)
    got, got_tl = c.dy.get("dw", 0)[0], c.dy.get("dw", 1)[0]
    worst = 0.0
    for k in range(c.npz):
        assert np.max(np.abs(ref[k][A])) > 0 and np.max(np.abs(ref_tl[k][A])) > 0, ("level without damping", k, lw[k])
        e = [relerr(got_nl[k][A], ref[k][A]), relerr(got[k][A], ref[k][A]), relerr(got_tl[k][A], ref_tl[k][A])]
        if verbose:
            print("dw level %d order %d: nl %.2e  tl values %.2e  tangent %.2e" % (k + 1, lw[k][0], *e))
        assert max(e) < tol, (k + 1, lw[k], e)
        worst = max(worst, *e)
    return worst, sorted({n for n, d in lw if d > 1.0e-5})


def dw_dot_product(c, through="w_m"):
    """<s, y'> = <w_ad, w'> for w' random over the whole padded plane (halo rows, corner squares and the spare row included) and every
    other tangent zero.  through = "w_m": s on the group's output w_m = transported w + dw, on is..ie, js..je -- the backward sweep as it
    is planned (first-write stores); through = "dw": s on dw itself, for a handle created with FV3LM_NO_AD_WRITE_MODE=1 (every work
    adjoint cleared and accumulated into), where the increment's adjoint can be seeded in place."""
    rng = np.random.default_rng(43)
    shp = (c.npz, c.ny + 7, c.nx + 7)
    w, w_tl = rng.standard_normal(shp), rng.standard_normal(shp)
    A = c.rect(1, c.nx, 1, c.ny)
    dsw_put(c, w, w_tl)
    c.dy.run_group("d_sw", TL)
    y = c.dy.get(through, 1)[0]
    s = np.zeros(shp); s[A] = rng.standard_normal(s[A].shape)
    lhs = float(np.sum(s * y))
    dsw_put(c, w, np.zeros(shp))
    c.dy.run_group("d_sw", NL)
    c.dy.zero_work_adjoint()
    for n in ("delp_o", "pt_o", "u_m", "v_m", "w_m", "crx", "cry", "xfx", "yfx"):
        c.dy.put(n, np.zeros(c.dy.shape(n)), 1)
    c.dy.put(through, s[None], 1)
    c.dy.run_group("d_sw", AD)
    w_ad = c.dy.get("w", 1)[0]
    rhs = float(np.sum(w_ad * w_tl))
    return lhs, rhs, w_ad


# ---- the whole chain as one LDS-tiled launch (csrc/del6.h, FV3LM_DEL6_FUSED=1) against the staged chain (FV3LM_DEL6_FUSED=0 and the default)
def tiled_and_staged(monkeypatch, make):
    """(case with the tiled launch, case with the staged chain); the switch is read where the programs are built"""
    monkeypatch.setenv("FV3LM_DEL6_FUSED", "1")
    tiled = make()
    monkeypatch.setenv("FV3LM_DEL6_FUSED", "0")
    staged = make()
    monkeypatch.delenv("FV3LM_DEL6_FUSED", raising=False)
    return tiled, staged


def dsw_fields(c):
    """dw of the d_sw group (NL run; TL run: values and tangent) and the adjoint of w for a fixed adjoint of w_m, with the launches of one TL run"""
    rng = np.random.default_rng(47)
    shp = (c.npz, c.ny + 7, c.nx + 7)
    w, w_tl = rng.standard_normal(shp), rng.standard_normal(shp)
    dsw_put(c, w, w_tl)
    c.dy.run_group("d_sw", NL)
    out = {"nl": c.dy.get("dw", 0).copy()}
    dsw_put(c, w, w_tl)
    n0 = c.dy.launch_count()
    c.dy.run_group("d_sw", TL)
    launches = c.dy.launch_count() - n0
    out["tl0"], out["tl1"] = c.dy.get("dw", 0).copy(), c.dy.get("dw", 1).copy()
    _, _, w_ad = dw_dot_product(c)
    out["ad"] = w_ad.copy()
    return out, launches


def check_tiled_equals_staged_dsw(monkeypatch, backend, nord, face, tol_fw, tol_ad):
    """tol_fw = 0: bit for bit"""
    t, s = tiled_and_staged(monkeypatch, lambda: dsw_case(backend, nord, face))
    a, la = dsw_fields(t)
    b, lb = dsw_fields(s)
    # an order-1 program keeps its Del6A + DswDw pair whatever the switch; order 2 on the periodic tile: Del6A + Del6B + DswDw2 -> Del6
    assert (la == lb) if nord < 2 else (la == lb - 2) if face is None else (la < lb), (la, lb)
    A = t.rect(1, t.nx, 1, t.ny)
    for key in ("nl", "tl0", "tl1"):
        x, y = a[key][0][A], b[key][0][A]
        assert np.abs(y).max() > 0
        e = relerr(x, y)
        print("tiled vs staged dw %s: %.2e" % (key, e))
        assert (np.array_equal(x, y) if tol_fw == 0 else e <= tol_fw), (key, e)
    e = relerr(a["ad"], b["ad"])
    print("tiled vs staged w_ad: %.2e" % e)
    assert np.abs(b["ad"]).max() > 0 and e <= tol_ad, e


def check_tiled_equals_staged_dyn_core(monkeypatch, backend, tol_fw, tol_ad):
    """two acoustic steps on the periodic tile of the oracle checks, nord 2: every tangent output, every adjoint input"""
    from test_oracle_nh import nh_state
    t, s = tiled_and_staged(monkeypatch, lambda: tile_case(backend, 2, oracle=False))
    res = []
    for c in (t, s):
        T, P = nh_state(c)
        N.put(c, T, P)
        c.dy.dyn_core(TL)
        fw = {(n, w): c.dy.get(n, w).copy() for n in N.OUTS for w in (0, 1)}
        rng = np.random.default_rng(11)
        A = c.rect(1, c.nx, 1, c.ny)
        N.put(c, T)
        c.dy.dyn_core(NL)
        for n in N.OUTS:
            sd = np.zeros((c.dy.levels(n), c.ny + 7, c.nx + 7))
            if n != "zh":
                sd[A] = rng.standard_normal(sd[A].shape)
            c.dy.put(n, sd[None], 1)
        c.dy.dyn_core(AD)
        res.append((fw, {n: c.dy.get(n, 1).copy() for n in N.INS}))
        assert "LDS" not in c.dy.lib.err()          # host emulation: the guard words behind the block's declared LDS are intact
    A = t.rect(1, t.nx, 1, t.ny)
    for key in res[0][0]:
        x, y = res[0][0][key][0][A], res[1][0][key][0][A]
        assert (np.array_equal(x, y) if tol_fw == 0 else relerr(x, y) <= tol_fw), (key, relerr(x, y))
    for n in N.INS:
        e = relerr(res[0][1][n], res[1][1][n])
        print("tiled vs staged dyn_core adjoint %s: %.2e" % (n, e))
        assert e <= tol_ad, (n, e)


def edge_tile_case(backend, layout):
    """C24 in 3 x 3 tiles per face: the middle tile of a face has no cube edge, the four beside it one edge and no corner -- on those five
    the tiled launch runs the adjoint too"""
    return CubeCase(n=24, npz=4, n_split=1, k_split=1, dt=300.0, nq=0, backend=backend, layout=layout, nord=2, **NH)


# ---- the setter
STEP = ["u", "v", "pt", "delp"]


def step_bits(c):
    """step_tl outputs (values and tangent) and step_ad inputs of a hydrostatic tile case, for bit comparisons"""
    from groups import step_state
    T, P = step_state(c)
    names = STEP + ["q%d" % (n + 1) for n in range(c.nq)]
    for n in names:
        c.dy.put(n, T[n][None], 0); c.dy.put(n, P[n][None], 1)
    c.dy.step_tl()
    out = {("tl", n, w): c.dy.get(n, w).copy() for n in names for w in (0, 1)}
    for n in names:
        c.dy.put(n, T[n][None], 0)
    c.dy.step_nl()
    rng = np.random.default_rng(5)
    for n in names:
        s = np.zeros(c.dy.shape(n)); A = c.rect(1, c.nx, 1, c.ny); s[A] = rng.standard_normal(s[A].shape)
        c.dy.put(n, s, 1)
    c.dy.step_ad()
    out.update({("ad", n, 1): c.dy.get(n, 1).copy() for n in names})
    return out


def assert_same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.isfinite(a[k]).all() and np.abs(a[k]).max() > 0, k
        assert np.array_equal(a[k], b[k]), (k, float(np.max(np.abs(a[k] - b[k]))))


def hydro_case(backend, nord, **kw):
    return Case(nx=12, ny=10, npz=12, n_split=2, k_split=1, dt=1800.0, backend=backend, oracle=False, nord=nord, nord_pert=1, **dict(COEF, **kw))


def check_set_equals_create(backend, start, target):
    a = hydro_case(backend, start)
    a.dy.set_trajectory_damping_order(target)
    assert a.dy.trajectory_damping_order() == target
    assert_same_bits(step_bits(a), step_bits(hydro_case(backend, target)))
