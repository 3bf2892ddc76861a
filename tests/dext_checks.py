"""Checks of the external-mode divergence damping (fv3lm_set_external_damping, csrc/dext.h) shared by the host-emulation and the GPU tests;
the reference is tests/dext_oracle.py (numpy restatement composed with the C++ oracle's pieces).  Tolerances are the project's own
(SURVEY.md section 8): relative L-infinity 1e-12 for the units, 1e-10 for whole steps, 1e-12 for the dot-product identity."""
import numpy as np
from oracle import NL, TL, AD
import groups as G
import dext_oracle as DO
from common import relerr

TOL_UNIT, TOL_STEP, TOL_DOT = 1e-12, 1e-10, 1e-12
D_EXT = 0.02
TILE = dict(nx=12, ny=10, npz=6)
FACE = dict(nx=12, ny=12, npz=6)
SPONGE = {"sponge": {}, "nosponge": dict(n_sponge=-1)}      # levels with nord_k = 0 on top / every level nord_k = nord
# split_damp with value and tangent branches that differ on a level: trajectory nord 2 (its sponge: nord_k = 0 on levels 1 .. 3 with these
# d2_bg_k1, d2_bg_k2), perturbation nord 1 with its own sponge of four levels -> level 4: value from divg_d, tangent from the nord = 0 divergence
SPLIT = dict(split_damp=1, nord=2, nord_pert=1, n_sponge_pert=4, dddmp=0.35, dddmp_pert=0.2, d4_bg=0.11, d4_bg_pert=0.15, d2_bg=0.02, d2_bg_pert=0.015,
             vtdm4=0.03, vtdm4_pert=0.0005, d2_bg_k1=0.18, d2_bg_k2=0.1)


def nords(c):
    """per level: the branch that gives the value of the divergence (the trajectory's nord_k) and the one that gives its tangent"""
    val = [c.dy.level_params(k)[0][5] for k in range(1, c.npz + 1)]
    o = c.opt
    tan = val if not o.split_damp else [0 if k <= o.n_sponge_pert else o.nord_pert for k in range(1, c.npz + 1)]
    return val, tan


def launches(c, fn):
    """-> (({kernel: launches} between fv3lm_profile_begin and _end -- the HIP library; the host-emulation build records none --, the number
    of launches), what fn returned)"""
    n0 = c.dy.launch_count()
    c.dy.profile_begin(); r = fn(); prof = c.dy.profile_end()
    return ({k: v[0] for k, v in prof.items()}, c.dy.launch_count() - n0), r


# ------------------------------------------------------------------------------------------------ 1. the unit
UNIT_IN = ["delp", "pt", "u", "v", "uc", "vc", "ua", "va", "divgd", "mfx", "mfy", "cx", "cy"]


def unit_inputs(c):
    T, P = G.make_inputs(c, "d_sw")
    if c.face is not None:      # the reference leaves ua, va at the corner-halo cells without a value: keep what nobody may read out of both sides
        for d in (T, P):
            for n in ("ua", "va"):
                d[n] = G.drop_face_corners(c, n, d[n])
    return T, P


def check_unit(c):
    """divg2 (values and tangent, through field_get) and the adjoint of a2b_ord2 + column mean against the restatement; returns the worst"""
    T, P = unit_inputs(c)
    val, tan = nords(c)
    u = DO.Unit(c, c.dy.external_damping(), val, tan)
    D, D_tl = u.forward(T, P)
    for n in UNIT_IN:
        c.dy.put(n, T[n][None], 0); c.dy.put(n, P[n][None], 1)
    c.dy.run_group("d_sw", TL); c.dy.run_group("d_ext", TL)
    r = c.rect(*G.rects(c)["B"])
    assert np.abs(D[r]).max() > 0 and np.abs(D_tl[r]).max() > 0
    e1, e2 = relerr(c.dy.get("divg2", 0)[0][r], D[r]), relerr(c.dy.get("divg2", 1)[0][r], D_tl[r])
    print("divg2: values %.2e tangent %.2e" % (e1, e2))
    assert e1 <= TOL_UNIT and e2 <= TOL_UNIT, (e1, e2)
    # adjoint of the unit: random divg2 adjoint in; adjoints of delp (ring of 1 included) and of the two divergences out
    rng = np.random.default_rng(23)
    seed = G.masked(c, rng.standard_normal(D.shape), "B")
    a = u.transpose(seed)
    names = ["delp", "dd_c", "dext_wk"] + (["divgd"] if c.opt.nord > 0 else [])
    for n in names:
        c.dy.put(n, np.zeros(c.dy.shape(n)), 1)
    c.dy.put("divg2", seed[None], 1)
    c.dy.run_group("d_ext", AD)
    worst = max(e1, e2)
    for n, ref in (("delp", a["delp"]), ("dd_c", a["div0"])) + ((("divgd", a["divgd"]),) if c.opt.nord > 0 else ()):
        got = c.dy.get(n, 1)[0]
        if np.abs(ref).max() == 0:
            assert np.abs(got).max() == 0, n
            continue
        e = relerr(got, ref)
        print("adjoint of %s: %.2e" % (n, e))
        assert e <= TOL_UNIT, (n, e)
        worst = max(worst, e)
    return worst


# ------------------------------------------------------------------------------------------------ 2. / 3. the place in the step
def state(c):
    return {n: c.traj[n][0] for n in DO.STATE}, {n: c.pert[n][0] for n in DO.STATE}


OUT4 = [("u", "U"), ("v", "V"), ("pt", "A"), ("delp", "A")]


def run_product(c, mode, seeds=None):
    if mode == AD:
        c.put_state(); c.dy.dyn_core(NL)
        for (n, rk), s in zip(G.DC_OUT, seeds):
            c.dy.put(n, s[None], 1)
        c.dy.dyn_core(AD)
        return {n: c.dy.get(n, 1)[0] for n in DO.STATE}
    c.put_state(pert=c.pert if mode == TL else None)
    c.dy.dyn_core(mode)
    return {n: c.dy.get(n, 0)[0] for n, _ in OUT4}, ({n: c.dy.get(n, 1)[0] for n, _ in OUT4} if mode == TL else None)


def ad_seeds(c, seed=5):
    rng = np.random.default_rng(seed)
    out = []
    for n, rk in G.DC_OUT:
        s = rng.standard_normal((c.dy.levels(n), c.ny + 7, c.nx + 7))
        out.append(G.masked(c, s, dict(OUT4)[n]) if n in dict(OUT4) else np.zeros_like(s))
    return out


def chain(comp, c, mode, nsteps, seeds=None):
    """nsteps acoustic steps of length dt_ac of the composition, one after the other -> like Composition.step"""
    from fv3_jedi_linearmodel_amd.grid import halo_fill_periodic as hf
    X, dX = state(c)
    dt = c.dt_ac
    fill = lambda d, ot: {n: hf(ot[m], c.nx, c.ny) for m, n in enumerate(DO.STATE)}
    if mode != AD:
        for _ in range(nsteps):
            if mode == NL:
                ot = comp.step(NL, dt, X); X = fill(X, ot)
            else:
                ot, op = comp.step(TL, dt, X, dX); X = fill(X, ot); dX = fill(dX, op)
        return X, (dX if mode == TL else None)
    traj = [X]
    for _ in range(nsteps - 1):
        traj.append(fill(None, comp.step(NL, dt, traj[-1])))
    ad = seeds
    for s in range(nsteps - 1, -1, -1):
        back = comp.step(AD, dt, traj[s], None, ad)
        if s > 0:      # the step's input halo was filled from its interior: fold the halo adjoints back (transpose of the periodic fill)
            ad = [hf_T(back[n], c.nx, c.ny) for n in DO.STATE] + [np.zeros_like(x) for x in seeds[4:]]
    return back


hf_T = DO.halo_fill_periodic_T


def check_step(c, mode, off=None):
    """fv3lm_dyn_core with n_split = 1 against the composition; off: the same case without the damping (the on/off difference of u must
    exceed the tolerance by 1e3, so the check cannot pass on a no-op)"""
    assert c.dims.n_split == 1 and c.dims.k_split == 1
    val, tan = nords(c)
    comp = DO.Composition(c, c.dy.external_damping(), val, tan)
    X, dX = state(c)
    worst = 0.0
    if mode == AD:
        seeds = ad_seeds(c)
        ref = comp.step(AD, c.dt_ac, X, None, seeds)
        got = run_product(c, AD, seeds)
        for n in DO.STATE:
            e = relerr(got[n], ref[n]); print("adjoint of %s: %.2e" % (n, e))
            assert e <= TOL_STEP, (n, e)
            worst = max(worst, e)
        if off is not None:
            g0 = run_product(off, AD, seeds)
            assert relerr(got["u"], g0["u"]) >= 1e3 * TOL_STEP or relerr(got["delp"], g0["delp"]) >= 1e3 * TOL_STEP
        return worst
    if mode == NL:
        ot, op = comp.step(NL, c.dt_ac, X), None
    else:
        ot, op = comp.step(TL, c.dt_ac, X, dX)
    gt, gp = run_product(c, mode)
    for m, (n, rk) in enumerate(OUT4):
        r = c.rect(*G.rects(c)[rk])
        e = relerr(gt[n][r], ot[m][r]); print("%s: values %.2e" % (n, e))
        assert e <= TOL_STEP, (n, e)
        worst = max(worst, e)
        if mode == TL:
            e = relerr(gp[n][r], op[m][r]); print("%s: tangent %.2e" % (n, e))
            assert e <= TOL_STEP, (n, "tl", e)
            worst = max(worst, e)
    if off is not None:
        g0, p0 = run_product(off, mode)
        r = c.rect(*G.rects(c)["U"])
        assert relerr(gt["u"][r], g0["u"][r]) >= 1e3 * TOL_STEP, "the damping changes nothing"
        if mode == TL:
            assert relerr(gp["u"][r], p0["u"][r]) >= 1e3 * TOL_STEP, "the damping changes no tangent"
        for n in ("pt", "delp"):      # untouched by the damping within one step
            assert np.array_equal(gt[n], g0[n]), n
    return worst


def control_chain(c, nsteps=2):
    """d_ext = 0 on the CPU: does chaining orc_dyn_core(n_split = 1, bdt / nsteps) reproduce orc_dyn_core(n_split = nsteps, bdt)?  -> worst
    relative difference over u v pt delp (values and tangent) on their own ranges"""
    from fv3_jedi_linearmodel_amd.grid import halo_fill_periodic as hf
    X, dX = state(c)
    bdt = c.dt_ac * nsteps
    ot, op = c.oracle.dyn_core(TL, bdt, nsteps, [X[n] for n in DO.STATE], [dX[n] for n in DO.STATE])
    for _ in range(nsteps):
        a, b = c.oracle.dyn_core(TL, c.dt_ac, 1, [X[n] for n in DO.STATE], [dX[n] for n in DO.STATE])
        X = {n: hf(a[m], c.nx, c.ny) for m, n in enumerate(DO.STATE)}; dX = {n: hf(b[m], c.nx, c.ny) for m, n in enumerate(DO.STATE)}
    worst = 0.0
    for m, (n, rk) in enumerate(OUT4):
        r = c.rect(*G.rects(c)[rk])
        worst = max(worst, relerr(X[n][r], ot[m][r]), relerr(dX[n][r], op[m][r]))
    return worst


def check_two_steps(c, mode):
    """n_split = 2 against the chained composition (the control above holds: DESIGN.md section 5)"""
    assert c.dims.n_split == 2 and c.dims.k_split == 1
    ctl = control_chain(c)
    print("control, d_ext = 0: chained n_split = 1 against n_split = 2: %.2e" % ctl)
    assert ctl <= TOL_STEP, ("the oracle's steps do not chain: hold n_split = 2 by the dot product and finite differences instead", ctl)
    val, tan = nords(c)
    comp = DO.Composition(c, c.dy.external_damping(), val, tan)
    worst = 0.0
    if mode == AD:
        seeds = ad_seeds(c)
        ref = chain(comp, c, AD, 2, seeds)
        got = run_product(c, AD, seeds)
        for n in DO.STATE:
            e = relerr(got[n], ref[n]); print("adjoint of %s: %.2e" % (n, e))
            assert e <= TOL_STEP, (n, e)
            worst = max(worst, e)
        return worst
    X, dX = chain(comp, c, TL, 2)
    gt, gp = run_product(c, TL)
    for n, rk in OUT4:
        r = c.rect(*G.rects(c)[rk])
        e1, e2 = relerr(gt[n][r], X[n][r]), relerr(gp[n][r], dX[n][r]); print("%s: values %.2e tangent %.2e" % (n, e1, e2))
        assert e1 <= TOL_STEP and e2 <= TOL_STEP, (n, e1, e2)
        worst = max(worst, e1, e2)
    return worst


# ------------------------------------------------------------------------------------------------ 5. / 6. off state, non-hydrostatic
def run_all(c):
    """step_tl, then step_nl + step_ad on the case's state: every output, and the launch lists of the two halves"""
    from fv3_jedi_linearmodel_amd.harness import step_state, cube_nh_state
    T, P = step_state(c)
    names = ["u", "v", "pt", "delp"] + ["q%d" % (n + 1) for n in range(c.nq)]
    if not c.opt.hydrostatic:
        o = c.opt
        delz = -(o.rdgas / o.grav) * T["pt"] * np.diff(T["peln"], axis=0)
        T.update(w=0.05 * c.pert["pt"][0], delz=delz); P.update(w=0.01 * c.pert["u"][0], delz=1e-3 * c.pert["delp"][0])
        names += ["w", "delz"]

    def tl():
        for n in names:
            c.dy.put(n, T[n][None], 0); c.dy.put(n, P[n][None], 1)
        c.dy.step_tl()
        return [c.dy.get(n, w) for n in names for w in (0, 1)]

    def ad():
        for n in names:
            c.dy.put(n, T[n][None], 0)
        c.dy.step_nl()
        rng = np.random.default_rng(3)
        for n in names:
            c.dy.put(n, G.masked(c, rng.standard_normal(c.dy.shape(n))[0], {"u": "U", "v": "V"}.get(n, "A"))[None], 1)
        c.dy.step_ad()
        return [c.dy.get(n, 1) for n in names]
    l1, o1 = launches(c, tl)
    l2, o2 = launches(c, ad)
    return o1 + o2, (l1, l2)


def check_same(a, b):
    (oa, la), (ob, lb) = run_all(a), run_all(b)
    assert la == lb, (la, lb)
    assert all(np.array_equal(x, y) for x, y in zip(oa, ob))
    return la


def check_refusals(c):
    """negative, NaN, Inf: refused by message, the getter unchanged after each, and the handle still steps"""
    import pytest
    from fv3_jedi_linearmodel_amd._lib import Fv3LmError
    before = c.dy.external_damping()
    for v, msg in ((-0.02, "d_ext < 0"), (float("nan"), "must be finite"), (float("inf"), "must be finite"), (float("-inf"), "must be finite")):
        with pytest.raises(Fv3LmError, match="fv3lm_set_external_damping: .*" + msg):
            c.dy.set_external_damping(v)
        assert c.dy.external_damping() == before, v
    lhs, rhs = G.dot_product_step(c)
    assert np.isfinite(lhs) and abs(lhs - rhs) <= TOL_DOT * abs(lhs), (lhs, rhs)


def check_added_launches(off, on, backend):
    """off, on: the launch records (step_tl half, step_nl + step_ad half) of run_all without and with the damping.  With it there are more
    launches in both halves; by name (HIP library): a2b_ord2, the column kernel and one_grad_p's form with divg2 forward, the column gather,
    the divg2 gather and a2b_ord2 backward -- and none of them without"""
    for (n0, c0), (n1, c1) in zip(off, on):
        assert c1 > c0, (c0, c1)
    if backend != "hip":
        return
    new = ("dext", "A2bOrd2", "OneGradPd")
    assert not any(t in k for half in off for k in half[0] for t in new), off
    tl, ad = on[0][0], on[1][0]
    for k in ("dext_col.tl", "A2bOrd2.tl", "OneGradPd.tl"):
        assert k in tl, (k, sorted(tl))
    assert "OneGradP.tl" not in tl
    for k in ("dext_col.ad", "dext_grad.ad", "A2bOrd2.ad", "OneGradPd.ad"):
        assert k in ad, (k, sorted(ad))
