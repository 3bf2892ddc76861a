"""The bulk of a2b_ord4 as one LDS-tiled launch per mode (csrc/a2b.h) against the two staged launches it replaces (FV3LM_A2B_FUSED=0,
read where the programs are built).  Nonlinear and tangent run the staged arithmetic in its order, so the step_tl outputs (trajectory
and tangent of every prognostic field) must agree BIT FOR BIT in the host emulation; the fused adjoint is the closed-form transpose and
sums in another order, so the step_ad outputs agree to 1e-13 of the field maximum.  On the device the two forms are different kernels
and hipcc contracts a*b+c per kernel: rtol 1e-12 there.

The cases are the smallest that cut a tile into several 64 x 16 blocks both ways and reach every special region: a periodic tile
(thin last block column, two block rows), six faces (rims, strips and corners beside a multi-block bulk), a non-hydrostatic periodic
tile (npz and npz+1 level fields through nh_p_grad) and six faces cut 2 x 2 (68-wide windows: one cube corner, two cube edges and two
interior boundaries each)."""
import os
import numpy as np
from groups import step_state, cube_step_state


def _names_and_state(c):
    cube = getattr(c, "face", None) == "cube"
    names = ["u", "v", "pt", "delp"] + ["q%d" % (n + 1) for n in range(c.nq)]
    if cube:
        T, P = cube_step_state(c)
        if not c.opt.hydrostatic:
            from fv3_jedi_linearmodel_amd.harness import cube_nh_state
            Tn, Pn = cube_nh_state(c)
            T.update(w=Tn[4], delz=Tn[5]); P.update(w=Pn[4], delz=Pn[5])
            names = ["u", "v", "pt", "delp", "w", "delz"] + ["q%d" % (n + 1) for n in range(c.nq)]
        return names, T, P
    if not c.opt.hydrostatic:          # w, delz prognostic: balanced state of the non-hydrostatic checks
        import nh_checks
        from test_oracle_nh import nh_state_fv
        names = nh_checks.fv_names(c)
        Tl, Pl = nh_state_fv(c)
        return names, {n: t[None] for n, t in zip(names, Tl)}, {n: p[None] for n, p in zip(names, Pl)}
    T, P = step_state(c)
    return names, {k: v[None] for k, v in T.items()}, {k: v[None] for k, v in P.items()}


def run_steps(make_case, fused):
    """step_tl outputs (values and tangent) and step_ad outputs of one model built with the fused (default) or the staged a2b_ord4"""
    old = os.environ.get("FV3LM_A2B_FUSED")
    if fused:
        os.environ.pop("FV3LM_A2B_FUSED", None)
    else:
        os.environ["FV3LM_A2B_FUSED"] = "0"
    try:
        c = make_case()
    finally:
        if old is None:
            os.environ.pop("FV3LM_A2B_FUSED", None)
        else:
            os.environ["FV3LM_A2B_FUSED"] = old
    names, T, P = _names_and_state(c)
    for n in names:
        c.dy.put(n, T[n], 0); c.dy.put(n, P[n], 1)
    l0 = c.dy.launch_count() if hasattr(c.dy, "launch_count") else 0
    c.dy.step_tl()
    l_tl = (c.dy.launch_count() - l0) if hasattr(c.dy, "launch_count") else None
    out = {("tl", n, w): c.dy.get(n, w).copy() for n in names for w in (0, 1)}
    rng = np.random.default_rng(5)
    for n in names:
        c.dy.put(n, T[n], 0)
    c.dy.step_nl()
    for n in names:
        c.dy.put(n, rng.standard_normal(c.dy.shape(n)), 1)
    c.dy.step_ad()
    out.update({("ad", n, 1): c.dy.get(n, 1).copy() for n in names})
    return out, l_tl


def check_fused_equals_staged(make_case, rtol=0.0):
    """rtol = 0 (host emulation): step_tl bit for bit, step_ad to 1e-13 of the field maximum.  rtol > 0 (device): every output to rtol of
    the field maximum.  Returns the worst relative difference."""
    a, la = run_steps(make_case, True)
    b, lb = run_steps(make_case, False)
    if la is not None:       # the fused form is what ran: one launch in place of two per a2b_ord4 in the tangent sweep
        assert la < lb, (la, lb)
    worst = 0.0
    for key in a:
        assert np.isfinite(a[key]).all() and np.abs(a[key]).max() > 0, key
        if rtol == 0.0 and key[0] != "ad":
            assert np.array_equal(a[key], b[key]), key
            continue
        e = float(np.max(np.abs(a[key] - b[key])) / np.max(np.abs(b[key])))
        print("a2b fused vs staged %s: %.3e" % (key, e))
        assert e <= (1e-13 if rtol == 0.0 else rtol), (key, e)
        worst = max(worst, e)
    return worst
