"""A hand-written LDS-tiled launch (csrc/tiled.h) against the staged launches it replaces.  Each has a switch that is read where the
programs are built; set to 0 it brings the staged form back:

FV3LM_TP_FUSED=0         fv_tp_2d as its seven stage launches + edge strips in every mode -- one of its two forms; the other, the default, is
                         csrc/tp2.h (nonlinear, tangent), the trajectory pass of csrc/tpfused.h (split levels) and csrc/tpad.h (adjoint).
FV3LM_A2B_FUSED=0        the bulk of a2b_ord4 as A2bA + A2bB (qx, qy through memory) instead of the one launch of csrc/a2b.h.
FV3LM_D2A2C_FUSED=0      the bulk of d2a2c_vect as CswInterpA + CswInterpC (utmp, vtmp through memory) instead of the one of csrc/d2a2c.h.

Nonlinear and tangent run the staged arithmetic in its order, so the step_tl outputs (trajectory and tangent of every prognostic field)
must agree BIT FOR BIT in the host emulation; the fused adjoints are closed-form transposes that sum in another order, so the step_ad
outputs agree to 1e-13 of the field maximum.  On the device the two forms are different kernels and hipcc contracts a*b+c per kernel:
rtol 1e-12 there.

The cases are the smallest that cut a tile into several 64 x 16 blocks both ways and reach every special region: a periodic tile (thin
last block column, two block rows), six faces (rims, bands, strips and corners beside a multi-block bulk), a non-hydrostatic periodic
tile (npz and npz+1 level fields) and six faces cut 2 x 2 (68-wide windows: one cube corner, two cube edges and two interior boundaries
each).  The run of a case with every switch at its default is kept and shared by every comparison against it."""
import os
import numpy as np
from groups import step_state, cube_step_state

SWITCHES = ("FV3LM_TP_FUSED", "FV3LM_A2B_FUSED", "FV3LM_D2A2C_FUSED")
_default_runs = {}


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


def run_steps(make_case, switch=None, value=None):
    """step_tl outputs (values and tangent) and step_ad outputs of one model built with every switch at its default, but `switch` set to
    `value`; -> (outputs, launches of the tangent sweep, the case)"""
    old = {s: os.environ.get(s) for s in SWITCHES}
    for s in SWITCHES:
        os.environ.pop(s, None)
    if switch is not None:
        os.environ[switch] = value
    try:
        c = make_case()
    finally:
        for s in SWITCHES:
            if old[s] is None:
                os.environ.pop(s, None)
            else:
                os.environ[s] = old[s]
    names, T, P = _names_and_state(c)
    for n in names:
        c.dy.put(n, T[n], 0); c.dy.put(n, P[n], 1)
    l0 = c.dy.launch_count()
    c.dy.step_tl()
    l_tl = c.dy.launch_count() - l0
    out = {("tl", n, w): c.dy.get(n, w).copy() for n in names for w in (0, 1)}
    rng = np.random.default_rng(5)
    for n in names:
        c.dy.put(n, T[n], 0)
    c.dy.step_nl()
    for n in names:
        c.dy.put(n, rng.standard_normal(c.dy.shape(n)), 1)
    c.dy.step_ad()
    out.update({("ad", n, 1): c.dy.get(n, 1).copy() for n in names})
    return out, l_tl, c


def check_fused_equals_staged(key, make_case, switch, rtol=0.0):
    """rtol = 0 (host emulation): step_tl bit for bit, step_ad to 1e-13 of the field maximum.  rtol > 0 (device): every output to rtol of
    the field maximum.  key names the case and its backend (the default run is kept per key).  Returns the worst relative difference."""
    assert switch in SWITCHES
    if key not in _default_runs:
        _default_runs[key] = run_steps(make_case)[:2]
    a, la = _default_runs[key]
    b, lb, _ = run_steps(make_case, switch, "0")
    print("%s %s: %d launches in the tangent sweep fused, %d staged" % (key, switch, la, lb))
    assert la < lb, (la, lb)      # the fused form is what ran: one launch in place of several in the tangent sweep
    worst = 0.0
    for k in a:
        assert np.isfinite(a[k]).all() and np.abs(a[k]).max() > 0, k
        if rtol == 0.0 and k[0] != "ad":
            assert np.array_equal(a[k], b[k]), k
            continue
        e = float(np.max(np.abs(a[k] - b[k])) / np.max(np.abs(b[k])))
        print("%s fused vs staged %s: %.3e" % (switch, k, e))
        assert e <= (1e-13 if rtol == 0.0 else rtol), (k, e)
        worst = max(worst, e)
    return worst
