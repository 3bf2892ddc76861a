"""The wind conversion of c_sw with its intermediates kept out of memory, against the staged launches it replaces.  The switch is read
where the programs are built:

FV3LM_D2A2C_FUSED=0      the bulk of d2a2c_vect as CswInterpA + CswInterpC (utmp, vtmp through memory) instead of the one LDS-tiled
                         launch of csrc/d2a2c.h.

Nonlinear and tangent run the staged arithmetic in its order, so the step_tl outputs (trajectory and tangent of every prognostic field)
must agree BIT FOR BIT in the host emulation; the adjoint sums in another order, so the step_ad outputs agree to 1e-13 of the field
maximum.  On the device the two forms are different kernels and hipcc contracts a*b+c per kernel: rtol 1e-12 there.

The cases are those of a2b_fused_checks.py: the smallest that cut a tile into several 64 x 16 blocks both ways and reach every special
region.  The fused run of a case is kept and shared by every comparison against it."""
import os
import numpy as np
from a2b_fused_checks import _names_and_state

SWITCHES = ("FV3LM_D2A2C_FUSED",)
_fused_runs = {}


def run_steps(make_case, off=None):
    """step_tl outputs (values and tangent) and step_ad outputs of one model built with the fused form (off=None) or with the switch
    `off` set to 0; -> (outputs, launches of the tangent sweep)"""
    old = {s: os.environ.get(s) for s in SWITCHES}
    for s in SWITCHES:
        os.environ.pop(s, None)
    if off is not None:
        os.environ[off] = "0"
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
    return out, l_tl


def check_fused_equals_staged(key, make_case, switch, rtol=0.0):
    """rtol = 0 (host emulation): step_tl bit for bit, step_ad to 1e-13 of the field maximum.  rtol > 0 (device): every output to rtol of
    the field maximum.  key names the case (the fused run is kept per key).  Returns the worst relative difference."""
    assert switch in SWITCHES
    if key not in _fused_runs:
        _fused_runs[key] = run_steps(make_case)
    a, la = _fused_runs[key]
    b, lb = run_steps(make_case, off=switch)
    print("%s %s: %d launches in the tangent sweep fused, %d staged" % (key, switch, la, lb))
    assert la < lb, (la, lb)      # the fused form is what ran: one launch in place of two per d2a2c_vect in the tangent sweep
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
