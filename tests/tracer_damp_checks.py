"""Checks of the tracer damping of tracer_2d (fv3lm_set_tracer_damping), shared by the host-emulation and the -m gpu test files.
Reference: tracer_damp_oracle.Tracer2d, the oracle's per-level fv_tp_2d composed by the rules of the reference's call site.

Tolerances are the project's own (the users of groups.py): 1e-11 trajectory and tangent, 1e-10 adjoint, 1e-11 dot-product residual.
FLOOR: on the reference alone, a damped case must move the transported tracers by more than 1e-8 relative L-inf -- 10^3 times the
comparison tolerance -- or the comparison could not tell the damped operator from the undamped one."""
import numpy as np
from oracle import NL, TL, AD
from common import relerr
from groups import _dyn_outputs, masked
import tracer_damp_oracle as TO

TOL_TL, TOL_AD, TOL_DOT, FLOOR = 1e-11, 1e-10, 1e-11, 1e-8
SPLIT = dict(hord_tr=8, hord_tr_pert=333)

# name -> (option keywords of the case, arguments of fv3lm_set_tracer_damping, a damped case?)
SETS = {
    "equal_nord0": ({}, dict(nord_tr=0, trdm2=0.05, nord_tr_pert=0, trdm2_pert=0.0, split_damp_tr=1), True),
    "equal_nord1": ({}, dict(nord_tr=1, trdm2=0.15, nord_tr_pert=0, trdm2_pert=0.0, split_damp_tr=1), True),
    "split_nord2": (SPLIT, dict(nord_tr=2, trdm2=0.15, nord_tr_pert=1, trdm2_pert=0.1, split_damp_tr=1), True),
    "split_pert_off": (SPLIT, dict(nord_tr=1, trdm2=0.15, nord_tr_pert=1, trdm2_pert=5e-5, split_damp_tr=1), True),
    "traj_off": (SPLIT, dict(nord_tr=1, trdm2=5e-5, nord_tr_pert=1, trdm2_pert=0.1, split_damp_tr=1), False),
    "no_split_damp": ({}, dict(nord_tr=0, trdm2=0.05, nord_tr_pert=1, trdm2_pert=0.15, split_damp_tr=0), True),
}


def inputs(c, scale=1.0):
    """dp1 mfx mfy cx cy q*: realistic fluxes from the oracle's dyn_core, as groups.check_tracer takes them (once per case and scale)"""
    key = ("tracer_damp_inputs", scale)
    if key not in c.__dict__:
        T, P = _dyn_outputs(c)
        T = {n: scale * T[n] for n in ("mfx", "mfy", "cx", "cy")}; P = {n: scale * P[n] for n in ("mfx", "mfy", "cx", "cy")}
        T["dp1"], P["dp1"] = c.traj["delp"][0], c.pert["delp"][0]
        for n in range(c.nq):
            T["q%d" % (n + 1)], P["q%d" % (n + 1)] = c.qtraj[n][0], c.qpert[n][0]
        c.__dict__[key] = (T, P)
    return c.__dict__[key]


def names(c):
    return ["dp1", "mfx", "mfy", "cx", "cy"] + ["q%d" % (n + 1) for n in range(c.nq)]


def seeds_of(c):
    rng = np.random.default_rng(21)
    return [masked(c, rng.standard_normal((c.npz, c.ny + 7, c.nx + 7)), "A") for _ in range(c.nq)]


def check_composition(c, scale=1.0):
    """damping off: the composition is the oracle's tracer_2d, to 1e-13 (values, tangent, adjoint on whole planes)"""
    T, P = inputs(c, scale)
    ins = names(c)
    t2 = TO.Tracer2d(c, TO.OFF)
    q, qp, nsplt = t2.forward(T, P)
    ot, op = c.oracle.tracer_2d(TL, c.nq, [T[n] for n in ins], [P[n] for n in ins])
    A = (Ellipsis,) + t2.A
    for n in range(c.nq):
        assert relerr(q[n][A], ot[n][A]) < 1e-13 and relerr(qp[n][A], op[n][A]) < 1e-13, n
    sd = seeds_of(c)
    _, iad = c.oracle.tracer_2d(AD, c.nq, [T[n] for n in ins], None, sd)
    mine = t2.adjoint(T, sd)
    for n, a in zip(ins, iad):
        assert relerr(mine[n], a) < 1e-13, (n, relerr(mine[n], a))
    return nsplt


def reference_floor(c, dmp, scale=1.0):
    """on the reference alone: relative L-inf distance between the damped and the undamped transported tracers"""
    T, _ = inputs(c, scale)
    A = (Ellipsis,) + TO.Tracer2d(c).A
    q1, _, _ = TO.Tracer2d(c, TO.Damping(**dmp)).forward(T)
    q0, _, _ = TO.Tracer2d(c, TO.OFF).forward(T)
    return min(relerr(a[A], b[A]) for a, b in zip(q1, q0))


def run_product(c, mode, scale=1.0):
    """fv3lm_tracer_2d on the case's inputs.  TL: -> (q values, q tangents) on whole planes; AD: -> the input adjoints, whole planes"""
    T, P = inputs(c, scale)
    ins = names(c)
    for n in ins:
        c.dy.put(n, T[n][None], 0)
    if mode == TL:
        for n in ins:
            c.dy.put(n, P[n][None], 1)
        c.dy.tracer_2d(TL)
        return [c.dy.get("q%d" % (n + 1), 0)[0] for n in range(c.nq)], [c.dy.get("q%d" % (n + 1), 1)[0] for n in range(c.nq)]
    c.dy.tracer_2d(NL)            # the forward sweep stores the sub-step trajectory the adjoint replays
    for n in ins:
        c.dy.put(n, T[n][None], 0); c.dy.put(n, np.zeros(c.dy.shape(n)), 1)
    for n, s in enumerate(seeds_of(c)):
        c.dy.put("q%d" % (n + 1), s[None], 1)
    c.dy.tracer_2d(AD)
    return {n: c.dy.get(n, 1)[0] for n in ins}


def check_unit(c, dmp, mode, scale=1.0, damped=True, want_nsplt=None):
    """the product (damping already set on c) against the composed reference; the adjoint on whole padded planes, halo of dp1 included"""
    T, P = inputs(c, scale)
    ref = TO.Tracer2d(c, TO.Damping(**dmp))
    A = (Ellipsis,) + ref.A
    if damped:
        fl = reference_floor(c, dmp, scale)
        print("reference: damped vs undamped tracers differ by %.3e" % fl)
        assert fl > FLOOR, fl
    if mode == TL:
        q, qp, nsplt = ref.forward(T, P)
        if want_nsplt is not None:
            assert nsplt >= want_nsplt, nsplt
        gq, gp = run_product(c, TL, scale)
        for n in range(c.nq):
            e1, e2 = relerr(gq[n][A], q[n][A]), relerr(gp[n][A], qp[n][A])
            print("q%d traj %.3e tl %.3e" % (n + 1, e1, e2))
            assert e1 < TOL_TL, (n, "traj", e1)
            assert e2 < TOL_TL, (n, "tl", e2)
        return
    want = ref.adjoint(T, seeds_of(c))
    got = run_product(c, AD, scale)
    if damped and ref.d.traj[1] > 1e-4 and (c.opt.hord_tr == c.opt.hord_tr_pert or ref.d.pert[1] > 1e-4):
        H = np.ones(want["dp1"].shape, bool); H[A] = False
        assert np.abs(want["dp1"][H]).max() > 0., "the reference's dp1 adjoint has nothing in the halo: the damping did not read it"
    for n in names(c):
        e = relerr(got[n], want[n])
        print("%s ad %.3e" % (n, e))
        assert e < TOL_AD, (n, "ad", e)


def check_same_as(c, other, mode, scale=1.0):
    """two handles give the same bits"""
    a, b = run_product(c, mode, scale), run_product(other, mode, scale)
    if mode == TL:
        a = {"t%d" % n: x for n, x in enumerate(a[0])} | {"p%d" % n: x for n, x in enumerate(a[1])}
        b = {"t%d" % n: x for n, x in enumerate(b[0])} | {"p%d" % n: x for n, x in enumerate(b[1])}
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def launches(c, fn):
    n0 = c.lib.L.fv3lm_launch_count(c.dy.h); fn(); return c.lib.L.fv3lm_launch_count(c.dy.h) - n0


def check_off_state(make_case):
    """a handle that never called the setter against (a) one that set (1, 0.15) and then (1, 0.0), (b) one whose trajectory coefficient
    is below the threshold while the perturbation's is not: same bits, same launch counts -- tracer_2d in the three modes and a step"""
    from groups import dot_product_step
    base = make_case()
    assert base.dy.tracer_damping() == ((0, 0.0), (0, 0.0))
    a = make_case(); a.dy.set_tracer_damping(1, 0.15, 0, 0.0, 1); a.dy.set_tracer_damping(1, 0.0, 0, 0.0, 1)
    b = make_case(); b.dy.set_tracer_damping(1, 5e-5, 1, 0.1, 1)
    for other in (a, b):
        for mode in (TL, AD):
            for scale in (1.0, 10.0):
                want = []; got = []
                nb = launches(base, lambda: want.append(run_product(base, mode, scale)))
                no = launches(other, lambda: got.append(run_product(other, mode, scale)))
                assert nb == no, (mode, scale, nb, no)
                x, y = want[0], got[0]
                if mode == TL:
                    x = dict(enumerate(x[0] + x[1])); y = dict(enumerate(y[0] + y[1]))
                for k in x:
                    assert np.array_equal(x[k], y[k]), (mode, scale, k)
        r0 = []; r1 = []
        nb = launches(base, lambda: r0.append(dot_product_step(base)))
        no = launches(other, lambda: r1.append(dot_product_step(other)))
        assert nb == no and r0 == r1, (nb, no, r0, r1)


REFUSALS = [
    ((0, float("nan"), 0, 0.0, 1), "finite"), ((0, 0.1, 0, float("inf"), 1), "finite"),
    ((0, -0.1, 0, 0.0, 1), "negative"), ((0, 0.1, 0, -1.0, 1), "negative"),
    ((0, 0.1, 0, 0.1, 2), "split_damp_tr must be 0 or 1"), ((0, 0.1, 0, 0.1, -1), "split_damp_tr must be 0 or 1"),
    ((0, 0.1, 2, 0.1, 1), "nord_tr_pert must be 0 or 1"), ((0, 0.1, -1, 0.1, 1), "nord_tr_pert must be 0 or 1"),
    ((3, 0.1, 0, 0.1, 1), "nord_tr must be 0, 1 or 2"), ((-1, 0.1, 0, 0.1, 1), "nord_tr must be 0, 1 or 2"),
    ((2, 0.1, 0, 0.1, 1), "nord_tr = 2 needs hord_tr != hord_tr_pert"),
]


def check_refusals(c):
    """c: equal schemes, damping set to (1, 0.15) / (0, 0.05): every refusal by its message, the getter unchanged after each"""
    import pytest
    from fv3_jedi_linearmodel_amd._lib import Fv3LmError
    before = c.dy.tracer_damping()
    assert before == ((1, 0.15), (0, 0.05))
    for args, msg in REFUSALS:
        with pytest.raises(Fv3LmError, match=msg):
            c.dy.set_tracer_damping(*args)
        assert c.dy.tracer_damping() == before, args


def check_step_traj(damped, off):
    """after step_tl the trajectory tracers are those after step_nl; and the damping is felt by the step"""
    from fv3_jedi_linearmodel_amd.harness import step_state
    out = {}
    for c in (damped, off):
        T, P = step_state(c)
        nm = ["u", "v", "pt", "delp"] + ["q%d" % (n + 1) for n in range(c.nq)]
        for n in nm:
            c.dy.put(n, T[n][None], 0); c.dy.put(n, P[n][None], 1)
        c.dy.step_tl()
        tl = [c.dy.get("q%d" % (n + 1), 0) for n in range(c.nq)]
        for n in nm:
            c.dy.put(n, T[n][None], 0)
        c.dy.step_nl()
        nl = [c.dy.get("q%d" % (n + 1), 0) for n in range(c.nq)]
        A = c.rect(1, c.nx, 1, c.ny)
        for a, b in zip(tl, nl):       # the same formulas on dual numbers and on doubles: equal to rounding, held to the trajectory tolerance
            e = relerr(a[A], b[A])
            print("step_tl vs step_nl trajectory %.3e" % e)
            assert e < TOL_TL, e
        out[c] = [a[A] for a in nl]
    d = min(relerr(a, b) for a, b in zip(out[damped], out[off]))
    print("step: damped vs undamped tracers differ by %.3e" % d)
    assert d > FLOOR, d


def check_later_substeps_launch_nothing(make_case):
    """the damping stages run in the first sub-step only: what a damped handle launches beyond an undamped one does not grow with the
    number of sub-steps"""
    off, on = make_case(), make_case(nord_tr=1, trdm2=0.15, nord_tr_pert=0, trdm2_pert=0.0, split_damp_tr=1)
    extra = {}
    for mode in (TL, AD):
        for scale in (1.0, 10.0):
            extra[mode, scale] = launches(on, lambda: run_product(on, mode, scale)) - launches(off, lambda: run_product(off, mode, scale))
        assert extra[mode, 1.0] > 0 and extra[mode, 10.0] == extra[mode, 1.0], extra
    assert off.dy.lib.L.fv3lm_tracer_nsplt(off.dy.h) > 1


def measure(c, runs=3):
    """HIP-event time (ms) of fv3lm_tracer_2d in the tangent and the adjoint mode: median of `runs` profiled calls after one warm-up.
    The fluxes are the library's own dyn_core's; no reference is involved."""
    c.put_state(pert=c.pert)
    for n in range(c.nq):
        c.dy.put("q%d" % (n + 1), c.qtraj[n], 0); c.dy.put("q%d" % (n + 1), c.qpert[n], 1)
    c.dy.dyn_core(TL)
    c.dy.put("dp1", c.traj["delp"], 0); c.dy.put("dp1", c.pert["delp"], 1)
    keep = {n: (c.dy.get(n, 0), c.dy.get(n, 1)) for n in names(c)}
    out = {}
    for mode in (TL, AD):
        t = []
        for r in range(runs + 1):
            for n, (a, b) in keep.items():
                c.dy.put(n, a, 0); c.dy.put(n, b, 1)
            if mode == AD:
                c.dy.tracer_2d(NL)
                for n, (a, b) in keep.items():
                    c.dy.put(n, a, 0)
            c.dy.sync(); c.dy.profile_begin()
            c.dy.tracer_2d(mode)
            t.append(sum(v[1] for v in c.dy.profile_end().values()))
        out[mode] = float(np.median(t[1:]))
    return out
