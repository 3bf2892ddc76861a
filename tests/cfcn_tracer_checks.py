"""Checks of the convective cloud fraction carried through the dynamics as a tracer (fv3lm_cloud_bind_cfcn; product csrc/cloud.h,
csrc/physics.h, csrc/model.h) shared by the host-emulation (test_emul_cfcn_tracer.py) and the MI355X (test_gpu_cfcn_tracer.py) runs.

With do_phy_mst /= 0 the reference's dycore has five tracers and the fifth is cfcn, trajectory and perturbation
(fv3jedi_lm_dynamics_mod.F90:159-163, :769, :831, :878, :912); ipert_to_zero (fv3jedi_lm_mod.F90:242-253) clears the perturbation before
and after a step and nothing clears it in between.  A bound handle does the same on the device.  The yardstick of check 1 is a second
handle that never binds and does by hand what the reference's arrays do: cfcn goes between tracer 4 and the cloud feature's own array
through the host, in the reference's order of the parts.

The state: the L40m2 soundings of tests/golden/cloud_ref.npz dealt over the periodic 12 x 10 tile (on L20 the cloud scheme's level loop,
which starts at level 30, never runs and cfcn cannot act), nq = 4 = qv qi ql cfcn, n_split = 2, the fixture's dt, two trajectory
times (two deals); the trajectory of tracer 4 is the fixture's cfcn.  The six-face case is CubeCase(n = 8) on the same fixture.

FLOOR, the "differ" of check 2: the largest difference between the bound and the unbound composed step, relative to the bound field's
largest value, measured once on the host emulation -- tangent 1.39e-3 (ql; T 5.7e-5, qv 2.8e-4, qi 0), adjoint 9.06e-4 (v; u 8.3e-4, delp 1.5e-4) -- and a tenth
of each asserted; the emulation and the device differ by contraction only."""
import numpy as np
import turbulence_checks as TC
import cloud_checks as KC
import lm_checks as LM

NL, TL, AD = 0, 1, 2
TAG = "L40m2"
IQC = 4
QC = "q%d" % IQC
MEASURED = {TL: 1.39e-3, AD: 9.06e-4}
FLOOR = {m: 0.1 * v for m, v in MEASURED.items()}
MOIST = ("pt", "q1", "q%d" % KC.IQI, "q%d" % KC.IQL)
WINDS = ("u", "v", "delp")


def tile_kw(size=(12, 10), **kw):
    fx = KC.fixture(TAG)
    return dict(nx=size[0], ny=size[1], npz=fx["lm"], n_split=2, dt=fx["dt"], nq=4, oracle=False, **KC.case_kw(fx), **kw)


def cube_kw(**kw):
    fx = KC.fixture(TAG)
    return dict(n=8, npz=fx["lm"], n_split=2, k_split=1, dt=fx["dt"], nq=4, **KC.case_kw(fx), **kw)


def times(c, nslots=2):
    """per slot what lm_checks.moist_times gives, on the L40m2 fixture and with the fixture's cfcn as the trajectory of tracer 4; the
    perturbation and the forcing carry nothing in tracer 4 (a step clears it first)"""
    fx = KC.fixture(TAG)
    out = []
    for s in range(nslots):
        T, sfc, cl, k = KC.placed(c, fx, KC.dealt(c, LM.SHIFTS[s]))
        T[QC] = KC.pad(c, cl[2])
        if not c.opt.hydrostatic:      # the hydrostatic thickness of the same state and a small smooth w (lm_checks.two_states)
            o = c.opt
            pe = np.concatenate([np.full_like(T["delp"][:, :1], o.ptop), o.ptop + np.cumsum(T["delp"], axis=1)], axis=1)
            T["delz"] = -(o.rdgas / o.grav) * T["pt"] * (1.0 + o.zvir * T["q1"]) * np.diff(np.log(pe), axis=1)
            T["w"] = 0.01 * T["u"]
        (P, cf, _), (PA, cfa) = KC.forcing(c, fx, k)
        P[QC][:] = 0.0; PA[QC][:] = 0.0
        out.append(dict(traj=LM.compact(c, T), phis=LM.phis_of(c, 1.0 + 0.1 * s), sfc=sfc, cl=cl, diag=TC.generated(c, seed=29 + s),
                        P=LM.compact(c, P), PA=LM.compact(c, PA)))
    return out


def prepare(c, ts, bind):
    """the three features and the trajectory store; bind: cfcn is tracer 4 and the slots take it from the resident trajectory"""
    fx = KC.fixture(TAG)
    n = len(ts)
    KC.ensure_created(c, fx, n)
    if bind:
        c.dy.cloud_bind_cfcn(IQC)
    TC.ensure_created(c, n)
    c.dy.lm_create(n, 1, 1, 1)
    for s, t in enumerate(ts):
        LM.upload(c, t)
        c.dy.convection_set(s, *t["sfc"])
        c.dy.cloud_set(s, *(t["cl"][:2] + [None] + t["cl"][3:] if bind else t["cl"]))
        c.dy.turbulence_set_diagonals(s, t["diag"])
        c.dy.lm_traj_save(s)
    return c


class World:
    """one bound handle (lm) and one that never binds (parts), both with the two times set; made once for a backend and a case"""
    _made = {}

    def __init__(self, make, parts):
        self.lm = make()
        self.times = times(self.lm)
        prepare(self.lm, self.times, True)
        self.parts = prepare(make(), self.times, False) if parts else None

    @classmethod
    def get(cls, make, key, parts=True):
        if key not in cls._made:
            cls._made[key] = cls(make, parts)
        return cls._made[key]


def zero_both(c):
    c.dy.put(QC, np.zeros(c.dy.shape(QC)), 1)
    c.dy.cloud_cfcn(LM.zeros(c))


def host_tl(c, t, s):
    """the tangent of the reference's arrays on a handle that never binds: pert%cfcn = 0 -> qp(:,:,:,5) (pert_to_fv3), the dynamics,
    qp(:,:,:,5) -> pert%cfcn (fv3_to_pert), the moist half reads and updates pert%cfcn, turbulence, pert%cfcn = 0"""
    LM.upload(c, t)
    zero_both(c)
    c.dy.step_tl()
    c.dy.cloud_cfcn(TC.comp(c, c.dy.get(QC, 1)))
    c.dy.convection(s, TL); c.dy.cloud(s, TL); c.dy.turbulence(s, TL)
    zero_both(c)


def host_ad(c, t, s):
    """the adjoint: pert%cfcn = 0, turbulence, the cloud scheme leaves its adjoint in pert%cfcn, pert_to_fv3 puts it into qp(:,:,:,5)
    with a zero halo, the backward dynamics, pert%cfcn = 0"""
    zero_both(c)
    c.dy.turbulence(s, AD); c.dy.cloud(s, AD)
    c.dy.put(QC, KC.pad(c, c.dy.cloud_cfcn()) * inside(c), 1)
    c.dy.convection(s, AD)
    LM.upload(c, t)
    c.dy.step_nl(); c.dy.step_ad()
    zero_both(c)


def inside(c):
    m = np.zeros(c.dy.shape(QC)); m[TC.dom(c)] = 1.0
    return m


# ---- 1, 6: composed and bound equals the parts through the host, bit for bit
def check_composed_equals_host(w, s, mode):
    t, lm, pa = w.times[s], w.lm, w.parts
    P = t["P"] if mode == TL else t["PA"]
    lm.dy.pert_to_fv3(P)
    lm.dy.put(QC, 1e-3 * np.random.default_rng(5).standard_normal(lm.dy.shape(QC)), 1)      # a cfcn the step has to clear first
    lm.dy.lm_step(s, mode)
    got = LM.pert(lm)
    assert not np.any(got[QC]) and not np.any(lm.dy.cloud_cfcn()), "tracer 4 and fv3lm_cloud_cfcn have to read back zero after a step"
    pa.dy.pert_to_fv3(P)
    (host_tl if mode == TL else host_ad)(pa, t, s)
    ref = LM.pert(pa)
    assert not np.any(ref[QC]) and not np.any(pa.dy.cloud_cfcn())
    LM.same(got, ref, "bound composed step, mode %d, slot %d" % (mode, s))
    assert any(not np.array_equal(got[n][TC.dom(lm)], P[n]) for n in got)


# ---- 2: the coupling is there
def check_condition(w, s=0):
    """from the unbound parts alone: the dynamics turns a zero cfcn' into a non-zero one, and the cloud tangent given only that cfcn'
    moves T or qv in at least four columns"""
    t, pa = w.times[s], w.parts
    pa.dy.pert_to_fv3(t["P"])
    LM.upload(pa, t)
    zero_both(pa)
    pa.dy.step_tl()
    cf = TC.comp(pa, pa.dy.get(QC, 1))
    assert np.any(cf), "the dynamics left no tangent in a tracer that went in as zeros"
    pa.dy.pert_to_fv3({n: np.zeros_like(a) for n, a in t["P"].items()})
    pa.dy.convection_sources([LM.zeros(pa)] * 4)
    pa.dy.cloud_cfcn(cf)
    pa.dy.cloud(s, TL)
    moved = np.zeros(cf.shape[:1] + cf.shape[2:], dtype=bool)
    for n in ("pt", "q1"):
        moved |= np.any(pa.dy.get(n, 1)[TC.dom(pa)] != 0.0, axis=1)
    zero_both(pa)
    print("cfcn' after step_tl from zeros: max %.2e; columns whose T' or qv' the cloud tangent moves from that cfcn' alone: %d of %d"
          % (np.abs(cf).max(), int(moved.sum()), moved.size))
    assert moved.sum() >= 4, ("no column in which cfcn' alone moves T' or qv'", int(moved.sum()))
    return float(np.abs(cf).max()), int(moved.sum())


def check_coupling(w, mode, s=0):
    """the bound composed step against the unbound composed step of the same configuration"""
    t = w.times[s]
    P = t["P"] if mode == TL else t["PA"]
    res = []
    for c in (w.lm, w.parts):
        c.dy.pert_to_fv3(P)
        c.dy.lm_step(s, mode)
        res.append(LM.pert(c))
    names = MOIST if mode == TL else WINDS
    d = {n: float(np.abs(res[0][n] - res[1][n]).max() / np.abs(res[0][n]).max()) for n in names}
    print("bound against unbound composed step, mode %d: largest difference relative to the bound field's largest value %s; floor %.1e"
          % (mode, " ".join("%s %.2e" % kv for kv in d.items()), FLOOR[mode]))
    assert max(d.values()) >= FLOOR[mode], ("cfcn does not reach the other side of the dynamics", d)
    return d


# ---- 3, 6: the bound composed adjoint is the transpose of the bound composed tangent
def check_dot_product(w, slots=(0,)):
    res, x, full = LM.check_dot_product(w, slots)
    assert not np.any(full[QC])
    return res


# ---- 4: the trajectory side
def check_trajectory_side(make):
    fx = KC.fixture(TAG)
    b, u = make(), make()
    t = times(b, 1)[0]
    D = TC.dom(b)
    for c in (b, u):
        KC.ensure_created(c, fx, 2)
        LM.upload(c, t)
        for s in (0, 1):
            c.dy.convection_set(s, *t["sfc"])
    b.dy.cloud_bind_cfcn(IQC)
    half = np.ascontiguousarray(0.5 * t["cl"][2])
    flat = lambda r: [r[0][n] for n in KC.OUT8] + [r[1][n] for n in KC.FRAC] + [r[2]]
    # NULL takes the resident trajectory of tracer 4: the fixture's cfcn, then half of it
    b.dy.cloud_set(0, *(t["cl"][:2] + [None] + t["cl"][3:]))
    b.dy.cloud_set(1, *t["cl"])
    first = flat(b.dy.cloud_get(0))
    assert all(np.array_equal(x, y) for x, y in zip(first, flat(b.dy.cloud_get(1)))), "cfcn = NULL != the same array passed"
    b.dy.put(QC, KC.pad(b, half), 0)
    b.dy.cloud_set(0, *(t["cl"][:2] + [None] + t["cl"][3:]))
    b.dy.cloud_set(1, *(t["cl"][:2] + [half] + t["cl"][3:]))      # a non-NULL array is still used, whatever the tracer holds
    second = flat(b.dy.cloud_get(0))
    assert all(np.array_equal(x, y) for x, y in zip(second, flat(b.dy.cloud_get(1))))
    assert any(not np.array_equal(x, y) for x, y in zip(first, second)), "the slot does not follow the trajectory of tracer 4"
    b.dy.put(QC, b.dy.get(QC, 0) + 7.0, 0)
    b.dy.cloud_set(1, *t["cl"])
    assert all(np.array_equal(x, y) for x, y in zip(first, flat(b.dy.cloud_get(1)))), "an explicit cfcn has to win over the tracer"
    # mode 0: CF_con into the trajectory of tracer 4 inside is..ie x js..je, nothing outside; unbound: tracer 4 is left alone
    u.dy.cloud_set(0, *t["cl"])
    rng = np.random.default_rng(11)
    for c, slot in ((b, 1), (u, 0)):
        before = rng.random(c.dy.shape(QC))
        c.dy.put(QC, before, 0)
        pert = {n: c.dy.get(n, 1) for n in TC.all_names(c)}
        c.dy.cloud(slot, NL)
        after = c.dy.get(QC, 0)
        cfcon = c.dy.cloud_get(slot, frac=False, pertmod=False)[0]["CF_con"]
        assert np.any(cfcon > 0), "no convective cloud: the check is empty"
        if c is b:
            assert np.array_equal(after[D], cfcon), "the trajectory of tracer 4 != CF_con"
            keep = after.copy(); keep[D] = before[D]
            assert np.array_equal(keep, before), "the trajectory of tracer 4 moved outside is..ie x js..je"
        else:
            assert np.array_equal(after, before), "unbound, mode 0 has to leave tracer 4 alone"
        assert all(np.array_equal(c.dy.get(n, 1), a) for n, a in pert.items())
    # fv3lm_cloud_cfcn, bound: is..ie x js..je of the tracer's perturbation
    cf = 0.05 * rng.standard_normal(TC.cshape(b))
    b.dy.put(QC, rng.standard_normal(b.dy.shape(QC)), 1)
    b.dy.cloud_cfcn(cf)
    assert np.array_equal(b.dy.get(QC, 1), KC.pad(b, cf) * inside(b)) and np.array_equal(b.dy.cloud_cfcn(), cf)


# ---- 5: refusals of the new call, by message; after each the perturbation is unchanged and the handle still steps
def check_refusals(make):
    import pytest
    from fv3_jedi_linearmodel_amd._lib import Fv3LmError
    fx = KC.fixture(TAG)
    c = make()
    t = times(c, 1)[0]
    LM.upload(c, t); c.dy.pert_to_fv3(t["P"])
    P0 = LM.pert(c)

    def refused(match, iqc):
        with pytest.raises(Fv3LmError, match=match):
            c.dy.cloud_bind_cfcn(iqc)
        assert all(np.array_equal(a, P0[n]) for n, a in LM.pert(c).items()), "a refused call moved the perturbation"
        c.dy.step_tl()
        assert all(np.all(np.isfinite(a)) for a in LM.pert(c).values())
        LM.upload(c, t); c.dy.pert_to_fv3(t["P"])
    refused("fv3lm_cloud_bind_cfcn: call fv3lm_cloud_create first", IQC)
    KC.ensure_created(c, fx, 1)
    for iqc in (1, 5, 0, -1):
        refused("iqc = -?[0-9] outside 2..nq = 2..4", iqc)
    refused("iqc = 2 is the tracer of cloud ice", KC.IQI)
    refused("iqc = 3 is the tracer of cloud liquid", KC.IQL)
    c.dy.cloud_bind_cfcn(IQC)
    refused("already bound to tracer 4", IQC)
    # the bound handle works: a slot from the tracer, a composed step
    TC.ensure_created(c, 1); c.dy.lm_create(1, 1, 1, 1)
    c.dy.convection_set(0, *t["sfc"]); c.dy.cloud_set(0, *(t["cl"][:2] + [None] + t["cl"][3:]))
    c.dy.turbulence_set_diagonals(0, t["diag"]); c.dy.lm_traj_save(0)
    c.dy.lm_step(0, TL)
    assert all(np.all(np.isfinite(a)) for a in LM.pert(c).values())
    # a trajectory cfcn that is not finite is seen by the gather: the slot is left unset
    good = c.dy.get(QC, 0)
    bad = good.copy(); bad[0, 33, TC.NG + 2, TC.NG + 1] = float("nan")
    c.dy.put(QC, bad, 0)
    with pytest.raises(Fv3LmError, match="not finite in the resident trajectory"):
        c.dy.cloud_set(0, *(t["cl"][:2] + [None] + t["cl"][3:]))
    with pytest.raises(Fv3LmError, match="never set"):
        c.dy.cloud(0, TL)
    c.dy.put(QC, good, 0)
    c.dy.cloud_set(0, *(t["cl"][:2] + [None] + t["cl"][3:]))
    c.dy.cloud(0, TL)
    # a handle whose slot has been set
    c = make()
    LM.upload(c, t); c.dy.pert_to_fv3(t["P"])
    P0 = LM.pert(c)
    KC.ensure_created(c, fx, 1)
    c.dy.convection_set(0, *t["sfc"])
    with pytest.raises(Fv3LmError, match="null array"):      # unbound, cfcn = NULL stays refused
        c.dy.cloud_set(0, *(t["cl"][:2] + [None] + t["cl"][3:]))
    c.dy.cloud_set(0, *t["cl"])
    refused("a cloud slot has been set", IQC)
    c.dy.cloud(0, TL)
