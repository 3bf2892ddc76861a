"""Checks of the composed model step (fv3lm_lm_create / _lm_traj_save / _lm_traj_load / _lm_step; product csrc/model.h) shared by the
host-emulation (test_emul_lm.py) and the MI355X (test_gpu_lm.py, test_gpu_lm_shim.py) runs.

The yardstick is the library's own parts in the reference's order (src/fv3jedi_lm_mod.F90:161-187, fv3jedi_lm_physics_mod.F90:121-122,
:137-138), driven through the entry points the earlier tests tie to the reference one by one: a composed step must equal them bit for
bit, and the order is pinned by a sequence with the two physics halves swapped, which has to differ.  The moist state is the one
physics_shim_checks.py and physics_launch_checks.py use (the L20 soundings of tests/golden/cloud_ref.npz dealt over the periodic
12 x 10 tile, cloud_checks.placed / forcing); the turbulence slot takes the generated diffusion-shaped diagonals of
turbulence_checks.generated, whose multipliers are well above 1.  Two times of a window are two deals of the soundings (shift 0 and 5).

BOUND, the dot-product bound of the whole step: the loosest one the dot-product tests of the parts use -- 1e-12 for convection, cloud
and turbulence (convection_checks, cloud_checks, turbulence_checks) and for the dynamics' step on one tile, 1e-11 for the dynamics' step
with the Rayleigh damping on a tile and on six faces (test_emul_rayleigh.py, test_gpu_parity.py).  A composition of exact transposes
is an exact transpose, so nothing looser."""
import os
import numpy as np
import turbulence_checks as TC
import cloud_checks as KC

NL, TL, AD = 0, 1, 2
TAG = "L20m1"
BOUND = 1e-11
SHIFTS = (0, 5)
PRESSURES = ("pe", "peln", "pk", "pkz")


def tile_kw(size=(12, 10)):
    fx = KC.fixture(TAG)
    return dict(nx=size[0], ny=size[1], npz=fx["lm"], n_split=2, dt=1800.0, nq=3, oracle=False, **KC.case_kw(fx))


def compact(c, D):
    return {n: TC.comp(c, D[n]) for n in TC.all_names(c)}


def phis_of(c, scale=1.0):
    return np.ascontiguousarray(scale * c.phis[:, TC.NG:TC.NG + c.ny, TC.NG:TC.NG + c.nx])


def upload(c, t):
    """the upload path: fv3lm_traj_to_fv3 of the time's compact arrays"""
    c.dy.traj_to_fv3({**t["traj"], "phis": t["phis"]})


# ---- the times of a window on the moist tile
def moist_times(c, nslots=2):
    """per slot: the compact trajectory and phis, the arguments of the three physics sets, a tangent perturbation and an adjoint forcing
    (fields compact, cfcn)"""
    fx = KC.fixture(TAG)
    out = []
    for s in range(nslots):
        T, sfc, cl, k = KC.placed(c, fx, KC.dealt(c, SHIFTS[s]))
        (P, cf, _), (PA, cfa) = KC.forcing(c, fx, k)
        out.append(dict(traj=compact(c, T), phis=phis_of(c, 1.0 + 0.1 * s), sfc=sfc, cl=cl, diag=TC.generated(c, seed=29 + s),
                        P=compact(c, P), cf=cf, PA=compact(c, PA), cfa=cfa))
    return out


def prepare(c, times, flags=(1, 1, 1), lm=True):
    """create the features of the flags and set slot s of each from time s while its trajectory is resident, as a host does"""
    fx = KC.fixture(TAG)
    n = len(times)
    if flags[2]:
        KC.ensure_created(c, fx, n)
    if flags[1]:
        TC.ensure_created(c, n)
    if lm:
        c.dy.lm_create(n, *flags)
    for s, t in enumerate(times):
        upload(c, t)
        if flags[2]:
            c.dy.convection_set(s, *t["sfc"]); c.dy.cloud_set(s, *t["cl"])
        if flags[1]:
            c.dy.turbulence_set_diagonals(s, t["diag"])
        if lm:
            c.dy.lm_traj_save(s)
    return c


def pert(c):
    return {n: c.dy.get(n, 1) for n in TC.all_names(c)}


def same(got, ref, what):
    assert list(got) == list(ref)
    for n in got:
        assert np.all(np.isfinite(got[n])), (what, n, "not finite")
        assert np.array_equal(got[n], ref[n]), (what, n, "composed step != parts", TC.relerr(got[n], ref[n]))


def zeros(c):
    return np.zeros(TC.cshape(c))


def parts_tl(c, t, s, flags=(1, 1, 1), swapped=False):
    """the explicit sequence of the tangent in the reference's order; swapped: the two physics halves the other way round"""
    if flags[0]:
        upload(c, t)
    if flags[2]:
        c.dy.cloud_cfcn(zeros(c))
    if flags[0]:
        c.dy.step_tl()
    moist = lambda: (c.dy.convection(s, TL), c.dy.cloud(s, TL))
    turb = lambda: c.dy.turbulence(s, TL)
    for part, on in ((turb, flags[1]), (moist, flags[2])) if swapped else ((moist, flags[2]), (turb, flags[1])):
        if on:
            part()


def parts_ad(c, t, s, flags=(1, 1, 1)):
    if flags[2]:
        c.dy.cloud_cfcn(zeros(c))
    if flags[1]:
        c.dy.turbulence(s, AD)
    if flags[2]:
        c.dy.cloud(s, AD); c.dy.convection(s, AD)
    if flags[0]:
        upload(c, t)
        c.dy.step_nl(); c.dy.step_ad()      # the dynamics' step_ad: forward sweep with the checkpoints, backward sweep


class World:
    """one composed handle and one handle for the parts, both with the two times set; made once for a backend and a size"""
    _made = {}

    def __init__(self, make, size, flags):
        self.lm, self.parts = make(**tile_kw(size)), make(**tile_kw(size))
        self.times = moist_times(self.lm)
        self.flags = flags
        prepare(self.lm, self.times, flags)
        prepare(self.parts, self.times, flags, lm=False)

    @classmethod
    def get(cls, make, key, size=(12, 10), flags=(1, 1, 1)):
        k = (key, size, flags)
        if k not in cls._made:
            cls._made[k] = cls(make, size, flags)
        return cls._made[k]


def check_state_acts(w, s):
    """some columns convect, and the turbulence systems are not the identity: otherwise the state cannot tell the orders apart"""
    dc = w.lm.dy.convection_get(s, jac=False)[1]
    assert set(np.unique(dc)) == {0, 1} and dc.sum() > 0, "DOCONVEC has no ones"
    fac = w.lm.dy.turbulence_get(s)
    for sys_ in range(3):      # the multipliers and the upper diagonal of an identity are zero
        assert np.abs(fac[3 * sys_]).max() > 1.0 and np.abs(fac[3 * sys_ + 2]).max() > 1.0, ("turbulence system %d is near the identity" % sys_)
    return int(dc.sum())


# ---- 1: load equals upload
def two_states(c):
    """two trajectories of any case (tile or cube, hydrostatic or not) with their own phis, and a perturbation random on the whole plane"""
    A, P = TC.unit_state(c, seed=3)
    B = {n: a * 1.02 + (1.5 if n == "pt" else 0.0) for n, a in A.items()}
    if not c.opt.hydrostatic:      # the hydrostatic thickness of the same state and a small smooth w
        o = c.opt
        for S in (A, B):
            pe = np.concatenate([np.full_like(S["delp"][:, :1], o.ptop), o.ptop + np.cumsum(S["delp"], axis=1)], axis=1)
            S["delz"] = -(o.rdgas / o.grav) * S["pt"] * (1.0 + o.zvir * (S["q1"] if c.nq else 0.0)) * np.diff(np.log(pe), axis=1)
            S["w"] = 0.01 * S["u"]
    return [dict(traj=compact(c, A), phis=phis_of(c)), dict(traj=compact(c, B), phis=phis_of(c, 1.1))], P


def check_load_equals_upload(make):
    """traj_to_fv3(A), save 0; traj_to_fv3(B), save 1; step_tl (the resident trajectory advances); load 0: every trajectory field
    fv3lm_field_get reads equals, bit for bit, what a fresh handle holds after traj_to_fv3(A) -- the prognostics and phis on their whole
    padded planes, halos and edge rows included, the pressures pe peln pk pkz on is..ie x js..je, where traj_to_fv3 computes them: it leaves
    their halos as the last step left them, on any handle.  So a twin handle goes through the same calls with an upload where the first
    loads, and there the whole planes of every field, pressures included, are equal.  Then load 1 and load 0 again.  Neither call touches
    the perturbation."""
    c, twin, fresh = make(), make(), make()
    (A, B), P = two_states(c)
    names = TC.all_names(c) + ["phis"] + list(PRESSURES)
    c.dy.lm_create(2, 1, 0, 0)
    for h in (c, twin):
        upload(h, A)
        for n in TC.all_names(c):
            h.dy.put(n, P[n], 1)
        if h is c:
            c.dy.lm_traj_save(0)
        upload(h, B)
    c.dy.lm_traj_save(1)
    assert all(np.array_equal(a, P[n]) for n, a in pert(c).items()), "the perturbation moved in a save"
    upload(fresh, B)
    for h in (c, twin):
        h.dy.step_tl()
    moved = [n for n in names if not np.array_equal(c.dy.get(n, 0), fresh.dy.get(n, 0))]
    assert all(n in moved for n in ("u", "pt", "delp", "pe", "pkz")), ("step_tl has to advance the resident trajectory", moved)
    before = pert(c)
    phis = []
    D = TC.dom(c)
    for slot, t in ((0, A), (1, B), (0, A)):
        c.dy.lm_traj_load(slot)
        upload(twin, t); upload(fresh, t)
        for n in names:
            a, b, f = c.dy.get(n, 0), twin.dy.get(n, 0), fresh.dy.get(n, 0)
            assert np.array_equal(a, b), (slot, n, "load != upload on a handle of the same history", TC.relerr(a, b))
            w = D if n in PRESSURES else Ellipsis
            assert np.array_equal(a[w], f[w]), (slot, n, "load != upload on a fresh handle", TC.relerr(a[w], f[w]))
            assert np.all(np.isfinite(a)) and np.any(a != 0), (slot, n)
        phis.append(c.dy.get("phis", 0))
    assert all(np.array_equal(a, before[n]) for n, a in pert(c).items()), "the perturbation moved in a load"
    assert not np.array_equal(phis[0], phis[1]) and np.array_equal(phis[0], phis[2]), "the two times have to differ in phis"


# ---- 2, 7: the composed tangent equals its parts in the reference's order, and not in the other
def check_tangent(w, s=0, batches=False):
    t, lm, pa = w.times[s], w.lm, w.parts
    active = check_state_acts(w, s)
    lm.dy.pert_to_fv3(t["P"]); lm.dy.cloud_cfcn(t["cf"])      # a cfcn the step has to clear (ipert_to_zero)
    lm.dy.lm_step(s, TL)
    got, cf = pert(lm), lm.dy.cloud_cfcn()
    assert np.any(t["cf"]) and not np.any(cf), "the cfcn given before the step has to read back zero after it"
    pa.dy.pert_to_fv3(t["P"])
    parts_tl(pa, t, s)
    same(got, pert(pa), "tangent, slot %d" % s)
    pa.dy.pert_to_fv3(t["P"])
    parts_tl(pa, t, s, swapped=True)
    other = pert(pa)
    d = {n: float(np.abs(got[n] - other[n]).max() / np.abs(got[n]).max()) for n in got}
    print("turbulence before convection: largest difference relative to the field's largest value", " ".join("%s %.1e" % kv for kv in d.items()))
    assert max(d.values()) > 1e-6, ("the state cannot tell the two orders of the physics halves apart", d)
    if batches:
        nb = {}
        for name, fn in (("convection", lambda: pa.dy.convection(s, TL)), ("cloud", lambda: pa.dy.cloud(s, TL))):
            n0 = pa.dy.launch_count(); fn(); nb[name] = pa.dy.launch_count() - n0
        print("%d columns, %d of them active: launches %s" % (np.prod(TC.cshape(lm)) // lm.npz, active, nb))
        assert nb["convection"] >= 2 and nb["cloud"] >= 2, ("every scheme has to run more than one batch", nb, active)
    return d


# ---- 3: the composed adjoint equals its parts
def check_adjoint(w, s=0):
    t, lm, pa = w.times[s], w.lm, w.parts
    lm.dy.pert_to_fv3(t["PA"]); lm.dy.cloud_cfcn(t["cfa"])
    lm.dy.lm_step(s, AD)
    got = pert(lm)
    assert np.any(t["cfa"]) and not np.any(lm.dy.cloud_cfcn()), "the cfcn given before the step has to read back zero after it"
    pa.dy.pert_to_fv3(t["PA"])
    parts_ad(pa, t, s)
    same(got, pert(pa), "adjoint, slot %d" % s)
    assert any(not np.array_equal(got[n][TC.dom(lm)], t["PA"][n]) for n in got)


# ---- 4, 5: adjointness of one step and of a window of two times
def draw(c, seed):
    rng = np.random.default_rng(seed)
    amp = dict(u=1.0, v=1.0, pt=0.5, delp=10.0, q1=1e-4)
    return {n: amp.get(n, 1e-5) * rng.standard_normal(TC.cshape(c)) for n in TC.all_names(c)}


def check_dot_product(w, slots=(0,)):
    """<L x, y> = <x, L' y> with L the tangent steps at the slots in turn and L' the adjoint steps backwards, through lm_step only; x and
    y random in every perturbation field, on the compute domain the host sees (pert_to_fv3 / fv3_to_pert)"""
    c = w.lm
    names = TC.all_names(c)
    x = draw(c, 17)
    c.dy.pert_to_fv3(x)
    for s in slots:
        c.dy.lm_step(s, TL)
    full = pert(c)
    Lx = c.dy.fv3_to_pert(names)
    # y is drawn before the adjoint runs and kept only if the sum that gives lhs does not cancel by chance below 1e-3 of its terms (a
    # random sum of N terms sits near N^-1/2 of them, 8e-3 here): the bound is relative to lhs, and a draw that cancels five digits
    # deep measures the round-off of the sum (1e-16 of its terms), not the operator.  Nothing of the adjoint enters the choice.
    for seed in range(19, 27):
        rng = np.random.default_rng(seed)
        y = {n: rng.standard_normal(Lx[n].shape) / max(1e-30, float(np.abs(Lx[n]).max())) for n in names}
        lhs = sum(float(np.sum(Lx[n] * y[n])) for n in names)
        if abs(lhs) >= 1e-3 * sum(float(np.sum(np.abs(Lx[n] * y[n]))) for n in names):
            break
    else:
        raise AssertionError("no draw of y with a well-conditioned <L x, y>")
    c.dy.pert_to_fv3(y)
    for s in reversed(slots):
        c.dy.lm_step(s, AD)
    Lty = c.dy.fv3_to_pert(names)
    rhs = sum(float(np.sum(Lty[n] * x[n])) for n in names)
    res = abs(lhs - rhs) / abs(lhs)
    print("dot product over slots %s: %.16e %.16e residual %.1e (bound %.0e)" % (list(slots), lhs, rhs, res, BOUND))
    assert np.isfinite(lhs) and res <= BOUND, (lhs, rhs, res)
    return res, x, full


def check_window(w):
    """tangent at 0 then 1, adjoint at 1 then 0: the dot product, and the tangent against the same window run with uploads and per-part calls"""
    res, x, got = check_dot_product(w, (0, 1))
    pa = w.parts
    pa.dy.pert_to_fv3(x)
    for s in (0, 1):
        parts_tl(pa, w.times[s], s)
    same(got, pert(pa), "window of two times")
    return res


# ---- 6: subsets of the flags
def check_subset(make, key, flags):
    w = World.get(make, key, flags=flags)
    lm, pa = w.lm, w.parts
    for s in (1, 0):
        t = w.times[s]
        for mode, P, run in ((TL, t["P"], parts_tl), (AD, t["PA"], parts_ad)):
            upload(lm, w.times[1 - s])      # another time is resident
            before = {n: lm.dy.get(n, 0) for n in TC.all_names(lm) + ["phis"] + list(PRESSURES)}
            lm.dy.pert_to_fv3(P)
            lm.dy.lm_step(s, mode)
            pa.dy.pert_to_fv3(P)
            run(pa, t, s, flags)
            same(pert(lm), pert(pa), "flags %s, slot %d, mode %d" % (flags, s, mode))
            if not flags[0]:
                for n, a in before.items():
                    assert np.array_equal(lm.dy.get(n, 0), a), (n, "physics only: the resident trajectory moved")
            else:
                assert not np.array_equal(lm.dy.get("delp", 0), before["delp"])


# ---- 8: refusals, by message; after each the perturbation and cfcn are unchanged and the handle still steps
def check_refusals(make):
    import pytest
    from fv3_jedi_linearmodel_amd._lib import Fv3LmError
    fx = KC.fixture(TAG)
    c = make(**tile_kw())
    times = moist_times(c)
    t = times[0]
    R = lambda m: pytest.raises(Fv3LmError, match=m)
    upload(c, t); c.dy.pert_to_fv3(t["P"])
    P0 = pert(c)
    state = {"cf": None}

    def unchanged():
        assert all(np.array_equal(a, P0[n]) for n, a in pert(c).items()), "a refused call moved the perturbation"
        if state["cf"] is not None:
            assert np.array_equal(c.dy.cloud_cfcn(), state["cf"]), "a refused call moved cfcn"

    def refused(match, fn):
        with R(match):
            fn()
        unchanged()
        c.dy.step_tl()                      # the handle still steps
        assert all(np.all(np.isfinite(a)) for a in pert(c).values())
        upload(c, t); c.dy.pert_to_fv3(t["P"])
    for fn in (lambda: c.dy.lm_traj_save(0), lambda: c.dy.lm_traj_load(0), lambda: c.dy.lm_step(0, TL)):
        refused("fv3lm_lm_create first", fn)
    refused("nslots < 1", lambda: c.dy.lm_create(0, 1, 1, 1))
    for flags, name in (((2, 1, 1), "do_dyn"), ((1, -1, 1), "do_phy_trb"), ((1, 1, 2), "do_phy_mst")):
        refused(name + " = -?[0-9] outside 0..1", lambda: c.dy.lm_create(2, *flags))
    refused("do_dyn = do_phy_trb = do_phy_mst = 0", lambda: c.dy.lm_create(2, 0, 0, 0))
    refused("allocation of [0-9]+ bytes failed.*FV3LM_TRAJ_SLOTS", lambda: c.dy.lm_create(2 ** 31 - 1, 1, 1, 1))
    refused("fv3lm_lm_create first", lambda: c.dy.lm_step(0, TL))      # as if never created, and the handle is usable:
    c.dy.lm_create(2, 1, 1, 1)                                        # flags before the features they name
    refused("already created", lambda: c.dy.lm_create(2, 1, 1, 1))
    for slot in (-1, 2):
        for fn in (lambda: c.dy.lm_traj_save(slot), lambda: c.dy.lm_traj_load(slot), lambda: c.dy.lm_step(slot, TL)):
            refused("out of range", fn)
    refused("trajectory slot 0 was never set \\(fv3lm_lm_traj_save\\)", lambda: c.dy.lm_traj_load(0))
    refused("trajectory slot 0 was never set", lambda: c.dy.lm_step(0, TL))
    upload(c, t); c.dy.lm_traj_save(0)
    for mode in (0, -1, 3):
        refused("the nonlinear step is composed from the parts", lambda: c.dy.lm_step(0, mode))
    refused("fv3lm_turbulence_create first", lambda: c.dy.lm_step(0, TL))
    TC.ensure_created(c, 2)
    refused("turbulence slot 0 was never set", lambda: c.dy.lm_step(0, AD))
    c.dy.turbulence_set_diagonals(0, t["diag"])
    refused("fv3lm_convection_create first", lambda: c.dy.lm_step(0, TL))
    c.dy.convection_create(2, c.dy.ras_default_params(12), fx["mst"]); c._conv_slots = 2
    refused("the cloud scheme not: the reference has no such half", lambda: c.dy.lm_step(0, TL))
    c.dy.cloud_create(c.dy.cloud_default_params(12), KC.IQI, KC.IQL)
    state["cf"] = t["cf"]; c.dy.cloud_cfcn(t["cf"])
    refused("the convection slot 0 was never set", lambda: c.dy.lm_step(0, TL))
    c.dy.convection_set(0, *t["sfc"])
    refused("slot 0 was never set \\(fv3lm_cloud_set\\)", lambda: c.dy.lm_step(0, AD))
    c.dy.cloud_set(0, *t["cl"])
    refused("trajectory slot 1 was never set", lambda: c.dy.lm_step(1, TL))
    for mode in (TL, AD):                                             # the handle still steps
        c.dy.lm_step(0, mode)
        assert all(np.all(np.isfinite(a)) for a in pert(c).values()) and not np.any(c.dy.cloud_cfcn())
    assert any(not np.array_equal(a, P0[n]) for n, a in pert(c).items())


# ---- 9: the Fortran host (fortran/shim_lm_driver.F90 through fortran/fv3lm_hip_lm_mod.F90)
FDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fortran")


def build_driver(libdir, libname, out):
    """amdflang: the two shim modules + fortran/shim_lm_driver.F90 -> executable linked against lib<libname>.so in libdir (rpath set),
    compiled from copies in a directory of its own so that no stale .mod next to the sources is picked up"""
    import shutil
    import subprocess
    srcs = [os.path.join(FDIR, f) for f in ("fv3lm_hip_mod.F90", "fv3lm_hip_lm_mod.F90", "shim_lm_driver.F90")]
    lib = os.path.join(libdir, "lib%s.so" % libname)
    if os.path.exists(out) and all(os.path.getmtime(out) >= os.path.getmtime(s) for s in srcs + [lib]):
        return out
    mod = os.path.join(os.path.dirname(out), "mod_" + libname + "_shim_lm_driver")
    os.makedirs(mod, exist_ok=True)
    for s_ in srcs:
        shutil.copy(s_, mod)
    for m in ("fv3lm_hip_mod", "fv3lm_hip_lm_mod"):
        subprocess.check_call(["amdflang", "-cpp", "-fPIC", "-c", m + ".F90", "-o", m + ".o"], cwd=mod)
    subprocess.check_call(["amdflang", "-cpp", "shim_lm_driver.F90", "fv3lm_hip_mod.o", "fv3lm_hip_lm_mod.o", "-o", out, "-L", libdir, "-l" + libname,
                           "-Wl,-rpath," + libdir], cwd=mod)
    return out


def write_input(path, c, times, bad):
    """header, the case as fortran/shim_physics_driver.F90 reads it, then per time the compact trajectory, phis, the arguments of the
    three sets; the perturbation of the tangent window and the forcing of the adjoint window"""
    assert c.dims.ntile == 1 and c.opt.hydrostatic and c.nq == 3
    fx = KC.fixture(TAG)
    names = TC.all_names(c)
    with open(path, "wb") as f:
        f.write(np.array([bad, fx["mst"], KC.IQI, KC.IQL, len(times)], dtype=np.int32).tobytes())
        for st in (c.dims, c.opt):
            raw = bytes(st)
            f.write(np.int32(len(raw)).tobytes()); f.write(raw)
        f.write(np.array([c.da_min, c.da_min_c]).tobytes())
        f.write(np.ascontiguousarray(np.stack([c.metrics[n][0] for n in c.lib.metric_names()], axis=0), dtype=np.float64).tobytes())
        for a in (c.phis, c.ak, c.bk):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        for t in times:
            for a in [t["traj"][n] for n in names] + [t["phis"]] + list(t["sfc"]) + list(t["cl"]) + list(t["diag"]):
                a = np.ascontiguousarray(a, dtype=np.float64)
                f.write(a.tobytes())
        for D in (times[0]["P"], times[0]["PA"]):
            for n in names:
                f.write(np.ascontiguousarray(D[n], dtype=np.float64).tobytes())


def run_shim(make, driver, tmpdir):
    """the window of two times driven by the Fortran program through fv3lm_hip_lm_step only, against the same window through ctypes on a
    fresh handle: the perturbation after the two tangent steps and after the two adjoint steps, bit for bit"""
    from physics_shim_checks import Reader, run_driver
    c = make(**tile_kw())
    times = moist_times(c)
    names = TC.all_names(c)
    fin, fout = os.path.join(tmpdir, "lm_in.bin"), os.path.join(tmpdir, "lm_out.bin")
    write_input(fin, c, times, 0)
    r = run_driver(driver, fin, fout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "shim_lm_driver OK" in r.stdout, r.stdout[-2000:]
    rd = Reader(fout)
    got = {tag + n: rd.take(TC.cshape(c)) for tag in ("tl_", "ad_") for n in names}
    rd.done()
    prepare(c, times)
    ref = {}
    for tag, D, order, mode in (("tl_", times[0]["P"], (0, 1), TL), ("ad_", times[0]["PA"], (1, 0), AD)):
        c.dy.pert_to_fv3(D)
        for s in order:
            c.dy.lm_step(s, mode)
        ref.update({tag + n: a for n, a in c.dy.fv3_to_pert(names).items()})
    for key in got:
        assert np.array_equal(got[key], ref[key]), (key, "Fortran caller != ctypes caller")
        assert np.all(np.isfinite(got[key])) and np.any(got[key] != 0), key
    assert not np.array_equal(got["tl_pt"], times[0]["P"]["pt"])


def run_shim_refusal(make, driver, tmpdir):
    """a step at a slot whose trajectory was never saved ends the host: exit status 1, FATAL and the library's message"""
    from physics_shim_checks import run_driver
    c = make(**tile_kw())
    fin, fout = os.path.join(tmpdir, "lm_bad_in.bin"), os.path.join(tmpdir, "lm_bad_out.bin")
    write_input(fin, c, moist_times(c), 1)
    r = run_driver(driver, fin, fout)
    assert r.returncode == 1 and "FATAL fv3lm_hip lm_step" in r.stdout and "never set (fv3lm_lm_traj_save)" in r.stdout and "shim_lm_driver OK" not in r.stdout, \
        (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
