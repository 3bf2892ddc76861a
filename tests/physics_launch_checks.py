"""How many launches every call of the column physics makes (fv3lm_turbulence_*, fv3lm_convection_*, fv3lm_cloud_*; host side
csrc/physics.h) and, on the device, what they are called; shared by the host-emulation (test_emul_physics_launches.py) and the MI355X
(test_gpu_physics_launches.py) runs.  No other test pins these, and a change of the host side could move them without moving a result.

LAUNCHES was recorded with this module on the host-emulation build of the commit before the host side left csrc/dynamics.h; it is not
taken from the code under test.  The boundary copies of a periodic tile are one launch a field; a convection or cloud call is one launch
a batch of 2,048 columns (the convection runs: of the slot's DOCONVEC columns; the gather of convection_set is one launch whatever the
size).  NAMES are the kernel names in the sources (run_turb_*, run_bl_driver, run_ras, run_cloud, compact_in / compact_out)."""
import numpy as np
import turbulence_checks as TC
import bl_driver_checks as BC
import cloud_checks as KC

NL, TL, AD = 0, 1, 2
TAG = "L20m1"

# (case, call) -> launches.  Cases: "moist" the periodic 12 x 10 tile on the L20 fixture (120 columns, one batch); "moist 64 x 40" the
# same fixture on 2,560 columns (two batches, the second partial); "turbulence" 12 x 10 x L12, four tracers; "bl_driver" 12 x 10 x L20
_MOIST = ["convection_create", "cloud_create", "convection_set", "convection_get", "convection_table", "convection_sources(put)", "convection_sources(get)",
          "convection(1)", "convection(2)", "convection(0)", "cloud_set", "cloud_get", "cloud_cfcn(put)", "cloud_cfcn(get)", "cloud(1)", "cloud(2)", "cloud(0)"]
LAUNCHES = {
    ("turbulence", "turbulence_create"): 0, ("turbulence", "turbulence_set_diagonals"): 10, ("turbulence", "turbulence_get"): 10,
    ("turbulence", "turbulence(0)"): 1, ("turbulence", "turbulence(1)"): 1, ("turbulence", "turbulence(2)"): 1, ("turbulence", "turbulence_set_simple"): 3,
    ("bl_driver", "turbulence_set_driver"): 13, ("bl_driver", "turbulence_set_driver(raw)"): 26,
}
LAUNCHES.update({("moist", call): n for call, n in zip(_MOIST, [0, 0, 2, 0, 0, 0, 0, 1, 1, 1, 1, 0, 0, 0, 1, 1, 1])})
LAUNCHES.update({("moist 64 x 40", call): n for call, n in zip(_MOIST, [0, 0, 3, 0, 0, 0, 0, 1, 1, 1, 2, 0, 0, 0, 2, 2, 2])})

UNPACK, PACK = "boundary_unpack", "boundary_pack"
NAMES = {
    "turbulence_create": set(),
    "turbulence_set_diagonals": {UNPACK, "turbulence_factorise"},
    "turbulence_set_simple": {UNPACK, "turbulence_blsimp", "turbulence_factorise"},
    "turbulence_set_driver": {UNPACK, "turbulence_bldriver", "turbulence_factorise"},
    "turbulence_set_driver(raw)": {UNPACK, PACK, "turbulence_bldriver", "turbulence_factorise"},
    "turbulence(0)": {"turbulence_solve.nl"}, "turbulence(1)": {"turbulence_solve.tl"}, "turbulence(2)": {"turbulence_solve.ad"},
    "turbulence_get": {PACK},
    "convection_create": set(), "cloud_create": set(),
    "convection_set": {"convection_gather", "convection_set"},
    "convection_get": set(), "convection_table": set(), "convection_sources(put)": set(), "convection_sources(get)": set(),
    "convection(0)": {"convection.nl"}, "convection(1)": {"convection.tl"}, "convection(2)": {"convection.ad"},
    "cloud_set": {"cloud_set"},
    "cloud_get": set(), "cloud_cfcn(put)": set(), "cloud_cfcn(get)": set(),
    "cloud(0)": {"cloud.nl"}, "cloud(1)": {"cloud.tl"}, "cloud(2)": {"cloud.ad"},
}


def turbulence_calls(c):
    """the calls of the unit on generated diagonals and on BL_simp; between them the state is put again (not counted)"""
    T, P = TC.unit_state(c)
    yield "turbulence_create", lambda: c.dy.turbulence_create(1)
    TC.put_all(c, T, P)
    diag = TC.generated(c)
    yield "turbulence_set_diagonals", lambda: c.dy.turbulence_set_diagonals(0, diag)
    yield "turbulence_get", lambda: c.dy.turbulence_get(0)
    for mode in (NL, TL, AD):
        TC.put_all(c, T, P)
        yield "turbulence(%d)" % mode, lambda: c.dy.turbulence(0, mode)
    TC.put_all(c, T, P)
    fro = TC.frocean(c)
    yield "turbulence_set_simple", lambda: c.dy.turbulence_set_simple(0, fro)


def bl_driver_calls(c, lm=20):
    fx = BC.fixture(lm)
    T, sfc, qi, ql, k = BC.placed(c, fx, BC.dealt(c, 0))
    c.dy.turbulence_create(1)
    TC.put_all(c, T)
    p = BC.params(c, fx)
    yield "turbulence_set_driver", lambda: c.dy.turbulence_set_driver(0, p, fx["dt"], sfc, qi, ql, 0, False)
    yield "turbulence_set_driver(raw)", lambda: c.dy.turbulence_set_driver(0, p, fx["dt"], sfc, qi, ql, 0, True)


def moist_calls(c, tag=TAG):
    fx = KC.fixture(tag)
    T, sfc, cl, k = KC.placed(c, fx, KC.dealt(c, 0))
    (P, cf, src), (PA, cfa) = KC.forcing(c, fx, k)
    rp, cp = c.dy.ras_default_params(12), c.dy.cloud_default_params(12)
    yield "convection_create", lambda: c.dy.convection_create(1, rp, fx["mst"])
    yield "cloud_create", lambda: c.dy.cloud_create(cp, KC.IQI, KC.IQL)
    TC.put_all(c, T, P)
    yield "convection_set", lambda: c.dy.convection_set(0, *sfc)
    got = []
    yield "convection_get", lambda: got.append(c.dy.convection_get(0))
    assert np.any(got[0][1] == 1), "no DOCONVEC column: the convection runs would launch nothing"
    yield "convection_table", lambda: c.dy.convection_table()
    yield "convection_sources(put)", lambda: c.dy.convection_sources(src)
    yield "convection_sources(get)", lambda: c.dy.convection_sources()
    for mode in (TL, AD, NL):
        TC.put_all(c, T, P)
        yield "convection(%d)" % mode, lambda: c.dy.convection(0, mode)
    TC.put_all(c, T, P)
    yield "cloud_set", lambda: c.dy.cloud_set(0, *cl)
    yield "cloud_get", lambda: c.dy.cloud_get(0)
    yield "cloud_cfcn(put)", lambda: c.dy.cloud_cfcn(cf)
    yield "cloud_cfcn(get)", lambda: c.dy.cloud_cfcn()
    for mode in (TL, AD, NL):
        TC.put_all(c, T, P)
        yield "cloud(%d)" % mode, lambda: c.dy.cloud(0, mode)


def record(c, calls, names=False):
    """-> {call: (launches, set of kernel names or None)}.  names: on the device, from profile_begin / profile_end, whose own count of
    launches must agree with launch_count()"""
    out = {}
    for call, fn in calls:
        if names:
            c.dy.profile_begin()
        n0 = c.dy.launch_count()
        fn()
        n = c.dy.launch_count() - n0
        prof = c.dy.profile_end() if names else None
        if names:
            assert sum(v[0] for v in prof.values()) == n, (call, n, prof)
        out[call] = (n, set(prof) if names else None)
    return out


def check(case, c, calls, names=False):
    got = record(c, calls, names)
    for call, (n, ks) in got.items():
        print("%s: %s %d launch(es)%s" % (case, call, n, " " + " ".join(sorted(ks)) if names else ""))
    for call, (n, ks) in got.items():
        assert n == LAUNCHES[case, call], (case, call, n, LAUNCHES[case, call])
        if names:
            assert ks == NAMES[call], (case, call, ks, NAMES[call])
    assert set((case, call) for call in got) == set(k for k in LAUNCHES if k[0] == case), "a call of the table was not made"
    return got
