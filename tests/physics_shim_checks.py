"""The physics and Rayleigh wrappers of the ISO_C_BINDING shim (fortran/fv3lm_hip_mod.F90, the public list from fv3lm_hip_set_rayleigh to
fv3lm_hip_cloud) driven by a Fortran program (fortran/shim_physics_driver.F90) against the same calls made through ctypes on a fresh
handle of the same library: every array the program writes, bit for bit.  The Fortran side numbers its slots from 1 and works on slot 2
of 2 where ctypes works on slot 1, so a wrong slot - 1 meets a slot that was never set; the arrays given in a c_ptr array differ from one
another, so a permuted array changes the result; the integer arrays are preset to -7 by the program and have to come back with both of
their values.  Shared by test_emul_physics_shim.py (host emulation) and test_gpu_physics_shim.py (MI355X).

A compact array [1, (npz,) ny, nx] in C order is the host's (nx, ny[, npz]) in Fortran order byte for byte, and a padded plane
[1, npz, ny+7, nx+7] is (isd:ied+1, jsd:jed+1, npz): nothing is transposed on the way, and the tile is 12 x 10 so that a transposed
(i, j) cannot pass."""
import os
import re
import subprocess
import numpy as np
import turbulence_checks as TC
import convection_checks as CC
import cloud_checks as KC
import bl_driver_checks as BC

MOIST, BL, RAYLEIGH = 1, 2, 3
LEGS = {"moist": MOIST, "boundary layer": BL, "rayleigh": RAYLEIGH}
FDIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fortran")
REFUSED = {MOIST: ("FATAL fv3lm_hip convection", "never set"), BL: ("FATAL fv3lm_hip turbulence", "never set"), RAYLEIGH: ("FATAL fv3lm_hip set_rayleigh", "tau < 0")}


# ---- completeness: every public procedure of the module is called by one of the two drivers (no compiler needed)
def public_procedures():
    """the fv3lm_hip_* names of the module's public :: lines (the derived types, fv3lm_options and the like, are not procedures)"""
    src = open(os.path.join(FDIR, "fv3lm_hip_mod.F90")).read()
    names = []
    for line in re.findall(r"^\s*public\s*::(.*)$", src, flags=re.M | re.I):
        names += [n.strip() for n in line.split("!")[0].split(",")]
    procs = [n for n in names if n.startswith("fv3lm_hip_") and n != "fv3lm_hip_type"]
    for n in procs:
        assert re.search(r"^\s*subroutine\s+%s\s*\(" % n, src, flags=re.M | re.I), (n, "public, but no such subroutine")
    types = [n for n in names if n not in procs]
    for n in types:
        assert re.search(r"^\s*type\s*(,\s*bind\(C\)\s*)?::\s*%s\s*$" % n, src, flags=re.M | re.I), (n, "public, neither a subroutine nor a type")
    return procs, types


def called_procedures(driver):
    src = open(os.path.join(FDIR, driver)).read()
    code = "\n".join(line.split("!")[0] for line in src.splitlines())       # comments do not count
    return set(re.findall(r"\bcall\s+(fv3lm_hip_\w+)", code, flags=re.I))


def check_completeness():
    procs, types = public_procedures()
    physics = procs[procs.index("fv3lm_hip_set_rayleigh"):]
    partypes = [n for n in types if n.endswith("_params")]
    # the public list from fv3lm_hip_set_rayleigh on: 24 procedures and the three bind(C) parameter types, 27 names
    assert len(procs) == len(set(procs)) and len(physics) == 24 and physics[-1] == "fv3lm_hip_cloud" and len(partypes) == 3, (len(physics), physics, partypes)
    first, second = called_procedures("shim_driver.F90"), called_procedures("shim_physics_driver.F90")
    missing = [n for n in procs if n not in first | second]
    assert not missing, ("public in fv3lm_hip_mod.F90 and called by neither Fortran driver", missing)
    not_in_second = [n for n in physics if n not in second]
    assert not not_in_second, ("a physics wrapper that shim_physics_driver.F90 does not call", not_in_second)
    code = open(os.path.join(FDIR, "shim_physics_driver.F90")).read()
    for n in partypes:
        assert re.search(r"^\s*type\(%s\)\s*::" % n, code, flags=re.M | re.I), (n, "a parameter type that shim_physics_driver.F90 does not declare")
    return procs, physics


# ---- the input file of the driver
def _fields(c):
    return ["u", "v", "pt", "delp"] + TC.qnames(c)


def write_input(path, c, leg, bad, T, P, PA, extra):
    """header, the case as fortran/shim_driver.F90 reads it, the three sets of padded planes, then what the leg reads (int32 / float64)"""
    assert c.dims.ntile == 1 and c.opt.hydrostatic
    with open(path, "wb") as f:
        f.write(np.array([leg, bad], dtype=np.int32).tobytes())
        for st in (c.dims, c.opt):
            raw = bytes(st)
            f.write(np.int32(len(raw)).tobytes()); f.write(raw)
        f.write(np.array([c.da_min, c.da_min_c]).tobytes())
        f.write(np.ascontiguousarray(np.stack([c.metrics[n][0] for n in c.lib.metric_names()], axis=0), dtype=np.float64).tobytes())
        for a in (c.phis, c.ak, c.bk):
            f.write(np.ascontiguousarray(a, dtype=np.float64).tobytes())
        for D in (T, P, PA):
            for n in _fields(c):
                assert D[n].shape == (1, c.npz, c.ny + 7, c.nx + 7)
                f.write(np.ascontiguousarray(D[n], dtype=np.float64).tobytes())
        for a in extra:
            a = np.ascontiguousarray(a)
            assert a.dtype in (np.int32, np.float64), a.dtype
            f.write(a.tobytes())


class Reader:
    """the driver's output file in the order it was written"""
    def __init__(self, path):
        self.raw, self.pos = np.fromfile(path, dtype=np.uint8), 0

    def take(self, shape, dtype=np.float64):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        assert self.pos + n <= self.raw.size, "the driver wrote less than the test expects"
        a = self.raw[self.pos:self.pos + n].view(dtype).reshape(shape)
        self.pos += n
        return a

    def done(self):
        assert self.pos == self.raw.size, (self.pos, self.raw.size, "the driver wrote more than the test read")


def run_driver(driver, fin, fout):
    """one run of the Fortran program as a fresh child; its exit status is looked at before anything else"""
    if os.path.exists(fout):
        os.remove(fout)
    return subprocess.run([driver, fin, fout], capture_output=True, text=True, timeout=120)


def compare(got, ref, acts=()):
    assert list(got) == list(ref)
    for key in got:
        a, b = got[key], ref[key]
        assert a.shape == b.shape and a.dtype == b.dtype, (key, a.shape, b.shape, a.dtype, b.dtype)
        assert np.array_equal(a, b), (key, "Fortran caller != ctypes caller")
        assert np.all(np.isfinite(a)), (key, "not finite")
    for key in acts:
        assert np.any(got[key] != 0), (key, "all zero where the scheme acts")


# ---- the legs: each returns (T, P, PA, extra input, read(Reader) -> dict, ctypes() -> dict, what acts)
def moist_leg(c):
    fx = KC.fixture("L40m2")
    assert c.nq == 3 and c.npz == fx["lm"] and (c.nx, c.ny) == (12, 10)
    T, sfc, cl, k = KC.placed(c, fx, CC.dealt(c))
    (P, cf, _), (PA, cfa) = KC.forcing(c, fx, k)
    cs, ps, names = TC.cshape(c), (1, c.npz, c.ny + 7, c.nx + 7), _fields(c)
    extra = [np.array([fx["mst"], KC.IQI, KC.IQL], dtype=np.int32)] + list(sfc) + list(cl) + [cf, cfa]

    def read(r):
        g = {"rpar": r.take(25), "cpar": r.take(57)}
        g.update({"set_" + n: r.take(cs) for n in CC.SETN}); g["doconvec"] = r.take(cs[:1] + cs[2:], np.int32)
        g["table"] = r.take(18301); g["constants"] = r.take(9)
        g.update({"cloud_" + n: r.take(cs) for n in KC.OUT8 + KC.FRAC}); g["pertmod"] = r.take(cs, np.int32)
        g.update({"tl_src_" + n: r.take(cs) for n in CC.SRC}); g["tl_cfcn"] = r.take(cs)
        g.update({"tl_" + n: r.take(ps) for n in names})
        g.update({"ad_src_" + n: r.take(cs) for n in CC.SRC})
        g.update({"ad_" + n: r.take(ps) for n in names}); g["ad_cfcn"] = r.take(cs)
        g.update({"ad_src_after_" + n: r.take(cs) for n in CC.SRC})
        g.update({"nl_conv_" + n: r.take(ps) for n in names}); g.update({"nl_cloud_" + n: r.take(ps) for n in names})
        return g

    def ctypes_calls():
        dy, slot = c.dy, 1
        rp, cp = dy.ras_default_params(12), dy.cloud_default_params(12)
        g = {"rpar": np.array(rp.r[:]), "cpar": np.array(cp.r[:])}
        dy.convection_create(2, rp, fx["mst"]); dy.cloud_create(cp, KC.IQI, KC.IQL)
        TC.put_all(c, T)
        dy.convection_set(slot, *sfc); dy.cloud_set(slot, *cl)
        out, dc, _ = dy.convection_get(slot, jac=False)
        g.update({"set_" + n: out[n] for n in CC.SETN}); g["doconvec"] = dc
        g["table"], g["constants"] = dy.convection_table()
        o8, fr, pm = dy.cloud_get(slot)
        g.update({"cloud_" + n: o8[n] for n in KC.OUT8}); g.update({"cloud_" + n: fr[n] for n in KC.FRAC}); g["pertmod"] = pm
        TC.put_all(c, T, P)
        dy.convection(slot, CC.TL)
        g.update({"tl_src_" + n: v for n, v in dy.convection_sources().items()})
        dy.cloud_cfcn(cf); dy.cloud(slot, CC.TL)
        g["tl_cfcn"] = dy.cloud_cfcn()
        g.update({"tl_" + n: dy.get(n, 1) for n in names})
        TC.put_all(c, T, PA)
        dy.cloud_cfcn(cfa); dy.cloud(slot, CC.AD)
        src = dy.convection_sources()
        g.update({"ad_src_" + n: v for n, v in src.items()})
        dy.convection_sources([src[n] * float(m + 2) for m, n in enumerate(CC.SRC)])
        dy.convection(slot, CC.AD)
        g.update({"ad_" + n: dy.get(n, 1) for n in names}); g["ad_cfcn"] = dy.cloud_cfcn()
        g.update({"ad_src_after_" + n: v for n, v in dy.convection_sources().items()})
        dy.convection(slot, CC.NL); g.update({"nl_conv_" + n: dy.get(n, 0) for n in names})
        dy.cloud(slot, CC.NL); g.update({"nl_cloud_" + n: dy.get(n, 0) for n in names})
        return g

    def more(g):
        assert 0 < int(g["doconvec"].sum()) < g["doconvec"].size and set(np.unique(g["doconvec"])) == {0, 1}, "DOCONVEC: a zeroed or mistyped integer array"
        assert set(np.unique(g["pertmod"])) == {0, 1}, "cloud_pertmod: both values have to occur"
        assert not any(np.any(g["ad_src_after_" + n]) for n in CC.SRC), "the convection's adjoint consumes its sources"
        assert all(np.any(g["ad_src_" + n] != g["tl_src_" + n]) for n in CC.SRC)
        for tag in ("tl_", "ad_"):
            for n in ("pt", "q1", "q%d" % KC.IQI, "q%d" % KC.IQL, "u", "v"):
                assert not np.array_equal(g[tag + n], (P if tag == "tl_" else PA)[n]), (tag + n, "the chain does nothing")
        assert not np.array_equal(g["nl_conv_pt"], T["pt"]) and not np.array_equal(g["nl_cloud_q%d" % KC.IQL], g["nl_conv_q%d" % KC.IQL])
    acts = ["set_" + n for n in CC.SETN] + ["cloud_" + n for n in KC.OUT8 + KC.FRAC] + ["tl_src_" + n for n in CC.SRC] + ["ad_src_" + n for n in CC.SRC] + ["tl_cfcn", "ad_cfcn", "table"]
    return T, P, PA, extra, read, ctypes_calls, acts, more


def boundary_layer_leg(c):
    fx = BC.fixture(20)
    assert c.npz == 20 and (c.nx, c.ny) == (12, 10) and c.nq >= 3
    T, sfc, qi, ql, k = BC.placed(c, fx, BC.dealt(c))
    P = BC.perturbation(c)
    sf = [sfc[n] for n in BC.SFC]
    assert all(not np.array_equal(a, b) for i, a in enumerate(sf) for b in sf[i + 1:]), "the nine surface fields have to differ from one another"
    fro = TC.frocean(c)
    cs, ps, names = TC.cshape(c), (1, c.npz, c.ny + 7, c.nx + 7), _fields(c)
    extra = [np.array([int(fx["ipar"][0])], dtype=np.int32), np.array([fx["dt"]])] + sf + [qi, ql, fro]

    def read(r):
        g = {"rpar": r.take(22), "ipar": r.take(4, np.int32), "driver_factors": r.take((10,) + cs)}
        for mode in ("nl", "tl", "ad"):
            g.update({mode + "_" + n: r.take(ps) for n in names})
        g["diagonals_factors"] = r.take((10,) + cs)
        g.update({"tl1_" + n: r.take(ps) for n in names})
        g["simple_factors"] = r.take((10,) + cs)
        return g

    def ctypes_calls():
        dy = c.dy
        dy.turbulence_create(2)
        bp = dy.bl_default_params(int(fx["ipar"][0]))
        g = {"rpar": np.array(bp.r[:]), "ipar": np.array(bp.i[:], dtype=np.int32)}
        TC.put_all(c, T)
        dy.turbulence_set_driver(1, bp, fx["dt"], sf, qi, ql, 0, False)
        fac = dy.turbulence_get(1)
        g["driver_factors"] = fac
        for mode, tag in enumerate(("nl", "tl", "ad")):
            TC.put_all(c, T, P)
            dy.turbulence(1, mode)
            g.update({tag + "_" + n: dy.get(n, min(mode, 1)) for n in names})
        TC.put_all(c, T, P)
        diag = [fac[n] * (1.0 + (n + 1) / 32.0) for n in range(9)]      # as the driver scales them: one exact factor, one rounding
        assert all(not np.array_equal(a, b) for i, a in enumerate(diag) for b in diag[i + 1:]), "the nine diagonals have to differ from one another"
        dy.turbulence_set_diagonals(0, diag)
        g["diagonals_factors"] = dy.turbulence_get(0)
        dy.turbulence(0, 1)
        g.update({"tl1_" + n: dy.get(n, 1) for n in names})
        dy.turbulence_set_simple(0, fro)
        g["simple_factors"] = dy.turbulence_get(0)
        return g

    def more(g):
        assert np.array_equal(g["rpar"], fx["rpar"]) and np.array_equal(g["ipar"], fx["ipar"]) and len(set(g["ipar"].tolist())) > 1
        for key in ("driver_factors", "diagonals_factors"):      # heat and moisture share their lower diagonal in BL_DRIVER
            f = g[key]
            same = [(i, j) for i in range(10) for j in range(i + 1, 10) if np.array_equal(f[i], f[j])]
            assert same == ([(3, 6)] if key == "driver_factors" else []), (key, same, "arrays of a slot that coincide")
        for tag, X in (("nl", T), ("tl", P), ("ad", P), ("tl1", P)):
            for n in TC.seven(c):
                assert not np.array_equal(g[tag + "_" + n], X[n]), (tag, n, "the solve does nothing")
        assert not np.array_equal(g["tl1_pt"], g["tl_pt"]) and not np.array_equal(g["simple_factors"], g["diagonals_factors"])
        assert np.array_equal(g["simple_factors"][9], g["driver_factors"][9]), "pk of the same trajectory"
    return T, P, P, extra, read, ctypes_calls, ["driver_factors", "diagonals_factors", "simple_factors"], more


def rayleigh_leg(c, tau=0.3, rf_cutoff=3.0e4):
    from groups import step_state
    T0, P0 = step_state(c)
    T = {n: np.array(T0[n][None], dtype=np.float64) for n in _fields(c)}
    P = {n: np.array(P0[n][None], dtype=np.float64) for n in _fields(c)}
    pj, pi = c.ny + 7, c.nx + 7
    j, i = np.meshgrid(np.arange(pj), np.arange(pi), indexing="ij")
    c2l = np.ascontiguousarray(c.c2l + 0.01 * np.arange(1, 5)[None, :, None, None] * np.cos(0.3 * i + 0.2 * j))      # non-constant, and i, j told apart
    assert c2l.shape == (1, 4, pj, pi) and all(np.ptp(c2l[0, q]) > 0 for q in range(4))
    ps, names = (1, c.npz, pj, pi), _fields(c)
    extra = [np.array([tau, rf_cutoff]), c2l]

    def read(r):
        g = {"rf": r.take(c.npz), "kmax": r.take(1, np.int32)}
        for tag in ("tl0", "tl1", "ad1"):
            g.update({tag + "_" + n: r.take(ps) for n in names})
        return g

    def ctypes_calls():
        dy = c.dy
        dy.set_rayleigh(tau, rf_cutoff, c2l)
        rf, kmax = dy.rayleigh_profile()
        g = {"rf": rf, "kmax": np.array([kmax], dtype=np.int32)}
        TC.put_all(c, T, P)
        dy.step_tl()
        g.update({"tl0_" + n: dy.get(n, 0) for n in names}); g.update({"tl1_" + n: dy.get(n, 1) for n in names})
        TC.put_all(c, T, P)
        dy.step_nl(); dy.step_ad()
        g.update({"ad1_" + n: dy.get(n, 1) for n in names})
        return g

    def more(g):
        kmax = int(g["kmax"][0])
        assert 0 < kmax < c.npz, (kmax, "the damping has to cover some layers and not all")
        assert np.all(g["rf"][:kmax] > 0) and not np.any(g["rf"][kmax:])
    return T, P, P, extra, read, ctypes_calls, ["rf", "kmax"] + [t + n for t in ("tl0_", "tl1_", "ad1_") for n in names], more


def run_physics_shim_check(make, leg, driver, tmpdir):
    """one leg: the Fortran program as a child, then the same calls through ctypes on the fresh handle of the case make() returns.  The
    child's exit status is asserted before anything else: after a non-zero status no further call is made."""
    c = make()
    T, P, PA, extra, read, ctypes_calls, acts, more = {MOIST: moist_leg, BL: boundary_layer_leg, RAYLEIGH: rayleigh_leg}[leg](c)
    fin, fout = os.path.join(tmpdir, "physics_in.bin"), os.path.join(tmpdir, "physics_out.bin")
    write_input(fin, c, leg, 0, T, P, PA, extra)
    r = run_driver(driver, fin, fout)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    assert "shim_physics_driver OK" in r.stdout, r.stdout[-2000:]
    rd = Reader(fout)
    got = read(rd)
    rd.done()
    ref = ctypes_calls()
    compare(got, ref, acts)
    more(got)
    return got


def run_physics_shim_refusal(make, leg, driver, tmpdir):
    """a refused physics call: the program ends non-zero with FATAL and the library's message in its output"""
    c = make()
    T, P, PA, extra, read, ctypes_calls, acts, more = {MOIST: moist_leg, BL: boundary_layer_leg, RAYLEIGH: rayleigh_leg}[leg](c)
    fin, fout = os.path.join(tmpdir, "physics_bad_in.bin"), os.path.join(tmpdir, "physics_bad_out.bin")
    write_input(fin, c, leg, 1, T, P, PA, extra)
    r = run_driver(driver, fin, fout)
    where, msg = REFUSED[leg]
    assert r.returncode == 1 and where in r.stdout and msg in r.stdout and "shim_physics_driver OK" not in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-2000:])
