"""Generates tests/golden/convection_ref.npz by running the reference's own RAS convection -- RASE0, RASE0_D, RASE_D, RASE_B of
physics/moist/convection{,_tl,_ad}.F90 with qsat_util.F90, utils/MAPL_Constants.F90 and utils/tapenade/adStack.c, adBuffer.f, compiled
where they lie under the reference checkout -- through our bind(C) wrapper convection_wrap.F90 on generated soundings.  Everything
compiled goes into a temporary directory; the fixture holds data only.

    python tests/golden/make_convection_golden.py [--seed N] [--time NCOL LM]

What set_ltraj (fv3jedi_lm_moist_mod.F90:649-832) prepares around the routines -- theta, CNV_PLE, SEEDRAS, the heating-rate filter and the
Jacobian filter -- is restated here in numpy around the reference's outputs.  The draw, what the generator asserts about it and how the
tolerance is measured: DESIGN.md section 5."""
import argparse
import ctypes as C
import os
import subprocess
import tempfile
import time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("FV3LM_REFERENCE_SRC", "/root/reference/src")
FFLAGS = ["-O2", "-fPIC", "-cpp", "-fdefault-real-8", "-fdefault-double-8"]
_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
LD = np.longdouble

P00, PTOP, DT = 100000.0, 100.0, 1800.0
KAPPA = (8314.47 / 28.965) / (3.5 * (8314.47 / 28.965))        # fv3jedi_lm_const_mod, as the module evaluates it
SETS = [(40, 32, 2), (72, 16, 2), (20, 16, 1)]                 # lm, columns, do_phy_mst
SET_OUT = ["PTT_C", "QVT_C", "CNV_DQLDT_C", "CNV_MFD_C", "CNV_PRC3_C", "CNV_UPDF_C"]
JAC = ["H_pert", "M_pert"]
TL_OUT = ["pt", "q1", "u", "v", "CNV_DQLDT", "CNV_MFD", "CNV_PRC3", "CNV_UPDF"]      # theta, qv, u, v, then the four sources
AD_OUT = ["pt", "q1", "u", "v"]


def ras_params(im):
    """create :120-148"""
    r = [1.0, 0.05, 0.0, 8.0e-4, 1800., 43200.0, -300., 4.0, 0.0, 200., 7.5e-4, 1.0, -1.0, 1.3, 1.3, 263., 0.5, 1.0, 0.0, 0.1, 0.8, 1.0, 0.0, 0.5, 0.65]
    ims = 4 * im
    r[22] = 4000.0 if ims <= 200 else 2000.0 if ims <= 400 else 700.0 if ims <= 800 else 450.0
    return np.array(r)


def build_reference(tmp):
    srcs = [os.path.join(REF, "utils", "MAPL_Constants.F90"), os.path.join(REF, "physics", "moist", "qsat_util.F90"),
            os.path.join(REF, "physics", "moist", "convection.F90"), os.path.join(REF, "physics", "moist", "convection_tl.F90"),
            os.path.join(REF, "utils", "tapenade", "adBuffer.f"), os.path.join(REF, "physics", "moist", "convection_ad.F90"),
            os.path.join(HERE, "convection_wrap.F90")]
    objs = []
    for n, s in enumerate(srcs):
        o = os.path.join(tmp, "f%d.o" % n)
        subprocess.check_call(["amdflang"] + FFLAGS + ["-module-dir", tmp, "-c", s, "-o", o], cwd=tmp)
        objs.append(o)
    o = os.path.join(tmp, "adStack.o")
    subprocess.check_call(["amdclang", "-O2", "-fPIC", "-c", os.path.join(REF, "utils", "tapenade", "adStack.c"), "-o", o], cwd=tmp)
    so = os.path.join(tmp, "libconvection_ref.so")
    subprocess.check_call(["amdflang", "-shared", "-o", so] + objs + [o], cwd=tmp)
    return C.CDLL(so)


def constants(L):
    c = np.zeros(9); tbl = np.zeros(18301)
    L.conv_constants(c.ctypes.data_as(_dp), tbl.ctypes.data_as(_dp))
    return dict(zip(["CP", "ALHL", "GRAV", "RGAS", "H2OMW", "AIRMW", "VIREPS", "P00", "KAPPA"], c)), tbl


def edges(lm):
    z = np.arange(lm + 1) / lm
    return 100.0 * (1.0 + 999.0 * (0.3 * z + 0.7 * z ** 2.2))      # Pa


def levels(lm):
    pe = edges(lm); z = np.arange(lm + 1) / lm
    return pe * (1.0 - z), pe * z / P00      # ak, bk: ak + bk p00 = the edges


def pressures(delp):
    """pe, pk as compute_pressures, in extended precision"""
    lm, ncol = delp.shape
    pe = np.zeros((lm + 1, ncol), dtype=LD); pe[0] = PTOP
    for l in range(lm):
        pe[l + 1] = pe[l] + LD(1) * delp[l]
    k = LD(KAPPA)
    pk = (pe[1:] ** k - pe[:-1] ** k) / (k * (np.log(pe[1:]) - np.log(pe[:-1])))
    return pe, pk


def draw(rng, lm, ncol):
    pe = edges(lm)
    delp = np.repeat(np.diff(pe)[:, None], ncol, axis=1)
    pm = 0.5 * (pe[1:] + pe[:-1])[:, None] / 100.0      # hPa
    n = np.arange(ncol)
    stable = n % 8 == 5
    tsfc = np.where(stable, rng.uniform(255., 262., ncol), rng.uniform(296., 302., ncol))
    t = np.maximum(200.0, (tsfc - 1.0)[None, :] * (pm / 1000.0) ** (287.05 * 6e-3 / 9.80665))
    rh = np.minimum(0.95, 0.35 + 0.5 * (pm / 1000.0) ** 2 + 0.1 * rng.random(ncol)[None, :]) * np.where(stable, 0.2, 1.0)[None, :]
    es = 6.112 * np.exp(17.67 * (t - 273.15) / (t - 29.65))      # Bolton, hPa
    qs = 0.622 * es / (pm - 0.378 * es)
    qv = np.where(pm > 100.0, rh * qs, 3e-6)
    zz = -7.5 * np.log(pm / 1000.0)
    u = rng.uniform(2., 10., ncol) * (1.0 + zz / 4.0) + rng.standard_normal((lm, ncol))
    v = rng.uniform(-5., 5., ncol) * (1.0 + zz / 6.0) + rng.standard_normal((lm, ncol))
    a = dict(delp=delp, T=t, u=u, v=v, qv=qv, kcbl=(lm - 3 - n % 3).astype(np.float64), ts=tsfc + 1.5, frland=np.where(n % 4 == 3, 1.0, 0.0))
    return a


def prepared(a, cst, move=None):
    """what set_ltraj hands to RASE0: theta by the JEDI p00, kappa and compute_pressures' pk; CNV_PLE; SEEDRAS by the GEOS form"""
    pe, pk = pressures(a["delp"])
    th = np.asarray(LD(P00) ** LD(KAPPA) * a["T"] / pk, dtype=np.float64)
    qv = a["qv"].copy()
    if move is not None:
        th = th * (1.0 + move[0]); qv = qv * (1.0 + move[1])
    ple = np.asarray(pe, dtype=np.float64) * 0.01
    plo = 0.5 * (ple[:-1] + ple[1:])
    temp = th * (plo / 1000.0) ** (cst["RGAS"] / cst["CP"])
    x = 100.0 * temp[-1]
    seed = (1000000 * (x - np.trunc(x))).astype(np.int32)
    return dict(th=th, qv=qv, ple=ple, pk=np.asarray(pk, dtype=np.float64), seed=seed)


class Ref:
    def __init__(self, L, lm, rpar, cst):
        self.L, self.lm, self.rpar, self.cst = L, lm, rpar, cst
        ak, bk = levels(lm)
        pref = ak + bk * cst["P00"]
        self.icmin = max(1, int(np.count_nonzero(pref < 3000.0)))
        self.sige = np.ascontiguousarray(pref / pref[lm])

    def _common(self, a, p):
        ncol = a["T"].shape[1]
        cols = lambda x: np.ascontiguousarray(np.asarray(x, dtype=np.float64).T)      # [lm, ncol] -> Fortran (lm, ncol)
        kc = np.ascontiguousarray(np.rint(a["kcbl"]).astype(np.int32))
        return ncol, cols, kc, np.ascontiguousarray(p["seed"]), np.ascontiguousarray(a["frland"]), np.ascontiguousarray(a["ts"])

    def rase0(self, a, p, thd=None):
        ncol, cols, kc, seed, fr, ts = self._common(a, p)
        th, qv, ple = cols(p["th"]), cols(p["qv"]), cols(p["ple"])
        d1 = cols(thd) if thd is not None else np.zeros_like(th); d2 = np.zeros_like(th)
        o = [np.zeros_like(th) for _ in range(4)]
        P = lambda x: x.ctypes.data_as(_dp)
        self.L.conv_rase0(C.c_int(0 if thd is None else 1), C.c_int(ncol), C.c_int(self.lm), C.c_int(self.icmin), C.c_double(DT), seed.ctypes.data_as(_ip),
                          P(self.sige), kc.ctypes.data_as(_ip), P(fr), P(ts), P(th), P(d1), P(qv), P(d2), P(ple), P(o[0]), P(o[1]), P(o[2]), P(o[3]), P(self.rpar))
        if thd is None:
            return [th.T, qv.T] + [x.T for x in o]
        return [d1.T, d2.T]

    def rase(self, which, a, p, x, xd, sd=None):
        """x: u v of the trajectory come from a; xd [4, lm, ncol]; sd [4, lm, ncol] (adjoint forcing of the sources)"""
        ncol, cols, kc, seed, fr, ts = self._common(a, p)
        X = np.ascontiguousarray(np.stack([cols(p["th"]), cols(p["qv"]), cols(a["u"]), cols(a["v"])]))
        XD = np.ascontiguousarray(np.stack([cols(v) for v in xd]))
        S = np.zeros_like(X); SD = np.ascontiguousarray(np.stack([cols(v) for v in sd])) if sd is not None else np.zeros_like(X)
        ple = cols(p["ple"])
        P = lambda x: x.ctypes.data_as(_dp)
        self.L.conv_rase(C.c_int(which), C.c_int(ncol), C.c_int(self.lm), C.c_int(self.icmin), C.c_double(DT), seed.ctypes.data_as(_ip), P(self.sige),
                         kc.ctypes.data_as(_ip), P(fr), P(ts), P(X), P(XD), P(ple), P(S), P(SD), P(self.rpar))
        T = lambda A: np.ascontiguousarray(np.transpose(A, (0, 2, 1)))
        return T(X), T(XD), T(S), T(SD)


def doconvec_filter(heat_new, th, kcbl, maxcondep):
    """set_ltraj :796-823 for every column -> 0 / 1"""
    lm, ncol = th.shape
    out = np.zeros(ncol, dtype=np.int32)
    for n in range(ncol):
        heat = (heat_new[:, n] - th[:, n]) / DT
        k = int(round(kcbl[n])); ctop = lm
        hm = np.max(np.abs(heat))
        for l in range(1, lm + 1):
            if abs(heat[l - 1]) > 0.01 * hm:
                ctop = l; break
        s = 0.0
        if ctop != lm and k - ctop > 0:
            seg = np.abs(heat[ctop - 1:k - 1])
            s = (seg.sum() - seg.max()) / (k - ctop)
        if k - ctop >= maxcondep:
            with np.errstate(divide="ignore", invalid="ignore"):
                if s / np.max(np.abs(heat[:k - 1])) > 0.125:
                    out[n] = 1
    return out


def everything(R, a, cst, X, Y, move=None):
    """all the reference gives for the columns a: set outputs, filter, Jacobian column, RASE_D on X, RASE_B on Y"""
    lm, ncol = a["T"].shape
    p = prepared(a, cst, move)
    r = {}
    s0 = R.rase0(a, p)
    for k, v in zip(SET_OUT, s0):
        r["set_" + k] = v
    e = np.zeros((lm, ncol)); e[np.rint(a["kcbl"]).astype(int) - 1, np.arange(ncol)] = 1.0
    jd = R.rase0(a, p, e)
    r["jac_H_pert"] = (jd[0] - e) / DT; r["jac_M_pert"] = jd[1] / DT
    r["heat_ok"] = doconvec_filter(s0[0], p["th"], a["kcbl"], R.maxcondep)
    steep = (np.abs(r["jac_H_pert"]).max(axis=0) > 1e-4) | (np.abs(r["jac_M_pert"]).max(axis=0) > 1e-7)
    r["doconvec"] = np.where((r["heat_ok"] == 1) & ~steep, 1, 0).astype(np.int32)
    xo, xd, so, sd = R.rase(1, a, p, None, X)
    for n, k in enumerate(TL_OUT):
        r["tl_" + k] = xd[n] if n < 4 else sd[n - 4]
    for n, k in enumerate(AD_OUT):
        r["nl_" + k] = xo[n]
    _, xb, _, _ = R.rase(2, a, p, None, Y[:4], Y[4:])
    for n, k in enumerate(AD_OUT):
        r["ad_" + k] = xb[n]
    r["fired"] = np.count_nonzero(so[1], axis=0)
    return r, p


def colrel(d, ref):
    s = np.abs(ref).max(axis=0)
    return np.abs(d).max(axis=0) / np.where(s > 0, s, 1.0)


def case(L, cst, seed, lm, ncol, mst):
    rpar = ras_params(12)
    assert rpar[22] == 4000.0
    R = Ref(L, lm, rpar, cst); R.maxcondep = 1 if mst == 1 else 10
    keys = None
    a, X, Y = None, None, None
    redrawn, draws = 0, 0
    have = []
    attempt = 0
    while sum(b["T"].shape[1] for b in have) < ncol:
        rng = np.random.default_rng([seed, lm, attempt]); attempt += 1
        b = draw(rng, lm, ncol)
        bX = (rng.standard_normal((4, lm, ncol)) * np.array([0.5, 1e-4, 1.0, 1.0])[:, None, None]).astype(np.float32).astype(np.float64)
        bY = (rng.standard_normal((8, lm, ncol)) * np.array([1.0, 1e3, 0.1, 0.1, 1e4, 1e1, 1e4, 1.0])[:, None, None]).astype(np.float32).astype(np.float64)
        ref, _ = everything(R, b, cst, bX, bY)
        worst = np.zeros(ncol)
        for sgn in (1.0, -1.0):
            mv = sgn * 1e-12 * rng.uniform(0.5, 1.0, (2, lm, ncol))
            o, _ = everything(R, b, cst, bX, bY, mv)
            for k in ref:
                if ref[k].ndim == 2:
                    worst = np.maximum(worst, colrel(o[k] - ref[k], ref[k]))
                elif k != "fired":
                    worst = np.maximum(worst, 1.0 * (o[k] != ref[k]))
        keep = worst <= 1e-6
        # keep the column's place in the recipe (KCBL, FRLAND, stable follow n): take kept columns only where still needed
        need = ncol - sum(x["T"].shape[1] for x in have)
        idx = np.nonzero(keep)[0][:need]
        draws += ncol; redrawn += int((~keep).sum())
        sel = lambda v: v[..., idx]
        have.append({k: sel(v) for k, v in b.items()}); have[-1]["X"] = sel(bX); have[-1]["Y"] = sel(bY)
        assert attempt < 10
    assert redrawn <= 0.1 * draws, (redrawn, draws)
    cat = lambda k: np.ascontiguousarray(np.concatenate([h[k] for h in have], axis=-1))
    a = {k: cat(k) for k in have[0] if k not in ("X", "Y")}
    X, Y = cat("X"), cat("Y")
    ref, p = everything(R, a, cst, X, Y)
    amp = 0.0
    spread = {k: 0.0 for k in ref if ref[k].ndim == 2}
    rng = np.random.default_rng([seed, lm, 999])
    for n in range(8):
        o, _ = everything(R, a, cst, X, Y, 1e-15 * rng.uniform(-1, 1, (2, lm, ncol)))
        for k in spread:
            spread[k] = max(spread[k], float(colrel(o[k] - ref[k], ref[k]).max()))
    # the reference's own dot product
    lhs = sum(float(np.sum(ref["tl_" + k] * Y[n])) for n, k in enumerate(TL_OUT))
    rhs = sum(float(np.sum(ref["ad_" + k] * X[n])) for n, k in enumerate(AD_OUT))
    print("L%d: %d columns, redrawn %d of %d; heat filter passes %d, doconvec %d; fired cloud types max %d; reference dot product residual %.1e"
          % (lm, ncol, redrawn, draws, ref["heat_ok"].sum(), ref["doconvec"].sum(), ref["fired"].max(), abs(lhs - rhs) / abs(lhs)))
    print("L%d: spread at 1e-15: " % lm + " ".join("%s %.1e" % kv for kv in spread.items()))
    assert abs(lhs - rhs) <= 1e-13 * abs(lhs)
    assert ref["doconvec"].sum() >= 0.3 * ncol and (ref["doconvec"] == 0).sum() >= 1, ref["doconvec"]
    assert ref["fired"].max() >= 5
    out = {}
    for k in ("delp", "T", "u", "v", "qv", "kcbl", "ts", "frland"):
        out["L%d_%s" % (lm, k)] = a[k]
    out["L%d_X" % lm] = X.astype(np.float32); out["L%d_Y" % lm] = Y.astype(np.float32)
    for k, v in ref.items():
        out["L%d_ref_%s" % (lm, k)] = v
    out["L%d_spread_names" % lm] = np.array(list(spread)); out["L%d_spread" % lm] = np.array([spread[k] for k in spread])
    ak, bk = levels(lm)
    out["L%d_ak" % lm] = ak; out["L%d_bk" % lm] = bk; out["L%d_rpar" % lm] = rpar; out["L%d_mst" % lm] = mst; out["L%d_icmin" % lm] = R.icmin
    out["L%d_seed" % lm] = p["seed"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20250607)
    ap.add_argument("--time", type=int, nargs=2, metavar=("NCOL", "LM"), help="only time the compiled reference on one core")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        L = build_reference(tmp)
        cst, tbl = constants(L)
        if args.time:
            ncol, lm = args.time
            a = draw(np.random.default_rng(args.seed), lm, ncol)
            R = Ref(L, lm, ras_params(12), cst); R.maxcondep = 10
            p = prepared(a, cst)
            X = np.ones((4, lm, ncol)); Y = np.ones((8, lm, ncol))
            for name, fn in (("RASE0", lambda: R.rase0(a, p)), ("RASE_D", lambda: R.rase(1, a, p, None, X)), ("RASE_B", lambda: R.rase(2, a, p, None, Y[:4], Y[4:]))):
                ts = []
                for n in range(3):
                    t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
                print("reference %s, one core: %d columns x L%d: %.3f s (best of 3) = %.1f us per column" % (name, ncol, lm, min(ts), 1e6 * min(ts) / ncol))
            return
        out = dict(lms=np.array([s[0] for s in SETS]), dt=DT, ptop=PTOP, kappa=KAPPA, p00=P00, constants=np.array([cst[k] for k in cst]),
                   constant_names=np.array(list(cst)), table_every_100th=tbl[::100].copy())
        for lm, ncol, mst in SETS:
            out.update(case(L, cst, args.seed, lm, ncol, mst))
        # the Jacobian filter's refusal is in the fixture: a column that passes the heating-rate filter and fails the thresholds
        steep = sum(int(np.sum((out["L%d_ref_heat_ok" % lm] == 1) & (out["L%d_ref_doconvec" % lm] == 0))) for lm, _, _ in SETS)
        print("columns the Jacobian filter refuses: %d" % steep)
        assert steep >= 1, "no column passes the heating-rate filter and fails the Jacobian filter: draw again with another seed"
        path = os.path.join(HERE, "convection_ref.npz")
        np.savez_compressed(path, **out)
        print("wrote %s: %d bytes" % (path, os.path.getsize(path)))
        assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
