"""Generates tests/golden/cloud_ref.npz by running the reference's own cloud scheme -- CLOUD_DRIVER, CLOUD_DRIVER_D, CLOUD_DRIVER_B of
physics/moist/cloud{,_tl,_ad}.F90 -- behind its own RASE0, compiled where they lie under the reference checkout, through our bind(C)
wrappers cloud_wrap.F90 and convection_wrap.F90 on generated soundings.  Everything compiled goes into a temporary directory; the fixture
holds data only.

    python tests/golden/make_cloud_golden.py [--seed N] [--time NCOL LM]

The reference's one outside symbol, LAPACK's DGEEV, is supplied by cloud_wrap.F90, which forwards the 8 x 8 matrix to eig() below
(numpy.linalg.eigvals, LAPACK's own DGEEV) and returns the real parts.  The stand-in records the Jacobian's largest |WR| and the switch
cloud_pertmod per cell, and can force the switch.  What set_ltraj (fv3jedi_lm_moist_mod.F90:834-874) prepares -- the IceFraction split and
the fractions -- is restated here in numpy.  The draw, what the generator asserts about it and how the tolerance is measured: DESIGN.md
section 5."""
import argparse
import ctypes as C
import os
import subprocess
import tempfile
import time
import numpy as np
import make_convection_golden as G

HERE = os.path.dirname(os.path.abspath(__file__))
REF = G.REF
_dp, _ip = G._dp, G._ip
DT = G.DT
KTOP = 30
SETS = [(40, 12, 2), (72, 12, 2), (72, 12, 1), (20, 12, 1)]      # lm, columns, do_phy_mst
OUT8 = ["th", "q", "QI_ls", "QL_ls", "QI_con", "QL_con", "CF_ls", "CF_con"]
SRC = ["CNV_DQLDT", "CNV_MFD", "CNV_PRC3", "CNV_UPDF"]
SPLIT = ["QILST", "QLLST", "QICNT", "QLCNT", "ILSF", "ICNF", "LLSF", "LCNF"]
CONST = ["RUNIV", "KAPPA", "AIRMW", "H2OMW", "GRAV", "ALHL", "ALHF", "PI", "RGAS", "CP", "VIREPS", "ALHS", "TICE", "RVAP", "P00"]


def tag(lm, mst):
    return "L%dm%d" % (lm, mst)


def cloud_params(im):
    """create :151-211"""
    r = [10.0, 4.0, 4.0, 1.0, 2.0e-3, 8.0e-4, 2.0, 1.0, -1.0, 0.0, 1.3, 1.0e-9, 3.3e-4, 20., 4.8, 4.8, 230., 1.0, 1.0, 230., 14400., 50., 0.01, 0.1, 200., 0., 0., 0.5,
         0.5, 2000., 0.8, 0.5, -40.0, 1.0, 4.0, 0.0, 0.0, 0.0, 1.0e-3, 8.0e-4, 1.0, 0.80, 1.0, 0.0, 750.0, 0.81, 1.0, 1.0, 0.0, 0.0, 10.e-6, 20.e-6, 21.e-6, 40.e-6,
         30.e-6, 1.0, 1.0]
    ims = 4 * im
    r[41] = 0.80 if ims <= 200 else 0.90 if ims <= 400 else 0.93 if ims <= 800 else 0.95 if ims <= 1600 else 0.97
    r[45] = r[41] + 0.01
    return np.array(r)


def build_reference(tmp):
    m, u = os.path.join(REF, "physics", "moist"), os.path.join(REF, "utils")
    srcs = [os.path.join(u, "MAPL_Constants.F90"), os.path.join(m, "qsat_util.F90"), os.path.join(m, "convection.F90"), os.path.join(m, "convection_tl.F90"),
            os.path.join(u, "tapenade", "adBuffer.f"), os.path.join(m, "convection_ad.F90"), os.path.join(HERE, "convection_wrap.F90"),
            os.path.join(m, "cloud.F90"), os.path.join(m, "cloud_tl.F90"), os.path.join(m, "cloud_ad.F90"), os.path.join(HERE, "cloud_wrap.F90")]
    objs = []
    for n, s in enumerate(srcs):
        o = os.path.join(tmp, "f%d.o" % n)
        subprocess.check_call(["amdflang"] + G.FFLAGS + ["-module-dir", tmp, "-c", s, "-o", o], cwd=tmp)
        objs.append(o)
    o = os.path.join(tmp, "adStack.o")
    subprocess.check_call(["amdclang", "-O2", "-fPIC", "-c", os.path.join(u, "tapenade", "adStack.c"), "-o", o], cwd=tmp)
    so = os.path.join(tmp, "libcloud_ref.so")
    subprocess.check_call(["amdflang", "-shared", "-o", so] + objs + [o], cwd=tmp)
    return C.CDLL(so)


class Eig:
    """the stand-in for DGEEV's second call: records per call the largest |WR| and the switch of cloud_tl.F90:466-479; force: WR = 2"""
    def __init__(self, L):
        self.rec, self.force, self.on = [], False, False
        self.cb = C.CFUNCTYPE(None, _dp, _dp)(self.call)
        L.cloud_set_eig(self.cb)

    def call(self, a, wr):
        J = np.ctypeslib.as_array(a, (64,)).reshape(8, 8, order="F")
        w = np.linalg.eigvals(J).real
        if self.force:
            w = np.full(8, 2.0)
        for n in range(8):
            wr[n] = w[n]
        if self.on:
            m = float(np.abs(w).max())
            self.rec.append((m, int(m > 1.001 or J[0, 0] < 0.6 or J[1, 0] > 0.75e-4 or J[4, 0] < -0.75e-4 or J[6, 0] < -1.10)))


class Cloud:
    def __init__(self, L, lm, cpar, mst, eig):
        self.L, self.lm, self.cpar, self.mst, self.eig = L, lm, np.ascontiguousarray(cpar), mst, eig

    def run(self, which, x, xd, ple, s, sd, frland, khu, khl, record=False):
        """x [8, lm, ncol], s [4, lm, ncol] ... -> x, xd, sd after the call (fresh copies)"""
        T = lambda A: np.ascontiguousarray(np.transpose(np.asarray(A, dtype=np.float64), (0, 2, 1)))
        ncol = x.shape[2]
        X, XD, S, SD = T(x), T(xd), T(s), T(sd)
        p = np.ascontiguousarray(np.asarray(ple, dtype=np.float64).T)
        P = lambda a: a.ctypes.data_as(_dp)
        ku, kl = np.ascontiguousarray(np.rint(khu).astype(np.int32)), np.ascontiguousarray(np.rint(khl).astype(np.int32))
        fr = np.ascontiguousarray(frland, dtype=np.float64)
        self.eig.rec, self.eig.on = [], record
        self.L.cloud_run(C.c_int(which), C.c_int(ncol), C.c_int(self.lm), C.c_double(DT), P(X), P(XD), P(p), P(S), P(SD), P(fr), ku.ctypes.data_as(_ip),
                         kl.ctypes.data_as(_ip), P(self.cpar), C.c_int(self.mst))
        self.eig.on = False
        return T(X), T(XD), T(SD)


def qsat(t, ph, tbl, cst):
    """DQSAT_BAC's QS in numpy (ph hPa)"""
    ti = np.clip(t, 150.0, 333.0 - .001)
    tt = (ti - 150.0) * 100 + 1
    it = tt.astype(int)
    qq = (tt - it) * (tbl[it] - tbl[it - 1]) + tbl[it - 1]
    esfac = cst["H2OMW"] / cst["AIRMW"]
    return esfac * qq / (ph * 100.0 - (1.0 - esfac) * qq)


def icefraction(temp):
    """utils/fv3jedi_lm_utils_mod.F90:295-319"""
    f = np.where(temp <= 233.16, 1.0, np.where(temp <= 273.16, 1.0 - (temp - 233.16) / (273.16 - 233.16), 0.0))
    f = np.minimum(np.maximum(f, 0.0), 1.0)
    return (f * f) * (f * f)


def draw_cloud(rng, a, lm, ncol, tbl, cst):
    """QLS, QCN, cfcn where RH is high; khu <= khl (indices) in the lower troposphere; the two special cells above level 30"""
    pe = G.edges(lm)
    pm = 0.5 * (pe[1:] + pe[:-1])[:, None] / 100.0
    rh = a["qv"] / qsat(a["T"], pm, tbl, cst)
    w = np.clip((rh - 0.5) / 0.4, 0.0, 1.0) ** 2 * (pm > 150.0)
    a["QLS"] = 6e-4 * w * rng.random((lm, ncol))
    a["QCN"] = 4e-4 * w * rng.random((lm, ncol)) * (rng.random((lm, ncol)) < 0.7)
    a["cfcn"] = 0.6 * w * rng.random((lm, ncol)) * (a["QCN"] > 0)
    a["khu"] = (lm - 12 + rng.integers(0, 5, ncol)).astype(np.float64)
    a["khl"] = np.minimum(lm - 3, a["khu"] + rng.integers(0, 6, ncol)).astype(np.float64)
    # every third column: the lowest three levels close to saturation and a thick cold large-scale cloud aloft, where the Jacobian of
    # LS_CLOUD_D has eigenvalues beyond 1.001
    wet = np.arange(ncol) % 3 == 2
    for l in range(lm - 3, lm):
        a["qv"][l] = np.where(wet, rng.uniform(0.975, 0.995, ncol) * qsat(a["T"][l], pm[l], tbl, cst), a["qv"][l])
    cold = (a["T"] < 240.0) & (pm > 150.0) & wet[None, :]
    a["QLS"] = np.where(cold, 5e-4 * rng.uniform(0.9, 1.2, (lm, ncol)), a["QLS"])
    # above every level RASE0 touches: level 2 of column 0 is supersaturated by 30 %, level 1 of column 1 is slightly negative
    # (by the temperature the cloud scheme sees: theta of the JEDI pk times the GEOS Exner function)
    p = G.prepared(a, cst)
    plo = 0.5 * (p["ple"][:-1] + p["ple"][1:])
    tg = p["th"] * (plo / 1000.0) ** (cst["RGAS"] / cst["CP"])
    a["qv"][1, 0] = 1.3 * qsat(tg[1, 0], plo[1, 0], tbl, cst)
    a["qv"][0, 1] = -1e-7
    return a


def everything(R, K, a, cst, Xh, Yh, move=None, force=False):
    """all the reference gives for the columns a: RASE0, the split, CLOUD_DRIVER, _D and _B; each call on fresh copies.  Xh: the host's
    perturbation of theta, qv, qi, ql, cfcn and the four sources; Yh: the forcing of theta, qv, qi, ql, cfcn.  step_tl :429-438 splits qi, ql
    by the fractions and clears cflsp; step_ad :542-551 gives both parts the full adjoint"""
    lm, ncol = a["T"].shape
    p = G.prepared(a, cst, move)
    s0 = R.rase0(a, p)
    plo = 0.5 * (p["ple"][:-1] + p["ple"][1:])
    temp = p["th"] * (plo / 1000.0) ** (cst["RGAS"] / cst["CP"])
    fqi = icefraction(temp)
    r = {"QILST": a["QLS"] * fqi, "QLLST": a["QLS"] * (1 - fqi), "QICNT": a["QCN"] * fqi, "QLCNT": a["QCN"] * (1 - fqi)}
    with np.errstate(divide="ignore", invalid="ignore"):
        si, sl = r["QILST"] + r["QICNT"], r["QLLST"] + r["QLCNT"]
        r["ILSF"] = np.where(si > 0, r["QILST"] / si, 0.0); r["ICNF"] = np.where(si > 0, r["QICNT"] / si, 0.0)
        r["LLSF"] = np.where(sl > 0, r["QLLST"] / sl, 0.0); r["LCNF"] = np.where(sl > 0, r["QLCNT"] / sl, 0.0)
    x = np.stack([s0[0], s0[1], r["QILST"], r["QLLST"], r["QICNT"], r["QLCNT"], np.zeros_like(temp), a["cfcn"]])
    s = np.stack(s0[2:6])
    ple = np.asarray(G.pressures(a["delp"])[0], dtype=np.float64)      # Pa, as ltraj%ple
    z8, z4 = np.zeros_like(x), np.zeros_like(s)
    args = (a["frland"], a["khu"], a["khl"])
    X = np.stack([Xh[0], Xh[1], Xh[2] * r["ILSF"], Xh[3] * r["LLSF"], Xh[2] * r["ICNF"], Xh[3] * r["LCNF"], 0 * Xh[0], Xh[4], Xh[5], Xh[6], Xh[7], Xh[8]])
    Y = np.stack([Yh[0], Yh[1], Yh[2], Yh[3], Yh[2], Yh[3], 0 * Yh[0], Yh[4]])
    r["X12"], r["Y8"] = X, Y
    for n, k in enumerate(SRC):
        r["src_" + k] = s[n]
    r["in_th"], r["in_q"] = x[0], x[1]
    o, _, _ = K.run(0, x, z8, ple, s, z4, *args)
    for n, k in enumerate(OUT8):
        r["out_" + k] = o[n]
    K.eig.force = force
    _, xd, _ = K.run(1, x, X[:8], ple, s, X[8:], *args, record=True)
    K.eig.force = False
    for n, k in enumerate(OUT8):
        r["tl_" + k] = xd[n]
    if K.mst == 2:
        rec = np.array(K.eig.rec).reshape(ncol, max(lm - KTOP + 1, 0), 2)
        wr = np.zeros((lm, ncol)); pm = np.ones((lm, ncol))
        wr[KTOP - 1:] = rec[:, :, 0].T; pm[KTOP - 1:] = rec[:, :, 1].T
        r["wr"], r["pertmod"] = wr, pm
    else:
        r["wr"], r["pertmod"] = np.zeros((lm, ncol)), np.ones((lm, ncol))
    _, xb, sb = K.run(2, x, Y, ple, s, z4, *args)
    for n, k in enumerate(OUT8):
        r["ad_" + k] = xb[n]
    for n, k in enumerate(SRC):
        r["ad_" + k] = sb[n]
    return r, p


def amplitudes(ref):
    """perturbation of the eight fields and the four sources; forcing of the eight outputs"""
    ax = [0.5, 1e-4, 1e-5, 1e-5, 0.05] + [0.1 * max(float(np.abs(ref["src_" + k]).max()), 1e-12) for k in SRC]
    ay = [1.0, 1e3, 1e4, 1e4, 1.0]
    return np.array(ax)[:, None, None], np.array(ay)[:, None, None]


def case(L, cst, tbl, seed, lm, ncol, mst, eig):
    R = G.Ref(L, lm, G.ras_params(12), cst); R.maxcondep = 1 if mst == 1 else 10
    cpar = cloud_params(12)
    K = Cloud(L, lm, cpar, mst, eig)
    ndraw = ncol + max(1, ncol // 10)      # at most 10 % of the draws may be dropped
    rng = np.random.default_rng([seed, lm, mst])
    a = draw_cloud(rng, G.draw(rng, lm, ndraw), lm, ndraw, tbl, cst)
    z = np.zeros((9, lm, ndraw))
    ref0, _ = everything(R, K, a, cst, z, z[:5])
    ax, ay = amplitudes(ref0)
    X = (rng.standard_normal((9, lm, ndraw)) * ax).astype(np.float32).astype(np.float64)
    Y = (rng.standard_normal((5, lm, ndraw)) * ay).astype(np.float32).astype(np.float64)
    # cloud_ad.F90:853-854 clears the incoming adjoint of CF_con in every level of the loop, which cloud_tl.F90 has no counterpart of: the
    # reference's pair is adjoint only for a forcing without CF_con there, and that is what is drawn
    Y[4, KTOP - 1:] = 0.0
    ref, _ = everything(R, K, a, cst, X, Y)
    judged = [k for k in ref if k[:3] in ("out", "tl_", "ad_")]
    worst = np.zeros(ndraw)
    for sgn in (1.0, -1.0):
        o, _ = everything(R, K, a, cst, X, Y, sgn * 1e-12 * rng.uniform(0.5, 1.0, (2, lm, ndraw)))
        for k in judged:
            worst = np.maximum(worst, G.colrel(o[k] - ref[k], ref[k]))
        worst = np.maximum(worst, 1.0 * np.any(o["pertmod"] != ref["pertmod"], axis=0))
    near = np.any(np.abs(ref["wr"] - 1.001) <= 1e-6, axis=0)
    keep = (worst <= 1e-6) & ~near
    assert keep[0] and keep[1], "the two special columns sit at a switch: draw again with another seed"
    idx = np.nonzero(keep)[0][:ncol]
    assert idx.size == ncol, ("more than 10 % of the draws sit at a switch", int((~keep).sum()), ndraw)
    a = {k: np.ascontiguousarray(v[..., idx]) for k, v in a.items()}
    X, Y = np.ascontiguousarray(X[..., idx]), np.ascontiguousarray(Y[..., idx])
    ref, p = everything(R, K, a, cst, X, Y)
    spread = {k: 0.0 for k in judged}
    rs = np.random.default_rng([seed, lm, mst, 999])
    for n in range(8):
        o, _ = everything(R, K, a, cst, X, Y, 1e-15 * rs.uniform(-1, 1, (2, lm, ncol)))
        for k in spread:
            spread[k] = max(spread[k], float(G.colrel(o[k] - ref[k], ref[k]).max()))
    t = tag(lm, mst)
    lhs = sum(float(np.sum(ref["tl_" + k] * ref["Y8"][n])) for n, k in enumerate(OUT8))
    rhs = sum(float(np.sum(ref["ad_" + k] * ref["X12"][n])) for n, k in enumerate(OUT8 + SRC))
    res = abs(lhs - rhs) / abs(lhs)
    print("%s: %d columns, dropped %d of %d; reference dot product residual %.1e; pertmod = 0 in %d of %d cells, largest |WR| %.4f"
          % (t, ncol, int((~keep).sum()), ndraw, res, int((ref["pertmod"] == 0).sum()), ref["pertmod"].size, ref["wr"].max()))
    print("%s: spread at 1e-15: " % t + " ".join("%s %.1e" % kv for kv in spread.items()))
    assert res <= 1e-13, res
    # the clean-ups of the tail are seen
    assert ref["out_q"][1, 0] < ref["in_q"][1, 0] and ref["in_q"][1, 0] > 0, "the RH-excess clean-up"
    assert ref["in_q"][0, 1] < 0 and ref["out_q"][0, 1] == 0.0, "the Q < 0 fill"
    other = ref["out_q"][5:min(KTOP - 1, lm), 1] / ref["in_q"][5:min(KTOP - 1, lm), 1]
    assert np.all(other < 1.0) and np.ptp(other) < 1e-12, ("the Q < 0 fill scales the others", other)
    if lm > KTOP:
        cf = ref["out_CF_ls"]
        assert np.any((cf > 0) & (cf < 1)) and np.any(ref["out_CF_con"] > 0)
        assert np.any(ref["out_QI_ls"] + ref["out_QI_con"] > 0) and np.any(ref["out_QL_ls"] + ref["out_QL_con"] > 0)
        # precipitation reaches the surface level: cloud liquid perturbed aloft only moves q or T of level LM (the levels talk through it alone)
        Xp = np.zeros_like(X); Xp[3, KTOP - 1:lm - 5] = 1e-5      # ql
        rp, _ = everything(R, K, a, cst, Xp, Y)
        assert np.any(rp["tl_q"][lm - 1] != 0.0) or np.any(rp["tl_th"][lm - 1] != 0.0), "no precipitation reaches the surface level"
    if mst == 2:
        assert np.any(ref["pertmod"][KTOP - 1:] == 0) and np.any(ref["pertmod"][KTOP - 1:] == 1), "both values of cloud_pertmod"
        assert ref["wr"].max() > 1.001
        rf, _ = everything(R, K, a, cst, X, Y, force=True)
        d = sum(G.colrel(rf["tl_" + k] - ref["tl_" + k], ref["tl_" + k]) for k in OUT8)
        assert np.any(d > 1e-8), "the forced switch changes nothing"
    out = {}
    for k in ("delp", "T", "u", "v", "qv", "kcbl", "ts", "frland", "QLS", "QCN", "cfcn", "khl", "khu"):
        out["%s_%s" % (t, k)] = a[k]
    out[t + "_X"] = X.astype(np.float32); out[t + "_Y"] = Y.astype(np.float32)
    for k, v in ref.items():
        if k in ("X12", "Y8"):
            continue
        out["%s_ref_%s" % (t, k)] = v.astype(np.int8) if k == "pertmod" else v
    out[t + "_spread_names"] = np.array(list(spread)); out[t + "_spread"] = np.array([spread[k] for k in spread])
    ak, bk = G.levels(lm)
    out[t + "_ak"] = ak; out[t + "_bk"] = bk; out[t + "_cpar"] = cpar; out[t + "_rpar"] = G.ras_params(12); out[t + "_dot"] = res
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20250611)
    ap.add_argument("--time", type=int, nargs=2, metavar=("NCOL", "LM"), help="only time the compiled reference on one core")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        L = build_reference(tmp)
        cst, tbl = G.constants(L)
        c15 = np.zeros(15); L.cloud_constants(c15.ctypes.data_as(_dp))
        eig = Eig(L)
        if args.time:
            ncol, lm = args.time
            rng = np.random.default_rng(args.seed)
            a = draw_cloud(rng, G.draw(rng, lm, ncol), lm, ncol, tbl, cst)
            for mst in (1, 2):
                R = G.Ref(L, lm, G.ras_params(12), cst); K = Cloud(L, lm, cloud_params(12), mst, eig)
                p = G.prepared(a, cst); s0 = R.rase0(a, p)
                x = np.stack([s0[0], s0[1], 0.3 * a["QLS"], 0.7 * a["QLS"], 0.3 * a["QCN"], 0.7 * a["QCN"], 0 * a["QLS"], a["cfcn"]]); s = np.stack(s0[2:6])
                one8, one4 = np.ones_like(x), np.ones_like(s)
                for name, w in (("CLOUD_DRIVER", 0), ("CLOUD_DRIVER_D", 1), ("CLOUD_DRIVER_B", 2)):
                    ts = []
                    for n in range(3):
                        t0 = time.perf_counter(); K.run(w, x, one8, np.asarray(G.pressures(a["delp"])[0], dtype=np.float64), s, one4, a["frland"], a["khu"], a["khl"]); ts.append(time.perf_counter() - t0)
                    print("reference %s, do_phy_mst %d, one core: %d columns x L%d: %.3f s (best of 3) = %.1f us per column%s"
                          % (name, mst, ncol, lm, min(ts), 1e6 * min(ts) / ncol, " (the eigenvalues by numpy through a callback)" if mst == 2 and w else ""))
            return
        out = dict(sets=np.array([tag(lm, mst) for lm, _, mst in SETS]), dt=DT, ptop=G.PTOP, kappa=G.KAPPA, p00=G.P00, constants=c15, constant_names=np.array(CONST),
                   table_every_100th=tbl[::100].copy())
        for lm, ncol, mst in SETS:
            out.update(case(L, cst, tbl, args.seed, lm, ncol, mst, eig))
        path = os.path.join(HERE, "cloud_ref.npz")
        np.savez_compressed(path, **out)
        print("wrote %s: %d bytes" % (path, os.path.getsize(path)))
        assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
