"""Generates tests/golden/bl_driver_ref.npz by running the reference's own BL_DRIVER (physics/turbulence/bldriver.F90 with the two
modules it uses, fv3jedi_lm_kinds_mod and fv3jedi_lm_const_mod, compiled where they lie under /root/reference/src) through our
bind(C) wrapper bl_driver_wrap.F90 on generated columns.  Everything compiled goes into a temporary directory; the fixture holds data
only: the drawn inputs, the parameters, the 13 outputs of the routine and the measured conditioning that sets the tests' tolerance.

    python tests/golden/make_bl_driver_golden.py [--seed N] [--ncol N] [--time NCOL LM]

What is drawn, what the generator asserts about its own draw (by the reference alone) and how the tolerance is measured: DESIGN.md §5."""
import argparse
import ctypes as C
import os
import subprocess
import tempfile
import time
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("FV3LM_REFERENCE_SRC", "/root/reference/src")      # the reference checkout, as in oracle/ref/Makefile
FFLAGS = ["-O2", "-fPIC", "-cpp", "-fdefault-real-8", "-fdefault-double-8"]
_dp = C.POINTER(C.c_double)
LD = np.longdouble

# the constants of fv3jedi_lm_const_mod the callers of BL_DRIVER use (set_ltraj: p00, kappa), evaluated as the module does
RUNIV, AIRMW = 8314.47, 28.965
RDRY = RUNIV / AIRMW
KAPPA = RDRY / (3.5 * RDRY)
P00 = 100000.0
PTOP = 1.0
DT = 1800.0

OUT3 = ["AKV", "BKV", "CKV", "AKS", "BKS", "CKS", "AKQ", "BKQ", "CKQ", "EKV", "FKV"]      # order of raw_out
OUTS = OUT3 + ["ZPBL", "CT"]
IN3 = ["u", "v", "th", "qv", "qi", "ql"]
SFC = ["FRLAND", "FROCEAN", "VARFLT", "ZPBL", "CM", "CT", "CQ", "USTAR", "BSTAR"]        # order of the sfc argument


def default_params(kpblmin):
    """the set documented at bldriver.F90:100-127"""
    r = [5.0, 160.0, 1.0, 160.0, 1.0, 3000., 3000., 0.1, 0.0030, 2.5101471e-8, 1500., 500., 1.0, 0.75, 0.50, 0.25, 0.85, 0.45, 20.0,
         1.5e-3, 0.5, -999.]
    return np.array(r), np.array([kpblmin, 1, 1, 0], dtype=np.int32)


def build_reference(tmp):
    srcs = [os.path.join(REF, "utils", "fv3jedi_lm_kinds_mod.F90"), os.path.join(REF, "utils", "fv3jedi_lm_const_mod.F90"),
            os.path.join(REF, "physics", "turbulence", "bldriver.F90"), os.path.join(HERE, "bl_driver_wrap.F90")]
    objs = []
    for n, s in enumerate(srcs):
        o = os.path.join(tmp, "f%d.o" % n)
        subprocess.check_call(["amdflang"] + FFLAGS + ["-module-dir", tmp, "-c", s, "-o", o], cwd=tmp)
        objs.append(o)
    so = os.path.join(tmp, "libbl_driver_ref.so")
    subprocess.check_call(["amdflang", "-shared", "-o", so] + objs, cwd=tmp)
    return C.CDLL(so)


def run_reference(L, a, rpar, ipar):
    """a: u v th qv qi ql [lm, ncol], pe [lm + 1, ncol], the nine surface fields [ncol] -> the 13 outputs"""
    lm, ncol = a["u"].shape
    w = {k: np.ascontiguousarray(a[k], dtype=np.float64).copy() for k in IN3 + ["pe"] + SFC}
    o = {k: np.zeros((lm, ncol)) for k in OUT3}
    P = lambda x: x.ctypes.data_as(_dp)
    rp = np.ascontiguousarray(rpar, dtype=np.float64); ip = np.ascontiguousarray(ipar, dtype=np.int32)
    L.bl_driver_wrap(C.c_int(ncol), C.c_int(lm), C.c_double(DT), P(w["u"]), P(w["v"]), P(w["th"]), P(w["qv"]), P(w["pe"]), P(w["qi"]), P(w["ql"]),
                     P(w["FRLAND"]), P(w["FROCEAN"]), P(w["VARFLT"]), P(w["ZPBL"]), P(w["CM"]), P(w["CT"]), P(w["CQ"]), P(rp),
                     ip.ctypes.data_as(C.POINTER(C.c_int)), P(w["USTAR"]), P(w["BSTAR"]),
                     P(o["AKS"]), P(o["BKS"]), P(o["CKS"]), P(o["AKQ"]), P(o["BKQ"]), P(o["CKQ"]), P(o["AKV"]), P(o["BKV"]), P(o["CKV"]),
                     P(o["EKV"]), P(o["FKV"]))
    o["ZPBL"], o["CT"] = w["ZPBL"], w["CT"]
    return o


def ice_fraction(t):
    """IceFraction (utils/fv3jedi_lm_utils_mod.F90:295-319)"""
    f = np.where(t <= 233.16, 1.0, np.where(t <= 273.16, 1.0 - (t - 233.16) / (273.16 - 233.16), 0.0))
    return np.clip(f, 0.0, 1.0) ** 4


def sigma(lm):
    """interfaces 0..lm of a stretched grid: thin layers at the surface and, in pressure, at the top"""
    return np.sin(0.5 * np.pi * np.arange(lm + 1) / lm) ** 2.5


def pressures(delp):
    """pe, pk, as compute_pressures, in extended precision, rounded once"""
    lm, ncol = delp.shape
    pe = np.zeros((lm + 1, ncol), dtype=LD); pe[0] = PTOP
    for l in range(lm):
        pe[l + 1] = pe[l] + LD(1) * delp[l]
    k = LD(KAPPA)
    pk = (pe[1:] ** k - pe[:-1] ** k) / (k * (np.log(pe[1:]) - np.log(pe[:-1])))
    return pe, pk


def draw(rng, lm, ncol):
    ps = rng.uniform(95000., 102000., ncol)
    s = sigma(lm)
    pe0 = PTOP + (ps[None, :] - PTOP) * s[:, None]
    delp = np.diff(pe0, axis=0) * (1.0 + 0.02 * rng.uniform(-1, 1, (lm, ncol)))
    pe, pk = pressures(delp)
    pm = np.asarray(0.5 * (pe[1:] + pe[:-1]), dtype=np.float64)
    z = -7500.0 * np.log(pm / np.asarray(pe[-1], dtype=np.float64)[None, :])
    ts = rng.uniform(262., 305., ncol); gam = rng.uniform(5.0e-3, 8.0e-3, ncol); zt = rng.uniform(9.0e3, 16.0e3, ncol)
    t = np.where(z < zt, ts - gam * z, ts - gam * zt + 1.0e-3 * (z - zt))
    t = t + rng.uniform(-4., 4., ncol) * np.exp(-z / rng.uniform(80., 300., ncol))      # surface inversion (< 0) or superadiabatic layer (> 0)
    t = t + 0.3 * rng.standard_normal((lm, ncol)) * np.exp(-z / 4000.)
    qv = rng.uniform(2.0e-3, 1.8e-2, ncol) * np.exp(-z / rng.uniform(1800., 3200., ncol)) + 2.0e-6
    cloudy = rng.random(ncol) < 0.6
    qc = cloudy * rng.uniform(1.0e-5, 5.0e-4, ncol) * np.exp(-((z - rng.uniform(400., 3000., ncol)) / rng.uniform(200., 600., ncol)) ** 2)
    qc = np.where(qc > 1.0e-9, qc, 0.0)
    f = ice_fraction(t)
    spd = rng.uniform(0.5, 1.5, ncol) * (3. + 12. * (1. - np.exp(-z / 500.)) + 20. * np.exp(-((z - 11.0e3) / 4.0e3) ** 2))
    ang = rng.uniform(0, 2 * np.pi, ncol) + rng.uniform(-0.8, 0.8, ncol) * (1. - np.exp(-z / 1000.))
    a = dict(delp=delp, T=t, u=spd * np.cos(ang), v=spd * np.sin(ang), qv=qv, qi=qc * f, ql=qc * (1.0 - f))
    a["FRLAND"] = rng.choice([0.0, 0.3, 0.7, 1.0], ncol); a["FROCEAN"] = 1.0 - a["FRLAND"]
    a["VARFLT"] = np.where(rng.random(ncol) < 0.7, rng.uniform(10., 500., ncol), 0.0)
    a["ZPBL"] = rng.uniform(100., 2500., ncol)
    for k in ("CM", "CT", "CQ"):
        a[k] = rng.uniform(0.005, 0.1, ncol)
    a["USTAR"] = rng.uniform(0.05, 0.6, ncol); a["BSTAR"] = rng.uniform(-0.01, 0.03, ncol)
    # what the caller (set_ltraj) hands to BL_DRIVER: pe and theta = p00^kappa T / pk, in extended precision, rounded once
    a["pe"] = np.asarray(pe, dtype=np.float64)
    a["th"] = np.asarray(LD(P00) ** LD(KAPPA) * t / pk, dtype=np.float64)
    return a


def perturbed(rng, a, eps):
    b = dict(a)
    for k in IN3 + ["pe"] + SFC:
        b[k] = a[k] * (1.0 + eps * rng.uniform(-1, 1, a[k].shape))
    return b


def movement(o, ref):
    """per output and column: largest change relative to the column maximum of the output"""
    m = {}
    for k in OUTS:
        d = np.abs(o[k] - ref[k]); s = np.abs(ref[k])
        if d.ndim == 2:
            d, s = d.max(axis=0), s.max(axis=0)
        m[k] = d / np.where(s > 0, s, 1.0)
    return m


def case(L, rng, lm, ncol):
    a = draw(rng, lm, ncol)
    pref = 0.5 * (PTOP + (1.0e5 - PTOP) * (sigma(lm)[1:] + sigma(lm)[:-1]))
    rpar, ipar = default_params(int(np.count_nonzero(pref < 50000.)))
    ref = run_reference(L, a, rpar, ipar)
    for k in OUTS:
        assert np.all(np.isfinite(ref[k])), (lm, k, "not finite")
    # columns near a branch: 8 copies at 1e-13; kept if no output moves by more than 1e-8 of its column maximum
    move = np.zeros(ncol)
    for n in range(8):
        m = movement(run_reference(L, perturbed(rng, a, 1e-13), rpar, ipar), ref)
        move = np.maximum(move, np.max([m[k] for k in OUTS], axis=0))
    keep = move <= 1e-8
    print("L%d: movement at 1e-13: median %.2e, largest %.2e, kept %d of %d" % (lm, np.median(move), move.max(), keep.sum(), ncol))
    assert keep.mean() >= 0.95, (lm, keep.mean())
    # conditioning: 8 copies at 1e-15 (a few ulp), per output the largest movement over the kept columns
    spread = {k: 0.0 for k in OUTS}
    for n in range(8):
        m = movement(run_reference(L, perturbed(rng, a, 1e-15), rpar, ipar), ref)
        for k in OUTS:
            spread[k] = max(spread[k], float(m[k][keep].max()))
    print("L%d: spread at 1e-15: " % lm + " ".join("%s %.1e" % (k, spread[k]) for k in OUTS))
    # the draw exercises the routine (by the reference alone)
    b0 = dict(a); b0["BSTAR"] = np.zeros(ncol)
    cks0 = run_reference(L, b0, rpar, ipar)["CKS"]
    changed = np.any(cks0 != ref["CKS"], axis=0)
    up = a["BSTAR"] > 0
    thv = a["th"] * (1.0 + (1.0 / (18.015 / 28.965) - 1.0) * a["qv"] - a["qi"] - a["ql"])
    qc = a["qi"] + a["ql"]
    st = dict(bstar_pos=up.mean(), bstar_nonpos=(~up).mean(), lock_decides=changed[up].mean(), lock_elsewhere=changed[~up].mean(),
              cks_large=np.mean(np.abs(ref["CKS"]) > 0.1), orodrag=np.mean((ref["BKV"] - 1.0 + ref["AKV"] + ref["CKV"] > 0) & (ref["FKV"] > 0)),
              ri_pos=np.mean(np.diff(thv, axis=0) < 0), ri_neg=np.mean(np.diff(thv, axis=0) > 0), sea=np.mean(a["FROCEAN"] == 1.0),
              hl_ice=np.mean((qc > 1e-6) & (a["T"] <= 253.16)), hl_mix=np.mean((qc > 1e-6) & (a["T"] > 253.16) & (a["T"] < 273.16)),
              hl_liq=np.mean((qc > 1e-6) & (a["T"] >= 273.16)), max_cks=np.abs(ref["CKS"]).max())
    print("L%d: " % lm + " ".join("%s %.3g" % kv for kv in st.items()))
    assert st["bstar_pos"] >= 0.30 and st["bstar_nonpos"] >= 0.20, st
    assert st["lock_decides"] >= 0.80 and st["lock_elsewhere"] == 0.0, st
    assert st["cks_large"] >= 0.10 and st["orodrag"] >= 0.10, st
    assert st["ri_pos"] > 0 and st["ri_neg"] > 0 and st["sea"] >= 0.15, st
    assert st["hl_ice"] > 0 and st["hl_mix"] > 0 and st["hl_liq"] > 0, st
    out = {}
    for k in ["delp", "T", "u", "v", "qv", "qi", "ql"] + SFC:
        out["L%d_%s" % (lm, k)] = np.ascontiguousarray(a[k][..., keep])
    for k in OUTS:
        out["L%d_out_%s" % (lm, k)] = np.ascontiguousarray(ref[k][..., keep])
    out["L%d_spread" % lm] = np.array([spread[k] for k in OUTS])
    out["L%d_rpar" % lm] = rpar; out["L%d_ipar" % lm] = ipar
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=20250301)
    ap.add_argument("--ncol", type=int, default=40)
    ap.add_argument("--time", type=int, nargs=2, metavar=("NCOL", "LM"), help="only time the compiled reference on one core")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        L = build_reference(tmp)
        rng = np.random.default_rng(args.seed)
        if args.time:
            ncol, lm = args.time
            a = draw(rng, lm, 128)          # the routine keeps its work arrays on the stack: 128 columns a call
            rpar, ipar = default_params(lm // 2)
            ts = []
            for n in range(3):
                t0 = time.perf_counter()
                for m in range(-(-ncol // 128)):
                    run_reference(L, a, rpar, ipar)
                ts.append(time.perf_counter() - t0)
            print("reference BL_DRIVER, one core: %d columns x L%d: %.3f s (best of 3) = %.2f us per column" % (ncol, lm, min(ts), 1e6 * min(ts) / ncol))
            return
        out = dict(lms=np.array([72, 127, 20]), outputs=np.array(OUTS), sfc=np.array(SFC), dt=DT, ptop=PTOP, kappa=KAPPA, p00=P00)
        for lm in (72, 127, 20):
            for attempt in range(20):      # a draw that misses one of the conditions is redrawn with another seed; no condition is loosened
                try:
                    out.update(case(L, np.random.default_rng([args.seed, lm, attempt]), lm, args.ncol))
                    break
                except AssertionError as e:
                    print("L%d: seed (%d, %d, %d) redrawn: %s" % (lm, args.seed, lm, attempt, str(e)[:200]))
            else:
                raise SystemExit("no draw met the conditions")
        path = os.path.join(HERE, "bl_driver_ref.npz")
        np.savez_compressed(path, **out)
        print("wrote %s: %d bytes" % (path, os.path.getsize(path)))
        assert os.path.getsize(path) < 1000000


if __name__ == "__main__":
    main()
