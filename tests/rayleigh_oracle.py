"""Independent numpy restatement of the Rayleigh damping of the upper layers, RAYLEIGH_SUPER with conserve = .true., not nested,
grid_type < 4 (reference model_tlmadm/fv_dynamics_tlm.F90:1749-1899, adjoint fv_dynamics_adm.F90:2327-2652), for the tests of
fv3lm_set_rayleigh / fv3lm_rayleigh:
  pm(k)       reference pressure of layer k (fv_dynamics_tlm.F90:419-423, p_ref = 1e5: fv_arrays_nlm.F90:403)
  rf(k), kmax the damping profile (:1810-1829; pi = FMS pi_8)
  c2l_ord2    D-grid to lat-lon winds at the cells (C2L_ORD2_TLM, fv_grid_utils_tlm.F90:349-450, do_halo = .false.)
  heating     of pt (temperature) by the kinetic energy removed (:1845-1866), then u, v, w times u2f = 1/(1+rf) (:1868-1896)
in the three modes: nl(), tl() (exact linearisation), ad() (its transpose, written as a scatter -- the product gathers).
Arrays are padded planes [ntile, nk, pj, pi]; Fortran (i, j) sits at [j + 2, i + 2]; compute domain i, j = 1..n.
Non-hydrostatic: the heated temperature is returned as "rf_pt" and pt itself is left alone (pt_in takes pkz from it)."""
import numpy as np

PI_8 = 3.14159265358979323846
P_REF = 1.0e5
SDAY = 86400.0


def pm_levels(ak, bk):
    ph1, ph2 = ak[:-1] + bk[:-1] * P_REF, ak[1:] + bk[1:] * P_REF
    return (ph2 - ph1) / np.log(ph2 / ph1)


def profile(ak, bk, tau, rf_cutoff, ptop, bdt):
    """-> rf[npz], kmax, pm[npz]"""
    pm = pm_levels(ak, bk)
    rf = np.zeros(len(pm)); kmax = 0
    if tau > 0:
        for k in range(len(pm)):
            if not pm[k] < rf_cutoff:
                break
            s = np.sin(0.5 * PI_8 * np.log(rf_cutoff / pm[k]) / np.log(rf_cutoff / ptop))
            rf[k] = abs(bdt) / (tau * SDAY) * (s * s)
            kmax = k + 1
    return rf, kmax, pm


class Rayleigh:
    def __init__(self, c, ak=None, bk=None):
        """c: a harness Case / CubeCase (tau, rf_cutoff, options, metrics, c2l, dims)"""
        o = c.opt
        self.nx, self.ny = c.dims.nx, c.dims.ny
        self.hydro = bool(o.hydrostatic)
        self.rf, self.kmax, self.pm = profile(c.ak if ak is None else ak, c.bk if bk is None else bk, c.tau, c.rf_cutoff, o.ptop, c.dims.dt)
        K = self.kmax
        self.u2f = (1.0 / (1.0 + self.rf[:K]))[None, :, None, None]
        self.den = (o.cp_air - o.rdgas * o.ptop / self.pm[:K])[None, :, None, None]
        self.rcv = 1.0 / (o.cp_air - o.rdgas)
        self.dx, self.dy = c.metrics["dx"], c.metrics["dy"]
        self.c2l = c.c2l
        n, m = self.nx, self.ny
        self.J, self.J1, self.I, self.I1 = slice(3, 3 + m), slice(4, 4 + m), slice(3, 3 + n), slice(4, 4 + n)
        self.UJ, self.VI = slice(3, 4 + m), slice(3, 4 + n)       # u rows js..je+1, v columns is..ie+1

    def _w(self):
        J, J1, I, I1 = self.J, self.J1, self.I, self.I1
        dx0, dx1 = self.dx[:, None, J, I], self.dx[:, None, J1, I]
        dy0, dy1 = self.dy[:, None, J, I], self.dy[:, None, J, I1]
        a = [self.c2l[:, q, None, J, I] for q in range(4)]
        return dx0, dx1, dy0, dy1, a

    def c2l_ord2(self, u, v):
        """(ua, va) at the cells of levels 1..kmax"""
        K, J, J1, I, I1 = self.kmax, self.J, self.J1, self.I, self.I1
        dx0, dx1, dy0, dy1, a = self._w()
        u1 = 2.0 * (u[:, :K, J, I] * dx0 + u[:, :K, J1, I] * dx1) / (dx0 + dx1)
        v1 = 2.0 * (v[:, :K, J, I] * dy0 + v[:, :K, J, I1] * dy1) / (dy0 + dy1)
        return a[0] * u1 + a[1] * v1, a[2] * u1 + a[3] * v1

    def nl(self, s):
        """s: dict u v pt (w) -> new dict (+ rf_pt when non-hydrostatic)"""
        K, J, I = self.kmax, self.J, self.I
        r = {k: v.copy() for k, v in s.items()}
        ua, va = self.c2l_ord2(s["u"], s["v"])
        f = 1.0 - self.u2f * self.u2f
        if self.hydro:
            r["pt"][:, :K, J, I] = s["pt"][:, :K, J, I] + 0.5 * (ua * ua + va * va) * f / self.den
        else:
            w = s["w"][:, :K, J, I]
            r["rf_pt"] = s["pt"][:, :K, J, I] + 0.5 * (ua * ua + va * va + w * w) * f * self.rcv
            r["w"][:, :K, J, I] = self.u2f * w
        r["u"][:, :K, self.UJ, I] = self.u2f * s["u"][:, :K, self.UJ, I]
        r["v"][:, :K, J, self.VI] = self.u2f * s["v"][:, :K, J, self.VI]
        return r

    def tl(self, s, d):
        """R'(s) d"""
        K, J, I = self.kmax, self.J, self.I
        r = {k: v.copy() for k, v in d.items()}
        ua, va = self.c2l_ord2(s["u"], s["v"])
        dua, dva = self.c2l_ord2(d["u"], d["v"])
        f = 1.0 - self.u2f * self.u2f
        if self.hydro:
            r["pt"][:, :K, J, I] = d["pt"][:, :K, J, I] + f * (ua * dua + va * dva) / self.den
        else:
            w, dw = s["w"][:, :K, J, I], d["w"][:, :K, J, I]
            r["rf_pt"] = d["pt"][:, :K, J, I] + f * self.rcv * (ua * dua + va * dva + w * dw)
            r["w"][:, :K, J, I] = self.u2f * dw
        r["u"][:, :K, self.UJ, I] = self.u2f * d["u"][:, :K, self.UJ, I]
        r["v"][:, :K, J, self.VI] = self.u2f * d["v"][:, :K, J, self.VI]
        return r

    def ad(self, s, b):
        """R'(s)^T b: b = adjoints of the outputs (u v pt (w rf_pt: levels 1..kmax, cells)) -> adjoints of the inputs (u v pt (w))"""
        K, J, J1, I, I1 = self.kmax, self.J, self.J1, self.I, self.I1
        r = {k: v.copy() for k, v in b.items() if k != "rf_pt"}
        r["u"][:, :K, self.UJ, I] = self.u2f * b["u"][:, :K, self.UJ, I]
        r["v"][:, :K, J, self.VI] = self.u2f * b["v"][:, :K, J, self.VI]
        ua, va = self.c2l_ord2(s["u"], s["v"])
        f = 1.0 - self.u2f * self.u2f
        if self.hydro:
            hb = b["pt"][:, :K, J, I]; fac = f / self.den
        else:
            hb = b["rf_pt"]; fac = f * self.rcv
            r["pt"][:, :K, J, I] += hb
            r["w"][:, :K, J, I] = self.u2f * b["w"][:, :K, J, I] + fac * s["w"][:, :K, J, I] * hb
        uab, vab = fac * ua * hb, fac * va * hb
        dx0, dx1, dy0, dy1, a = self._w()
        u1b, v1b = a[0] * uab + a[2] * vab, a[1] * uab + a[3] * vab
        r["u"][:, :K, J, I] += 2.0 * dx0 * u1b / (dx0 + dx1)
        r["u"][:, :K, J1, I] += 2.0 * dx1 * u1b / (dx0 + dx1)
        r["v"][:, :K, J, I] += 2.0 * dy0 * v1b / (dy0 + dy1)
        r["v"][:, :K, J, I1] += 2.0 * dy1 * v1b / (dy0 + dy1)
        return r
