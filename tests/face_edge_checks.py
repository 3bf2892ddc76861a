"""The face-edge operators of the product, point by point, against tests/face_oracle.py: the restatement of d2a2c_vect, divergence_corner,
the area-flux scaling of c_sw and what follows it (transport of delp, pt, kinetic energy, vorticity, wind update: c_sw_rest), the first
loops of d_sw and what follows them (B-grid winds, xtp_u / ytp_v, kinetic energy, vorticity, divergence damping, del6_vt_flux:
d_sw_rest, with u_m, v_m by composition), the transports of d_sw through fv_tp_2d with every trajectory scheme and u_m, v_m fully
restated (d_sw_transport, d_sw_transport_nh), a2b_ord4 / one_grad_p and p_grad_c written from the reference's nonlinear
Fortran (whole faces: check; six faces cut into tiles: check_layout).  The library receives
the RESTATEMENT's metrics (harness metrics_hook), with 1e30 in every entry the reference leaves undefined, so product and reference share
the corner points and nothing else.  Values and tangent through put / run_group(TL) / get; the adjoint with seeds on the compared outputs
only, against the transpose of the restated statements (their Jacobian, column by column, by complex step on the trajectory's branches).

Error of a point: relative to the largest reference value of the same output, level and region, the regions being the bulk, the four
edge strips and the four corner blocks (3 cells wide, halo included), so that an edge error is never divided by a bulk maximum.  Bound per
output, region and mode: 8 x the movement of the restatement itself -- float64 on inputs moved by <= 1 ulp (three draws) against
longdouble on the unmoved ones -- and at least 1e-12.  Every point of the rects of groups.py is compared, except those the reference
itself forms from poisoned entries (poison_checks.drop_undefined).  Measured figures: DESIGN.md section 5."""
import numpy as np
from oracle import NL, TL, AD
import groups as G
import face_oracle as fo
import poison_checks as PC

FLOOR, H = 1.0e-12, 1.0e-30
_REST = {}


def restatement(n, dtype):
    if (n, dtype) not in _REST:
        from fv3_jedi_linearmodel_amd import cube
        _REST[(n, dtype)] = fo.face_metrics(cube.cube_corner_points(n), dtype=dtype)
    return _REST[(n, dtype)]


def face_metrics_of(n, face, dtype):
    m, poison, edge, ecorner, _ = restatement(n, dtype)
    M = {k: np.where(poison[k][face], np.nan, v[face]) for k, v in m.items()}       # poison as NaN: a read shows in the reference too
    npx = n + 1
    for r in ((1, npx, 1, 1), (1, npx, npx, npx), (1, 1, 1, npx), (npx, npx, 1, npx)):
        fo.V(M["rsina"], *r)[...] = fo.BIG
    return M, edge[face], ecorner[face]


def restatement_hook(n, face=None, value=1.0e30):
    """metrics_hook: the library gets the float64 restatement, `value` where it is undefined"""
    m, poison, edge, ecorner, _ = restatement(n, np.float64)
    ok = fo.defined(m, poison)
    sel = slice(None) if face is None else slice(face, face + 1)

    def hook(metrics, e, ec):
        assert set(metrics) == set(m)
        return ({k: np.where(ok[k][sel], m[k][sel], value) for k in metrics}, np.where(np.isfinite(edge[sel]), edge[sel], value), ecorner[sel].copy())
    return hook


def detuned(M, lengths=False):
    """sin_sg<k>, cos_sg<k> scaled by factors of their own (1 + 0.01 k, 1 - 0.005 k).  On the gnomonic cube the two cells across a face
    edge hold the same angle, sin_sg(i, j-1, 4) = sin_sg(i, j, 2) to rounding, so which of the two a branch selects cannot show on the
    true metrics; with these factors it does.  The planes stop being a geometry, which no operator here minds: product and restatement
    get the same numbers.
    lengths: dxa, dya as well, by the smooth factor 1 + 0.01 i - 0.007 j, symmetric across no edge: on the cube dxa(0, j) = dxa(1, j) and
    dxa(-1, j) = dxa(2, j) to rounding, so a swap inside the two-sided edge value of xppm / yppm cannot show on the true metrics."""
    f = lambda k: (1 + 0.01 * int(k[-1])) if k.startswith("sin_sg") else (1 - 0.005 * int(k[-1])) if k.startswith("cos_sg") else 1.0
    out = {k: v * f(k) for k, v in M.items()}
    if lengths:
        pj = M["dxa"].shape[-1]
        J, I = np.meshgrid(np.arange(pj) - 2.0, np.arange(pj) - 2.0, indexing="ij")
        for k in ("dxa", "dya"):
            out[k] = M[k] * (1 + 0.01 * I - 0.007 * J)
    return out


regions, region_errors = G.regions, G.region_errors


def compared_mask(c, name, rk):
    one = np.ones((1, c.ny + 7, c.nx + 7))
    return PC.drop_undefined(c, name, G.masked(c, one, rk))[0] != 0


def ulp_move(rng, a):
    return a + rng.integers(-1, 2, size=a.shape) * np.spacing(np.abs(a))


def noise(rng, shape, amp):
    return amp * rng.standard_normal(shape)


def both_signs(vals):
    big = np.max(np.abs(vals))
    return bool((vals > 0).any() and (vals < 0).any() and np.all(np.abs(vals) > 1e-6 * big))


# ------------------------------------------------------------------------------------------------------------ the operators
class CSw:
    level_local = True
    group, ins = "c_sw", ["u", "v"]
    outs = [("ua", "Ah"), ("va", "Ah"), ("utf", "UTF"), ("vtf", "VTF"), ("divgd", "B")]

    def __init__(self, c):
        self.n, self.dt2 = c.nx, 0.5 * c.dt_ac

    def fixed(self, c):
        return {"delp": c.traj["delp"][0], "pt": c.traj["pt"][0]}

    def draw(self, c, rng):
        shp = (c.npz, c.ny + 7, c.nx + 7)
        return {k: noise(rng, shp, 10.0) for k in self.ins}, {k: noise(rng, shp, 1.0) for k in self.ins}

    def apply(self, x, M, edge, ecorner):
        return fo.c_sw_winds(x["u"], x["v"], M, self.n, self.dt2)

    def signs_ok(self, x, M, edge, ecorner):
        """both signs of ut, vt on every edge row and in every corner-halo block, none near zero"""
        o, n = self.apply(x, M, edge, ecorner), self.n
        npx = n + 1
        rows = [fo.V(o["ut"], i, i, 0, n + 1) for i in (1, npx)] + [fo.V(o["vt"], 0, n + 1, j, j) for j in (1, npx)]
        for (i0, j0) in ((1, 0), (npx - 1, 0), (1, n + 1), (npx - 1, n + 1)):        # (ut(0|npx+1, 0|n+1) itself holds no value)
            rows.append(fo.V(o["ut"], i0, i0 + 1, j0, j0))
        for (i0, j0) in ((0, 1), (n + 1, 1), (0, npx - 1), (n + 1, npx - 1)):
            rows.append(fo.V(o["vt"], i0, i0, j0, j0 + 1))
        return all(both_signs(np.real(r)) for r in rows)


class OneGradP:
    group, ins = "one_grad_p", ["u_m", "v_m", "pk", "gzd"]
    outs = [("u_o", "U"), ("v_o", "V")]

    def __init__(self, c):
        self.n, self.dt, self.ptk = c.nx, c.dt_ac, c.opt.ptop ** c.opt.akap

    def fixed(self, c):
        return {}

    def draw(self, c, rng):
        npz, shp = c.npz, (c.npz, c.ny + 7, c.nx + 7)
        shp1 = (npz + 1,) + shp[1:]
        base = (c.opt.ptop + np.arange(npz + 1) * 1.0e5 / npz) ** c.opt.akap
        T = dict(u_m=noise(rng, shp, 10.0), v_m=noise(rng, shp, 10.0), pk=base[:, None, None] * (1 + noise(rng, shp1, 0.01)),
                 gzd=1.0e4 * (npz + 1 - np.arange(npz + 1))[:, None, None] * (1 + noise(rng, shp1, 0.01)))
        P = dict(u_m=noise(rng, shp, 1.0), v_m=noise(rng, shp, 1.0), pk=noise(rng, shp1, 1e-2), gzd=noise(rng, shp1, 10.0))
        return T, P

    def apply(self, x, M, edge, ecorner):
        return fo.one_grad_p(x["u_m"], x["v_m"], x["pk"], x["gzd"], M, edge, ecorner, self.n, self.dt, self.ptk)

    def signs_ok(self, *a):
        return True


class PGradC:
    group, ins = "p_grad_c", ["pkc", "gz", "uc1", "vc1"]
    outs = [("uc", "V"), ("vc", "U")]

    def __init__(self, c):
        self.n, self.dt2 = c.nx, 0.5 * c.dt_ac

    fixed = OneGradP.fixed

    def draw(self, c, rng):
        T, P = OneGradP.draw(self, c, rng)
        ren = dict(u_m="uc1", v_m="vc1", pk="pkc", gzd="gz")
        return {ren[k]: v for k, v in T.items()}, {ren[k]: v for k, v in P.items()}

    def apply(self, x, M, edge, ecorner):
        return fo.p_grad_c(x["pkc"], x["gz"], x["uc1"], x["vc1"], M, self.n, self.dt2)

    def signs_ok(self, *a):
        return True


class DSw:
    """the first loops of d_sw: uc, vc -> crx, cry, xfx, yfx; the other inputs of the group are given plausible data and no seed"""
    level_local = True
    group, ins = "d_sw", ["uc", "vc"]
    outs = [("crx", "CX"), ("cry", "CY"), ("xfx", "CX"), ("yfx", "CY")]

    def __init__(self, c):
        self.n, self.dt = c.nx, c.dt_ac

    def fixed(self, c):
        rng = np.random.default_rng(5)
        shp = (c.npz, c.ny + 7, c.nx + 7)
        out = {"delp": c.traj["delp"][0], "pt": c.traj["pt"][0]}
        out.update({k: noise(rng, shp, 5.0) for k in ("u", "v", "ua", "va")})
        out.update({k: noise(rng, shp, 1e-6) for k in ("divgd",)})
        out.update({k: np.zeros(shp) for k in ("mfx", "mfy", "cx", "cy")})
        return out

    def draw(self, c, rng):
        shp = (c.npz, c.ny + 7, c.nx + 7)
        return {k: noise(rng, shp, 10.0) for k in self.ins}, {k: noise(rng, shp, 1.0) for k in self.ins}

    def apply(self, x, M, edge, ecorner):
        return fo.d_sw_courant(x["uc"], x["vc"], M, self.n, self.dt)

    def signs_ok(self, x, M, edge, ecorner):
        """both signs of the Courant numbers on every edge row and in every corner-halo block (rows j <= 0, j >= npy of crx, columns
        i <= 0, i >= npx of cry, next to the face edges), none near zero"""
        o, n = self.apply(x, M, edge, ecorner), self.n
        npx = n + 1
        rows = [fo.V(o["crx"], i, i, 1, n) for i in (1, npx)] + [fo.V(o["cry"], 1, n, j, j) for j in (1, npx)]
        for i in (1, 2, npx - 1, npx):
            rows += [fo.V(o["crx"], i, i, -2, 0), fo.V(o["crx"], i, i, npx, n + 3)]
        for j in (1, 2, npx - 1, npx):
            rows += [fo.V(o["cry"], -2, 0, j, j), fo.V(o["cry"], npx, n + 3, j, j)]
        return all(both_signs(np.real(r)) for r in rows)


class CSwRest:
    """c_sw after the area fluxes (sw_core_nlm.F90:177-486): delp, pt, u, v -> delpc, ptc, the C-grid kinetic energy and absolute
    vorticity, the time-centred winds uc1, vc1 and the d2a2c_vect winds uc0, vc0 they start from.  The operator's name in OPERATORS is
    not the library's group: the whole group c_sw runs and the work fields are read back."""
    level_local = True
    group, ins = "c_sw", ["delp", "pt", "u", "v"]
    outs = [("delpc", "Ah"), ("ptc", "Ah"), ("ke_c", "Ah"), ("vort_c", "B"), ("uc1", "V"), ("vc1", "U"), ("uc0", "UTF"), ("vc0", "VTF")]

    def __init__(self, c):
        self.n, self.dt2 = c.nx, 0.5 * c.dt_ac

    def fixed(self, c):
        return {}

    def draw(self, c, rng):
        shp = (c.npz, c.ny + 7, c.nx + 7)
        T = dict(delp=1.0e3 * (1 + noise(rng, shp, 0.1)), pt=300.0 * (1 + noise(rng, shp, 0.05)), u=noise(rng, shp, 10.0), v=noise(rng, shp, 10.0))
        P = dict(delp=noise(rng, shp, 10.0), pt=noise(rng, shp, 1.0), u=noise(rng, shp, 1.0), v=noise(rng, shp, 1.0))
        return T, P

    def apply(self, x, M, edge, ecorner):
        return fo.c_sw_rest(x["delp"], x["pt"], x["u"], x["v"], M, self.n, self.dt2)

    def signs_ok(self, x, M, edge, ecorner):
        """both signs, none near zero, of: ut, vt on every edge row and corner block (the upwind cell of the transport, CSw.signs_ok);
        ua on the columns 0, 1, npx-1, npx and va on the rows 0, 1, npy-1, npy (the sin_sg / cos_sg forms of the kinetic energy,
        :318-353), whole and in each corner block; the vorticity-flux winds fy1 on the columns 1, npx and fx1 on the rows 1, npy (:438, :453)"""
        if not CSw.signs_ok(self, x, M, edge, ecorner):
            return False
        o, n = self.apply(x, M, edge, ecorner), self.n
        npx = n + 1
        rows = []
        for i in (0, 1, npx - 1, npx):
            rows += [fo.V(o["ua"], i, i, 1, n), fo.V(o["va"], 1, n, i, i)]
            rows += [fo.V(o["ua"], i, i, 1, 3), fo.V(o["ua"], i, i, n - 2, n), fo.V(o["va"], 1, 3, i, i), fo.V(o["va"], n - 2, n, i, i)]
        for i in (1, npx):
            rows += [fo.V(o["fy1v"], i, i, 1, n), fo.V(o["fx1v"], 1, n, i, i)]
        return all(both_signs(np.real(r)) for r in rows)


CAP = 0.20


class CSwRestNh(CSwRest):
    """c_sw_rest on a non-hydrostatic case: w joins the inputs (fill_4corners, sw_core_nlm.F90:211, :258) and wc the outputs (:280-281)"""
    ins = CSwRest.ins + ["w"]
    outs = CSwRest.outs + [("wc", "Ah")]

    def draw(self, c, rng):
        T, P = CSwRest.draw(self, c, rng)
        shp = T["u"].shape
        T["w"], P["w"] = noise(rng, shp, 1.0), noise(rng, shp, 0.1)
        return T, P

    def apply(self, x, M, edge, ecorner):
        return fo.c_sw_rest(x["delp"], x["pt"], x["u"], x["v"], M, self.n, self.dt2, w=x["w"])


class DSwRest:
    """d_sw after its first loops (sw_core_nlm.F90:898-907, :1047-1221, :1260-1434, :1449-1470, :1487-1490): u, v, uc, vc, ua, va, divgd ->
    ra_x, ra_y, the B-grid winds vb, ub, the kinetic energy ke, wk, vort_abs, the divergence dd_c, the corner vorticity vort_b, the damped
    kinetic energy ke2 and the del-4 Laplacian del6_d2 (on the levels whose vorticity damping runs nord_v = 1).  u_m, v_m by composition
    (`compose`): the restated last statements fed the restatement's own ke2 and del6 fluxes and the product's fxv, fyv as data.
    Every level carries two parameter sets, restated (fo.level_rules, fo.level_rules_pert) and held to the library's: the trajectory's
    and the perturbation's.  The linearised model differentiates the damping with the perturbation's set: with split_damp = 0 its
    divergence damping is the trajectory's, its vorticity damping still its own; with split_damp = 1 the VALUES of ke2 (and of u_m, v_m)
    are the trajectory's damping -- nord up to 3, the loop with fill_corners -- and every tangent and adjoint the perturbation's.
    The winds of every level are scaled so that the argument x of max(d2_bg, min(0.20, dddmp x)) straddles the floor / linear switch
    (amplify > 1: the 0.20 cap)."""
    level_local = True
    per_level = True                 # apply takes level0: the level a one-level slice stands for
    group, ins = "d_sw", ["u", "v", "uc", "vc", "ua", "va", "divgd"]
    outs = [("ra_x", "RAX"), ("ra_y", "RAY"), ("vb", "B"), ("ub", "B"), ("ke", "B"), ("wk", "cells"), ("vort_abs", "cells"), ("vort_b", "B"),
            ("dd_c", "B"), ("ke2", "B"), ("del6_d2", "Ah")]
    composed = [("u_m", "U"), ("v_m", "V")]
    amplify = 1.0

    def __init__(self, c):
        self.n, self.dt, self.da_min_c, self.npz = c.nx, c.dt_ac, c.da_min_c, c.npz
        o = c.opt
        self.par, self.parp = [], []
        for k in range(1, c.npz + 1):
            ks = k <= o.n_sponge_pert - 1 and o.hord_ks_pert            # model_tlmadm/dyn_core_tlm.F90:862-875
            iord = o.hord_mt_ks_pert if ks else o.hord_mt_pert
            iord_t = o.hord_mt_ks_traj if (k <= o.n_sponge_pert - 1 and o.hord_ks_traj) else o.hord_mt      # the values' scheme (sw_core_tlm.F90:1987-2002, :2059-2072)
            t = dict(fo.level_rules(o, k, c.npz), dddmp=o.dddmp, d4_bg=o.d4_bg, iord=iord, iord_t=iord_t)
            q = dict(fo.level_rules_pert(o, k), dddmp=o.dddmp_pert, d4_bg=o.d4_bg_pert, iord=iord, iord_t=iord_t)
            if not o.split_damp:        # run_setup_pert has made the two namelists equal; the divergence damping then takes the trajectory's level rule
                q.update(nord=t["nord"], d2_divg=t["d2_divg"], dddmp=t["dddmp"], d4_bg=t["d4_bg"])
            dy = getattr(c, "dy", None)
            if dy is not None:          # the restated level rules against the library's
                ip, rp = dy.level_params(k)
                assert (ip[0], ip[5], ip[6], ip[9]) == (iord, t["nord"], t["nord_v"], q["nord_v"]), (k, ip, t, q)
                assert (rp[0], rp[1], rp[5]) == (t["d2_divg"], t["damp_vt"], q["damp_vt"]), (k, rp, t, q)
            assert t["nord"] in (0, 1, 2, 3) and q["nord"] in (0, 1), (t, q)
            self.par.append(t); self.parp.append(q)
        self.face = c.face if isinstance(c.face, int) else None
        self._next = 0

    def forms(self):
        """(trajectory nord, perturbation nord, iord, trajectory nord_v) of each level, from the level parameters"""
        return [(t["nord"], q["nord"], q["iord"], t["nord_v"]) for t, q in zip(self.par, self.parp)]

    def levels_of(self, name):
        if name == "del6_d2":       # the reference forms the inner Laplacian where a vorticity damping with nord_v = 1 runs
            return [l for l, (t, q) in enumerate(zip(self.par, self.parp))
                    if (t["nord_v"] == 1 and t["damp_vt"] > 1.0e-5) or (q["nord_v"] == 1 and q["damp_vt"] > 1.0e-5)]
        return None

    def fixed(self, c):
        out = {"delp": c.traj["delp"][0], "pt": c.traj["pt"][0]}
        out.update({k: np.zeros((c.npz, c.ny + 7, c.nx + 7)) for k in ("mfx", "mfy", "cx", "cy")})
        return out

    def draw(self, c, rng):
        n, npz = self.n, self.npz
        shp = (npz, n + 7, n + 7)
        face = self.face if self.face is not None else self._next % 6
        self._next += 1
        unit = {k: noise(rng, shp, 1.0) for k in self.ins[:-1]}
        d6 = noise(rng, (6, n + 7, n + 7, npz), n / 1.0e7)              # a divergence: wind / grid length; the halo by the data motion of the
        fo._update_domains(n, "corner", d6)                             # corner-scalar exchange on six faces
        unit["divgd"] = np.ascontiguousarray(np.moveaxis(d6[face], -1, 0))
        x = self.apply(unit, *face_metrics_of(n, face, np.float64))["smag_x"]
        T, P = {k: np.empty(shp) for k in self.ins}, {k: np.empty(shp) for k in self.ins}
        for l, p in enumerate(self.parp):
            xs = p["d2_divg"] / p["dddmp"]
            xl = np.sort(np.abs(fo.V(x[l], 1, n + 1, 1, n + 1)).ravel())
            q = int(0.45 * xl.size)                                     # the switch between two neighbours of the sorted x, clear of both
            if self.amplify > 1.0:                                      # the cap draw: the same quantile of x on the cap's switch instead
                xs = CAP / p["dddmp"]
            amp = xs / np.sqrt(xl[q] * xl[q + 1]) if (p["d2_divg"] < CAP or self.amplify > 1.0) else 0.5 / xl[xl.size // 2]
            for k in self.ins:
                T[k][l] = amp * unit[k][l]
                P[k][l] = 0.1 * amp * rng.standard_normal(shp[1:]) * (n / 1.0e7 if k == "divgd" else 1.0)
        return T, P

    def _level(self, x, l, p, M, edge, ecorner):
        return fo.d_sw_rest_level(*[x[k][..., l, :, :] for k in self.ins], M, edge, ecorner, self.n, self.dt, self.da_min_c, p)

    def apply(self, x, M, edge, ecorner, level0=0):
        """the perturbation's chain on every level (values, and the imaginary part that check() reads as tangent and adjoint); where the
        trajectory's divergence damping differs (split_damp), the real part of ke2 from the trajectory's.  A trajectory hord_mt of its own
        acts inside the level: the values of the xtp_u / ytp_v fluxes alone (fo.d_sw_rest_level)"""
        lv = []
        for l in range(x["u"].shape[-3]):
            t, q = self.par[level0 + l], self.parp[level0 + l]
            o = self._level(x, l, q, M, edge, ecorner)
            if any(t[k] != q[k] for k in ("nord", "d2_divg", "dddmp", "d4_bg")):
                ot = self._level(x, l, t, M, edge, ecorner)
                o["ke2"] = np.real(ot["ke2"]) + 1j * np.imag(o["ke2"]) if np.iscomplexobj(o["ke2"]) else ot["ke2"]
            lv.append(o)
        return {k: np.stack([o[k] for o in lv], axis=-3) for k in lv[0]}

    def compose(self, x, fxv, fyv, M, edge, ecorner):
        """u_m, v_m (:1474-1483, :1527-1539) from the restatement's ke2 and del6 fluxes and the given fxv, fyv.  The values with the
        trajectory's vorticity damping; the tangent (imaginary part) with the perturbation's nord_v, damp_vt where the two differ."""
        o = self.apply(x, M, edge, ecorner)
        us, vs = [], []
        for l in range(x["u"].shape[-3]):
            t, q, L_ = self.par[l], self.parp[l], (lambda a: a[..., l, :, :])

            def momentum(p):
                fx2 = fy2 = None
                if p["damp_vt"] > 1.0e-5:
                    _, fx2, fy2 = fo.del6_vt_flux(p["nord_v"], (p["damp_vt"] * self.da_min_c) ** (p["nord_v"] + 1), L_(o["wk"]), M, self.n)
                return fo.d_sw_momentum(L_(x["u"]), L_(x["v"]), L_(o["ke2"]), L_(fxv), L_(fyv), fx2, fy2, M, self.n, p["damp_vt"])
            a, b = momentum(t)
            if (q["nord_v"], q["damp_vt"]) != (t["nord_v"], t["damp_vt"]):
                ap, bp = momentum(q)
                a, b = np.real(a) + 1j * np.imag(ap), np.real(b) + 1j * np.imag(bp)
            us.append(a); vs.append(b)
        return dict(u_m=np.stack(us, axis=-3), v_m=np.stack(vs, axis=-3))

    def branch_fractions(self, o):
        """{(level, region): (floor, linear, cap)}: the fractions of the corner points 1..npx, 1..npy of the region on which each branch of
        max(d2_bg, min(0.20, dddmp x)) is taken, on every level whose floor lies under the cap (a sponge level with d2_bg = 0.20 has no
        linear branch); and whether every point is clear of a switch"""
        n = self.n
        reg = regions(n, (1, n + 1, 1, n + 1))
        out, clear = {}, True
        for l in range(o["smag_x"].shape[0]):
            p = self.parp[l]
            if p["d2_divg"] >= CAP:
                continue
            y = p["dddmp"] * np.real(o["smag_x"][l]).astype(np.float64)
            for sw in (p["d2_divg"], CAP):
                clear = clear and bool(np.all(np.abs(fo.V(y, 1, n + 1, 1, n + 1) - sw) > 1.0e-6 * sw))
            for name, m in reg.items():
                v = y[m]
                out[(l, name)] = (float(np.mean(v <= p["d2_divg"])), float(np.mean((v > p["d2_divg"]) & (v < CAP))), float(np.mean(v >= CAP)))
        return out, clear

    def signs_ok(self, x, M, edge, ecorner):
        """On the restatement alone: both signs, none near zero, of the Courant numbers (DSw.signs_ok), of vb, ub on every edge row and the
        row next to it (the c > 0 branch of xtp_u / ytp_v with the one-sided edge values), of vc(., 1), vc(., npy), uc(1, .), uc(npx, .)
        (the sin_sg selection of the nord = 0 divergence, :1288, :1308, :1315); on every level (branch_fractions) the floor and the linear
        branch of max(d2_bg, min(0.20, dddmp x)) each at >= 10 % of the points of every region, no point within 1e-6 (relative) of a
        switch.  amplify > 1: instead the cap at >= 10 % of the bulk and at least one point of every strip and corner block."""
        if not DSw.signs_ok(self, x, M, edge, ecorner):
            return False
        o, n = self.apply(x, M, edge, ecorner), self.n
        npx = n + 1
        rows = []
        for i in (1, 2, npx - 1, npx):
            for f in ("vb", "ub"):
                rows += [fo.V(o[f], i, i, 1, npx), fo.V(o[f], 1, npx, i, i)]
        for i in (1, npx):
            rows += [fo.V(x["vc"], 0, n + 1, i, i), fo.V(x["uc"], i, i, 0, n + 1)]
        if not all(both_signs(np.real(r)) for r in rows):
            return False
        frac, clear = self.branch_fractions(o)
        if not clear:
            return False
        for (l, name), (fl, li, cp) in frac.items():
            if self.amplify > 1.0:
                if not (cp >= 0.10 if name == "bulk" else cp > 0.0):
                    return False
            elif fl < 0.10 or li < 0.10:
                return False
        return True


# Which selectors of tests/face_oracle.py's census a trajectory scheme must have taken BOTH ways somewhere on the face (any of the three
# transported fields, any of the four sweeps) before a draw is accepted.  al < 0 of scheme 7 cannot fire on delp or pt (positive): the
# absolute vorticity, of both signs, covers it, and so it does the clip of the six edge values.  near_zero asks for three neighbouring
# cells with dm = 0 EXACTLY, and dm is an exact zero at every local extremum: grid-scale noise holds runs of three extrema all over
# the face, in the outer sweeps too (so under hord = 10, whose inner sweeps run scheme 8, the outer ones cover it).  No flat patch is
# drawn: in an exactly flat run q_i, q_j are flat only to rounding, the last bit decides whether the cell NEXT to the run (whose
# slopes are finite) passes near_zero, and the restatement itself then moves by 7e-7 between float64 and longdouble.
# The schemes 8 and 11 limit by min / max alone.
BULK_BRANCHES = {1: [], 2: [], 333: [], 3: ["smt5", "smt6", "piecewise_linear"], 4: ["smt5", "smt6"], 5: ["bl*br<0"], 6: ["|3b0|<|bl-br|"],
                 7: ["|3b0|<|bl-br|", "al<0"], 8: [], 9: ["|3b0|>|bl-br|", "near_zero", "pd:limited"], 10: ["|3b0|>|bl-br|", "near_zero"], 11: [],
                 12: ["|3b0|>|bl-br|", "near_zero"], 13: ["|3b0|>|bl-br|", "near_zero", "pd:limited"]}
# xtp_u / ytp_v (hord_mt): 7 is 6, 9 limits everywhere, 11 .. 13 are unlimited; each sweep direction on its own.  PERT_PPM runs on ONE cell
# per row next to each edge (n + 1 points): there the draw is asked for both outcomes of al ar < 0 on each side, the two sweeps together.
MT_BRANCHES = {1: [], 2: [], 3: ["smt5", "smt6", "piecewise_linear"], 4: ["smt5", "smt6"], 5: ["bl*br<0"], 6: ["|3b0|<|bl-br|"], 7: ["|3b0|<|bl-br|"],
               8: [], 9: [], 10: ["|dm|<near_zero", "|3b0|>|bl-br|"], 11: [], 12: [], 13: []}
EDGE_BRANCHES = ["std:al*ar<0", "std:a6da<-da2", "std:a6da>da2"]           # PERT_PPM(iv = 1) of the two edge blocks of 8 .. 13, per sweep direction


class DSwTransport(DSwRest):
    """The transports of d_sw and what they feed (sw_core_nlm.F90:898-1031, :1449-1483, :1527-1539): delp, pt, u, v, uc, vc -> the fluxes
    fx, fy of delp, gx, gy of pt, fxv, fyv of the absolute vorticity (fo.fv_tp_2d with the level's hord_dp, hord_tm, hord_vt and the
    del-n damping nord_v / damp_v of delp, nord_t / damp_t of pt), delp_o, pt_o, and u_m, v_m fully restated (the chain of DSwRest with
    the restated vorticity fluxes).  ua, va, divgd are data (fixed).  Where the trajectory's scheme or damping differs from the
    perturbation's, every fv_tp_2d gives its VALUES with the trajectory's and its tangent (the imaginary part) with the perturbation's
    (sw_core_tlm.F90:1664-1682, :1787-1803, :2407-2420), stage by stage, as the reference overwrites fx, fy after the tangent call."""
    ins = ["delp", "pt", "u", "v", "uc", "vc"]
    outs = [("fx", "V"), ("fy", "U"), ("gx", "V"), ("gy", "U"), ("fxv", "V"), ("fyv", "U"), ("delp_o", "A"), ("pt_o", "A"), ("u_m", "U"), ("v_m", "V")]
    composed = []
    seeded = ["delp_o", "pt_o", "u_m", "v_m"]
    metrics64 = True                 # the longdouble reference runs on the float64 metrics the library is given
    detune_dxa = True

    def __init__(self, c):
        DSwRest.__init__(self, c)
        o, self.da_min = c.opt, c.da_min
        self.tr, self.trp = [], []
        for k in range(1, c.npz + 1):
            ks = k <= o.n_sponge_pert - 1                                        # model_tlmadm/dyn_core_tlm.F90:862-875
            t = {f: getattr(o, "hord_%s_ks_traj" % f) if (ks and o.hord_ks_traj) else getattr(o, "hord_" + f) for f in ("dp", "tm", "vt")}
            q = {f: getattr(o, "hord_%s_ks_pert" % f) if (ks and o.hord_ks_pert) else getattr(o, "hord_%s_pert" % f) for f in ("dp", "tm", "vt")}
            t.update(nord_t=min(2, o.nord), damp_t=o.vtdm4 if o.do_vort_damp else 0.0)                     # model/dyn_core_nlm.F90:591-594: before the sponge rules
            q.update(nord_t=min(2, o.nord_pert), damp_t=o.vtdm4_pert if o.do_vort_damp_pert else 0.0)      # dyn_core_tlm.F90:856-859
            dy = getattr(c, "dy", None)
            if dy is not None:
                ip, rp = dy.level_params(k)
                assert (ip[1], ip[2], ip[3], ip[8]) == (q["vt"], q["tm"], q["dp"], t["nord_t"]) and rp[3] == t["damp_t"], (k, ip, rp, t, q)
            self.tr.append(t); self.trp.append(q)
        self.split_damp = bool(o.split_damp)
        rng = np.random.default_rng(5)
        shp = (c.npz, self.n + 7, self.n + 7)
        self.fix6 = [dict(ua=noise(rng, shp, 5.0), va=noise(rng, shp, 5.0), divgd=noise(rng, shp, 1.0e-6)) for _ in range(6)]      # data, face by face
        self._census = self._cen_mt = None
        self._level0 = 0

    def _level(self, x, l, p, M, edge, ecorner):
        if self._cen_mt is not None:                                            # the census of xtp_u / ytp_v
            p = dict(p, cen=self._cen_mt, tag="L%d:mt:" % (self._level0 + l))
        return fo.d_sw_rest_level(*[x[k][..., l, :, :] for k in DSwRest.ins], M, edge, ecorner, self.n, self.dt, self.da_min_c, p)

    @property
    def fix(self):
        return self.fix6[self.face if self.face is not None else 0]

    def fixed(self, c):
        out = dict(self.fix)
        out.update({k: np.zeros((c.npz, c.ny + 7, c.nx + 7)) for k in ("mfx", "mfy", "cx", "cy")})
        return out

    def draw(self, c, rng):
        """grid-scale noise: Courant numbers of either sign well inside (-1, 1); delp, pt positive over a wide range (the positive-definite
        limiter of 9 / 13 needs cells far below their neighbours); u, v of both signs, so the absolute vorticity takes both"""
        n, npz = self.n, self.npz
        shp = (npz, n + 7, n + 7)
        cw = 0.15 * (1.0e7 / n) / self.dt
        T = dict(delp=1.0e3 * np.exp(noise(rng, shp, 0.5)), pt=300.0 * np.exp(noise(rng, shp, 0.5)), u=noise(rng, shp, 30.0), v=noise(rng, shp, 30.0),
                 uc=noise(rng, shp, cw), vc=noise(rng, shp, cw))
        P = dict(delp=noise(rng, shp, 10.0), pt=noise(rng, shp, 1.0), u=noise(rng, shp, 1.0), v=noise(rng, shp, 1.0), uc=noise(rng, shp, 0.03 * cw),
                 vc=noise(rng, shp, 0.03 * cw))
        return T, P

    def _tp(self, q, o, ht, hp, kt, kp, same, M, cen, tag, **kw):
        """one fv_tp_2d of the reference's d_sw_tlm: the values with the trajectory's scheme and damping, the tangent with the perturbation's"""
        args = (o["crx"], o["cry"])
        rest = (o["xfx"], o["yfx"], o["ra_x"], o["ra_y"], M, self.n)
        a = fo.fv_tp_2d(q, *args, ht, *rest, da_min=self.da_min, cen=cen, tag=tag, **kw, **kt)
        if same or not np.iscomplexobj(a[0]):
            return a
        b = fo.fv_tp_2d(q, *args, hp, *rest, da_min=self.da_min, **kw, **kp)
        return tuple(np.real(x) + 1j * np.imag(y) for x, y in zip(a, b))

    def apply(self, x, M, edge, ecorner, level0=0):
        nl = x["u"].shape[-3]
        census = {} if x["u"].ndim == 3 else None                               # a single evaluation, not a batch of Jacobian columns
        fix = {k: v[level0:level0 + nl] for k, v in self.fix.items()}
        y = dict(x, **fix)
        self._cen_mt, self._level0 = census, level0
        base = DSwRest.apply(self, {k: y[k] for k in DSwRest.ins}, M, edge, ecorner, level0)      # the perturbation's chain, ke2 with the trajectory's values
        self._cen_mt = None
        n, lv = self.n, []
        for l in range(nl):
            k = level0 + l
            t, q, ht, hp = self.par[k], self.parp[k], self.tr[k], self.trp[k]
            L_ = lambda a: a[..., l, :, :]
            o = {f: L_(base[f]) for f in ("crx", "cry", "xfx", "yfx", "ra_x", "ra_y", "vort_abs", "ke2", "wk")}
            cen = (lambda f: census) if census is not None else (lambda f: None)
            sd = self.split_damp
            delp, pt = L_(x["delp"]), L_(x["pt"])
            fx, fy = self._tp(delp, o, ht["dp"], hp["dp"], dict(nord=t["nord_v"], damp_c=t["damp_vt"]), dict(nord=q["nord_v"], damp_c=q["damp_vt"]),
                              ht["dp"] == hp["dp"] and not sd, M, cen("dp"), "L%d:dp:" % k)
            gx, gy = self._tp(pt, o, ht["tm"], hp["tm"], dict(nord=ht["nord_t"], damp_c=ht["damp_t"]), dict(nord=hp["nord_t"], damp_c=hp["damp_t"]),
                              ht["tm"] == hp["tm"] and not sd, M, cen("tm"), "L%d:tm:" % k, mfx=fx, mfy=fy, mass=delp)
            fxv, fyv = self._tp(o["vort_abs"], o, ht["vt"], hp["vt"], {}, {}, ht["vt"] == hp["vt"], M, cen("vt"), "L%d:vt:" % k)
            new = lambda: np.full(fx.shape, np.nan, dtype=fx.dtype)
            delp_o, pt_o = new(), new()
            r = (1, n, 1, n)                                                    # sw_core_nlm.F90:1018-1031
            ra = fo.V(M["rarea"], *r)
            fo.V(delp_o, *r)[...] = fo.V(delp, *r) + ((fo.V(fx, *r) - fo.V(fx, *r, di=1)) + (fo.V(fy, *r) - fo.V(fy, *r, dj=1))) * ra
            fo.V(pt_o, *r)[...] = (fo.V(pt, *r) * fo.V(delp, *r) + ((fo.V(gx, *r) - fo.V(gx, *r, di=1)) + (fo.V(gy, *r) - fo.V(gy, *r, dj=1))) * ra) / fo.V(delp_o, *r)

            def momentum(p):                                                    # :1474-1490, :1527-1539
                fx2 = fy2 = None
                if p["damp_vt"] > 1.0e-5:
                    _, fx2, fy2 = fo.del6_vt_flux(p["nord_v"], (p["damp_vt"] * self.da_min_c) ** (p["nord_v"] + 1), o["wk"], M, n)
                return fo.d_sw_momentum(L_(x["u"]), L_(x["v"]), o["ke2"], fxv, fyv, fx2, fy2, M, n, p["damp_vt"])
            um, vm = momentum(t)
            if (q["nord_v"], q["damp_vt"]) != (t["nord_v"], t["damp_vt"]) and np.iscomplexobj(um):
                ap, bp = momentum(q)
                um, vm = np.real(um) + 1j * np.imag(ap), np.real(vm) + 1j * np.imag(bp)
            lv.append(dict(fx=fx, fy=fy, gx=gx, gy=gy, fxv=fxv, fyv=fyv, delp_o=delp_o, pt_o=pt_o, u_m=um, v_m=vm, crx=o["crx"], cry=o["cry"]))
            if "w" in x:                                                        # sw_core_nlm.F90:940-961, :1236-1248
                w, (nord_w, damp_w) = L_(x["w"]), self.wpar[k]
                dw, w_m = new(), new()
                fo.V(dw, *r)[...] = 0.0
                if damp_w > 1.0e-5:
                    _, fx2, fy2 = fo.del6_vt_flux(nord_w, (damp_w * self.da_min_c) ** (nord_w + 1), w, M, n)
                    fo.V(dw, *r)[...] = ((fo.V(fx2, *r) - fo.V(fx2, *r, di=1)) + (fo.V(fy2, *r) - fo.V(fy2, *r, dj=1))) * ra
                gxw, gyw = self._tp(w, o, ht["vt"], hp["vt"], {}, {}, ht["vt"] == hp["vt"], M, cen("w"), "L%d:w:" % k, mfx=fx, mfy=fy)
                fo.V(w_m, *r)[...] = (fo.V(delp, *r) * fo.V(w, *r) + ((fo.V(gxw, *r) - fo.V(gxw, *r, di=1)) + (fo.V(gyw, *r) - fo.V(gyw, *r, dj=1))) * ra) / fo.V(delp_o, *r)
                if damp_w > 1.0e-5:
                    fo.V(w_m, *r)[...] = fo.V(w_m, *r) + fo.V(dw, *r)
                lv[-1].update(dw=dw, gxw=gxw, gyw=gyw, w_m=w_m)
        if census is not None:
            self._census = census
        return {k: np.stack([o_[k] for o_ in lv], axis=-3) for k in lv[0]}

    def census_ok(self, cen):
        """(b) every branch of the schemes under test taken both ways somewhere, the PERT_PPM branches of the edge blocks on each of the four
        edges; (c) no discontinuous selector within 1e-6 (relative) of its switch, anywhere: no point is left out of the comparison"""
        for name, (fired, margin, hard, live) in cen.items():
            if hard and not np.all(margin[live] >= 1.0e-6):
                return False, "near a switch: " + name
        for k in range(self.npz):
            for f in ("dp", "tm", "vt"):
                h = self.tr[k][f]
                for br in BULK_BRANCHES[h]:
                    planes = [v[0] for nm, v in cen.items() if nm.endswith(":" + br) and nm.split(":")[0] == "L%d" % k]
                    if not (any(p.any() for p in planes) and any((~p).any() for p in planes)):
                        return False, "never taken both ways: L%d %s" % (k, br)
                if h in fo.MONOTONE:
                    for side in ("west:", "east:"):
                        for sweep in ("in_x:", "in_y:", "out_x:", "out_y:"):
                            for br in EDGE_BRANCHES:
                                p = cen["L%d:%s:%s%s%s" % (k, f, sweep, side, br)][0]
                                if not (p.any() and (~p).any()):
                                    return False, "edge block: L%d %s %s%s%s" % (k, f, sweep, side, br)
                if f == "dp":                                                   # xtp_u / ytp_v with the level's hord_mt
                    hm = self.par[k]["iord_t"]
                    for br in MT_BRANCHES[hm]:
                        for sweep in ("x:", "y:"):
                            p = cen["L%d:mt:%s%s" % (k, sweep, br)][0]
                            if not (p.any() and (~p).any()):
                                return False, "xtp_u / ytp_v: L%d %s%s" % (k, sweep, br)
                    if hm >= 8:
                        for side in ("west:", "east:"):
                            ps = [cen["L%d:mt:%s%sstd:al*ar<0" % (k, sweep, side)][0] for sweep in ("x:", "y:")]
                            if not (any(p.any() for p in ps) and any((~p).any() for p in ps)):
                                return False, "xtp_u / ytp_v edge cell: L%d %s" % (k, side)
                if h == 7 and f == "vt":
                    for sweep in ("in_x:", "in_y:", "out_x:", "out_y:"):
                        ps = [v[0] for nm, v in cen.items() if nm.startswith("L%d:vt:%sedge_al>0" % (k, sweep))]
                        if not (any(p.any() for p in ps) and any((~p).any() for p in ps)):
                            return False, "edge clip of scheme 7: L%d %s" % (k, sweep)
        return True, ""

    def signs_ok(self, x, M, edge, ecorner):
        if not DSw.signs_ok(self, x, M, edge, ecorner):
            return False
        o, n = self.apply(x, M, edge, ecorner), self.n
        npx = n + 1
        rows = []
        for i in (1, 2, npx - 1, npx):                                          # both signs of c at the four flux points the edge blocks feed
            rows += [fo.V(o["crx"], i, i, 1, n), fo.V(o["cry"], 1, n, i, i)]
        if not all(both_signs(np.real(r)) for r in rows):
            return False
        ok, why = self.census_ok(self._census)
        self.why = why
        return ok


class DSwTransportNh(DSwTransport):
    """d_sw_transport on a non-hydrostatic case: w joins the inputs; its del-n damping increment dw (del6_vt_flux with the level's nord_w,
    damp_w, the trajectory's in values and tangent alike: sw_core_tlm.F90:1713-1741), its fluxes gxw, gyw (fv_tp_2d with hord_vt and the
    mass fluxes of delp, :1746-1764) and w_m (sw_core_nlm.F90:956-960, :1236-1248) the outputs"""
    ins = DSwTransport.ins + ["w"]
    outs = DSwTransport.outs + [("dw", "A"), ("gxw", "V"), ("gyw", "U"), ("w_m", "A")]
    seeded = DSwTransport.seeded + ["w_m"]

    def __init__(self, c):
        DSwTransport.__init__(self, c)
        o, self.wpar = c.opt, []
        for k in range(1, c.npz + 1):                                           # model/dyn_core_nlm.F90:591-630: nord_w, damp_w
            r = fo.level_rules(o, k, c.npz)
            sponge = r["nord"] == 0 and not (c.npz == 1 or o.n_sponge < 0) and (k == 1 or r["d2_divg"] != min(0.20, o.d2_bg))
            pw = (0, r["d2_divg"]) if sponge else (min(2, o.nord), o.vtdm4 if o.do_vort_damp else 0.0)
            dy = getattr(c, "dy", None)
            if dy is not None:
                ip, rp = dy.level_params(k)
                assert (ip[7], rp[2]) == pw, (k, ip, rp, pw)
            self.wpar.append(pw)

    def draw(self, c, rng):
        T, P = DSwTransport.draw(self, c, rng)
        shp = T["u"].shape
        T["w"], P["w"] = noise(rng, shp, 1.0), noise(rng, shp, 0.1)
        return T, P


OPERATORS = {"c_sw": CSw, "one_grad_p": OneGradP, "p_grad_c": PGradC, "d_sw": DSw, "c_sw_rest": CSwRest, "d_sw_rest": DSwRest, "c_sw_rest_nh": CSwRestNh,
             "d_sw_transport": DSwTransport, "d_sw_transport_nh": DSwTransportNh}
# geopk outputs, and delp, pt as c_sw receives them: the corner-halo columns hold no data (the exchange leaves them alone); NaN for the
# restatement, 1e30 for the library
GHOST_FREE = ("pk", "gzd", "pkc", "gz", "delp", "pt", "w")


def _ghost_fill(c, x, value):
    g = fo._ghost(c.nx)
    out = {}
    for k, v in x.items():
        out[k] = v.copy()
        if k in GHOST_FREE:
            out[k][:, g] = value
    return out


def _tangent(op, T, P, M, edge, ecorner, dtype):
    ct = np.clongdouble if dtype == np.longdouble else np.complex128
    z = {k: T[k].astype(ct) + 1j * ct(H) * P[k].astype(ct) for k in T}
    o = op.apply(z, M, edge, ecorner)
    return {k: (np.real(v).astype(dtype), (np.imag(v) / dtype(H)).astype(dtype)) for k, v in o.items()}


SPACING, REACH = 14, 6


def _adjoint(op, T, seeds, M, edge, ecorner, dtype, points, chunk=192, coloured=False, level0=0):
    """J^T s at the listed input points {input: boolean [nlev, pj, pj]}: one unit perturbation per column, complex step.
    coloured: the statements are local -- an input point reaches no output further than REACH cells away, the corner rotations of
    d2a2c_vect and the replace of a2b_ord4 included -- so one column perturbs a whole lattice of points SPACING apart on one level and
    every point collects the seeds in its own window.  test_emul_face_edges.py::test_coloured_adjoint_is_the_exact_one holds this
    to the one-point-per-column form."""
    ct = np.clongdouble if dtype == np.longdouble else np.complex128
    if getattr(op, "level_local", False) and next(iter(T.values())).shape[0] > 1:      # no statement couples two levels: one at a time
        parts = [_adjoint(op, {k: v[l:l + 1] for k, v in T.items()}, {k: v[l:l + 1] for k, v in seeds.items()}, M, edge, ecorner, dtype,
                          {k: v[l:l + 1] for k, v in points.items()}, chunk, coloured, level0=l) for l in range(next(iter(T.values())).shape[0])]
        return {k: np.concatenate([p_[k] for p_ in parts], axis=0) for k in T}
    res = {k: np.zeros(T[k].shape, dtype=dtype) for k in T}
    lkw = {"level0": level0} if getattr(op, "per_level", False) else {}      # the level a one-level slice stands for (per-level parameters)

    def seeded(o):
        out = {}
        for on, s in seeds.items():
            d = np.where(s != 0, np.imag(o[on]) / dtype(H), 0)
            assert np.all(np.isfinite(d.astype(np.float64))), ("the restatement read an undefined entry", on)
            assert np.all(np.isfinite(np.where(s != 0, np.real(o[on]), 0).astype(np.float64))), ("a seeded output the restatement does not form", on)
            out[on] = d * s
        return out
    for name in T:
        if coloured:
            nlev, pj = T[name].shape[0], T[name].shape[-1]
            cols = [(l, a, b) for l in range(nlev) for a in range(SPACING) for b in range(SPACING) if points[name][l, a::SPACING, b::SPACING].any()]
            for c0 in range(0, len(cols), chunk):
                sub = cols[c0:c0 + chunk]
                z = {k: np.broadcast_to(T[k].astype(ct), (len(sub),) + T[k].shape) for k in T}
                zz = z[name].copy()
                for q, (l, a, b) in enumerate(sub):
                    zz[q, l, a::SPACING, b::SPACING] += 1j * ct(H)
                z[name] = zz
                ds = seeded(op.apply(z, M, edge, ecorner, **lkw))
                tot = sum(v.sum(axis=1) for v in ds.values())          # over the output levels: [ncol, pj, pj]
                pad = np.zeros((len(sub), pj + 2 * REACH, pj + 2 * REACH), dtype=dtype)
                pad[:, REACH:-REACH, REACH:-REACH] = tot
                csum = np.cumsum(np.cumsum(pad, axis=1), axis=2)
                csum = np.pad(csum, ((0, 0), (1, 0), (1, 0)))
                w = 2 * REACH + 1                                       # window sums centred on every point
                win = csum[:, w:, w:] - csum[:, :-w, w:] - csum[:, w:, :-w] + csum[:, :-w, :-w]
                for q, (l, a, b) in enumerate(sub):
                    res[name][l, a::SPACING, b::SPACING] = win[q, a::SPACING, b::SPACING]
            res[name] = np.where(points[name], res[name], 0)
            continue
        idx = np.argwhere(points[name])
        for c0 in range(0, len(idx), chunk):
            sub = idx[c0:c0 + chunk]
            z = {k: np.broadcast_to(T[k].astype(ct), (len(sub),) + T[k].shape) for k in T}
            zz = z[name].copy()
            zz[np.arange(len(sub)), sub[:, 0], sub[:, 1], sub[:, 2]] += 1j * ct(H)
            z[name] = zz
            ds = seeded(op.apply(z, M, edge, ecorner, **lkw))
            res[name][sub[:, 0], sub[:, 1], sub[:, 2]] = sum(v.reshape(len(sub), -1).sum(axis=1) for v in ds.values())
    return res


def near_edge(n, cells=4):
    pj = n + 7
    J, I = np.meshgrid(np.arange(pj) - 2, np.arange(pj) - 2, indexing="ij")
    return (I <= cells + 1) | (I >= n + 1 - cells) | (J <= cells + 1) | (J >= n + 1 - cells)


def _compose(op, T, P, fl, M, edge, ecorner, dtype):
    """values and tangent of the outputs an operator forms by composition (op.compose): the restated statements on T + i h P, with the
    product's own fields fl = {name: (values, tangent)} as data"""
    ct = np.clongdouble if dtype == np.longdouble else np.complex128
    z = {k: T[k].astype(ct) + 1j * ct(H) * P[k].astype(ct) for k in T}
    zf = {k: a.astype(ct) + 1j * ct(H) * b.astype(ct) for k, (a, b) in fl.items()}
    o = op.compose(z, zf["fxv"], zf["fyv"], M, edge, ecorner)
    return {k: (np.real(v).astype(dtype), (np.imag(v) / dtype(H)).astype(dtype)) for k, v in o.items()}


def _print_figures(label, rows):
    """one line per mode and region class: worst movement of the restatement, worst error, worst error / bound (pytest -s / -rP shows them)"""
    cls = lambda r: "bulk" if r == "bulk" else "corner" if r in ("sw", "se", "ne", "nw") else "strip" if r in ("west", "east", "south", "north") else r
    w = {}
    for (mode, out, reg, mv, bound, err) in rows:
        a = w.setdefault((mode, cls(reg)), [0.0, 0.0, 0.0])
        a[0], a[1], a[2] = max(a[0], mv), max(a[1], err), max(a[2], err / bound)
    for (mode, c_), a in sorted(w.items()):
        print("figures %s %s %s: movement %.1e error %.1e error/bound %.2f" % (label, mode, c_, a[0], a[1], a[2]))


def check(*args, env=None, **kw):
    """_check with the switches of `env` in the environment from the creation of the instance to the last launch: the library reads
    FV3LM_TP_FUSED, the one switch of fv_tp_2d, where the programs of an instance are built"""
    import os
    old = {k: os.environ.get(k) for k in (env or {})}
    os.environ.update(env or {})
    try:
        return _check(*args, **kw)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _check(backend, group, n, face, npz=3, adjoint_all=True, seed=0, report=None, coloured=False, adjoint_levels=None, opt=None,
           amplify=None, adjoint_on=None, adjoint_thin=1, detune=False, observe=None):
    """values, tangent and adjoint of one operator on one whole face; returns [(mode, output, region, movement, bound, error)].
    adjoint_all: J^T s entry by entry at every input point; otherwise at the points within four cells of a face edge on the first
    adjoint_levels levels (None: all), and four random dot products <s, J dx> = <J^T s, dx> for all the other points.
    adjoint_on: a list of levels; entry by entry at every point of these levels and the dot products for the other levels.
    adjoint_thin = k > 1: of the points so chosen, entry by entry only those on every k-th offset of the coloured lattice (1 in k of the
    reference's columns); the others join the dot products.
    opt: options of the case (default_options keywords); amplify: the operator's draw amplified (DSwRest: the 0.20 cap).
    detune: library and restatement both get the metrics with every sin_sg / cos_sg plane scaled by a factor of its own (detuned).
    observe: called with (case, {mode: {kernel name: launches}}) after the last launch: which forms of the group's kernels ran."""
    from common import Case
    hook = restatement_hook(n, face)
    if detune:
        plain = hook
        lengths = bool(getattr(OPERATORS[group], "detune_dxa", False))
        hook = lambda m, e, ec: (lambda r: (detuned(r[0], lengths), r[1], r[2]))(plain(m, e, ec))
    c = Case(nx=n, ny=n, npz=npz, n_split=2, dt=1800.0, backend=backend, face=face, oracle=False, metrics_hook=hook, **(opt or {}))
    op = OPERATORS[group](c)
    ran = {}

    def run_group(mode):
        n0 = c.dy.launch_count()
        c.dy.profile_begin()
        c.dy.run_group(op.group, mode)
        ran[mode] = dict({k: v[0] for k, v in c.dy.profile_end().items()}, launches=c.dy.launch_count() - n0)
    if amplify is not None:
        op.amplify = amplify
    M64, e64, ec64 = face_metrics_of(n, face, np.float64)
    ML, eL, ecL = face_metrics_of(n, face, np.longdouble)
    if detune:
        M64 = detuned(M64, bool(getattr(op, "detune_dxa", False)))
        ML = {k: v.astype(np.longdouble) for k, v in M64.items()}       # the float64 numbers the library holds, exactly
    if getattr(op, "metrics64", False):                      # the longdouble run on the float64 metrics the library holds, exactly: what
        ML, eL, ecL = {k: v.astype(np.longdouble) for k, v in M64.items()}, e64.astype(np.longdouble), ec64.astype(np.longdouble)      # is left is rounding
    rng = np.random.default_rng(1000 * n + 10 * face + seed)
    for _ in range(50):                                      # redraw until the trajectory takes both branches everywhere, clear of zero
        T, P = op.draw(c, rng)
        if op.signs_ok(T, M64, e64, ec64):
            break
    else:
        raise AssertionError("no trajectory with both signs on every edge row " + getattr(op, "why", ""))
    Tn, Pn = _ghost_fill(c, T, np.nan), _ghost_fill(c, P, np.nan)
    rects, rows = G.rects(c), []
    composed = list(getattr(op, "composed", []))
    masks = {o: compared_mask(c, o, rk) for o, rk in op.outs + composed}
    for o, m in masks.items():                               # what poison_checks.drop_undefined took out of the rect
        nd = int(G.masked(c, np.ones((1, n + 7, n + 7)), dict(op.outs + composed)[o])[0].sum()) - int(m.sum())
        if nd:
            print("dropped (formed from undefined entries by the reference itself): %s %d points" % (o, nd))
    lv = {o: (op.levels_of(o) if hasattr(op, "levels_of") and op.levels_of(o) is not None else slice(None)) for o, _ in op.outs + composed}
    S = lambda a, o: a[lv[o]]                                 # the levels on which the reference forms the output
    L = lambda d: {k: v.astype(np.longdouble) for k, v in d.items()}
    ref = _tangent(op, L(Tn), L(Pn), ML, eL, ecL, np.longdouble)
    census = getattr(op, "_census", None)                     # the branches the longdouble run took (DSwTransport)
    moved = lambda r, d: {k: ulp_move(r, v) for k, v in d.items()}
    # ---- values and tangent
    fixed = op.fixed(c)
    for k, v in fixed.items():
        c.dy.put(k, v[None], 0); c.dy.put(k, np.zeros_like(v)[None], 1)
    Tg, Pg = _ghost_fill(c, T, 1.0e30), _ghost_fill(c, P, 1.0e30)
    for k in op.ins:
        c.dy.put(k, Tg[k][None], 0); c.dy.put(k, Pg[k][None], 1)
    run_group(TL)
    got = {o: (c.dy.get(o, 0)[0], c.dy.get(o, 1)[0]) for o, _ in op.outs + composed}
    if composed:                                             # the product's vorticity fluxes as data of the restated last statements
        fl = {k: (c.dy.get(k, 0)[0], c.dy.get(k, 1)[0]) for k in ("fxv", "fyv")}
        ref.update(_compose(op, L(Tn), L(Pn), fl, ML, eL, ecL, np.longdouble))
    move = {}
    for d in range(3):
        Td, Pd = moved(rng, Tn), {k: ulp_move(rng, v) for k, v in Pn.items()}
        r64 = _tangent(op, Td, Pd, M64, e64, ec64, np.float64)
        if census is not None:                                # a flipped branch must not inflate a bound
            for nm, (fired, _, _, _) in census.items():
                assert np.array_equal(fired, op._census[nm][0]), ("a moved draw left the reference's branch", nm)
        if composed:
            r64.update(_compose(op, Td, Pd, fl, M64, e64, ec64, np.float64))
        for o, rk in op.outs + composed:
            for w, tag in ((0, "values"), (1, "tangent")):
                for reg, e in region_errors(S(r64[o][w], o), S(ref[o][w], o), masks[o], n, rects[rk]).items():
                    move[(tag, o, reg)] = max(move.get((tag, o, reg), 0.0), e)
    for o, rk in op.outs + composed:
        for w, tag in ((0, "values"), (1, "tangent")):
            for reg, e in region_errors(S(got[o][w], o), S(ref[o][w], o), masks[o], n, rects[rk]).items():
                mv = move[(tag, o, reg)]
                rows.append((tag, o, reg, mv, max(8 * mv, FLOOR), e))
    # ---- adjoint: seeds on the compared outputs only
    seeded = list(getattr(op, "seeded", [o for o, _ in op.outs]))      # an operator's true outputs, where it also compares work fields
    seeds = {}
    for o in seeded:
        on = np.zeros((c.dy.levels(o), 1, 1), bool)
        on[lv[o]] = True
        seeds[o] = np.where(masks[o] & on, rng.standard_normal((c.dy.levels(o), n + 7, n + 7)), 0.0)
    for k, v in fixed.items():
        c.dy.put(k, v[None], 0)
    for k in op.ins:
        c.dy.put(k, Tg[k][None], 0)
    run_group(NL)
    c.dy.zero_work_adjoint()
    _, _, gins, gouts = G.table(c)[op.group]
    for k in set(gins) | set(op.ins) | {o for o, _ in gouts if o}:
        c.dy.put(k, np.zeros(c.dy.shape(k)), 1)
    for o, s in seeds.items():
        c.dy.put(o, s[None], 1)
    run_group(AD)
    gota = {k: c.dy.get(k, 1)[0] for k in op.ins}
    ne = near_edge(n)
    if adjoint_on is not None:
        adjoint_all, ne = False, np.ones_like(ne)
    pts = {k: np.broadcast_to(ne if not adjoint_all else np.ones_like(ne), T[k].shape).copy() for k in op.ins}
    nl = {}                                                   # levels compared entry by entry
    for k in op.ins:
        if k in GHOST_FREE:
            pts[k][:, fo._ghost(n)] = False                   # no data there: nothing to differentiate with respect to
        nl[k] = list(range(T[k].shape[0]))
        if adjoint_on is not None:
            nl[k] = [l for l in nl[k] if l in adjoint_on]
        elif not adjoint_all and adjoint_levels is not None:
            nl[k] = nl[k][:adjoint_levels]
        pts[k][[l for l in range(T[k].shape[0]) if l not in nl[k]]] = False
        if adjoint_thin > 1:
            J_, I_ = np.meshgrid(np.arange(n + 7) % SPACING, np.arange(n + 7) % SPACING, indexing="ij")
            pts[k] &= ((J_ * SPACING + I_ + face) % adjoint_thin == 0)
    refa = _adjoint(op, L(Tn), L(seeds), ML, eL, ecL, np.longdouble, pts, coloured=coloured)
    mva = {}
    for d in range(3):
        r64 = _adjoint(op, moved(rng, Tn), seeds, M64, e64, ec64, np.float64, pts, coloured=coloured)
        for k in op.ins:
            for reg, e in (region_errors(r64[k][nl[k]], refa[k][nl[k]], pts[k][nl[k][0]], n, rects["full"]).items() if nl[k] else ()):
                mva[(k, reg)] = max(mva.get((k, reg), 0.0), e)
    for k in op.ins:
        for reg, e in (region_errors(gota[k][nl[k]], refa[k][nl[k]], pts[k][nl[k][0]], n, rects["full"]).items() if nl[k] else ()):
            rows.append(("adjoint", k, reg, mva[(k, reg)], max(8 * mva[(k, reg)], FLOOR), e))
    if not adjoint_all:                                        # the rest of the plane: four random dot products <s, J dx> = <J^T s, dx>
        for d in range(4):
            dx = {k: np.where(pts[k], 0.0, noise(rng, T[k].shape, 1.0)) for k in op.ins}
            for k in GHOST_FREE:
                if k in dx:
                    dx[k][:, fo._ghost(n)] = 0.0
            jdx = _tangent(op, L(Tn), L(dx), ML, eL, ecL, np.longdouble)
            lhs = sum(float(np.sum(np.where(seeds[o] != 0, jdx[o][1], 0) * seeds[o])) for o in seeded)
            rhs = sum(float(np.sum(gota[k] * dx[k])) for k in op.ins)
            scale = sum(float(np.sum(np.abs(np.where(seeds[o] != 0, jdx[o][1], 0) * seeds[o]))) for o in seeded)
            rows.append(("adjoint", "dot%d" % d, "rest", 0.0, FLOOR, abs(lhs - rhs) / scale))
    if report is not None:
        report.extend((group, n, face) + r for r in rows)
    _print_figures("%s %s C%d face %d" % (backend, group, n, face), rows)
    bad = [r for r in rows if not r[5] <= r[4]]
    assert not bad, (group, n, face, bad[:8])
    if observe is not None:
        observe(c, ran)
    return rows


# The levels of the d_sw_rest cases, as (trajectory nord, perturbation nord, iord, nord_v).  d2_bg_k2 = 0.03 keeps level 2 a sponge level with a
# floor well under the cap (0.12 leaves a linear window of 0.6 < x < 1 that a 4-point bulk rarely meets) and lets level 3 run nord = 1;
# C70 with npz = 2 needs d2_bg_k2 = 0 for a level with nord = 1 and d2_bg_k1 = 0.02 for a floor under the cap on level 1.
# split_damp: level 2 runs the trajectory's nord = 2 / 3 (values of ke2 through fill_corners) over the perturbation's nord = 1, every
# coefficient of the two sets apart, the trajectory's vorticity damping with nord_v = 2.
DSW_REST = dict(npz=3, opt=dict(n_sponge_pert=2, d2_bg_k2=0.03, d2_bg_k2_pert=0.03), forms=[(0, 0, 1, 0), (0, 0, 2, 0), (1, 1, 2, 1)])
DSW_REST_C70 = dict(npz=2, opt=dict(n_sponge_pert=2, d2_bg_k1=0.02, d2_bg_k2=0.0, d2_bg_k1_pert=0.02, d2_bg_k2_pert=0.0), forms=[(0, 0, 1, 0), (1, 1, 2, 1)])
_SPLIT = dict(split_damp=1, nord_pert=1, n_sponge_pert=1, dddmp=0.35, dddmp_pert=0.2, d4_bg=0.11, d4_bg_pert=0.15, d2_bg=0.02, d2_bg_pert=0.015,
              vtdm4=0.03, vtdm4_pert=0.0005, d2_bg_k1=0.18, d2_bg_k2=0.0)
DSW_SPLIT = {nord: dict(npz=2, opt=dict(_SPLIT, nord=nord), forms=[(0, 0, 2, 0), (nord, 1, 2, 2)]) for nord in (2, 3)}


def transport_opt(h, pert=2, **more):
    """options of a d_sw_transport case: the trajectory scheme h for delp, pt and the vorticity over the perturbation scheme `pert`, the
    sponge levels' own schemes (hord_*_ks_*) switched off so that both levels run them"""
    o = dict(hord_ks_traj=0, hord_ks_pert=0, hord_dp=h, hord_tm=h, hord_vt=h, hord_dp_pert=pert, hord_tm_pert=pert, hord_vt_pert=pert)
    if h != 333:                                                 # the nonlinear xtp_u / ytp_v hold no scheme 333 (sw_core_tlm.F90:4396-4406)
        o.update(hord_mt=h, hord_mt_pert=pert if pert != 333 else 2)
    o.update(more)
    return o


# level 2 off the trajectory's sponge rules: nord_v = nord_t = 1 with a coefficient well above the 1e-4 threshold, so that DELN_FLUX runs
# its nord = 1 loop without (delp) and with (pt) the mass, beside the nord_v = 0 form of level 1
TRANSPORT_DAMPED = dict(d2_bg_k2=0.0, d2_bg_k2_pert=0.0, vtdm4=0.03, vtdm4_pert=0.03)


def transport_forms(env):
    """observe of check(): the device form of fv_tp_2d that `env` selects is the one that ran, from the names of the hand-written launches
    in the three run_group calls, the launch counts (the staged form of one fv_tp_2d is seven launches and its strips; the group holds
    three) and the library's count of launches in the wavefront layout (tp2.h, whose profile name is TpFused).  Two forms: the staged
    stages in every mode under FV3LM_TP_FUSED=0, the tiled launches (tp2.h, tpad.h) otherwise; the half-fused adjoint TpOuter is gone."""
    env = env or {}

    def observe(c, ran):
        staged = lambda m: not any(k.startswith(("TpFused", "TpAd", "TpOuter")) for k in ran[m]) and ran[m]["launches"] >= 3 * 7
        tp2 = c.dy.tp2_launch_count()
        assert not any(k.startswith("TpOuter") for m in (NL, TL, AD) for k in ran[m]), ran
        if env.get("FV3LM_TP_FUSED") == "0":                                    # the staged stages in every mode
            assert staged(TL) and staged(NL) and staged(AD) and tp2 == 0, (ran, tp2)
            return
        assert ran[TL].get("TpFused.tl", 0) > 0 and ran[NL].get("TpFused.nl", 0) > 0 and ran[AD].get("TpAd.ad", 0) > 0, ran
        assert not staged(TL) and not staged(NL) and not staged(AD) and tp2 > 0, (ran, tp2)
    return observe


def check_transport(backend, n, face, h, pert=2, more=None, **kw):
    """check() of d_sw_transport, npz = 2 (3 on a non-hydrostatic case, the least the library takes): values and tangent at every point; the adjoint entry by entry (one perturbed point per column of
    the restated Jacobian: two +-3 sweeps, the Courant stencil and copy_corners reach too far for a lattice on these faces) within four
    cells of an edge on the first level, thinned, and four dot products for the rest"""
    kw.setdefault("adjoint_thin", 4)
    kw.setdefault("observe", transport_forms(kw.get("env")))
    group = "d_sw_transport_nh" if (more or {}).get("hydrostatic", 1) == 0 else "d_sw_transport"
    return check(backend, group, n, face, npz=3 if group.endswith("nh") else 2, opt=transport_opt(h, pert, **(more or {})), adjoint_all=False, adjoint_levels=1, **kw)


def check_d_sw_rest(backend, n, face, case=None, **kw):
    """check() of d_sw_rest on a case whose levels run the forms it names: asserted here from the level parameters (fo.level_rules,
    fo.level_rules_pert, which DSwRest holds to the library's own), before anything is computed"""
    from fv3_jedi_linearmodel_amd import default_options
    case = case or DSW_REST
    o = default_options(**case["opt"])
    got = []
    for k in range(1, case["npz"] + 1):
        t, q = fo.level_rules(o, k, case["npz"]), fo.level_rules_pert(o, k)
        iord = o.hord_mt_ks_pert if (k <= o.n_sponge_pert - 1 and o.hord_ks_pert) else o.hord_mt_pert
        got.append((t["nord"], q["nord"] if o.split_damp else t["nord"], iord, t["nord_v"]))
    assert got == case["forms"], got
    assert 0 in {f[1] for f in got} and 1 in {f[1] for f in got}
    return check(backend, "d_sw_rest", n, face, npz=case["npz"], opt=case["opt"], **kw)


# ------------------------------------------------------------------------------------------------------------ faces cut into tiles
class _FaceShape:
    """what the operator classes and groups.py read of a case, for a whole face of the cube behind a tiled CubeCase"""
    def __init__(self, c):
        self.nx = self.ny = c.n
        self.npz, self.dt_ac, self.opt, self.face, self.da_min_c, self.da_min = c.npz, c.dt_ac, c.opt, "cube", c.da_min_c, c.da_min

    def rect(self, i0, i1, j0, j1):
        return (Ellipsis, slice(j0 + 2, j1 + 3), slice(i0 + 2, i1 + 3))


def check_layout(backend, group, n=16, layout=2, npz=3, report=None, opt=None):
    """Six faces of C<n> cut layout x layout (the tile offset into edge[] and the clipped strip rects of the a2b builders): every tile's
    outputs on its own rects against the windows of the whole-face restatement, values and tangent per point and region (regions of the
    tile), and the adjoint through four dot products <s, J dx> = <J^T s, dx> summed over the tiles, dx and J dx from the restatement.
    (The outputs an operator forms by composition, DSwRest.composed, are not compared here.)"""
    from common import CubeCase
    from fv3_jedi_linearmodel_amd import cube
    c = CubeCase(n=n, npz=npz, n_split=2, backend=backend, layout=layout, oracle=False, metrics_hook=restatement_hook(n), **(opt or {}))
    fc = _FaceShape(c)
    op = OPERATORS[group](fc)
    lv = {o: (op.levels_of(o) if hasattr(op, "levels_of") and op.levels_of(o) is not None else slice(None)) for o, _ in op.outs}

    def at(f):                                                   # the operator on face f (DSwTransport: the face's data fields)
        op.face = f
        return op
    nt, tl = c.nt, c.tiles
    W = lambda a: cube.tile_window(a, tl, nt)                    # [6, ..., pj, pj] -> [ntile, ..., nt+7, nt+7]
    rng = np.random.default_rng(7 * n + layout)
    Ms = [face_metrics_of(n, f, np.float64) for f in range(6)]
    MLs = [face_metrics_of(n, f, np.longdouble) for f in range(6)]
    if getattr(op, "metrics64", False):                          # as in check(): the float64 metrics the library holds, exactly
        MLs = [({k: v.astype(np.longdouble) for k, v in m.items()}, e.astype(np.longdouble), ec.astype(np.longdouble)) for m, e, ec in Ms]
    T6, P6 = [], []
    for f in range(6):
        op.face = f                                              # (DSwRest: the face whose divgd halo and metrics the draw takes)
        for _ in range(50):
            T, P = op.draw(fc, rng)
            if op.signs_ok(T, *Ms[f]):
                break
        else:
            raise AssertionError("no trajectory with both signs on every edge row")
        T6.append(T); P6.append(P)
    stack = lambda d6, fill: {k: np.stack([_ghost_fill(fc, d, fill)[k] for d in d6]) for k in d6[0]}
    L = lambda d: {k: v.astype(np.longdouble) for k, v in d.items()}
    Tn, Pn = [_ghost_fill(fc, d, np.nan) for d in T6], [_ghost_fill(fc, d, np.nan) for d in P6]
    ref = [_tangent(at(f), L(Tn[f]), L(Pn[f]), *MLs[f], np.longdouble) for f in range(6)]
    refw = {o: [W(np.stack([ref[f][o][w] for f in range(6)])) for w in (0, 1)] for o, _ in op.outs}
    # masks per tile: the tile's own rect minus the windows of the points that hold no value on the face
    rects = G.rects(c)
    one = np.ones((6, 1, n + 7, n + 7))
    masks = {}
    for o, rk in op.outs:
        dropped = W(np.stack([G.drop_face_corners(fc, o, one[f]) for f in range(6)]))[:, 0] == 0
        masks[o] = (G.masked(c, np.ones((len(tl), 1, nt + 7, nt + 7)), rk)[:, 0] != 0) & ~dropped
    # the inputs of the library's group that the operator leaves alone: delp, pt of the case, plausible winds (DSw), empty accumulators
    _, _, gins, gouts = G.table(c)[op.group]
    frng = np.random.default_rng(5)
    fixed = {}
    for k in gins:
        if k in op.ins:
            continue
        fixed[k] = c.traj[k] if k in ("delp", "pt") else np.zeros(c.dy.shape(k)) if k in ("mfx", "mfy", "cx", "cy") else \
            W(np.stack([d[k] for d in op.fix6])) if hasattr(op, "fix6") else noise(frng, c.dy.shape(k), 1e-6 if k == "divgd" else 5.0)
    for k, v in fixed.items():
        c.dy.put(k, v, 0); c.dy.put(k, np.zeros_like(v), 1)
    Tg = {k: W(v) for k, v in stack(T6, 1.0e30).items()}; Pg = {k: W(v) for k, v in stack(P6, 1.0e30).items()}
    for k in op.ins:
        c.dy.put(k, Tg[k], 0); c.dy.put(k, Pg[k], 1)
    c.dy.run_group(op.group, TL)
    got = {o: (c.dy.get(o, 0), c.dy.get(o, 1)) for o, _ in op.outs}
    move, rows = {}, []
    for d in range(3):
        r64 = [_tangent(at(f), {k: ulp_move(rng, v) for k, v in Tn[f].items()}, {k: ulp_move(rng, v) for k, v in Pn[f].items()}, *Ms[f], np.float64)
               for f in range(6)]
        for o, rk in op.outs:
            for w, tag in ((0, "values"), (1, "tangent")):
                rw = W(np.stack([r64[f][o][w] for f in range(6)]))
                for t in range(len(tl)):
                    for reg, e in region_errors(rw[t][lv[o]], refw[o][w][t][lv[o]], masks[o][t], nt, rects[rk]).items():
                        move[(tag, o, reg)] = max(move.get((tag, o, reg), 0.0), e)
    err = {}
    for o, rk in op.outs:
        for w, tag in ((0, "values"), (1, "tangent")):
            for t in range(len(tl)):
                for reg, e in region_errors(got[o][w][t][lv[o]], refw[o][w][t][lv[o]], masks[o][t], nt, rects[rk]).items():
                    err[(tag, o, reg)] = max(err.get((tag, o, reg), 0.0), e)
    for k, e in sorted(err.items()):
        rows.append(k + (move[k], max(8 * move[k], FLOOR), e))
    # ---- adjoint: seeds on the compared outputs of every tile
    seeds = {}
    seeded = list(getattr(op, "seeded", [o for o, _ in op.outs]))
    for o in seeded:
        on = np.zeros((1, got[o][0].shape[1], 1, 1), bool)
        on[:, lv[o]] = True
        seeds[o] = np.where(masks[o][:, None] & on, rng.standard_normal(got[o][0].shape), 0.0)
    for k, v in fixed.items():
        c.dy.put(k, v, 0)
    for k in op.ins:
        c.dy.put(k, Tg[k], 0)
    c.dy.run_group(op.group, NL)
    c.dy.zero_work_adjoint()
    for k in set(gins) | set(op.ins) | {o for o, _ in gouts if o}:
        c.dy.put(k, np.zeros(c.dy.shape(k)), 1)
    for o, s in seeds.items():
        c.dy.put(o, s, 1)
    c.dy.run_group(op.group, AD)
    gota = {k: c.dy.get(k, 1) for k in op.ins}
    g6 = fo._ghost(n)
    for d in range(4):
        dx6 = []
        for f in range(6):
            dx = {k: noise(rng, T6[f][k].shape, 1.0) for k in op.ins}
            for k in GHOST_FREE:
                if k in dx:
                    dx[k][:, g6] = 0.0
            dx6.append(dx)
        jdx = [_tangent(at(f), L(Tn[f]), L(dx6[f]), *MLs[f], np.longdouble) for f in range(6)]
        lhs = scale = 0.0
        for o in seeded:
            jw = W(np.stack([jdx[f][o][1] for f in range(6)]))
            term = np.where(seeds[o] != 0, jw, 0) * seeds[o]
            lhs += float(np.sum(term)); scale += float(np.sum(np.abs(term)))
        rhs = sum(float(np.sum(gota[k] * W(np.stack([dx6[f][k] for f in range(6)])))) for k in op.ins)
        rows.append(("adjoint", "dot%d" % d, "tiles", 0.0, FLOOR, abs(lhs - rhs) / scale))
    if report is not None:
        report.extend((group, n, "2x2") + r for r in rows)
    _print_figures("%s %s C%d cut %dx%d" % (backend, group, n, layout, layout), rows)
    bad = [r for r in rows if not r[5] <= r[4]]
    assert not bad, (group, n, layout, bad[:8])
    return rows
