"""Independent numpy restatement of the vertical remap (Lagrangian_to_Eulerian with remap_option 0), restated from the reference
Fortran for the column tests of fv3lm_remap (remap_checks.py):
  edges()      the tridiagonal edge-value solve of cs_profile / scalar_profile, iv = -1, 0, 1 and the iv = -2 form with the surface value qs
               (model/fv_mapz_nlm.F90:1748-1810 / :2131-2193; TL file fv_mapz_tlm.F90:8356-8509, :8513-8666)
  limited()    the constraints of the limited profiles kord 8 .. 15 (scalar_profile :1812-2110 with the qmin tests, cs_profile :2195-2464)
               and cs_limiters (:2467-2542)
  map_loop()   the conservative mapping loop of map_scalar / map1_ppm / map1_q2 (:1270-1327, :1365-1420, :1574-1629)
  hydro(), nh() the drivers: T_v in log p, tracers in p, u and v on pressures averaged across the edge, new pe, peln, pk, pkz, delp and the
               temperature hand-over (model_tlmadm/fv_mapz_tlm.F90:1586-1951 and its last-step / other-step conversions :2203-2250); the
               non-hydrostatic additions (density pt -> T through delz :1607-1613, delz as -delz/delp :1635-1641 mapped with iv = 1 and
               |kord_tm| :1782-1796, w with iv = -2 and ws under kord_wz :1772-1780, pkz from the equation of state :1852-1857).
Everything is computed in np.longdouble, vectorised over columns with a Python loop over k.  The tangent is a complex step (np.clongdouble)
through the linear profile (|kord| > 16), the one the reference differentiates (fv_mapz_tlm.F90:8653-8666); when the trajectory's kord is a
limited one (split_kord) the values come from the limited profile and the sensitivities from the linear one, as in the reference's TL code
(:494-523, :596-637, :780-827) -- a map returns limited(x) + i Im(linear(x + i h dx)), and everything after it uses those values.
The adjoint reference is the transpose of that tangent (jt_s(): one complex-step direction per input entry, columns coloured)."""
import numpy as np

LD, CLD = np.longdouble, np.clongdouble
H_CS = 1e-40          # complex step: far below the longdouble resolution of every value the tests use


def _re(x):
    return x.real if np.iscomplexobj(x) else x


def _r(x, num, den):
    """the constant num / den in the real precision of x"""
    t = _re(np.asarray(x)).dtype.type
    return t(num) / t(den)


# ------------------------------------------------------------------------------------------------ profile
def edges(a1, dp, iv, qs=None):
    """Edge values q(1..km+1) of the layer means a1 [n, km] on thicknesses dp [n, km] -> [n, km+1] (index 0 = Fortran edge 1).
    iv = -2: fv_mapz_nlm.F90:2131-2156 (the lower boundary value qs given); otherwise :2158-2193."""
    n, km = a1.shape
    q = np.zeros((n, km + 1), dtype=a1.dtype)
    gam = np.zeros((n, km + 1), dtype=a1.dtype)
    A = lambda k: a1[:, k - 1]            # 1-based layer
    D = lambda k: dp[:, k - 1]
    if iv == -2:
        gam[:, 2 - 1] = 0.5
        q[:, 0] = 1.5 * A(1)
        for k in range(2, km):
            grat = D(k - 1) / D(k)
            bet = 2. + grat + grat - gam[:, k - 1]
            q[:, k - 1] = (3. * (A(k - 1) + A(k)) - q[:, k - 2]) / bet
            gam[:, k] = grat / bet
        grat = D(km - 1) / D(km)
        q[:, km - 1] = (3. * (A(km - 1) + A(km)) - grat * qs - q[:, km - 2]) / (2. + grat + grat - gam[:, km - 1])
        q[:, km] = qs
        for k in range(km - 1, 0, -1):
            q[:, k - 1] = q[:, k - 1] - gam[:, k] * q[:, k]
        return q
    grat = D(2) / D(1)
    bet = grat * (grat + 0.5)
    q[:, 0] = ((grat + grat) * (grat + 1.) * A(1) + A(2)) / bet
    gam[:, 0] = (1. + grat * (grat + 1.5)) / bet
    d4 = grat
    for k in range(2, km + 1):
        d4 = D(k - 1) / D(k)
        bet = 2. + d4 + d4 - gam[:, k - 2]
        q[:, k - 1] = (3. * (A(k - 1) + d4 * A(k)) - q[:, k - 2]) / bet
        gam[:, k - 1] = d4 / bet
    a_bot = 1. + d4 * (d4 + 1.5)
    q[:, km] = (2. * d4 * (d4 + 1.) * A(km) + A(km - 1) - a_bot * q[:, km - 1]) / (d4 * (d4 + 0.5) - a_bot * gam[:, km - 1])
    for k in range(km, 0, -1):
        q[:, k - 1] = q[:, k - 1] - gam[:, k - 1] * q[:, k]
    return q


def linear(a1, q):
    """|kord| > 16: a2, a3, a4 straight from the edge values (:1812-1821)"""
    a2, a3 = q[:, :-1], q[:, 1:]
    return a2, a3, 3. * (2. * a1 - (a2 + a3))


def _cs_limiters(a1, a2, a3, a4, extm, mode):
    """cs_limiters (fv_mapz_nlm.F90:2467-2542) on one layer's vectors; mode 0 positive definite, 1 monotone by the edges, 2 by extm"""
    a2, a3, a4 = a2.copy(), a3.copy(), a4.copy()
    if mode == 0:
        neg = a1 <= 0.
        chk = ~neg & (np.abs(a3 - a2) < -a4)
        with np.errstate(divide="ignore", invalid="ignore"):
            fix = chk & (a1 + 0.25 * (a3 - a2) ** 2 / a4 + a4 * _r(a1, 1, 12) < 0.)
        f1 = fix & (a1 < a3) & (a1 < a2)
        f2 = fix & ~f1 & (a3 > a2)
        f3 = fix & ~f1 & ~f2
        n2, n3, n4 = a2.copy(), a3.copy(), a4.copy()
        n2[neg | f1] = a1[neg | f1]; n3[neg | f1] = a1[neg | f1]; n4[neg | f1] = 0.
        n4[f2] = 3. * (a2[f2] - a1[f2]); n3[f2] = a2[f2] - n4[f2]
        n4[f3] = 3. * (a3[f3] - a1[f3]); n2[f3] = a3[f3] - n4[f3]
        return n2, n3, n4
    flat = (a1 - a2) * (a1 - a3) >= 0. if mode == 1 else extm
    da1 = a3 - a2
    da2 = da1 * da1
    a6da = a4 * da1
    lo = ~flat & (a6da < -da2)
    hi = ~flat & ~lo & (a6da > da2)
    n2, n3, n4 = a2.copy(), a3.copy(), a4.copy()
    n2[flat] = a1[flat]; n3[flat] = a1[flat]; n4[flat] = 0.
    n4[lo] = 3. * (a2[lo] - a1[lo]); n3[lo] = a2[lo] - n4[lo]
    n4[hi] = 3. * (a3[hi] - a1[hi]); n2[hi] = a3[hi] - n4[hi]
    return n2, n3, n4


def limited(a1, q, iv, kord, scalar, qmin=0.):
    """scalar_profile (scalar = True: the a4(1) < qmin tests, :1812-2110) / cs_profile (:2195-2464) for 8 <= |kord| <= 15, real columns.
    a1 [n, km], q [n, km+1] the unlimited edge values -> a2, a3, a4 [n, km]"""
    n, km = a1.shape
    ak = abs(kord)
    assert 8 <= ak <= 15 and km >= 6
    A = np.zeros((n, km + 2), dtype=a1.dtype); A[:, 1:km + 1] = a1          # A[:, k] = a4(1, k), 1-based
    Q = np.zeros((n, km + 2), dtype=a1.dtype); Q[:, 1:km + 2] = q           # Q[:, k] = q(k)
    Q[:, 2] = np.maximum(np.minimum(Q[:, 2], np.maximum(A[:, 1], A[:, 2])), np.minimum(A[:, 1], A[:, 2]))
    G = np.zeros((n, km + 2), dtype=a1.dtype)
    for k in range(2, km + 1):
        G[:, k] = A[:, k] - A[:, k - 1]
    for k in range(3, km):
        lo, hi = np.minimum(A[:, k - 1], A[:, k]), np.maximum(A[:, k - 1], A[:, k])
        same = G[:, k - 1] * G[:, k + 1] > 0.
        up = ~same & (G[:, k - 1] > 0.)
        dn = ~same & ~up
        x = Q[:, k].copy()
        x[same] = np.maximum(np.minimum(x[same], hi[same]), lo[same])
        x[up] = np.maximum(x[up], lo[up])
        x[dn] = np.minimum(x[dn], hi[dn])
        if iv == 0:
            x[dn] = np.maximum(0., x[dn])
        Q[:, k] = x
    Q[:, km] = np.maximum(np.minimum(Q[:, km], np.maximum(A[:, km - 1], A[:, km])), np.minimum(A[:, km - 1], A[:, km]))
    a2 = {k: Q[:, k].copy() for k in range(1, km + 1)}
    a3 = {k: Q[:, k + 1].copy() for k in range(1, km + 1)}
    a4 = {}
    extm = {}
    for k in range(1, km + 1):
        if k == 1 or k == km:
            extm[k] = (a2[k] - A[:, k]) * (a3[k] - A[:, k]) > 0.
        else:
            extm[k] = G[:, k] * G[:, k + 1] < 0.
    if iv == 0:
        a2[1] = np.maximum(0., a2[1])
    elif iv == -1:
        a2[1] = np.where(a2[1] * A[:, 1] <= 0., 0., a2[1])
    f4 = lambda k: 3. * (2. * A[:, k] - (a2[k] + a3[k]))
    a4[1] = f4(1)
    a2[1], a3[1], a4[1] = _cs_limiters(A[:, 1], a2[1], a3[1], a4[1], extm[1], 1)
    a4[2] = f4(2)
    a2[2], a3[2], a4[2] = _cs_limiters(A[:, 2], a2[2], a3[2], a4[2], extm[2], 2)
    for k in range(3, km - 1):
        a = A[:, k]
        b2, b3 = a2[k].copy(), a3[k].copy()
        small = (a < qmin) if scalar else np.zeros(n, bool)

        def huynh(b2, b3, m):
            pmp_1 = a - 2. * G[:, k + 1]
            lac_1 = pmp_1 + 1.5 * G[:, k + 2]
            c2 = np.minimum(np.maximum(b2, np.minimum(np.minimum(a, pmp_1), lac_1)), np.maximum(np.maximum(a, pmp_1), lac_1))
            pmp_2 = a + 2. * G[:, k]
            lac_2 = pmp_2 - 1.5 * G[:, k - 1]
            c3 = np.minimum(np.maximum(b3, np.minimum(np.minimum(a, pmp_2), lac_2)), np.maximum(np.maximum(a, pmp_2), lac_2))
            return np.where(m, c2, b2), np.where(m, c3, b3)
        ex, exm, exp_ = extm[k], extm[k - 1], extm[k + 1]
        if ak < 9:
            b2, b3 = huynh(b2, b3, np.ones(n, bool))
            b4 = 3. * (2. * a - (b2 + b3))
            flat = np.zeros(n, bool)
        elif ak == 9:
            flat = (ex & exm) | (ex & exp_) | (ex & small)
            f9 = (lambda x2, x3: 3. * (2. * a - (x2 + x3))) if scalar else (lambda x2, x3: 6. * a - 3. * (x2 + x3))
            b4 = f9(b2, b3)
            m = ~flat & (np.abs(b4) > np.abs(b2 - b3))
            b2, b3 = huynh(b2, b3, m)
            b4 = np.where(m, f9(b2, b3), b4)
        elif ak in (10, 12):
            flat = ex & (small | exm | exp_) if ak == 10 else ex.copy()
            b4 = 6. * a - 3. * (b2 + b3)
            m = ~ex & (np.abs(b4) > np.abs(b2 - b3))
            b2, b3 = huynh(b2, b3, m)
            b4 = np.where(m, 6. * a - 3. * (b2 + b3), b4)
        elif ak == 13:
            flat = ex & exm & exp_
            b2, b3 = huynh(b2, b3, ex & ~flat)
            b4 = 3. * (2. * a - (b2 + b3))
        elif ak == 14:
            flat = np.zeros(n, bool)
            b4 = 3. * (2. * a - (b2 + b3))
        else:                # 11, 15 (the ELSE branch)
            flat = ex & (exm | exp_ | small)
            b4 = 3. * (2. * a - (b2 + b3))
        b2 = np.where(flat, a, b2); b3 = np.where(flat, a, b3); b4 = np.where(flat, 0., b4)
        if iv == 0:
            b2, b3, b4 = _cs_limiters(a, b2, b3, b4, ex, 0)
        a2[k], a3[k], a4[k] = b2, b3, b4
    if iv == 0:
        a3[km] = np.maximum(0., a3[km])
    elif iv == -1:
        a3[km] = np.where(a3[km] * A[:, km] <= 0., 0., a3[km])
    for k, mode in ((km - 1, 2), (km, 1)):
        a4[k] = f4(k)
        a2[k], a3[k], a4[k] = _cs_limiters(A[:, k], a2[k], a3[k], a4[k], extm[k], mode)
    st = lambda d: np.stack([d[k] for k in range(1, km + 1)], axis=1)
    return st(a2), st(a3), st(a4)


# ------------------------------------------------------------------------------------------------ mapping
def map_loop(pe1, a1, a2, a3, a4, pe2):
    """The conservative loop of map_scalar / map1_ppm / map1_q2 (fv_mapz_nlm.F90:1270-1327): pe1, pe2 [n, km+1], a* [n, km] -> [n, km].
    Every column keeps its own k0 / l / m; the search runs on the real parts (the branches of the trajectory)."""
    n, km = a1.shape
    R3, R23 = _r(a1, 1, 3), _r(a1, 2, 3)
    p1 = _re(pe1)
    dp1 = pe1[:, 1:] - pe1[:, :-1]
    cols = np.arange(n)
    q2 = np.zeros((n, km), dtype=np.result_type(a1, pe1, pe2))
    qsum = np.zeros(n, dtype=q2.dtype)
    k0 = np.zeros(n, dtype=int)                      # 0-based layer index
    for k in range(km):
        p2t, p2b = pe2[:, k], pe2[:, k + 1]
        t, b = _re(p2t), _re(p2b)
        # locate the top edge: the first l >= k0 with pe1(l) <= pe2(k) <= pe1(l+1)
        l = k0.copy()
        while True:
            lc = np.minimum(l, km - 1)
            hit = (t >= p1[cols, lc]) & (t <= p1[cols, lc + 1])
            adv = (l < km) & ~hit
            if not adv.any():
                break
            l = l + adv
        found = l < km
        lc = np.minimum(l, km - 1)
        P1l, P1r, D = pe1[cols, lc], pe1[cols, lc + 1], dp1[cols, lc]
        A1, A2, A3, A4 = a1[cols, lc], a2[cols, lc], a3[cols, lc], a4[cols, lc]
        pl = (p2t - P1l) / D
        inside = found & (b <= p1[cols, lc + 1])
        pr = (p2b - P1l) / D
        q_in = A2 + 0.5 * (A4 + A3 - A2) * (pr + pl) - A4 * R3 * (pr * (pr + pl) + pl * pl)
        part = found & ~inside
        qs = (P1r - p2t) * (A2 + 0.5 * (A4 + A3 - A2) * (1. + pl) - A4 * (R3 * (1. + pl * (1. + pl))))
        m = lc + 1
        while True:            # whole layers
            mc = np.minimum(m, km - 1)
            whole = part & (m < km) & (b > p1[cols, np.minimum(m + 1, km)])
            if not whole.any():
                break
            qs = qs + np.where(whole, dp1[cols, mc] * a1[cols, mc], 0.)
            m = m + whole
        bottom = part & (m < km)
        mc = np.minimum(m, km - 1)
        dp = p2b - pe1[cols, mc]
        esl = dp / dp1[cols, mc]
        B2, B3, B4 = a2[cols, mc], a3[cols, mc], a4[cols, mc]
        qs = np.where(bottom, qs + dp * (B2 + 0.5 * esl * (B3 - B2 + B4 * (1. - R23 * esl))), qs)
        qsum = np.where(part, qs, qsum)              # not found: the reference divides a stale qsum (never taken for ordered levels)
        q2[:, k] = np.where(inside, q_in, qsum / (p2b - p2t))
        k0 = np.where(inside, lc, np.where(bottom, mc, k0))
        assert found.all(), "target edge outside the source column"
    return q2


def map_col(pe1, q1, pe2, iv, kord, scalar=False, qmin=0., qs=None):
    """one field: profile + mapping.  Real inputs: the values of kord's profile.  Complex inputs: limited(x) + i Im(linear(z)) when kord is
    a limited one, the linear profile through and through otherwise."""
    dp = pe1[:, 1:] - pe1[:, :-1]
    q = edges(q1, dp, iv, qs)
    lin = map_loop(pe1, q1, *linear(q1, q), pe2)
    if abs(kord) > 16:
        return lin
    r = lambda x: _re(x) if x is not None else None
    p1r, q1r = r(pe1), r(q1)
    qr = edges(q1r, p1r[:, 1:] - p1r[:, :-1], iv, r(qs))
    val = map_loop(p1r, q1r, *limited(q1r, qr, iv, kord, scalar, qmin), r(pe2))
    return val + 1j * lin.imag if np.iscomplexobj(lin) else val


# ------------------------------------------------------------------------------------------------ drivers
def rects(nx, ny):
    return dict(A=(1, nx, 1, ny), U=(1, nx, 1, ny + 1), V=(1, nx + 1, 1, ny), Ah=(0, nx + 1, 0, ny + 1))


def cols(arr, r):
    """plane [nk, pj, pi] -> columns [ncol, nk] of Fortran rectangle r = (i0, i1, j0, j1), j slowest"""
    i0, i1, j0, j1 = r
    a = arr[:, j0 + 2:j1 + 3, i0 + 2:i1 + 3]
    return a.reshape(a.shape[0], -1).T


def plane(c, r):
    """columns [ncol, nk] -> [nk, nj, ni] on rectangle r"""
    i0, i1, j0, j1 = r
    return c.T.reshape(c.shape[1], j1 - j0 + 1, i1 - i0 + 1)


class Remap:
    """the remap of one case: c.opt (kords, constants), c.ak / c.bk, dims; S: dict of padded planes [nk, ny+7, nx+7] (no tile axis):
    pe, peln, pk (npz+1), pt, u, v, q1.. (npz); non-hydrostatic also delp, delz, w (npz) and ws (1)."""

    def __init__(self, c, last_step, real=LD):
        """real: the precision of the reference (np.longdouble; np.float64 measures how far double rounding alone moves a column)"""
        o = c.opt
        LD = self.real = real
        self.nx, self.ny, self.km, self.nq = c.nx, c.ny, c.npz, c.nq
        self.hydro = bool(o.hydrostatic)
        self.last = bool(last_step)
        self.ak, self.bk = np.asarray(c.ak, dtype=LD), np.asarray(c.bk, dtype=LD)
        self.ptop, self.akap, self.zvir = LD(o.ptop), LD(o.akap), LD(o.zvir)
        self.rrg = -LD(o.rdgas) / LD(o.grav)
        self.k1k = LD(o.rdgas) / (LD(o.cp_air) - LD(o.rdgas))        # rdgas / cv_air
        self.kord_tm, self.kord_mt, self.kord_tr, self.kord_wz = abs(o.kord_tm), o.kord_mt, o.kord_tr, o.kord_wz
        self.R = rects(c.nx, c.ny)
        self.inputs = ["pe", "peln", "pk", "pt", "u", "v"] + ["q%d" % (n + 1) for n in range(c.nq)] + \
                      ([] if self.hydro else ["delp", "delz", "w", "ws"])
        self.outputs = [("pe", "A"), ("peln", "A"), ("pk", "A"), ("pkz", "A"), ("pt", "A"), ("delp", "A"), ("u", "U"), ("v", "V")] + \
                       [("q%d" % (n + 1), "A") for n in range(c.nq)] + ([] if self.hydro else [("w", "A"), ("delz", "A")])

    def _target(self, ps):
        km = self.km
        return np.stack([np.full_like(ps, self.ptop)] + [self.ak[k] + self.bk[k] * ps for k in range(1, km)] + [ps], axis=1)

    def run(self, S):
        """-> {output name: [nk, nj, ni] on its rectangle}; dtype follows S (longdouble or clongdouble)"""
        km, A = self.km, self.R["A"]
        C = lambda n, r="A": cols(S[n], self.R[r])
        pe1, pn1, pk1 = C("pe"), C("peln"), C("pk")
        ps = pe1[:, km]
        pe2 = self._target(ps)
        dp2 = pe2[:, 1:] - pe2[:, :-1]
        pn2 = np.concatenate([pn1[:, :1], np.log(pe2[:, 1:km]), pn1[:, km:]], axis=1)
        pk2 = np.concatenate([pk1[:, :1], np.exp(self.akap * pn2[:, 1:km]), pk1[:, km:]], axis=1)
        pt = C("pt")
        out = {}
        q2 = [map_col(pe1, C("q%d" % (n + 1)), pe2, 0, self.kord_tr, True, 0.) for n in range(self.nq)]
        if self.hydro:
            tv = pt * (pk1[:, 1:] - pk1[:, :-1]) / (self.akap * (pn1[:, 1:] - pn1[:, :-1]))           # :1590-1596
            t2 = map_col(pn1, tv, pn2, 1, self.kord_tm, True, 184.)                                    # map_scalar, t_min
            pkz = (pk2[:, 1:] - pk2[:, :-1]) / (self.akap * (pn2[:, 1:] - pn2[:, :-1]))
        else:
            delp, delz = C("delp"), C("delz")
            tv = pt * np.exp(self.k1k * np.log(self.rrg * delp / delz * pt))                          # :1598-1604
            t2 = map_col(pn1, tv, pn2, 1, self.kord_tm, True, 184.)
            w2 = map_col(pe1, C("w"), pe2, -2, self.kord_wz, False, 0., qs=C("ws")[:, 0])              # map1_ppm, iv = -2
            dz2 = -(map_col(pe1, -(delz / delp), pe2, 1, self.kord_tm, False) * dp2)                 # map1_ppm, |kord_tm|
            pkz = np.exp(self.akap * np.log(self.rrg * dp2 / dz2 * t2))
            out["w"], out["delz"] = plane(w2, A), plane(dz2, A)
        if self.last:
            ptn = t2 / (1. + self.zvir * q2[0]) if self.nq else t2
        else:
            ptn = t2 / pkz
        pe_out = np.concatenate([pe1[:, :1], pe2[:, 1:km], pe1[:, km:]], axis=1)
        out.update(pe=plane(pe_out, A), peln=plane(pn2, A), pk=plane(pk2, A), pkz=plane(pkz, A), pt=plane(ptn, A), delp=plane(dp2, A))
        for n in range(self.nq):
            out["q%d" % (n + 1)] = plane(q2[n], A)
        out["u"] = plane(self._wind(S, 0), self.R["U"])
        out["v"] = plane(self._wind(S, 1), self.R["V"])
        return out

    def _wind(self, S, d):
        """u (d = 0) at i = 1..nx, j = 1..ny+1 between pe(i, j-1) and pe(i, j); v (d = 1) at i = 1..nx+1, j = 1..ny between pe(i-1, j) and
        pe(i, j) (:1863-1934).  Top: pe0(1) = pe(i, j, 1); pe3(1) = ak(1) + bk(1) ps for u, ak(1) for v."""
        km = self.km
        i0, i1, j0, j1 = self.R["U" if d == 0 else "V"]
        sh = (i0, i1, j0 - 1, j1 - 1) if d == 0 else (i0 - 1, i1 - 1, j0, j1)
        pa, pb = cols(S["pe"], (i0, i1, j0, j1)), cols(S["pe"], sh)
        pe0 = np.concatenate([pa[:, :1], 0.5 * (pb[:, 1:] + pa[:, 1:])], axis=1)
        pss = pb[:, km] + pa[:, km]
        pe3 = np.stack([self.ak[k] + (0.5 * self.bk[k]) * pss for k in range(km + 1)], axis=1)
        if d == 1:
            pe3[:, 0] = self.ak[0]
        return map_col(pe0, cols(S["u" if d == 0 else "v"], (i0, i1, j0, j1)), pe3, -1, self.kord_mt, False)

    # -------------------------------------------------------------------------------------------- modes
    def nl(self, S):
        return self.run({k: np.asarray(v, dtype=self.real) for k, v in S.items()})

    def tl(self, S, P):
        """(values, tangent) by one complex step"""
        LD = self.real
        Z = {k: np.asarray(S[k], dtype=LD) + 1j * H_CS * np.asarray(P[k], dtype=LD) if k in P else np.asarray(S[k], dtype=LD) + 0j for k in S}
        out = self.run(Z)
        return {k: v.real for k, v in out.items()}, {k: v.imag / H_CS for k, v in out.items()}

    def jt_s(self, S, seeds):
        """J^T s of the tangent, entry by entry: one complex-step direction per (input, level), every column at once.  pe is read by the
        winds of the neighbouring columns too, so its directions are coloured by (i mod 2, j mod 2): each output then sees one perturbed
        column, to which its s * y is attributed."""
        nx, ny = self.nx, self.ny
        pj, pi = ny + 7, nx + 7
        I, J = np.meshgrid(np.arange(pi) - 2, np.arange(pj) - 2)            # Fortran i, j of every plane point
        res = {n: np.zeros(np.shape(S[n]), dtype=LD) for n in self.inputs}
        zero = {n: np.zeros(np.shape(S[n])) for n in self.inputs}

        def attribute(y, acc, color):
            for name, rk in self.outputs:
                i0, i1, j0, j1 = self.R[rk]
                w = np.sum(seeds[name][:, j0 + 2:j1 + 3, i0 + 2:i1 + 3] * y[name], axis=0)
                ii, jj = I[j0 + 2:j1 + 3, i0 + 2:i1 + 3], J[j0 + 2:j1 + 3, i0 + 2:i1 + 3]
                if color is None:                       # own-column inputs
                    acc[jj + 2, ii + 2] += w
                    continue
                ci, cj = color
                if rk == "A":
                    m = (ii % 2 == ci) & (jj % 2 == cj)
                    acc[jj[m] + 2, ii[m] + 2] += w[m]
                elif rk == "U":
                    m = ii % 2 == ci
                    tj = np.where(jj % 2 == cj, jj, jj - 1)
                    np.add.at(acc, (tj[m] + 2, ii[m] + 2), w[m])
                else:
                    m = jj % 2 == cj
                    ti = np.where(ii % 2 == ci, ii, ii - 1)
                    np.add.at(acc, (jj[m] + 2, ti[m] + 2), w[m])

        for name in self.inputs:
            nk = np.shape(S[name])[0]
            colors = [(a, b) for a in (0, 1) for b in (0, 1)] if name == "pe" else [None]
            for k in range(nk):
                for col in colors:
                    X = dict(zero)
                    X[name] = np.zeros(np.shape(S[name]))
                    X[name][k] = 1.0 if col is None else ((I % 2 == col[0]) & (J % 2 == col[1])).astype(float)
                    _, y = self.tl(S, X)
                    acc = np.zeros((pj, pi), dtype=LD)
                    attribute(y, acc, col)
                    if col is not None:
                        acc *= (I % 2 == col[0]) & (J % 2 == col[1])
                    res[name][k] += acc
        return res
