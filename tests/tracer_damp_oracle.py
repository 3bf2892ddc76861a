"""tracer_2d with the tracer damping (nord_tr, trdm2 and their *_pert), composed in numpy around the oracle's per-level fv_tp_2d
(oracle/capi.cpp orc_fv_tp_2d: every scheme, the mass-weighted deln_flux of any order, nonlinear / tangent / adjoint).  Test
infrastructure only.  The oracle's own tracer_2d has no damping; with the damping off this composition reproduces it (asserted by
tracer_damp_checks.check_composition).

The rules of the call site (fv_tracer2d_tlm.F90:1045-1111, fv_control_tlmadm.F90:232-234), as the issue states them:
  1. split_damp_tr = 0: the trajectory's pair is overwritten by the perturbation's;
  2. gate: it == 1 and the TRAJECTORY's trdm2 > 1e-4;
  3. gate open, equal schemes: one differentiated call, mass = dp1, the trajectory's pair;
  4. gate open, split schemes: the differentiated call with hord_tr_pert and the perturbation's pair, then the values again with hord_tr
     and the trajectory's pair;
  5. inside fv_tp_2d the damping is applied only where the damp_c passed is > 1e-4 (the oracle's fv_tp_2d does that itself).
Planes are the padded (ny+7, nx+7) ones of the product: Fortran index i sits at array index i + 2."""
import numpy as np
from oracle import NL, TL, AD


class Damping:
    """the effective pairs after rule 1"""

    def __init__(self, nord_tr=0, trdm2=0.0, nord_tr_pert=0, trdm2_pert=0.0, split_damp_tr=1):
        self.pert = (int(nord_tr_pert), float(trdm2_pert))
        self.traj = (int(nord_tr), float(trdm2)) if split_damp_tr else self.pert

    @property
    def on(self):
        return self.traj[1] > 1.e-4


OFF = Damping()


def _s(i0, i1, j0, j1):
    return (slice(j0 + 2, j1 + 3), slice(i0 + 2, i1 + 3))


def _sh(r, di=0, dj=0):
    return (slice(r[0].start + dj, r[0].stop + dj), slice(r[1].start + di, r[1].stop + di))


class Tracer2d:
    def __init__(self, c, damping=OFF):
        assert c.face is None or c.face != "cube"
        self.c, self.O, self.d = c, c.oracle, damping
        self.nx, self.ny, self.npz, self.nq = c.nx, c.ny, c.npz, c.nq
        self.m = {k: v[0] for k, v in c.metrics.items()}
        self.hord, self.hord_p = c.opt.hord_tr, c.opt.hord_tr_pert
        nx, ny = self.nx, self.ny
        self.A = _s(1, nx, 1, ny)
        self.RX = _s(1, nx + 1, -2, ny + 3)      # cx, xfx: is..ie+1, jsd..jed
        self.RY = _s(-2, nx + 3, 1, ny + 1)      # cy, yfx: isd..ied, js..je+1
        self.FX = _s(1, nx + 1, 1, ny)           # mfx, fx
        self.FY = _s(1, nx, 1, ny + 1)           # mfy, fy
        self.RAX = _s(1, nx, -2, ny + 3)
        self.RAY = _s(-2, nx + 3, 1, ny)

    # ---- the call site: one level, one tracer, sub-step it.  ins = [q, cx, cy, xfx, yfx, ra_x, ra_y, mfx, mfy, dp1] (planes)
    def _pair(self, it, pert):
        if not (it == 1 and self.d.on):
            return None
        return self.d.pert if pert else self.d.traj

    def _tp(self, mode, hord, pair, ins, ins_p=None, outs_p=None):
        sel = ins if pair is not None else ins[:9]
        sel_p = None if ins_p is None else (ins_p if pair is not None else ins_p[:9])
        nord, dc, um = (pair[0], pair[1], 1) if pair is not None else (-1, 0.0, 0)
        ot, op = self.O.fv_tp_2d(mode, hord, nord, dc, 1, um, [a[None] for a in sel], None if sel_p is None else [a[None] for a in sel_p],
                                 None if outs_p is None else [a[None] for a in outs_p])
        op = None if op is None else [a[0] for a in op]
        if mode == AD and pair is None:
            op = op + [np.zeros_like(ins[9])]
        return [a[0] for a in ot], op

    def call(self, mode, it, ins, ins_p=None, outs_p=None):
        """-> (fx, fy) values and, TL: their tangents / AD: the ten input adjoints"""
        split = self.hord != self.hord_p
        ot, op = self._tp(mode, self.hord_p, self._pair(it, split), ins, ins_p, outs_p)
        if split:
            ot, _ = self._tp(NL, self.hord, self._pair(it, False), ins)
        return ot, op

    # ---- what precedes the sub-steps: area fluxes, sub-step counts, scaling by frac (fv_tracer2d_tlm.F90:1248-1345)
    def _xfx_factor(self, cx, cy):
        m = self.m
        fx = np.zeros_like(cx); fy = np.zeros_like(cy)
        up = np.roll(m["dxa"] * m["sin_sg3"], 1, axis=1) * m["dy"]; dn = m["dxa"] * m["dy"] * m["sin_sg1"]
        fx[(Ellipsis,) + self.RX] = np.where(cx > 0., up, dn)[(Ellipsis,) + self.RX]
        up = np.roll(m["dya"] * m["sin_sg4"], 1, axis=0) * m["dx"]; dn = m["dya"] * m["dx"] * m["sin_sg2"]
        fy[(Ellipsis,) + self.RY] = np.where(cy > 0., up, dn)[(Ellipsis,) + self.RY]
        return fx, fy

    def _ksplt(self, cx, cy):
        A, npz = self.A, self.npz
        cmax = np.zeros(npz)
        for k in range(npz):
            c_ = np.maximum(np.abs(cx[k][A]), np.abs(cy[k][A]))
            if not (k + 1 < npz // 6):
                c_ = c_ + 1. - self.m["sin_sg5"][A]
            cmax[k] = max(0., c_.max())
        nsplt = int(1. + cmax.max())
        ks = [int(1. + cmax[k]) if nsplt != 1 else 1 for k in range(npz)]
        return nsplt, ks

    def _scale(self, ks, cx, cy, mfx, mfy, xf, yf):
        """the arrays the sub-steps read: cxs, cys, xfx, yfx, mfxs, mfys (linear in cx, cy, mfx, mfy for given signs)"""
        fr = np.array([1. / k for k in ks])[:, None, None]
        E = Ellipsis
        cxs, cys, mfxs, mfys = cx.copy(), cy.copy(), mfx.copy(), mfy.copy()
        cxs[(E,) + self.RX] = (cx * fr)[(E,) + self.RX]; cys[(E,) + self.RY] = (cy * fr)[(E,) + self.RY]
        mfxs[(E,) + self.FX] = (mfx * fr)[(E,) + self.FX]; mfys[(E,) + self.FY] = (mfy * fr)[(E,) + self.FY]
        return cxs, cys, cx * xf * fr, cy * yf * fr, mfxs, mfys

    def _halo(self, a):
        from fv3_jedi_linearmodel_amd import grid as G
        return G.halo_fill_periodic(a, self.nx, self.ny)

    def _halo_ad(self, a):
        """transpose of the periodic fill: every point's adjoint lands on the interior point it was copied from"""
        pj, pi = a.shape[-2:]
        ii = (np.arange(pi) - 3) % self.nx + 3; jj = (np.arange(pj) - 3) % self.ny + 3
        out = np.zeros_like(a)
        np.add.at(out, (Ellipsis, jj[:, None], ii[None, :]), a)
        return out

    # ---- nonlinear / tangent
    def forward(self, T, P=None, tape=None):
        """T, P: dicts dp1 mfx mfy cx cy q1.. of (npz, pj, pi) arrays.  -> (q values, q tangents or None, nsplt)"""
        tl = P is not None
        A, m, npz, nq = self.A, self.m, self.npz, self.nq
        xf, yf = self._xfx_factor(T["cx"], T["cy"])
        nsplt, ks = self._ksplt(T["cx"], T["cy"])
        assert nsplt == 1 or self.c.face is None, "sub-cycling: the periodic tile only"
        sc = self._scale(ks, T["cx"], T["cy"], T["mfx"], T["mfy"], xf, yf)
        sp = self._scale(ks, P["cx"], P["cy"], P["mfx"], P["mfy"], xf, yf) if tl else None
        q = [T["q%d" % (n + 1)].copy() for n in range(nq)]; dp1 = T["dp1"].copy()
        qp = [P["q%d" % (n + 1)].copy() for n in range(nq)] if tl else None; dp1p = P["dp1"].copy() if tl else None
        z = np.zeros_like(dp1[0])
        if tape is not None:
            tape.update(nsplt=nsplt, ks=ks, xf=xf, yf=yf, sc=sc, steps={})

        def pre(s, k, d1, base):
            cxs, cys, xfx, yfx, mfxs, mfys = s
            dp2, rax, ray = z.copy(), z.copy(), z.copy()
            dp2[A] = d1[k][A] + (mfxs[k][A] - mfxs[k][_sh(A, 1)] + (mfys[k][A] - mfys[k][_sh(A, 0, 1)])) * m["rarea"][A]
            rax[self.RAX] = base * m["area"][self.RAX] + (xfx[k][self.RAX] - xfx[k][_sh(self.RAX, 1)])
            ray[self.RAY] = base * m["area"][self.RAY] + (yfx[k][self.RAY] - yfx[k][_sh(self.RAY, 0, 1)])
            return dp2, rax, ray

        for it in range(1, nsplt + 1):
            for k in range(npz):
                if it > ks[k]:
                    continue
                dp2, rax, ray = pre(sc, k, dp1, 1.)
                if tl:
                    dp2p, raxp, rayp = pre(sp, k, dp1p, 0.)
                for n in range(nq):
                    ins = [q[n][k], sc[0][k], sc[1][k], sc[2][k], sc[3][k], rax, ray, sc[4][k], sc[5][k], dp1[k]]
                    ins_p = [qp[n][k], sp[0][k], sp[1][k], sp[2][k], sp[3][k], raxp, rayp, sp[4][k], sp[5][k], dp1p[k]] if tl else None
                    (fx, fy), fp = self.call(TL if tl else NL, it, ins, ins_p)
                    div = (fx[A] - fx[_sh(A, 1)] + (fy[A] - fy[_sh(A, 0, 1)])) * m["rarea"][A]
                    num = q[n][k][A] * dp1[k][A] + div
                    if tape is not None:
                        tape["steps"][(it, k, n)] = (ins[0].copy(), dp1[k].copy(), dp2.copy(), rax, ray, (num / dp2[A]).copy())
                    if tl:
                        divp = (fp[0][A] - fp[0][_sh(A, 1)] + (fp[1][A] - fp[1][_sh(A, 0, 1)])) * m["rarea"][A]
                        nump = qp[n][k][A] * dp1[k][A] + q[n][k][A] * dp1p[k][A] + divp
                        qp[n][k][A] = (nump * dp2[A] - num * dp2p[A]) / dp2[A] ** 2
                    q[n][k][A] = num / dp2[A]
                if it != nsplt:
                    dp1[k][A] = dp2[A]
                    if tl:
                        dp1p[k][A] = dp2p[A]
            if it != nsplt:
                q = [self._halo(a) for a in q]
                if tl:
                    qp = [self._halo(a) for a in qp]
        return q, qp, nsplt

    # ---- adjoint: seeds = adjoints of the transported tracers; -> dict of input adjoints on whole padded planes
    def adjoint(self, T, seeds):
        A, m, npz, nq = self.A, self.m, self.npz, self.nq
        tape = {}
        self.forward(T, None, tape)
        nsplt, ks, sc = tape["nsplt"], tape["ks"], tape["sc"]
        qa = [np.array(s, dtype=np.float64) for s in seeds]
        z3 = np.zeros_like(T["dp1"])
        dp1a = z3.copy(); sa = [z3.copy() for _ in range(6)]      # adjoints of cxs cys xfx yfx mfxs mfys
        ra = m["rarea"]
        for it in range(nsplt, 0, -1):
            if it != nsplt:
                qa = [self._halo_ad(a) for a in qa]
            for k in range(npz):
                if it > ks[k]:
                    continue
                dp2a = np.zeros_like(dp1a[k]); raxa = np.zeros_like(dp2a); raya = np.zeros_like(dp2a)
                if it != nsplt:
                    dp2a[A] = dp1a[k][A]; dp1a[k][A] = 0.
                for n in range(nq - 1, -1, -1):
                    q0, d1, dp2, rax, ray, qnew = tape["steps"][(it, k, n)]
                    g = qa[n][k][A].copy()
                    dva = g * ra[A] / dp2[A]
                    dp2a[A] -= g * qnew / dp2[A]
                    dp1a[k][A] += g * q0[A] / dp2[A]
                    qa[n][k][A] = g * d1[A] / dp2[A]
                    fxa = np.zeros_like(dp2a); fya = np.zeros_like(dp2a)
                    fxa[A] += dva; fxa[_sh(A, 1)] -= dva; fya[A] += dva; fya[_sh(A, 0, 1)] -= dva
                    ins = [q0, sc[0][k], sc[1][k], sc[2][k], sc[3][k], rax, ray, sc[4][k], sc[5][k], d1]
                    _, ia = self.call(AD, it, ins, None, [fxa, fya])
                    qa[n][k] += ia[0]
                    for j, t in enumerate((1, 2, 3, 4)):
                        sa[j][k] += ia[t]
                    raxa += ia[5]; raya += ia[6]; sa[4][k] += ia[7]; sa[5][k] += ia[8]; dp1a[k] += ia[9]
                dp1a[k][A] += dp2a[A]
                w = dp2a[A] * ra[A]
                sa[4][k][A] += w; sa[4][k][_sh(A, 1)] -= w; sa[5][k][A] += w; sa[5][k][_sh(A, 0, 1)] -= w
                sa[2][k][self.RAX] += raxa[self.RAX]; sa[2][k][_sh(self.RAX, 1)] -= raxa[self.RAX]
                sa[3][k][self.RAY] += raya[self.RAY]; sa[3][k][_sh(self.RAY, 0, 1)] -= raya[self.RAY]
        fr = np.array([1. / k for k in ks])[:, None, None]
        E = Ellipsis
        cxa = sa[2] * tape["xf"] * fr; cya = sa[3] * tape["yf"] * fr
        mfxa, mfya = sa[4].copy(), sa[5].copy()
        for dst, src, r in ((cxa, sa[0], self.RX), (cya, sa[1], self.RY)):
            rest = src.copy(); rest[(E,) + r] = 0.
            dst[(E,) + r] += (src * fr)[(E,) + r]; dst += rest
        for a, r in ((mfxa, self.FX), (mfya, self.FY)):
            a[(E,) + r] = (a * fr)[(E,) + r]
        out = dict(dp1=dp1a, mfx=mfxa, mfy=mfya, cx=cxa, cy=cya)
        for n in range(nq):
            out["q%d" % (n + 1)] = qa[n]
        return out
