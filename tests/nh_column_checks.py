"""Column checks of the non-hydrostatic column operators (csrc/nh.h, nh_ad.h) shared by the host-emulation (test_emul_nh_column.py) and the
MI355X (test_gpu_nh_column.py) runs, against the numpy restatement tests/nh_column_oracle.py.  The product is driven as groups.check_group
drives it: put of the named work fields, fv3lm_run_group, get.  The columns are built here, one kind per point of a 12 x 10 periodic tile
(the kind follows from the point's index, so the halo ring that riem_c covers holds copies of every kind):
  quiet      balanced column, thickness noise +-5 %
  ratio      adjacent delp in ratios of 1e-2 .. 1e2, dz hydrostatic
  stretched  remap_checks.stretched_levels: about 1 Pa at the top, about 1500 Pa at the bottom
  lifted     interfaces below the one beneath + dz_min: one interior level / a run of >= 3 / level 1 / level km / every level
  floored    two or three layers 8 .. 30 times thicker than hydrostatic, so that p_fac pm >= p1 + pm: at level km / interior / level 1
  both       a lifted level and floored layers in one column
on every kind w up to +-3 m/s, zs - zh(km+1) of both signs (ws != 0), temperatures 150 .. 320 K.
Errors are measured per output field and column: max |product - reference| over the column / max |reference| over it; adjoint dot
products per column: |<ad, x> - <s, J x>| / sum |s . J x|."""
import numpy as np
from oracle import NL, TL, AD
import nh_column_oracle as O
from remap_checks import stretched_levels
from fv3_jedi_linearmodel_amd.grid import halo_fill_periodic

NX, NY = 12, 10
LD = np.longdouble
KINDS = ["quiet", "ratio", "stretched", "lift_one", "lift_run", "lift_top", "lift_bot", "lift_all", "floor_bot", "floor_mid", "floor_top", "both",
         "lift_one", "floor_mid", "lift_run", "both", "quiet", "ratio", "stretched", "lift_top", "lift_bot", "floor_bot", "floor_top", "floor_mid"]
GROUP_OF = dict(quiet="quiet", ratio="ratio", stretched="stretched", lift_one="lifted", lift_run="lifted", lift_top="lifted", lift_bot="lifted",
                lift_all="lifted", floor_bot="floored", floor_mid="floored", floor_top="floored", both="both")
SETTINGS = {"sim1": dict(a_imp=1.0, scale_z=0.3), "sim075": dict(a_imp=0.75, scale_z=0.0), "sim06": dict(a_imp=0.6, scale_z=0.3)}
P_FACS = (0.05, 0.25)
DT_AC = 2.0            # acoustic step of every handle (riem_c runs on half of it): the floor fires for short steps (see floored_layers)
TOL_QUIET, TOL_FLOOR, FACTOR = 1e-11, 1e-12, 8.0


def case_kwargs(npz, setting, p_fac, backend):
    ak, bk = stretched_levels(npz)
    return dict(nx=NX, ny=NY, npz=npz, n_split=2, dt=2 * DT_AC, backend=backend, oracle=False, hydrostatic=0, p_fac=p_fac, levels=(ak, bk),
                **SETTINGS[setting])


def consts(c, half=False):
    o = c.opt
    return O.Consts(c.dt_ac * (0.5 if half else 1.0), o.akap, o.ptop, o.rdgas, o.grav, o.a_imp, o.p_fac, o.scale_z)


# ------------------------------------------------------------------------------------------------ the columns
def kinds_of_tile(seed=3):
    rng = np.random.default_rng(seed)
    base = [KINDS[n % len(KINDS)] for n in range(NX * NY)]
    return [base[n] for n in rng.permutation(NX * NY)]


def lifted_layers(kind, km):
    """0-based layers k whose upper interface violates dz_min against the (fixed) interface beneath"""
    mid = km // 2
    if kind == "lift_one":
        return [mid]
    if kind == "lift_run":
        n = 3 if km < 16 else 4
        return list(range(max(0, mid - n // 2), max(0, mid - n // 2) + n))
    if kind == "lift_top":
        return [0]
    if kind == "lift_bot":
        return [km - 1]
    if kind == "lift_all":
        return list(range(km))
    if kind == "both":
        return [0] if km < 6 else [1]
    return []


def floored_layers(kind, km):
    """layers made far thicker than hydrostatic: their pressure starts at 8**-1.4 .. 30**-1.4 of pm, and over a short step the new p1 + pm stays
    near that (the p1 recurrence inverts the interface interpolation), below p_fac pm"""
    n = 1 if km < 5 else 2 if km < 12 else 3
    if kind in ("floor_bot", "both"):
        return list(range(km - n, km))
    if kind == "floor_mid":
        m = km // 2
        return list(range(m - (n - 1) // 2, m - (n - 1) // 2 + n)) if km > 3 else [1]
    if kind == "floor_top":
        return list(range(n))
    return []


def draw(c, seed=3):
    """-> dict: kinds [NY*NX], and the planes [nk, pj, pi] (halo filled) of zh_a, w, pt, delp for riem3 / riem_c"""
    o, km = c.opt, c.npz
    kinds = kinds_of_tile(seed)
    rng = np.random.default_rng(seed + 1000 * km)
    ak, bk = np.asarray(c.ak), np.asarray(c.bk)
    zs = (np.asarray(c.phis).reshape(NY + 7, NX + 7) / o.grav)[3:3 + NY, 3:3 + NX].reshape(-1)
    F = {n: np.zeros((km + (n == "zh"), NY * NX)) for n in ("zh", "w", "pt", "delp")}
    for col, kind in enumerate(kinds):
        ps = 1.0e5 * (1.0 + 0.02 * rng.uniform(-1.0, 1.0))
        if kind == "stretched":
            dp = np.diff(ak) + np.diff(bk) * ps
        elif kind == "ratio":
            dp = 10.0 ** (np.where(np.arange(km) % 2 == 0, 1.0, -1.0) * rng.uniform(0.6, 1.0, km))
            dp *= (ps - o.ptop) / dp.sum()
        else:
            dp = (0.3 + np.arange(1, km + 1) / km) * (1.0 + 0.2 * rng.uniform(-1.0, 1.0, km))
            if kind == "floor_mid":         # SIM_SOLVER's scale_m dm(1) couples w across the levels and smooths the floor away in short columns: light top layer
                dp[0] *= 0.02
            dp *= (ps - o.ptop) / dp.sum()
        T = rng.uniform(150.0, 320.0, km)
        L, Fl = lifted_layers(kind, km), floored_layers(kind, km)
        p = o.ptop                      # lifted layers hold little mass, so that 2 m is 0.7 .. 1.4 of their balanced thickness
        for k in range(km):
            if k in L:
                dp[k] = 2.0 * o.grav * p / (o.rdgas * T[k]) * rng.uniform(0.7, 1.4)
            p += dp[k]
        pe = o.ptop + np.concatenate([[0.0], np.cumsum(dp)])
        pm = dp / np.diff(np.log(pe))
        thick = (dp / o.grav) * o.rdgas * T / pm
        thick *= 1.0 + (0.05 if kind == "quiet" else 0.02) * rng.uniform(-1.0, 1.0, km)
        for k in Fl:
            thick[k] *= rng.uniform(20.0, 30.0) if km < 5 else rng.uniform(8.0, 30.0)
        zh = np.zeros(km + 1)
        zh[km] = zs[col] + DT_AC * rng.uniform(0.05, 0.5) * (1.0 if rng.uniform() < 0.5 else -1.0)      # ws = -+(0.05 .. 0.5) m/s on the full step
        zfix = zh.copy()
        for k in range(km - 1, -1, -1):
            if k in L:
                zh[k] = zfix[k + 1] + rng.uniform(-1.0, 1.9)
                zfix[k] = zfix[k + 1] + O.DZ_MIN
            else:
                zh[k] = zfix[k] = zfix[k + 1] + thick[k]
        F["zh"][:, col], F["delp"][:, col], F["pt"][:, col] = zh, dp, T / pm ** o.akap
        # w up to +-3 m/s, smooth in the vertical: uncorrelated levels would squeeze the light upper layers into the floor in every column
        F["w"][:, col] = rng.uniform(1.0, 3.0) * np.sin(2.0 * np.pi * (rng.integers(1, 3) * np.arange(km) / km + rng.uniform())) + 0.02 * rng.uniform(-1.0, 1.0, km)

    def plane(a):
        p = np.zeros((a.shape[0], NY + 7, NX + 7))
        p[:, 3:3 + NY, 3:3 + NX] = a.reshape(a.shape[0], NY, NX)
        return halo_fill_periodic(p, NX, NY)
    kp = np.full((NY + 7, NX + 7), -1)
    kp[3:3 + NY, 3:3 + NX] = np.arange(NY * NX).reshape(NY, NX)
    kp = halo_fill_periodic(kp, NX, NY)
    return dict(kinds=kinds, col_of_point=kp, planes={n: plane(a) for n, a in F.items()})


class Op:
    """one column operator of the product: group, fields, rectangle, and the restatement as f(X, cols) on [ncol, nk] arrays"""

    def __init__(self, c, name, last=0):
        nx, ny = c.nx, c.ny
        self.c, self.name, self.last = c, name, last
        self.skip = None
        if name == "riem_c":
            self.group, self.ins, self.outs, self.rect = "riem_c", ["gz_a", "wc", "ptc", "delpc"], ["gz", "pkc"], (0, nx + 1, 0, ny + 1)
            self.C = consts(c, half=True)
        elif name == "riem3":
            self.group, self.ins, self.rect = "riem3", ["zh_a", "w_m", "pt_o", "delp_o"], (1, nx, 1, ny)
            self.outs = ["w_o", "delz_o", "zh_o", "ppe", "pk3"] + (["pe", "peln", "pk", "ws"] if last else [])
            self.C = consts(c)
        elif name in ("ring_pk3", "ring_pe"):
            self.group, self.ins, self.outs = "p_ring", ["delp_o"], ["pk3" if name == "ring_pk3" else "pe"]
            self.rect = (-1, nx + 2, -1, ny + 2) if name == "ring_pk3" else (0, nx + 1, 0, ny + 1)
            self.skip = (1, nx, 1, ny)
            self.C = consts(c)
        elif name in ("edge_x", "edge_y"):
            x = name == "edge_x"
            self.group = "update_dz_d"
            self.ins, self.outs = (["crx", "xfx"], ["crx_e", "xfx_e"]) if x else (["cry", "yfx"], ["cry_e", "yfx_e"])
            self.rect = (1, nx + 1, -2, ny + 3) if x else (-2, nx + 3, 1, ny + 1)
            self.C = consts(c)
        else:
            raise ValueError(name)
        i0, i1, j0, j1 = self.rect
        jj, ii = np.meshgrid(np.arange(j0, j1 + 1), np.arange(i0, i1 + 1), indexing="ij")
        keep = np.ones(jj.shape, dtype=bool)
        if self.skip:
            keep = ~((ii >= self.skip[0]) & (ii <= self.skip[1]) & (jj >= self.skip[2]) & (jj <= self.skip[3]))
        self.pj, self.pi = (jj[keep] + 2), (ii[keep] + 2)
        self.hs = np.asarray(c.phis).reshape(ny + 7, nx + 7)[self.pj, self.pi]
        self.dp0 = O.dp_ref(c.ak, c.bk)

    def cols(self, plane):
        """[nk, pj, pi] -> [ncol, nk] on the operator's points"""
        return np.ascontiguousarray(plane[:, self.pj, self.pi].T)

    def scatter(self, a, nk):
        p = np.zeros((nk, self.c.ny + 7, self.c.nx + 7))
        p[:, self.pj, self.pi] = np.asarray(a, dtype=np.float64).T
        return p

    def f(self, X, cols=None, info=None):
        hs = self.hs if cols is None else self.hs[cols]
        hs = np.asarray(hs, dtype=O._re(next(iter(X.values()))[:1, :1]).dtype)
        n = self.name
        if n == "riem_c":
            return O.riem_solver_c(self.C, X, hs, info)
        if n == "riem3":
            return O.riem_solver3(self.C, X, hs, self.last, info)
        if n == "ring_pk3":
            return dict(pk3=O.pk3_halo(self.C, X["delp_o"])[:, 1:])        # level 1 belongs to riem3
        if n == "ring_pe":
            return dict(pe=O.pe_halo(self.C, X["delp_o"]))
        a, b = O.edge_profile(X[self.ins[0]], X[self.ins[1]], self.dp0)
        return {self.outs[0]: a, self.outs[1]: b}

    def out_cols(self, name, plane):
        a = self.cols(plane)
        return a[:, 1:] if self.name == "ring_pk3" else a


def solver_inputs(op, D):
    P = D["planes"]
    src = dict(zip(op.ins, ("zh", "w", "pt", "delp")))
    return {n: op.cols(P[src[n]]) for n in op.ins}


def other_inputs(op, seed=17):
    """p_ring: the drawn delp; edge_profile: Courant numbers and area fluxes of either sign on every point"""
    rng = np.random.default_rng(seed)
    km, n = op.c.npz, len(op.pj)
    if op.group == "p_ring":
        return None
    area = float(np.mean(op.c.metrics["area"]))
    return {op.ins[0]: 0.3 * rng.uniform(-1.0, 1.0, (n, km)), op.ins[1]: 0.05 * area * rng.uniform(-1.0, 1.0, (n, km))}


# ------------------------------------------------------------------------------------------------ conditions on the draw
def as_ld(X):
    return {n: np.asarray(a, dtype=LD) for n, a in X.items()}


def check_draw(op, D, X):
    """conditions, by the restatement alone: every branch fires in >= 4 columns, no column sits at a switch, all pivots positive"""
    info = {}
    op.f(as_ld(X), info=info)
    kinds = np.array([D["kinds"][n] for n in D["col_of_point"][op.pj, op.pi]])
    km = op.c.npz
    lift, flo = info["lifted"], info["floored"]
    assert np.all(info["min_pivot"] > 0.0), (op.name, "pivot", float(info["min_pivot"].min()), kinds[np.argmin(info["min_pivot"])])
    assert np.all(info["lift_margin"] > 1e-6), (op.name, "lift margin", float(info["lift_margin"].min()))
    assert np.all(info["floor_margin"] > 1e-6), (op.name, "floor margin", float(info["floor_margin"].min()))
    for s in (1.0 + 1e-12, 1.0 - 1e-12):
        i2 = {}
        op.f({n: np.asarray(a, dtype=LD) * LD(s) for n, a in X.items()}, info=i2)
        assert np.array_equal(i2["lifted"], lift) and np.array_equal(i2["floored"], flo), (op.name, "a flag flips under inputs x", s)
    # the drawn lifts are the ones that fire
    for col in range(len(kinds)):
        want = np.zeros(km, dtype=bool)
        want[lifted_layers(kinds[col], km)] = True
        assert np.all(lift[col][want]), (op.name, kinds[col], "drawn lifted levels", np.where(want)[0], "fired", np.where(lift[col])[0])
    inner = np.zeros(len(kinds), dtype=bool)          # a floored level or run of levels with an unfloored level right above and right below
    for col in np.where(np.any(flo, axis=1))[0]:
        k = 1
        while k < km - 1:
            if flo[col, k] and not flo[col, k - 1]:
                e = k
                while e < km - 1 and flo[col, e]:
                    e += 1
                inner[col] = inner[col] or not flo[col, e]
                k = e
            k += 1
    runs = lift[:, 2:] & lift[:, 1:-1] & lift[:, :-2] if km >= 3 else lift[:, :0]
    fired = {"lift interior": np.any(lift[:, 1:-1] & ~lift[:, :-2] & ~lift[:, 2:], axis=1) if km >= 3 else np.zeros(len(kinds), bool),
             "lift run >= 3": np.any(runs, axis=1), "lift level 1": lift[:, 0], "lift level km": lift[:, -1], "lift every level": np.all(lift, axis=1),
             "floor level km": flo[:, -1], "floor interior": inner, "floor level 1": flo[:, 0],
             "both": np.any(lift, axis=1) & np.any(flo, axis=1)}
    counts = {n: int(np.sum(v)) for n, v in fired.items()}
    for n, v in counts.items():
        assert v >= 4, (op.name, op.c.npz, op.C.p_fac, op.C.a_imp, n, "fires in", v, "columns", counts)
    groups = np.array([GROUP_OF[k] for k in kinds])
    return dict(kinds=kinds, groups=groups, lifted=lift, floored=flo, counts=counts)


# ------------------------------------------------------------------------------------------------ the product
def _put(op, name, a, which):
    c = op.c
    c.dy.put(name, op.scatter(a, c.dy.levels(name))[None], which)


def _zero_adjoints(op):
    c = op.c
    c.dy.zero_work_adjoint()
    for n in set(op.ins) | set(op.outs) | ({"pe", "peln", "pk", "ws", "pk3"} if op.group in ("riem3", "p_ring") else set()):
        c.dy.put(n, np.zeros(c.dy.shape(n)), 1)


def product(op, mode, X, dX=None, S=None):
    """NL: {output: [ncol, nk]};  TL: (values, tangent);  AD: {input: adjoint} from the output seeds S (every other adjoint of the group zero)"""
    c = op.c
    for n in op.ins:
        _put(op, n, X[n], 0)
    if mode == AD:
        c.dy.run_group(op.group, NL)
        _zero_adjoints(op)
        for n in op.outs:
            full = np.zeros((len(op.pj), c.dy.levels(n)))
            full[:, full.shape[1] - S[n].shape[1]:] = S[n]
            _put(op, n, full, 1)
        c.dy.run_group(op.group, AD)
        return {n: op.cols(c.dy.get(n, 1)[0]) for n in op.ins}
    if mode == TL:
        for n in op.ins:
            _put(op, n, dX[n], 1)
    c.dy.run_group(op.group, mode)
    v = {n: op.out_cols(n, c.dy.get(n, 0)[0]) for n in op.outs}
    if mode == NL:
        return v
    return v, {n: op.out_cols(n, c.dy.get(n, 1)[0]) for n in op.outs}


def make_last(c):
    """run_group takes last_call from the handle's last fv3lm_dyn_core: one nonlinear dyn_core on the balanced state makes it true"""
    from test_oracle_nh import nh_state
    import nh_checks
    T, _ = nh_state(c)
    nh_checks.put(c, T)
    c.dy.dyn_core(NL)


# ------------------------------------------------------------------------------------------------ errors and tolerances
def col_err(got, ref):
    """per column: max |got - ref| over the column / max |ref| over it"""
    got, ref = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD)
    s = np.max(np.abs(ref), axis=1)
    return np.asarray(np.max(np.abs(got - ref), axis=1) / np.where(s > 0, s, 1.0), dtype=np.float64)


def bounds(groups, move):
    """tolerance per column from its kind: quiet 1e-11; the others 8 x the largest float64-vs-longdouble movement of the restatement on
    that kind, at least 1e-12"""
    tol = np.full(len(groups), TOL_QUIET)
    meas = {}
    for g in np.unique(groups):
        m = groups == g
        meas[g] = float(np.max(move[m]))
        if g != "quiet":
            tol[m] = max(TOL_FLOOR, FACTOR * meas[g])
    return tol, meas


def _report(tag, groups, err, tol, meas):
    for g in np.unique(groups):
        m = groups == g
        print("%-34s %-9s move %.2e  tol %.2e  err %.2e" % (tag, g, meas[g], float(tol[m][0]), float(np.max(err[m]))))


def _assert(tag, groups, err, move):
    tol, meas = bounds(groups, move)
    _report(tag, groups, err, tol, meas)
    bad = np.where(~(err <= tol))[0]
    assert bad.size == 0, (tag, [(int(b), groups[b], float(err[b]), float(tol[b])) for b in bad[:6]])
    return {g: (meas[g], float(np.max(err[groups == g]))) for g in np.unique(groups)}


def perturbation(X, seed=29):
    rng = np.random.default_rng(seed)
    sc = dict(zh=0.2, w=0.3, pt=0.05, delp=None, cr=0.1, fx=None)
    key = dict(gz_a="zh", zh_a="zh", wc="w", w_m="w", ptc="pt", pt_o="pt", delpc="delp", delp_o="delp", crx="cr", cry="cr", xfx="fx", yfx="fx")
    out = {}
    for n, a in X.items():
        r = rng.standard_normal(a.shape)
        out[n] = 0.02 * a * r if key[n] == "delp" else 0.1 * np.max(np.abs(a)) * r if key[n] == "fx" else sc[key[n]] * r
    return out


def seeds(op, ref, seed=31):
    """output adjoints scaled by 1 / max |reference| of each output's column, so that every output weighs in"""
    rng = np.random.default_rng(seed)
    out = {}
    for n in op.outs:
        r = np.asarray(ref[n], dtype=np.float64)
        s = np.max(np.abs(r), axis=1, keepdims=True)
        out[n] = rng.standard_normal(r.shape) / np.where(s > 0, s, 1.0)
    return out


JITTER = 3


def jitters(X):
    """the inputs and JITTER - 1 copies moved by -1, 0 or +1 ulp per entry.  The float64 movement of the restatement is the largest distance of
    these evaluations from the longdouble reference at the inputs themselves: one evaluation samples the rounding error of an ill-conditioned
    column once (on the stretched 3-level column the samples spread over 1.3e-13 .. 2.5e-12), and no double-precision code can do better than
    the exact result for inputs one ulp away"""
    rng = np.random.default_rng(71)
    out = [X]
    for _ in range(JITTER - 1):
        out.append({n: np.asarray(a) * (1.0 + rng.integers(-1, 2, np.shape(a)) * 2.0 ** -53) for n, a in X.items()})
    return out


_REF = {}


def cached(op, what, make):
    """references shared by the tests of one process that differ only in how the product computes (hand-written / taped adjoint)"""
    key = (what, op.name, op.last, op.c.npz, op.C.a_imp if op.name != "riem_c" else 1.0, op.C.p_fac, op.C.scale_m if op.name != "riem_c" else 0.0, op.C.dt)
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def check_values_tangent(op, X, groups, tag):
    """NL values, TL values and tangent of every output against the longdouble restatement -> {mode.output: {kind: (move, err)}}"""
    dX = perturbation(X)
    rv, rt = O.tangent(op.f, X, dX)
    Z64 = [O.tangent(op.f, Xj, dX, cdtype=np.complex128) for Xj in jitters(X)]
    got = product(op, NL, X)
    gv, gt = product(op, TL, X, dX)
    m = {}
    for n in op.outs:
        mv = np.max([col_err(v[n], rv[n]) for v, _ in Z64], axis=0)
        mt = np.max([col_err(t[n], rt[n]) for _, t in Z64], axis=0)
        m["nl." + n] = _assert("%s %s nl.%s" % (tag, op.name, n), groups, col_err(got[n], rv[n]), mv)
        _assert("%s %s tl-values.%s" % (tag, op.name, n), groups, col_err(gv[n], rv[n]), mv)
        m["tl." + n] = _assert("%s %s tl.%s" % (tag, op.name, n), groups, col_err(gt[n], rt[n]), mt)
    return m


def _ref_values(op, X):
    return op.f(as_ld(X))


def check_adjoint_jacobian(op, X, groups, tag, S=None):
    """npz <= 8: J^T s of the reference entry by entry"""
    def make():
        S = seeds(op, _ref_values(op, X))
        ref = O.jt_s(op.f, X, S)
        r64 = [O.jt_s(op.f, Xj, S, cdtype=np.complex128) for Xj in jitters(X)]
        return S, ref, {n: np.max([col_err(r[n], ref[n]) for r in r64], axis=0) for n in op.ins}
    S, ref, mov = cached(op, "jac", make)
    ad = product(op, AD, X, S=S)
    m = {}
    for n in op.ins:
        m["ad." + n] = _assert("%s %s ad.%s" % (tag, op.name, n), groups, col_err(ad[n], ref[n]), mov[n])
    return m


def switch_entries(op, flags):
    """(column, input, level) of every input at every switched level and its two neighbours.  With last_call the solver only adds outputs that
    read the pressures and the bottom interface (ws): the levels were pinned one by one on the same columns with last_call false, and this run
    keeps the entries around a lifted level km"""
    sw = flags["lifted"] | flags["floored"]
    if op.last:
        sw = sw & False
        sw[:, -1] = flags["lifted"][:, -1]
    ent = []
    for col in np.where(np.any(sw, axis=1))[0]:
        ks = set()
        for k in np.where(sw[col])[0]:
            ks.update((k - 1, k, k + 1))
        for n in op.ins:
            nk = op.c.npz + (n in ("zh_a", "gz_a"))
            ent += [(int(col), n, int(k)) for k in sorted(ks) if 0 <= k < nk]
        if sw[col, -1]:
            ent.append((int(col), op.ins[0], op.c.npz))       # the bottom interface, which the surface velocity also reads
    return ent


def check_adjoint_dots(op, X, groups, flags, tag, nx_=4, S=None):
    """any npz: <ad, x> = <s, J_ref x> per column for nx_ random x, and for the unit vectors of switch_entries (each one entry of J^T s)"""
    def make():
        S = seeds(op, _ref_values(op, X))
        rnd = []
        for t in range(nx_):
            dx = perturbation(X, seed=50 + t)
            _, y = O.tangent(op.f, X, dx)
            rhs = sum(np.sum(S[o] * y[o], axis=1) for o in op.outs)
            sc = sum(np.sum(np.abs(S[o] * y[o]), axis=1) for o in op.outs)
            mv = np.zeros(len(groups))
            for Xj in jitters(X):
                _, y64 = O.tangent(op.f, Xj, dx, cdtype=np.complex128)
                mv = np.maximum(mv, np.asarray(np.abs(sum(np.sum(S[o] * y64[o], axis=1) for o in op.outs) - rhs) / sc, dtype=np.float64))
            rnd.append((dx, rhs, sc, mv))
        ent = switch_entries(op, flags) if flags is not None else []
        eref = None
        if ent:
            ref, sc = O.jt_s_entries(op.f, X, S, ent)
            sc = np.where(sc > 0, sc, 1.0)
            mv = np.zeros(len(ent))
            for Xj in jitters(X)[:2]:           # the inputs and one jittered copy: the entries are the costly part of the deep cases
                r64, _ = O.jt_s_entries(op.f, Xj, S, ent, cdtype=np.complex128)
                mv = np.maximum(mv, np.asarray(np.abs(r64 - ref) / sc, dtype=np.float64))
            eref = (ref, sc, mv)
        return S, rnd, ent, eref
    S, rnd, ent, eref = cached(op, "dots", make)
    ad = product(op, AD, X, S=S)
    worst = {}
    err, mov = np.zeros(len(groups)), np.zeros(len(groups))
    for dx, rhs, sc, mv in rnd:
        lhs = sum(np.sum(ad[n] * dx[n], axis=1) for n in op.ins)
        err = np.maximum(err, np.asarray(np.abs(lhs - rhs) / sc, dtype=np.float64))
        mov = np.maximum(mov, mv)
    worst["ad.random"] = _assert("%s %s ad.random" % (tag, op.name), groups, err, mov)
    if ent:
        ref, sc, mv = eref
        got = np.array([ad[n][col, k] for col, n, k in ent])
        cols = np.array([e[0] for e in ent])
        e1, m1 = np.zeros(len(groups)), np.zeros(len(groups))
        np.maximum.at(e1, cols, np.asarray(np.abs(got - ref) / sc, dtype=np.float64))
        np.maximum.at(m1, cols, mv)
        touched = np.zeros(len(groups), dtype=bool)
        touched[cols] = True
        worst["ad.entries"] = _assert("%s %s ad.entries(%d)" % (tag, op.name, len(ent)), groups[touched], e1[touched], m1[touched])
    return worst


def check_solver(c, name, last, D, tag, modes=("values", "adjoint")):
    """one solver on the drawn columns -> measured {check: {kind: (movement, error)}}"""
    op = Op(c, name, last)
    X = solver_inputs(op, D)
    flags = check_draw(op, D, X)
    m = {}
    if "values" in modes:
        m.update(check_values_tangent(op, X, flags["groups"], tag))
    if "adjoint" in modes:
        if c.npz <= 8:
            m.update(check_adjoint_jacobian(op, X, flags["groups"], tag))
        else:
            m.update(check_adjoint_dots(op, X, flags["groups"], flags, tag))
    return m


def check_small(c, name, D, tag):
    """edge_col (+ edge_col_ad), ring_col (+ ring_col_ad): values, tangent, adjoint on every point of their rectangles"""
    op = Op(c, name)
    X = other_inputs(op)
    if X is None:
        X = {"delp_o": op.cols(D["planes"]["delp"])}
    groups = np.array(["other"] * len(op.pj))
    m = check_values_tangent(op, X, groups, tag)
    if c.npz <= 8:
        m.update(check_adjoint_jacobian(op, X, groups, tag))
    else:
        m.update(check_adjoint_dots(op, X, groups, None, tag))
    return m


def run_solvers(c, tag, modes):
    """both solvers on one handle, first with last_call false (fresh handle), then true; riem_c does not read last_call and runs once"""
    D = draw(c)
    m = {}
    for last in (0, 1):
        if last:
            make_last(c)
        for name in ("riem_c", "riem3") if not last else ("riem3",):
            m[(name, last)] = check_solver(c, name, last, D, "%s last %d" % (tag, last), modes)
    return m


def run_small(c, tag):
    D = draw(c)
    m = {}
    for name in ("edge_x", "edge_y", "ring_pk3"):
        m[(name, 0)] = check_small(c, name, D, tag)
    make_last(c)
    for name in ("ring_pe", "ring_pk3"):        # the pe ring runs at the last acoustic step only
        m[(name, 1)] = check_small(c, name, D, tag + " last")
    return m
