"""The reference promises that the metric entries it leaves poisoned (tiny_number / big_number after grid_utils_init, and what lies outside
its arrays) are never read; a host that passes FMS's own arrays through include/fv3lm.h relies on the product keeping that promise.
Every stage is run three times -- metrics as they are, the entries tests/face_oracle.py marks undefined set to 1e30, and to -3e33 (finite:
the library is built with -ffinite-math-only) -- through harness.Case / CubeCase(metrics_hook=...), and the three runs must agree bit for
bit on the rects groups.py calls defined: the six kernel groups (tangent and adjoint) and tracer_2d on one C8 face and on six C8 faces,
and one fv_dynamics step in each of its three modes on the six faces (a single face has no exchange tables to step with)."""
import numpy as np
from oracle import NL, TL, AD
import groups as G
import face_oracle as fo

VALUES = (None, 1.0e30, -3.0e33)
GROUPS = ["c_sw", "geopk_c", "p_grad_c", "d_sw", "geopk_d", "one_grad_p"]
N, NPZ = 8, 3
_MASKS = {}


def undefined(n):
    """({plane: boolean [6, pj, pj]}, boolean [6, 4, pj] for the a2b edge weights): True where the reference holds no value"""
    if n not in _MASKS:
        from fv3_jedi_linearmodel_amd import cube
        m, poison, edge, _, _ = fo.face_metrics(cube.cube_corner_points(n))
        _MASKS[n] = ({k: ~v for k, v in fo.defined(m, poison).items()}, ~np.isfinite(edge))
    return _MASKS[n]


def poison_hook(n, value, face=None):
    """metrics_hook that writes `value` over every undefined entry (face: the single face of a harness.Case)"""
    if value is None:
        return None
    bad, bad_edge = undefined(n)
    sel = slice(None) if face is None else slice(face, face + 1)

    def hook(metrics, edge, ecorner):
        return {k: np.where(bad[k][sel], value, v) for k, v in metrics.items()}, np.where(bad_edge[sel], value, edge), ecorner
    return hook


drop_undefined = G.drop_face_corners        # the outputs the reference itself forms from poisoned entries take no part


def _rect(c, arr, rk):
    return arr[c.rect(*G.rects(c)[rk])].copy()


def _run_groups(c, inputs, lead):
    """every kernel group, tangent (trajectory + perturbation outputs on their rects) and adjoint (input adjoints, whole planes)"""
    out = {}
    L = (lambda a: a[None]) if lead == 1 else (lambda a: np.ascontiguousarray(np.broadcast_to(a, (lead,) + a.shape)))
    for g in GROUPS:
        _, _, ins, outs = G.table(c)[g]
        T, P = inputs[g]
        for n in ins:
            c.dy.put(n, L(T[n]), 0); c.dy.put(n, L(P[n]), 1)
        c.dy.run_group(g, TL)
        for n, rk in outs:
            if n is None:
                continue
            for which in (0, 1):
                a = c.dy.get(n, which)
                out[(g, "tl", n, which)] = np.stack([_rect(c, drop_undefined(c, n, a[t]), rk) for t in range(a.shape[0])])
        rng = np.random.default_rng(11)
        seeds = {n: drop_undefined(c, n, G.masked(c, rng.standard_normal((c.dy.levels(n), c.ny + 7, c.nx + 7)), rk)) for n, rk in outs if n}
        for n in ins:
            c.dy.put(n, L(T[n]), 0)
        c.dy.run_group(g, NL)
        c.dy.zero_work_adjoint()
        for n in set(ins) | set(seeds):
            c.dy.put(n, np.zeros(c.dy.shape(n)), 1)
        for n, s in seeds.items():
            c.dy.put(n, L(s), 1)
        c.dy.run_group(g, AD)
        for n in ins:
            out[(g, "ad", n)] = c.dy.get(n, 1).copy()
    return out


def _run_tracer(c, T, P, lead):
    out = {}
    L = (lambda a: a[None]) if lead == 1 else (lambda a: a)
    names = ["dp1", "mfx", "mfy", "cx", "cy", "q1"]
    for n in names:
        c.dy.put(n, L(T[n]), 0); c.dy.put(n, L(P[n]), 1)
    c.dy.tracer_2d(TL)
    for which in (0, 1):
        out[("tracer", "tl", which)] = _rect(c, c.dy.get("q1", which), "A")
    rng = np.random.default_rng(21)
    seed = G.masked(c, rng.standard_normal(c.dy.shape("q1")), "A")
    for n in names:
        c.dy.put(n, L(T[n]), 0)
    c.dy.tracer_2d(NL)
    for n in names:
        c.dy.put(n, L(T[n]), 0); c.dy.put(n, np.zeros(c.dy.shape(n)), 1)
    c.dy.put("q1", seed, 1)
    c.dy.tracer_2d(AD)
    for n in names:
        out[("tracer", "ad", n)] = c.dy.get(n, 1).copy()
    return out


def _run_fv_dynamics(c, T, P, lead):
    out = {}
    L = (lambda a: a[None]) if lead == 1 else (lambda a: a)
    ins = ["u", "v", "pt", "delp", "pe", "peln", "pk", "pkz", "q1"]
    outs = [("u", "U"), ("v", "V"), ("pt", "A"), ("delp", "A"), ("q1", "A")]
    for mode, tag in ((NL, "nl"), (TL, "tl")):
        for n in ins:
            c.dy.put(n, L(T[n]), 0); c.dy.put(n, L(P[n]), 1)
        c.dy.fv_dynamics(mode)
        for n, rk in outs:
            for which in ((0,) if mode == NL else (0, 1)):
                out[("fv_dynamics", tag, n, which)] = _rect(c, c.dy.get(n, which), rk)
    rng = np.random.default_rng(41)
    seeds = {n: G.masked(c, rng.standard_normal(c.dy.shape(n)), rk) for n, rk in outs}
    for n in ins:
        c.dy.put(n, L(T[n]), 0)
    c.dy.fv_dynamics(NL)
    for n in ins:
        c.dy.put(n, np.zeros(c.dy.shape(n)), 1)
    for n, s in seeds.items():
        c.dy.put(n, s, 1)
    c.dy.fv_dynamics(AD)
    for n in ins:
        if n not in ("pe", "peln", "pk"):
            out[("fv_dynamics", "ad", n)] = c.dy.get(n, 1).copy()
    return out


def _compare(runs):
    base = runs[0]
    bad = []
    for v, r in zip(VALUES[1:], runs[1:]):
        assert set(r) == set(base)
        for k in sorted(base, key=str):
            if not np.array_equal(base[k], r[k]):
                d = np.argwhere(base[k] != r[k])
                bad.append((v, k, len(d), tuple(d[0])))
    assert not bad, "a poisoned metric entry was read: (value, output, entries that differ, first) %s" % (bad[:12],)


def check_face(backend, face=2):
    from common import Case
    runs, shared = [], None
    for v in VALUES:
        c = Case(nx=N, ny=N, npz=NPZ, n_split=2, dt=1800.0, backend=backend, face=face, nq=1, oracle=(v is None),
                 metrics_hook=poison_hook(N, v, face))
        if v is None:       # inputs once, from the oracle on the metrics as they are
            Td, Pd = G._dyn_outputs(c)
            Td["dp1"], Pd["dp1"], Td["q1"], Pd["q1"] = c.traj["delp"][0], c.pert["delp"][0], c.qtraj[0][0], c.qpert[0][0]
            shared = ({g: G.make_inputs(c, g) for g in GROUPS}, (Td, Pd))
        out = _run_groups(c, shared[0], 1)
        out.update(_run_tracer(c, *shared[1], 1))       # (fv_dynamics needs the exchange tables: six faces only)
        runs.append(out)
    _compare(runs)
    return len(runs[0])


def check_cube(backend):
    from common import Case, CubeCase
    from fv3_jedi_linearmodel_amd import cube
    from fv3_jedi_linearmodel_amd.harness import cube_step_state
    f0 = Case(nx=N, ny=N, npz=NPZ, n_split=2, dt=1800.0, backend="none", face=2, nq=1, oracle=True)
    ginputs = {g: G.make_inputs(f0, g) for g in GROUPS}     # arbitrary smooth group inputs, the same on all six faces
    runs, shared = [], None
    for v in VALUES:
        c = CubeCase(n=N, npz=NPZ, n_split=2, backend=backend, nq=1, oracle=(v is None), metrics_hook=poison_hook(N, v))
        if v is None:
            ins = ["u", "v", "pt", "delp"]
            ot, op = c.oracle.dyn_core(TL, c.dims.dt / c.dims.k_split, c.dims.n_split, [c.traj[n] for n in ins], [c.pert[n] for n in ins])
            qt, qp = c.qtraj[0].copy(), c.qpert[0].copy()
            cube.apply_table(c.tables["cell"], qt); cube.apply_table(c.tables["cell"], qp)
            Td = dict(dp1=c.traj["delp"], mfx=ot[4], mfy=ot[5], cx=ot[6], cy=ot[7], q1=qt)
            Pd = dict(dp1=c.pert["delp"], mfx=op[4], mfy=op[5], cx=op[6], cy=op[7], q1=qp)
            shared = ((Td, Pd), cube_step_state(c))
        out = _run_groups(c, ginputs, 6)
        out.update(_run_tracer(c, *shared[0], 6))
        out.update(_run_fv_dynamics(c, *shared[1], 6))
        runs.append(out)
    _compare(runs)
    return len(runs[0])
