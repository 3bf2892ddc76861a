"""CPU (-m "not gpu"): the vertical remap with the source window (csrc/remap.h: map_loop, edge_solve, sweep C of map_col_ad_s) on columns whose
windows move differently in neighbouring lanes, on the host-emulation build.  States (built here from remap_checks.column_state):
  per_column   every column draws its own warp: source layers of 0.08 .. 3 target layers, runs of thin ones (up to ten in a target at
               npz = 20: the window runs through them in the sum over the layers inside a target) and thick ones (the window stays);
               the non-hydrostatic case: thicknesses within 10 % of the targets, the amplitude drawn per column
  ties         every second source interface is the target interface bit for bit (both comparisons of the search hold at once), the others
               sit up to 30 % of the thinner neighbouring layer off
Checked against the numpy restatement (remap_checks, its own tolerances: NL / TL 1e-12, adjoint dot products 1e-11), both values of last.
The rewrite changed which loads feed the arithmetic, not the arithmetic, so the host-emulation results are also compared bit for bit
(np.array_equal) with tests/golden/remap_window/*.npz: NL values and TL tangents of the remapped fields, the adjoints of every input,
written by the library of the commit before the window on the same states (tools/make_remap_window_golden.py <library>).  A difference
there means an expression or an order of summation changed.  The goldens keep every second point in i and j.
Shared with test_gpu_remap_window.py (the MI355X build has no goldens: hipcc contracts a * b + c, g++ -O2 does not)."""
import os
import numpy as np
import pytest
from common import Case
from oracle import NL, TL, AD
import remap_checks as RC

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "remap_window")
# name: (npz, hydrostatic, limited kord of the trajectory or None, state)
CASES = {
    "per_column_12": (12, 1, None, "per_column"),
    "ties_12": (12, 1, None, "ties"),
    "per_column_20": (20, 1, None, "per_column"),
    "ties_20": (20, 1, None, "ties"),
    "nh_per_column_12": (12, 0, None, "per_column"),
    "kord9_per_column_12": (12, 1, 9, "per_column"),
}


def make_case(name, backend="emul"):
    npz, hydro, kord, _ = CASES[name]
    kw = dict(kord_tm=-kord, kord_tr=kord, kord_mt=kord) if kord else {}
    return Case(nx=8, ny=9, npz=npz, nq=2, oracle=False, hydrostatic=hydro, backend=backend, **kw)


def _with_pressures(c, S, pe):
    """S with the source interfaces pe: T_v, the tracers and the winds of every layer stay, the pressure functions follow"""
    o = c.opt
    S = dict(S)
    pkz0 = np.diff(S["pk"], axis=0) / (o.akap * np.diff(S["peln"], axis=0))
    tv = S["pt"] * pkz0
    peln = np.log(pe)
    pk = np.exp(o.akap * peln)
    S.update(pe=pe, peln=peln, pk=pk, pt=tv / (np.diff(pk, axis=0) / (o.akap * np.diff(peln, axis=0))))
    if not o.hydrostatic:
        S["delz"] = -(o.rdgas / o.grav) * tv * np.diff(peln, axis=0)
        S["delp"] = np.diff(pe, axis=0)
    return S


def _thicknesses(km, pj, pi, rng):
    """source thicknesses in units of target layers, every column its own: a bounded random walk in log thickness (0.08 .. 3, at most a
    factor 2.5 between neighbours: larger jumps make the edge-value solve ill-conditioned and the comparison one of rounding), and in a
    third of the columns a run of thin layers (0.09 of a target layer each: a target then holds up to ten) from which the others grow
    geometrically"""
    lo, hi, step = np.log(0.08), np.log(3.0), np.log(2.5)
    lt = np.empty((km, pj, pi))
    lt[0] = rng.uniform(lo, hi, (pj, pi))
    for n in range(1, km):
        x = lt[n - 1] + step * rng.uniform(-1.0, 1.0, (pj, pi))
        x = np.where(x > hi, 2.0 * hi - x, x)
        lt[n] = np.where(x < lo, 2.0 * lo - x, x)
    nb = 9 if km >= 20 else 5
    lev = np.arange(km)
    for j in range(pj):
        for i in range(pi):
            if rng.uniform() < 0.35:
                s0 = rng.integers(0, km - nb + 1)
                dist = np.maximum(0, np.maximum(s0 - lev, lev - (s0 + nb - 1)))
                r0, r1 = 1.0, 50.0      # the ratio at which the column sums to km target layers
                for _ in range(60):
                    r = 0.5 * (r0 + r1)
                    r0, r1 = (r, r1) if np.sum(0.09 * r ** dist) < km else (r0, r)
                lt[:, j, i] = np.log(0.09 * r0 ** dist)
    return np.exp(lt)


def make_state(c, name):
    kind = CASES[name][3]
    km = c.npz
    seed = sum(ord(ch) for ch in name)
    S = RC.column_state(c, "small", seed=seed, hard=True)
    rng = np.random.default_rng(seed + 1)
    pj, pi = S["pe"].shape[1:]
    ps = S["pe"][km]
    pe2 = np.asarray(c.ak)[:, None, None] + np.asarray(c.bk)[:, None, None] * ps[None]
    pe2[0], pe2[km] = c.opt.ptop, ps
    if kind == "per_column" and not c.opt.hydrostatic:
        # -delz / delp goes like 1 / p and the unlimited profile takes it below zero under larger displacements: thicknesses within 10 %
        # of the targets, the amplitude drawn per column (a window still moves by 0, 1 or 2 layers, differently from its neighbour)
        d = np.diff(pe2, axis=0) * (1.0 + 0.1 * rng.uniform(0.0, 1.0, (1, pj, pi)) * rng.uniform(-1.0, 1.0, (km, pj, pi)))
        pe = c.opt.ptop + np.concatenate([np.zeros((1, pj, pi)), np.cumsum(d, axis=0) * ((ps - c.opt.ptop) / d.sum(axis=0))[None]], axis=0)
    elif kind == "per_column":
        inc = _thicknesses(km, pj, pi, rng)
        xi = np.concatenate([np.zeros((1, pj, pi)), np.cumsum(inc, axis=0)], axis=0)
        xi *= km / xi[-1]
        k0 = np.minimum(np.floor(xi).astype(int), km - 1)
        lo = np.take_along_axis(pe2, k0, axis=0)
        hi = np.take_along_axis(pe2, k0 + 1, axis=0)
        pe = lo + (xi - k0) * (hi - lo)
    elif kind == "ties":
        d = np.diff(pe2, axis=0)
        room = np.concatenate([d[:1], np.minimum(d[1:], d[:-1]), d[-1:]], axis=0)
        pe = pe2 + 0.3 * rng.uniform(-1.0, 1.0, pe2.shape) * room
        pe[::2] = pe2[::2]
    else:
        raise ValueError(kind)
    pe[0], pe[km] = c.opt.ptop, ps
    assert np.all(np.diff(pe, axis=0) > 0.0)
    return _with_pressures(c, S, pe)


def sources_per_target(c, S):
    """per column and target layer: how many source interfaces lie strictly inside it (= how far the window moves for it)"""
    km = c.npz
    ps = S["pe"][km]
    pe2 = np.asarray(c.ak)[:, None, None] + np.asarray(c.bk)[:, None, None] * ps[None]
    pe2[0] = c.opt.ptop
    src = S["pe"][1:km]
    return np.array([np.sum((src > pe2[k]) & (src < pe2[k + 1]), axis=0) for k in range(km)])


def run_checks(c, S):
    """remap_checks' own bounds, both values of last; the non-hydrostatic adjoint by dot products as well"""
    for last in (0, 1):
        RC.check_nl_tl(c, S, last)
        RC.check_ad_dot(c, S, last)


def bits(c, S, last):
    """what the goldens hold, from the library behind c"""
    import remap_oracle as RO
    R = RO.Remap(c, last)
    mapped = ["pt", "u", "v"] + ["q%d" % (n + 1) for n in range(c.nq)] + ([] if c.opt.hydrostatic else ["w", "delz"])
    out = {}
    nl = RC.product(c, NL, last, S)
    _, tl = RC.product(c, TL, last, S, RC.perturbation(S))
    ad = RC.product(c, AD, last, S, seeds=RC.make_seeds(c, R))
    for n in mapped:
        out["nl.%s.%d" % (n, last)] = np.ascontiguousarray(RC.on_rect(R, n, nl[n])[:, ::2, ::2])
        out["tl.%s.%d" % (n, last)] = np.ascontiguousarray(RC.on_rect(R, n, tl[n])[:, ::2, ::2])
    for n in R.inputs:
        out["ad.%s.%d" % (n, last)] = np.ascontiguousarray(ad[n][:, 2:c.ny + 4:2, 2:c.nx + 4:2])
    return out


@pytest.fixture(scope="module", params=list(CASES))
def case(request):
    c = make_case(request.param)
    return request.param, c, make_state(c, request.param)


def test_windows_move_differently_in_neighbouring_lanes():
    """the states are what the header says: per_column reaches 0 and >= 8 layers per target and differs between neighbours; ties tie"""
    for name, most in (("per_column_20", 8), ("per_column_12", 5), ("nh_per_column_12", 2)):
        c = make_case(name)
        n = sources_per_target(c, make_state(c, name))
        assert n.min() == 0 and n.max() >= most, (name, n.min(), n.max())
        assert np.mean(np.any(n[:, :, 1:] != n[:, :, :-1], axis=0)) > 0.9, name
    c = make_case("ties_20")
    S = make_state(c, "ties_20")
    pe2 = np.asarray(c.ak)[:, None, None] + np.asarray(c.bk)[:, None, None] * S["pe"][c.npz][None]
    assert np.array_equal(S["pe"][2:-1:2], pe2[2:-1:2]) and not np.any(S["pe"][1:-1:2] == pe2[1:-1:2])


def test_against_the_restatement(case):
    _, c, S = case
    run_checks(c, S)


def test_bit_identical_to_the_golden(case):
    name, c, S = case
    gold = np.load(os.path.join(GOLDEN, name + ".npz"))
    seen = 0
    for last in (0, 1):
        for key, a in bits(c, S, last).items():
            assert np.array_equal(a, gold[key]), (name, key, float(np.max(np.abs(a - gold[key]))))
            seen += 1
    assert seen == len(gold.files)
