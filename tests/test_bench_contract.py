"""bench.py's own arithmetic and helpers (CPU): the contract byte count against BASELINE.md §3's worked example, the workload
string derived from the options in force, and one worker of the cpu_baseline leg end to end on a tiny tile."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_contract_bytes_match_baseline_md():
    cells = 6 * 192 * 192 * 127
    # C192L127 hydrostatic, k_split=2, n_split=6, nq=4 -> 326 GB (TL), 897 GB (TL+AD)
    b = bench.algorithmic_bytes(cells, 2, 6, 4)
    assert abs(b / 2.75 - 326e9) < 1e9 and abs(b - 897e9) < 2e9
    # non-hydrostatic: 1280 B per cell and acoustic step, 384 B remap
    bn = bench.algorithmic_bytes(cells, 2, 6, 4, nonhydrostatic=True)
    assert abs(bn / 2.75 / cells / 2 - (6 * 1280 + 208 + 384)) < 1e-6


def test_workload_string_follows_the_options():
    import fv3_jedi_linearmodel_amd as fv3
    o = fv3.default_options()
    s = bench.scheme_string(o, False)
    assert "2/2/2/2/2" in s and "sponge: 1/1/1/1 below level 9" in s and "a_imp" not in s
    o2 = fv3.default_options(hord_ks_pert=0, hord_ks_traj=0, hydrostatic=0, a_imp=1.0)
    s2 = bench.scheme_string(o2, True)
    assert "sponge: off" in s2 and "a_imp=1 (SIM1)" in s2


def test_cpu_baseline_worker_runs():
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "cpu_baseline_worker.py"), "8", "6", "2", "1", "1", "450", "0", "3"],
                                  text=True)
    r = json.loads(out.strip().splitlines()[-1])
    assert r["columns"] == 64 and r["t_tl"] > 0 and r["t_ad"] > 0
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "cpu_baseline_worker.py"), "8", "6", "2", "1", "1", "450", "1", "3"],
                                  text=True)
    assert json.loads(out.strip().splitlines()[-1])["columns"] == 64


def test_default_layout_balances_the_gpus():
    """whole faces where six deal out evenly, the 24 sub-face tiles elsewhere; every GPU then holds the same number of tiles at 4 and 8"""
    from fv3_jedi_linearmodel_amd import cube
    assert [bench.default_layout(w) for w in range(1, 9)] == [1, 1, 1, 2, 2, 1, 2, 2]
    for w in (1, 2, 3, 6):
        assert len({len(cube.faces_of(r, w, 6)) for r in range(w)}) == 1
    for w in (4, 8):
        assert len({len(cube.faces_of(r, w, 24)) for r in range(w)}) == 1
    # position-major order: the six tiles of a 4-GPU rank share one window of their faces (one tile class)
    tl = cube.tiles(48, 2)
    for r in range(4):
        assert len({(tl[t][1], tl[t][2]) for t in cube.faces_of(r, 4, 24)}) == 1


def test_dump_sample_is_fixed_and_inside_the_compute_domain():
    import numpy as np
    # the headline workload: six C192 faces, L127, 8 state fields, 4 arrays each (tl_traj, tl_pert, ad_traj, ad_adj)
    a = bench.dump_sample_index(6, 127, 192, 192, 32)
    assert np.array_equal(a, bench.dump_sample_index(6, 127, 192, 192, 32))
    assert a.size == bench.DUMP_PER_ARRAY and np.all(np.diff(a) > 0)
    assert 32 * (8 * a.size + 1024) <= bench.DUMP_LIMIT_BYTES
    t, k, j, i = np.unravel_index(a, (6, 127, 199, 199))
    assert j.min() >= 3 and j.max() < 195 and i.min() >= 3 and i.max() < 195 and len(set(t.tolist())) == 6 and len(set(k.tolist())) == 127
    # many arrays: each gets fewer points, the total stays under the limit
    b = bench.dump_sample_index(6, 127, 192, 192, 400)
    assert 400 * (8 * b.size + 1024) <= bench.DUMP_LIMIT_BYTES
    # a small domain is dumped whole, in order
    c = bench.dump_sample_index(1, 2, 4, 5, 8)
    x = np.zeros((1, 2, 11, 12)); x[:, :, 3:7, 3:8] = np.arange(40).reshape(1, 2, 4, 5)
    assert np.array_equal(x.reshape(-1)[c], np.arange(40))


def test_write_dump_writes_float64_npy(tmp_path):
    import numpy as np
    info = bench.write_dump(str(tmp_path / "d"), {"tl_pert_u": np.arange(5.0), "ad_adj_u": np.ones(5, dtype=np.float32)})
    assert info["arrays"] == 2 and info["bytes"] <= bench.DUMP_LIMIT_BYTES
    for n in ("tl_pert_u", "ad_adj_u"):
        assert np.load(str(tmp_path / "d" / (n + ".npy"))).dtype == np.float64


def test_cube_inputs_built_ahead_equal_the_case_built_in_place():
    """start_cube_inputs + answered_ahead: the case gets the same fields and exchange tables as one that builds them itself, every call
    started ahead is taken, and cube's functions are themselves again afterwards"""
    import numpy as np
    from fv3_jedi_linearmodel_amd import cube
    from fv3_jedi_linearmodel_amd.harness import CubeCase
    saved = (cube.cube_fields, cube.all_tables, cube.tiled_tables)
    for layout, nq, kw in ((1, 2, {}), (2, 0, dict(hord_mt=5))):
        pool, started = bench.start_cube_inputs(24, 8, nq, layout)
        with bench.answered_ahead(cube, started):
            a = CubeCase(n=24, npz=8, nq=nq, layout=layout, backend="none", seed=bench.CUBE_SEED, **kw)
        pool.shutdown()
        assert not started and (cube.cube_fields, cube.all_tables, cube.tiled_tables) == saved
        b = CubeCase(n=24, npz=8, nq=nq, layout=layout, backend="none", **kw)
        for k in ("traj", "pert"):
            assert all(np.array_equal(getattr(a, k)[f], getattr(b, k)[f]) for f in getattr(b, k))
        assert all(np.array_equal(x, y) for x, y in zip(a.qtraj + a.qpert, b.qtraj + b.qpert)) and len(a.qtraj) == nq
        assert np.array_equal(a.phis, b.phis) and np.array_equal(a.ak, b.ak) and np.array_equal(a.bk, b.bk)
        assert a.tables.keys() == b.tables.keys() and all(np.array_equal(a.tables[k], b.tables[k]) for k in b.tables)


def test_bench_rejects_bad_arguments_before_touching_a_gpu():
    for extra in (["--steps", "0"], ["--gpus", "2", "--dump-outputs", "x"], ["--profile-out", "x"]):
        p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + extra, capture_output=True, text=True)
        assert p.returncode == 2 and "error" in p.stderr, (extra, p.stderr)
