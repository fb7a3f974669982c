"""bench.py's CPU-side pieces (no GPU): the CPU baseline leg (the oracle's
tree built once, queries timed apart) and the reference tree handle it uses."""
import argparse

import numpy as np
import torch

import oracle_ctypes as O


def test_tree_handle_matches_repulsion_queries():
    rng = np.random.default_rng(3)
    for scale in (1e-4, 1.0, 20.0):
        Y = rng.normal(size=(3000, 2)) * scale
        Y[7] = Y[11]                                    # a duplicate pair
        Q = Y[rng.choice(3000, 200, replace=False)]
        tree = O.Tree(Y)
        r1, z1, v = tree.query(0.5, Q, threads=4)
        r2, z2 = O.repulsion_queries(Y, 0.5, Q, threads=1)
        tree.close()
        assert np.array_equal(r1, r2) and np.array_equal(z1, z2)
        assert v >= len(Q)


def test_cpu_baseline_block():
    import bench
    rng = np.random.default_rng(0)
    n, k = 2000, 30
    X = rng.normal(size=(n, 8))
    idx, dist = O.knn(X, k)
    rp = np.arange(0, n * k + 1, k, dtype=np.int64)
    p, _ = O.affinities(rp, dist.ravel(), 10.0)
    jr, jc, jv = O.joint(rp, idx.ravel(), p, n)
    snaps = {t: rng.normal(size=(n, 2)) * s for t, s in ((1, 1e-4), (100, 1.0), (1000, 30.0))}
    a = argparse.Namespace(theta=0.5, iterations=1000, cpu_budget=0.05, k=k, cpu_knn_sample=8)
    out, detail = bench.cpu_baseline(snaps, a, n, X, (torch.from_numpy(jr), torch.from_numpy(jc),
                                                       torch.from_numpy(jv)))
    assert out["kind"] == "port" and out["value"] > 0 and out["knn_pts_per_s"] > 0
    assert set(out["per_iteration_s_at"]) == {"1", "100", "1000"}
    for t in ("1", "100", "1000"):
        assert detail[t]["queries"] >= 2 * 16 and detail[t]["build_s"] > 0
    # the near-exact early snapshot does more reference work per query than the
    # late one (counted, not timed: at n = 2000 the timings are within noise)
    assert all(out["per_iteration_s_at"][t] > 0 for t in ("1", "100", "1000"))
    assert detail["1"]["visits_per_query"] > detail["1000"]["visits_per_query"]


def test_plain_run_leaves_the_extra_legs_to_full(monkeypatch):
    import bench
    monkeypatch.setattr("sys.argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup) == (7, 2) and not a.full
    assert a.trace == 0 and a.no_cpu_baseline and a.no_cli_e2e and a.detail_out == "" and a.dump_outputs == ""
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-dir", "d"])
    a = bench.parse()
    assert a.full and a.trace == 50 and not a.no_cpu_baseline and not a.no_cli_e2e
    assert a.detail_out.replace("\\", "/") == "d/bench_detail.json"
    monkeypatch.setattr("sys.argv", ["bench.py", "--detail-out", "x.json", "--dump-outputs", "o"])
    a = bench.parse()
    assert a.detail_out == "x.json" and a.dump_outputs == "o"


def test_dump_outputs_arrays(tmp_path):
    import bench
    rng = np.random.default_rng(1)
    n = 1000
    Y, upd, gains = rng.normal(size=(n, 2)), rng.normal(size=(n, 2)), rng.uniform(size=(n, 2))
    losses = {20: 3.5, 10: 4.0}
    bench.dump_outputs(str(tmp_path / "all"), Y, torch.from_numpy(upd), torch.from_numpy(gains), losses)
    got = {p.stem: np.load(p) for p in (tmp_path / "all").iterdir()}
    assert set(got) == {"Y", "update", "gains", "loss_iterations", "losses"}
    assert all(v.dtype == np.float64 for v in got.values())
    assert np.array_equal(got["Y"], Y) and np.array_equal(got["update"], upd) and np.array_equal(got["gains"], gains)
    assert got["loss_iterations"].tolist() == [10.0, 20.0] and got["losses"].tolist() == [4.0, 3.5]
    # over the byte budget: the same seeded rows of all three, identical from call to call
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), Y, upd, gains, losses, budget=3 * 2 * 8 * 100)
    s1 = {p.stem: np.load(p) for p in (tmp_path / "s1").iterdir()}
    s2 = {p.stem: np.load(p) for p in (tmp_path / "s2").iterdir()}
    rows = s1["rows"].astype(np.int64)
    assert 0 < len(rows) <= 100 and np.all(np.diff(rows) > 0)
    assert sum(v.nbytes for v in s1.values()) <= 3 * 2 * 8 * 100 + 32
    assert np.array_equal(s1["Y"], Y[rows]) and np.array_equal(s1["gains"], gains[rows])
    assert all(np.array_equal(s1[k], s2[k]) for k in s1)
