"""The native CLI's --quality K / --qualitySample S / --qualityFile PATH
(tsne-flink_amd/host): the three values written after the fit equal
Context.embeddingQuality on the input rows and the map read back from the
output CSV (javaDouble round-trips, so the CSV holds the map's bits), on the
device chain, with --hostChain, with a sample and in 3-D; nothing changes
without the flag; the refused combinations.  600 points, d = 12, 30 iterations."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import tsne_amd as T

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "tsne-flink_amd" / "tsne_hip"
N, D, PERPLEXITY, ITERATIONS, THETA, K = 600, 12, 10.0, 30, 0.5, 10


def run(*args, cwd=None):
    return subprocess.run([str(CLI), *args], capture_output=True, text=True, cwd=cwd)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    rng = np.random.default_rng(11)
    X = np.abs(rng.normal(size=(4, D)))[rng.integers(0, 4, N)] * 3 + rng.random((N, D))
    d = tmp_path_factory.mktemp("quality_cli")
    (d / "in.csv").write_text("\n".join(f"{i},{j},{float(X[i, j])!r}" for i in range(N) for j in range(D)) + "\n")
    return d, X


def cli(d, *extra, nc=2, method="bruteforce"):
    for f in ("quality.txt", "q2.txt"):
        (d / f).unlink(missing_ok=True)
    r = run("--input", "in.csv", "--output", "out.csv", "--dimension", str(D), "--knnMethod", method,
            "--perplexity", str(PERPLEXITY), "--iterations", str(ITERATIONS), "--nComponents", str(nc),
            "--theta", str(THETA), "--loss", "loss.txt", *extra, cwd=d)
    assert r.returncode == 0, r.stderr
    return (d / "out.csv").read_bytes(), (d / "loss.txt").read_bytes(), r.stderr


def embedding(raw, nc):
    rows = [l.split(",") for l in raw.decode().splitlines()]
    assert [int(r[0]) for r in rows] == list(range(N)) and all(len(r) == 1 + nc for r in rows)
    return np.array([[float(v) for v in r[1:]] for r in rows])


def quality_file(path):
    lines = path.read_text().splitlines()
    assert [l.split("=")[0] for l in lines] == ["trustworthiness", "continuity", "knnRecall"]
    return tuple(float(l.split("=")[1]) for l in lines)


@pytest.mark.gpu
@pytest.mark.parametrize("flags,nc,rows,metric", [
    (["--qualitySample", "0"], 2, None, "sqeuclidean"),
    (["--qualitySample", "50"], 2, 50, "sqeuclidean"),
    (["--qualitySample", "0", "--hostChain"], 2, None, "sqeuclidean"),
    (["--qualitySample", "50", "--hostChain"], 2, 50, "sqeuclidean"),
    (["--qualitySample", "0"], 3, None, "sqeuclidean"),
    (["--qualitySample", "0", "--metric", "cosine", "--pcaDimension", "5"], 2, None, "cosine"),   # scored on the rows as read
    ([], 2, None, "sqeuclidean"),                                     # default sample 10000, clamped to n
])
def test_quality_file_equals_python(data, flags, nc, rows, metric):
    d, X = data
    out, _, err = cli(d, "--quality", str(K), *flags, nc=nc)
    assert "[tsne_hip] quality in " in err
    Y = embedding(out, nc)
    with T.Context(0) as ctx:
        q = ctx.embeddingQuality(X, Y, K, metric=metric, rows=rows)
    assert quality_file(d / "quality.txt") == (q.trustworthiness, q.continuity, q.knn_recall)
    assert all(0.0 <= v <= 1.0 for v in (q.trustworthiness, q.continuity, q.knn_recall))


@pytest.mark.gpu
def test_quality_with_projection_knn_and_file_name(data):
    d, X = data
    out, _, _ = cli(d, "--quality", str(K), "--qualitySample", "0", "--qualityFile", "q2.txt", method="project")
    with T.Context(0) as ctx:
        q = ctx.embeddingQuality(X, embedding(out, 2), K)
    assert quality_file(d / "q2.txt") == (q.trustworthiness, q.continuity, q.knn_recall)
    assert not (d / "quality.txt").exists()


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [[], ["--hostChain"]])
def test_nothing_changes_without_the_flag(data, chain):
    d, _ = data
    a = cli(d, *chain)
    assert not (d / "quality.txt").exists() and "quality" not in a[2]
    b = cli(d, *chain)
    assert a[:2] == b[:2]
    c = cli(d, "--quality", str(K), *chain)            # the fit itself is the same with the flag
    assert (d / "quality.txt").exists() and c[:2] == a[:2]


@pytest.mark.gpu
def test_refused_for_the_size_of_the_input(data):
    """2 n - 3 K - 1 <= 0 is known once the rows are read: refused before the fit."""
    d, _ = data
    (d / "quality.txt").unlink(missing_ok=True)       # an earlier test's
    r = run("--input", "in.csv", "--output", "o2.csv", "--dimension", str(D), "--knnMethod", "bruteforce",
            "--quality", "400", cwd=d)
    assert r.returncode == 2 and "java.lang.IllegalArgumentException" in r.stderr and "2 n - 3 K - 1" in r.stderr
    assert not (d / "o2.csv").exists() and not (d / "quality.txt").exists()


@pytest.mark.parametrize("flags", [
    ["--quality", "10", "--inputDistanceMatrix"],
    ["--quality", "0"],
    ["--quality", "-3"],
    ["--quality"],
    ["--quality", "10", "--qualitySample", "-1"],
])
def test_refused_combinations(flags):
    """Argument errors: IllegalArgumentException and exit status 2, before any file or device is touched."""
    r = run("--input", "x", "--output", "y", "--dimension", "12", "--knnMethod", "bruteforce", *flags)
    assert r.returncode == 2 and "java.lang.IllegalArgumentException" in r.stderr
