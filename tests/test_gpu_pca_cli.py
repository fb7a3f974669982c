"""The native CLI's --init pca and --pcaDimension (tsne-flink_amd/host): the
device chain against --hostChain text for text, both against the Python
chain of the same operators, the refused combinations, and the defaults
unchanged.  400 points, d = 12, 30 iterations."""
import subprocess
from pathlib import Path

import numpy as np
import pytest

import tsne_amd as T
from tsne_amd.api import default_params

ROOT = Path(__file__).resolve().parent.parent
CLI = ROOT / "tsne-flink_amd" / "tsne_hip"
N, D, PERPLEXITY, ITERATIONS, THETA = 400, 12, 10.0, 30, 0.5


def run(*args, cwd=None):
    return subprocess.run([str(CLI), *args], capture_output=True, text=True, cwd=cwd)


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    rng = np.random.default_rng(7)
    X = np.abs(rng.normal(size=(4, D)))[rng.integers(0, 4, N)] * 3 + rng.random((N, D))
    d = tmp_path_factory.mktemp("pca_cli")
    (d / "in.csv").write_text("\n".join(f"{i},{j},{float(X[i, j])!r}" for i in range(N) for j in range(D)) + "\n")
    return d, X


def cli(d, *extra, nc=2):
    r = run("--input", "in.csv", "--output", "out.csv", "--dimension", str(D), "--knnMethod", "bruteforce",
            "--perplexity", str(PERPLEXITY), "--iterations", str(ITERATIONS), "--nComponents", str(nc),
            "--theta", str(THETA), "--loss", "loss.txt", *extra, cwd=d)
    assert r.returncode == 0, r.stderr
    return (d / "out.csv").read_text(), (d / "loss.txt").read_text()


def embedding(text, nc):
    rows = [l.split(",") for l in text.splitlines()]
    assert [int(r[0]) for r in rows] == list(range(N)) and all(len(r) == 1 + nc for r in rows)
    return np.array([[float(v) for v in r[1:]] for r in rows])


def python_chain(X, nc, init_pca, p):
    """kNearestNeighbors -> pairwiseAffinities -> jointDistribution -> the working set -> optimize."""
    with T.Context(0) as ctx:
        k = 3 * int(PERPLEXITY)                       # the CLI's default --neighbors
        if p:
            scores, _, eig, _ = ctx.pca(X, max(p, nc if init_pca else 0))
            idx, dist = ctx.kNearestNeighbors(np.ascontiguousarray(scores[:, :p]), k)
        else:
            idx, dist = ctx.kNearestNeighbors(X, k)
        rp = np.arange(0, N * k + 1, k, dtype=np.int64)
        cond = ctx.pairwiseAffinities(rp, dist.ravel(), PERPLEXITY)
        jr, jc, jv = ctx.jointDistribution(rp, idx.ravel(), cond, N)
        Y, upd, gains = ctx.initWorkingSetPCA(X, nc) if init_pca else ctx.initWorkingSet(N, nc, seed=0)
        ctx.optimize(jr, jc, jv, Y, upd, gains, default_params(iterations=ITERATIONS, theta=THETA, n_components=nc))
        return Y


@pytest.mark.gpu
@pytest.mark.parametrize("flags,nc,init_pca,p", [
    (["--init", "pca"], 2, True, 0),
    (["--pcaDimension", "5"], 2, False, 5),
    (["--init", "pca", "--pcaDimension", "5"], 2, True, 5),      # one PCA call serves both uses
    (["--init", "pca", "--pcaDimension", "2"], 3, True, 2),      # fewer kNN columns than components
])
def test_device_chain_equals_host_chain_and_python(data, flags, nc, init_pca, p):
    d, X = data
    dev = cli(d, *flags, nc=nc)
    host = cli(d, *flags, "--hostChain", nc=nc)
    assert dev == host
    Y = embedding(dev[0], nc)
    assert np.isfinite(Y).all() and "10=" in dev[1] and "30=" in dev[1]
    Yp = python_chain(X, nc, init_pca, p)
    assert np.abs(Y - Yp).max() <= 1e-9 * np.abs(Yp).max()


@pytest.mark.gpu
def test_init_pca_with_projection_knn(data):
    """--init pca is valid with every --knnMethod: project takes the host chain."""
    d, _ = data
    r = run("--input", "in.csv", "--output", "out.csv", "--dimension", str(D), "--knnMethod", "project",
            "--perplexity", str(PERPLEXITY), "--iterations", "10", "--init", "pca", "--loss", "loss.txt", cwd=d)
    assert r.returncode == 0, r.stderr
    assert np.isfinite(embedding((d / "out.csv").read_text(), 2)).all()


@pytest.mark.gpu
def test_defaults_unchanged(data):
    """Neither flag = --init random given explicitly (and --pcaDimension 0): the same files."""
    d, _ = data
    plain = cli(d)
    assert plain == cli(d, "--init", "random")
    assert plain == cli(d, "--init", "random", "--pcaDimension", "0")
    assert plain != cli(d, "--init", "pca")


@pytest.mark.parametrize("flags", [
    ["--pcaDimension", "5", "--knnMethod", "project"],
    ["--init", "pca", "--knnMethod", "bruteforce", "--inputDistanceMatrix"],
    ["--pcaDimension", "5", "--knnMethod", "bruteforce", "--inputDistanceMatrix"],
    ["--pcaDimension", "13", "--knnMethod", "bruteforce"],
    ["--pcaDimension", "65", "--knnMethod", "bruteforce", "--dimension", "100"],
    ["--init", "spectral", "--knnMethod", "bruteforce"],
])
def test_refused_combinations(flags):
    """Argument errors: the IllegalArgumentException message and exit status of
    the CLI's other argument errors, before any file or device is touched."""
    r = run("--input", "x", "--output", "y", "--dimension", "12", *flags)
    assert r.returncode == 2 and "java.lang.IllegalArgumentException" in r.stderr
