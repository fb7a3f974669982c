"""Every cell of the 2-D attraction's launch ladders (attract.hip): row-block
shape ("attract_cfg" 0..3) x metric x loss / non-loss launch x the stream,
claimed-slice ("attract_dyn" 1) and round-robin forms of attract_tiles, and
attract_rows ("attract_tiles" 0) for every metric -- one optimizer step each
against the oracle, by the helpers and the bounds of test_gpu_opt_step.

A ladder cell wired to the wrong instantiation (another metric, another
shape's row bits, the loss form where the sums alone are wanted) computes a
different attraction, far outside check_state's bounds, or reports another
configuration.

n = 6001: two 5888-label windows (the second of 113 labels) and, on a device
of >= 94 CUs, 64-row blocks whose last holds 49 rows.  T = 50, so t = 10 (a
loss launch) and t = 11 (a non-loss launch) both run at exaggeration 4 and
share one oracle gradient per metric."""
import pytest

from test_gpu_opt_step import check_state, one_step, problem, random_state, reference, schedule, shared_gradient
from tsne_amd.api import default_params

pytestmark = pytest.mark.gpu
NAME, N, SEED = "knn6001k8", 6001, 180   # (72,244 entries; the smallest k whose P has no underflowed entry)
T_, LR = 50, 200.0
METRICS = ["sqeuclidean", "euclidean", "cosine"]
ARMS = {
    "stream": {"attract_stream": 1},
    "dyn": {"attract_stream": 0, "attract_dyn": 1},
    "static": {"attract_stream": 0, "attract_dyn": 0},
}


def step_and_check(opts, metric, t, kernel, cfg, what):
    assert schedule(t, T_)[0] == 4.0
    P = problem(NAME)
    state = random_state(N, 2, SEED)
    prm = default_params(iterations=T_, theta=0.0, learning_rate=LR, metric=metric)
    ref = reference(P, state, t, T_, metric, LR, r=shared_gradient(NAME, 2, metric, 4.0, SEED))
    got = one_step(opts, P, state, t, prm, full=True)
    assert got["kernel"] == kernel and got["cfg"] == cfg, (what, got["kernel"], got["cfg"])
    check_state(got, ref, LR, t, "%s %s" % (what, metric))


@pytest.mark.parametrize("t", [10, 11])
@pytest.mark.parametrize("arm", list(ARMS))
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("cfg", [0, 1, 2, 3])
def test_tile_ladder_cell(cfg, metric, arm, t):
    """attract_tiles / attract_tiles_stream of shape `cfg` ran (kernel 1, the
    configuration reported) and the step matches the oracle's."""
    step_and_check({"attract_cfg": cfg, **ARMS[arm]}, metric, t, 1, cfg, "cfg %d %s" % (cfg, arm))


@pytest.mark.parametrize("t", [10, 11])
@pytest.mark.parametrize("metric", METRICS)
def test_rows_ladder_cell(metric, t):
    """"attract_tiles" 0: attract_rows (kernel 0, no configuration)."""
    step_and_check({"attract_tiles": 0}, metric, t, 0, -1, "rows")
