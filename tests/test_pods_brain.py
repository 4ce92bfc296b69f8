"""The per-pod test (docs/BRAIN_SPEC.md 4.3) off the GPU: the numpy definition
against scipy, the setting through ``Brain.score_rows`` on the CPU, and the
refusals."""
import numpy as np
import pytest
import scipy.stats
import torch

from foremast_amd.config import BrainConfig
from foremast_amd.engine.brain import Brain, Row
from foremast_amd.engine.scorer import CanaryScorer
from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref
from foremast_amd.service.store import MemoryStore

ON = {"ML_PAIRWISE_POD_TEST": "KRUSKAL_DUNN"}
P, W = 8, 10


def _row(seed=1, shift=15.0):
    """8 pods x 10 of N(100, 5), pod 3 shifted by 3 sigma; as many baseline points."""
    rng = np.random.default_rng(seed)
    cur = rng.normal(100, 5, P * W).astype(np.float32)
    cur[3 * W:4 * W] += shift
    return rng.normal(100, 5, 600).astype(np.float32), cur, rng.normal(100, 5, P * W).astype(np.float32)


@pytest.mark.parametrize("tied", [False, True])
def test_definition_matches_scipy_kruskal(tied):
    _, cur, base = _row()
    if tied:
        cur, base = np.round(cur / 4), np.round(base / 4)
    pods, pod_z, pod_n, *_ = ref.pairwise_pods(cur[None], np.arange(W, P * W + 1, W)[None], base[None], 5)
    want = scipy.stats.kruskal(base, *cur.reshape(P, W))
    np.testing.assert_allclose(pods[0, :2], [want.statistic, want.pvalue], rtol=1e-6)
    assert pods[0, 4] == 3 and pods[0, 5] == P and (pod_n == W).all() and int(np.argmax(np.abs(pod_z))) == 3


def _score(env, monkeypatch=None):
    hist, cur, base = _row()
    brain = Brain(MemoryStore(), BrainConfig.from_env({"ML_ALGORITHM": "moving_average_all", **env}), device="cpu",
                  resident_history=False)
    if monkeypatch is not None:
        monkeypatch.setattr(C, "pairwise_pods", lambda *a, **k: pytest.fail("the pod test ran with the setting off"))
    row = Row(0, "error4xx", "m", hist, 0.0, cur, np.zeros(0), base, cur_pods=np.full(P, W, np.int64))
    return brain.score_rows([row])


def test_brain_flags_the_bad_pod_only_with_the_setting(monkeypatch):
    on, off = _score(ON), _score({}, monkeypatch)
    assert off["diff"].tolist() == [0] and on["diff"].tolist() == [1]
    # off: the pod test is never called (the monkeypatch) and the verdict is the pooled tests' alone;
    # the OFF spelling is the default
    _, cur, base = _row()
    _, _, d = C.pairwise_tests(torch.from_numpy(cur[None]), torch.from_numpy(base[None]), C.PairwiseConfig())
    assert off["diff"].tolist() == d.tolist()
    for k in ("upper", "lower", "count", "score", "valid"):
        np.testing.assert_array_equal(off[k], _score({"ML_PAIRWISE_POD_TEST": "OFF"})[k])


def test_unknown_setting_stops_the_brain_and_the_scorer_refuses():
    with pytest.raises(ValueError, match="pod test"):
        Brain(MemoryStore(), BrainConfig.from_env({"ML_PAIRWISE_POD_TEST": "ANOVA"}), device="cpu")
    with pytest.raises(ValueError, match="min_points"):
        Brain(MemoryStore(), BrainConfig.from_env({**ON, "MIN_POD_DATA_POINTS": "0"}), device="cpu")
    # the scorer's rows carry no pod boundaries: it refuses a tick with a baseline and ticks without one as ever
    hist, cur, base = (torch.from_numpy(a[None]) for a in _row())
    on, off = (CanaryScorer(["error4xx"], BrainConfig.from_env(e), device="cpu") for e in (ON, {}))
    with pytest.raises(ValueError, match="ML_PAIRWISE_POD_TEST"):
        on.score(hist, base, cur, 600)
    with pytest.raises(ValueError, match="ML_PAIRWISE_POD_TEST"):
        CanaryScorer(["error4xx"], BrainConfig.from_env(ON), device="cpu", mode="fused")
    assert torch.equal(on.score(hist, None, cur, 600).packed, off.score(hist, None, cur, 600).packed)
