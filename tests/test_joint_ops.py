"""The joint multi-metric test (docs/BRAIN_SPEC.md 4.4) off the GPU: the numpy
definition's identities, ``joint_diff`` and the settings."""
import numpy as np
import pytest
import torch

from foremast_amd.config import BrainConfig
from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref

ROWS = np.asarray([[0, 1, 2, -1, -1, -1, -1, -1]], np.int32)


def _job(tied, seed=3, k=3, nc=40, nb=120):
    """k correlated members, member 0's current side half a sigma up."""
    rng = np.random.default_rng(seed)
    x = 0.7 * rng.normal(0, 1, nc + nb) + rng.normal(0, 1, (k, nc + nb))
    x[0, :nc] += 0.5
    x = np.round(x, 1) if tied else x
    return x[:, :nc].astype(np.float32), x[:, nc:].astype(np.float32)


@pytest.mark.parametrize("tied", [False, True])
def test_one_member_is_the_tie_corrected_kruskal_wallis(tied):
    cur, base = _job(tied)
    P, S, _ = ref.pairwise_tests(cur, base, 63, 0, 0.05, 5, 5, 5)
    for r in range(len(cur)):
        joint = ref.pairwise_joint(cur, base, [[r] + [-1] * 7], [1], 5)[0]
        np.testing.assert_allclose(joint[0, :2], [S[r, 2], P[r, 2]], rtol=1e-6)
        assert joint[0, 2] == 1 and joint[0, 4] == 0


@pytest.mark.parametrize("tied", [False, True])
def test_statistic_is_invariant(tied):
    cur, base = _job(tied)
    L = lambda c, b, rows=ROWS: ref.pairwise_joint(c, b, rows, [3], 5)[0][0, 0]  # noqa: E731
    want = L(cur, base)
    assert np.isfinite(want) and want > 0
    np.testing.assert_allclose(L(cur, base, [[2, 0, 1] + [-1] * 5]), want, rtol=1e-6)   # the members permuted
    c, b = cur.copy(), base.copy()
    c[1], b[1] = c[1] ** 3, b[1] ** 3                                                   # strictly increasing
    np.testing.assert_allclose(L(c, b), want, rtol=1e-6)
    # current and baseline swapped (40 + 120 columns either way round)
    np.testing.assert_allclose(L(base, cur), want, rtol=1e-6)


def test_joint_diff_sets_the_members_of_flagged_groups_and_clears_nothing():
    cur, base = _job(False, k=7)
    cur[4:, :] = base[4:, :40]                                 # rows 4..6: no difference
    cur, base = torch.from_numpy(cur), torch.from_numpy(base)
    rows = torch.tensor([[2, 0, -1, -1, -1, -1, -1, -1], [5, 4, 6, -1, -1, -1, -1, -1]], dtype=torch.int32)
    K = torch.tensor([2, 3])
    test = C.JointTest("RANK_SUM", 0.05, 20)
    assert C.pairwise_joint(cur, base, rows, K, test).joint_diff.tolist() == [1, 0]
    diff = torch.tensor([0, 0, 0, 0, 0, 1, 0], dtype=torch.int8)
    assert C.joint_diff(diff, cur, base, rows, K, test).tolist() == [1, 0, 1, 0, 0, 1, 0]
    assert C.joint_diff(diff, cur, base, rows, K, C.JointTest("OFF")) is diff


def test_settings():
    for bad in ("HOTELLING", "on"):
        with pytest.raises(ValueError, match="joint test"):
            C.JointTest(bad)
    with pytest.raises(ValueError, match="min_points"):
        C.JointTest("RANK_SUM", 0.05, 0)
    assert not C.JointTest().enabled and not C.JointTest("off").enabled and C.JointTest(" rank_sum ").enabled
    cfg = BrainConfig.from_env({})
    assert (cfg.pairwise_joint_test, cfg.min_joint_points) == ("", 20)
    cfg = BrainConfig.from_env({"ML_PAIRWISE_JOINT_TEST": "RANK_SUM", "MIN_JOINT_DATA_POINTS": "7",
                                "ML_PAIRWISE_THRESHOLD": "0.01"})
    assert C.JointTest.from_config(cfg) == C.JointTest("RANK_SUM", 0.01, 7)
