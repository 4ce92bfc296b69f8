"""The drift test's numpy definition (docs/BRAIN_SPEC.md 4.5) against scipy and a
plain loop, the property that motivates it, and its wiring on the CPU."""
import numpy as np
import pytest
import scipy.stats
import torch

from foremast_amd.config import BrainConfig
from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref


def _rows(tied):
    rng = np.random.default_rng(3)
    x = rng.normal(0, 1, (4, 40)) + np.linspace(0, 1.5, 40)
    return np.round(x) if tied else x


@pytest.mark.parametrize("tied", [False, True])
def test_definition_against_kendalltau_and_a_plain_loop(tied):
    x = _rows(tied).astype(np.float32)
    base = x[::-1].copy()
    drift, counts, pod_S, pod_n, k = ref.pairwise_drift(x, np.full((4, 1), 40), base, 10)
    for r in range(4):
        S = sum(int(np.sign(x[r, j] - x[r, i])) for j in range(40) for i in range(j))
        tau = scipy.stats.kendalltau(np.arange(40), x[r]).statistic
        assert counts[r, 0, 0] == pod_S[r, 0] == S and pod_n[r, 0] == 40 and k[r] == 1
        np.testing.assert_allclose(drift[r, 3], tau, rtol=1e-6)
        # the per-sample tie term telescopes to the classical sum over tie runs
        t = np.unique(x[r], return_counts=True)[1].astype(np.int64)
        assert counts[r, 0, 3] == 40 * 39 * 85 - int((t * (t - 1) * (2 * t + 5)).sum())
        assert counts[r, 0, 2] == int((t * (t - 1)).sum()) and counts[r, 0, 1] == 780
        # the baseline is the row mirrored: z = (z_c - z_b) / sqrt 2 by hand
        zc, zb = (float((c[0] - np.sign(c[0])) / np.sqrt(c[3] / 18.0)) for c in counts[r])
        np.testing.assert_allclose(drift[r, [0, 2, 4]], [(zc - zb) / np.sqrt(2.0), zc, zb], rtol=1e-6)


def test_shuffling_within_pods_moves_only_the_drift_test():
    rng = np.random.default_rng(5)
    cur = (rng.normal(100, 2, (1, 60)) + np.tile(np.linspace(0, 6, 20), 3)).astype(np.float32)
    base = rng.normal(103, 2.5, (1, 60)).astype(np.float32)
    seg = np.array([[20, 40, 60]], np.int32)
    # the paired tests (Wilcoxon, Friedman) pair column i with column i, so the baseline's columns move along
    perm = np.concatenate([a + rng.permutation(20) for a in (0, 20, 40)])
    mixed, mixed_base = cur[:, perm], base[:, perm]
    a, b = ref.pairwise_drift(cur, seg, base, 10), ref.pairwise_drift(mixed, seg, mixed_base, 10)
    assert ref.drift_verdict(a[0], 0.05)[0] == 1 and ref.drift_verdict(b[0], 0.05)[0] == 0
    assert a[1][0, 0, 0] > 3 * abs(b[1][0, 0, 0]) and (a[3] == b[3]).all()
    pa, pb = (ref.pairwise_tests(c, d, 63, 0, 0.05, 10, 10, 10)[0] for c, d in ((cur, base), (mixed, mixed_base)))
    np.testing.assert_array_equal(pa, pb)


def test_drift_diff_only_sets_and_off_is_the_identity():
    rng = np.random.default_rng(7)
    cur = torch.from_numpy((rng.normal(0, 1, (2, 30)) + np.stack([np.arange(30) * 0.3, np.zeros(30)])).astype(np.float32))
    base = torch.from_numpy(rng.normal(0, 1, (2, 30)).astype(np.float32))
    seg = torch.full((2, 1), 30, dtype=torch.int32)
    on = C.DriftTest("MANN_KENDALL")
    assert C.pairwise_drift(cur, seg, base, on).drift_diff.tolist() == [1, 0]
    for diff in ([0, 0], [0, 1], [1, 1]):
        d = torch.tensor(diff, dtype=torch.int8)
        assert C.drift_diff(d, cur, seg, base, on).tolist() == [1, diff[1]]
        assert C.drift_diff(d, cur, seg, base, C.DriftTest("OFF")) is d
    # a floor on |tau| above the row's keeps the verdict off
    assert C.pairwise_drift(cur, seg, base, C.DriftTest("MANN_KENDALL", min_tau=0.99)).drift_diff.tolist() == [0, 0]


def test_settings():
    c = BrainConfig.from_env({"ML_PAIRWISE_DRIFT_TEST": "mann_kendall", "MIN_DRIFT_DATA_POINTS": "12",
                              "ML_PAIRWISE_DRIFT_MIN_TAU": "0.2", "ML_PAIRWISE_THRESHOLD": "0.01"})
    assert C.DriftTest.from_config(c) == C.DriftTest("MANN_KENDALL", 0.01, 12, 0.2)
    assert not C.DriftTest.from_config(BrainConfig()).enabled and not C.DriftTest("off").enabled
    for bad in (dict(test="THEIL_SEN"), dict(test="MANN_KENDALL", min_points=2), dict(test="MANN_KENDALL", min_tau=1.5),
                dict(test="MANN_KENDALL", min_tau=-0.1)):
        with pytest.raises(ValueError):
            C.DriftTest(**bad)
