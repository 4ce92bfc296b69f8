"""The tail test's numpy definition (docs/BRAIN_SPEC.md 4.6) against scipy and a
plain loop, its level rules, its symmetry, and its wiring on the CPU."""
import numpy as np
import pytest
import scipy.stats
import torch

from foremast_amd.config import BrainConfig
from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref

Q = (9000, 9500, 9900)


def _rows(seed=3, nc=128, nb=512):
    rng = np.random.default_rng(seed)
    cur, base = rng.lognormal(4, 0.3, (3, nc)), rng.lognormal(4, 0.3, (3, nb))
    cur[1] = np.where(cur[1] > np.quantile(cur[1], 0.8), cur[1] * 1.2, cur[1])
    cur[2, ::9], base[2, 1::7] = np.nan, np.inf
    return cur.astype(np.float32), base.astype(np.float32)


def test_definition_against_scipy_and_a_plain_loop():
    cur, base = _rows()
    tail, which, J, n, counts = ref.pairwise_tail(cur, base, Q, "BOTH", None, 20, 5)
    for r in range(3):
        c, b = (x[np.isfinite(x)] for x in (cur[r], base[r]))
        N, pooled = len(c) + len(b), sorted(np.concatenate([c, b]).tolist())
        assert n[r].tolist() == [len(c), len(b)] and J[r] == 6
        ps = []
        for s in (0, 1):
            for l, q in enumerate(Q):
                k = min(N - 1, (q * N + 9999) // 10000)
                t = pooled[k - 1] if s == 0 else pooled[N - k]
                a = sum(1 for v in c if (v > t if s == 0 else v < t))
                bb = sum(1 for v in b if (v > t if s == 0 else v < t))
                assert counts[r, s, l].tolist() == [a, bb, k]
                ps.append(scipy.stats.hypergeom.sf(a - 1, N, a + bb, len(c)))
                np.testing.assert_allclose(ref.hypergeom_upper_tail(a, a + bb, len(c), len(b)), ps[-1], rtol=1e-9)
        best = int(np.argmin(ps))
        a, bb, _ = counts[r].reshape(6, 3)[best]
        assert which[r] == best
        np.testing.assert_allclose(tail[r, :3], [min(1, 6 * ps[best]), ps[best], a / len(c) - bb / len(b)], rtol=1e-6)
    assert ref.tail_verdict(tail, 0.05).tolist() == [0, 1, 0] and which[1] < 3


def test_duplicate_levels_and_min_tail_points_on_a_zero_inflated_row():
    rng = np.random.default_rng(5)
    cur, base = np.zeros((1, 100), np.float32), np.zeros((1, 300), np.float32)
    cur[0, :12], base[0, :8] = rng.lognormal(4, 0.3, 12), rng.lognormal(4, 0.3, 8)
    cur[0, 50:], base[0, 100:] = -0.0, -0.0
    # 380 zeros of both signs tie: ranks 360 and 380 fall into their run (m = 20 twice, one test), rank 396 leaves
    # m = 4 < MIN_TAIL_POINTS: J = 1, and p is p_min
    tail, which, J, _, counts = ref.pairwise_tail(cur, base, Q, "UPPER", None, 20, 5)
    assert counts[0, 0].tolist() == [[12, 8, 360], [12, 8, 380], [counts[0, 0, 2, 0], 4 - counts[0, 0, 2, 0], 396]]
    assert J[0] == 1 and which[0] == 0 and tail[0, 0] == tail[0, 1] and tail[0, 3] == 0 and not counts[0, 1].any()
    assert ref.pairwise_tail(cur, base, Q, "UPPER", None, 20, 4)[2][0] == 2


def test_lower_side_is_the_upper_side_of_the_negated_row():
    cur, base = _rows(7, 90, 150)
    lo = ref.pairwise_tail(cur, base, Q, "LOWER", None, 20, 5)
    up = ref.pairwise_tail(-cur, -base, Q, "UPPER", None, 20, 5)
    np.testing.assert_array_equal(lo[4][:, 1], up[4][:, 0])
    np.testing.assert_array_equal(lo[0][:, :3], up[0][:, :3])
    np.testing.assert_array_equal(lo[0][:, 3], -up[0][:, 3])
    np.testing.assert_array_equal(lo[1], up[1] + 3)
    # BOUND reads the row's code: 1 upper, 2 lower, anything else both
    by = ref.pairwise_tail(cur, base, Q, "BOUND", np.array([1, 2, 0]), 20, 5)
    up0 = ref.pairwise_tail(cur, base, Q, "UPPER", None, 20, 5)
    assert not by[4][0, 1].any() and not by[4][1, 0].any() and by[4][2, :, :, 2].all()
    assert by[2].tolist() == [up0[2][0], lo[2][1], up0[2][2] + lo[2][2]]


def test_tail_diff_only_sets_and_off_is_the_identity():
    cur, base = (torch.from_numpy(a[:2]) for a in _rows())
    on, bound = C.TailTest("EXCEEDANCE"), torch.tensor([1], dtype=torch.int32)
    assert C.pairwise_tail(cur, base, on, bound, 1).tail_diff.tolist() == [0, 1]
    for diff in ([0, 0], [1, 0], [1, 1]):
        d = torch.tensor(diff, dtype=torch.int8)
        assert C.tail_diff(d, cur, base, on, bound, 1).tolist() == [diff[0], 1]
        assert C.tail_diff(d, cur, base, C.TailTest("OFF"), bound, 1) is d
    # a floor on the excess above the row's, or the wrong side, keeps the verdict off
    for test in (C.TailTest("EXCEEDANCE", min_excess=0.5), C.TailTest("EXCEEDANCE", sides="LOWER")):
        assert C.pairwise_tail(cur, base, test, bound, 1).tail_diff.tolist() == [0, 0]
    out = torch.ops.foremast.pairwise_tail(cur, base, bound, "0.9,0.95,0.99", "BOUND", 0.05, 20, 5, 0.0)
    assert out[3].tolist() == [0, 1] and out[2].shape == (2, 2, 3, 3)


def test_settings():
    c = BrainConfig.from_env({"ML_PAIRWISE_TAIL_TEST": "exceedance", "ML_PAIRWISE_TAIL_QUANTILES": "0.75, 0.9999",
                              "ML_PAIRWISE_TAIL_SIDES": "both", "MIN_TAIL_DATA_POINTS": "30", "MIN_TAIL_POINTS": "3",
                              "ML_PAIRWISE_TAIL_MIN_EXCESS": "0.05", "ML_PAIRWISE_THRESHOLD": "0.01"})
    t = C.TailTest.from_config(c)
    assert t == C.TailTest("EXCEEDANCE", 0.01, (0.75, 0.9999), "BOTH", 30, 3, 0.05) and t.q_i == (7500, 9999)
    d = C.TailTest.from_config(BrainConfig())
    assert not d.enabled and not C.TailTest("off").enabled and d.q_i == Q and d.sides == "BOUND"
    on = dict(test="EXCEEDANCE")
    for bad in (dict(test="HILL"), dict(on, sides="INNER"), dict(on, quantiles="0.9,0.9"), dict(on, quantiles="0.95,0.9"),
                dict(on, quantiles="0.4"), dict(on, quantiles="0.99999"), dict(on, quantiles="0.5,0.6,0.7,0.8,0.9"),
                dict(on, quantiles=""), dict(on, quantiles="p99"), dict(on, min_points=1), dict(on, min_tail_points=0),
                dict(on, min_excess=1.0), dict(on, min_excess=-0.1)):
        with pytest.raises(ValueError):
            C.TailTest(**bad)
