"""The dependence gate's numpy definition (docs/BRAIN_SPEC.md 4.7): a plain loop, its invariance, its settings
and what it does to the false-positive rate of the rank-sum test on autocorrelated windows."""
import math

import numpy as np
import pytest

from foremast_amd.config import BrainConfig
from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref


def _ar1(rng, rho, shape):
    e = rng.normal(0, 1, shape)
    for i in range(1, shape[-1]):
        e[..., i] += rho * e[..., i - 1]
    return e


def _by_loops(cur, ends, base, L, need):
    """One row straight from the definition, value by value."""
    x = [float(v) for v in cur] + [float(v) for v in base]
    fin = [math.isfinite(v) for v in x]
    n1, n2 = sum(fin[:len(cur)]), sum(fin[len(cur):])
    N = n1 + n2
    a = [sum(2 * (fin[j] and x[j] < x[i]) + (fin[j] and x[j] == x[i]) for j in range(len(x))) + 1 - (N + 1)
         if fin[i] else None for i in range(len(x))]
    T = sum(a[i] for i in range(len(cur)) if fin[i])
    A = sum(v * v for v in a if v is not None)
    segs = [[(lo, hi) for lo, hi in zip([0] + list(ends[:-1]), ends)], [(len(cur), len(x))]]
    vif, rho, pairs = [], [], []
    for s, n_side in ((0, n1), (1, n2)):
        C0, Ck, mk = 0.0, [0.0] * L, [0] * L
        for lo, hi in segs[s]:
            idx = [i for i in range(lo, hi) if fin[i]]
            if len(idx) < need:
                continue
            mean = sum(a[i] for i in idx) / len(idx)
            C0 += sum((a[i] - mean) ** 2 for i in idx)
            for k in range(1, min(L, len(idx) // 4) + 1):
                for i in idx:
                    if i + k < hi and fin[i + k]:
                        Ck[k - 1] += (a[i] - mean) * (a[i + k] - mean)
                        mk[k - 1] += 1
        r = [c / C0 if C0 > 0 else 0.0 for c in Ck]
        rho.append(r)
        pairs.append(mk)
        vif.append(min(max(1.0, 1.0 + 2.0 * sum((1.0 - k / (L + 1.0)) * r[k - 1] for k in range(1, L + 1))),
                       max(1.0, n_side / 2.0)))
    z = T / math.sqrt(n1 * n2 / (N * (N - 1.0)) * A)
    z_adj = z * math.sqrt((1.0 / n1 + 1.0 / n2) / (vif[0] / n1 + vif[1] / n2))
    return (math.erfc(abs(z_adj) / math.sqrt(2.0)), z_adj, z, vif[0], vif[1], N), rho, (n1, n2), (T, A), pairs


def test_definition_against_a_plain_loop():
    rng = np.random.default_rng(11)
    cur = np.round(_ar1(rng, 0.8, (2, 24)) * 2).astype(np.float32)      # rounded: ties, signed zeros among them
    base = np.round(_ar1(rng, 0.8, (2, 17)) * 2 + 1).astype(np.float32)
    cur[0, [3, 9]], cur[1, 14], base[1, 5] = (np.nan, np.inf), -np.inf, np.nan
    cur[1, 2] = -0.0
    ends = np.array([[10, 24], [7, 20]], np.int32)                      # (row 1: the last four columns belong to no pod)
    dep, rho, n, TA, kept, pairs = ref.pairwise_dependence(cur, ends, base, 3, 4)
    for r in range(2):
        d, rh, nn, ta, pr = _by_loops(cur[r], ends[r], base[r], 3, 4)
        np.testing.assert_allclose(dep[r], d, rtol=1e-6)
        np.testing.assert_allclose(rho[r, :, :3], rh, rtol=1e-6, atol=1e-7)
        assert tuple(n[r]) == nn and tuple(TA[r]) == ta and pairs[r, :, :3].tolist() == pr
        assert not rho[r, :, 3:].any() and not pairs[r, :, 3:].any()
    assert kept.tolist() == [[2, 1], [2, 1]]


def test_every_output_is_invariant_to_a_monotone_transform():
    rng = np.random.default_rng(12)
    cur, base = rng.integers(-20, 21, (3, 60)).astype(np.float32), rng.integers(-18, 23, (3, 45)).astype(np.float32)
    cur[0, 7], base[2, 3] = np.nan, np.nan
    ends = np.tile(np.array([20, 45, 60], np.int32), (3, 1))
    a = ref.pairwise_dependence(cur, ends, base, 8, 12)
    b = ref.pairwise_dependence(cur ** 3, ends, base ** 3, 8, 12)       # (exact in fp32, and odd: the zeros stay)
    for u, v in zip(a, b):
        np.testing.assert_array_equal(u, v)


def test_settings():
    c = BrainConfig.from_env({"ML_PAIRWISE_DEPENDENCE": "rank_acf", "ML_PAIRWISE_ACF_MAX_LAG": "5",
                              "MIN_ACF_DATA_POINTS": "9", "ML_PAIRWISE_THRESHOLD": "0.01"})
    assert C.DependenceGate.from_config(c) == C.DependenceGate("RANK_ACF", 0.01, 5, 9)
    assert C.DependenceGate.from_config(BrainConfig()) == C.DependenceGate("off", 0.05, 8, 12) and not C.DependenceGate().enabled
    for bad in (dict(gate="NEWEY_WEST"), dict(gate="RANK_ACF", max_lag=0), dict(gate="RANK_ACF", max_lag=17),
                dict(gate="RANK_ACF", min_points=3)):
        with pytest.raises(ValueError):
            C.DependenceGate(**bad)


def _rates(rho, draws=400):
    """(share of draws with raw p < 0.05, share the gate keeps) over healthy AR(1) windows, 4 pods x 30 vs 120."""
    rng = np.random.default_rng(33)
    cur, base = _ar1(rng, rho, (draws, 4, 30)).reshape(draws, 120), _ar1(rng, rho, (draws, 120))
    ends = np.tile(np.array([30, 60, 90, 120], np.int32), (draws, 1))
    dep = ref.pairwise_dependence(cur.astype(np.float32), ends, base.astype(np.float32), 8, 12)[0]
    raw = np.array([math.erfc(abs(z) / math.sqrt(2.0)) for z in dep[:, 2]]) < 0.05
    return raw.mean(), (raw & (ref.dependence_verdict(dep, 0.05) == 1)).mean()


def test_false_positive_rate_on_autocorrelated_windows():
    raw, kept = _rates(0.7)
    assert raw > 0.25 and kept <= 0.6 * raw, (raw, kept)
    raw0, kept0 = _rates(0.0)
    assert raw0 - kept0 <= raw0 / 5, (raw0, kept0)
