"""K34 rolling robust bands: the vectorised definition vs a per-window loop over
ref_robust_stats and the rolling_bands rules (CPU), and the gfx950 sliding
window kernel vs the definition (GPU)."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from foremast_amd.ops import misc as MI

C = MI.ROLLING_ROBUST_CHUNK


def _batch(T, w, seed=0):
    """One row of every kind the sorted window has to survive, [17, T] fp32."""
    rng = np.random.default_rng(seed + 1000 * w + T)
    g = lambda: rng.normal(0, 1, T)
    ties = np.round(g(), 1)
    ties[ties == 0] = rng.choice([0.0, -0.0], int((ties == 0).sum()))
    rows = [g(), ties, np.full(T, 3.25), np.where(rng.random(T) < 0.9, 0.0, g()),
            np.arange(T) * 0.5, -np.arange(T) * 0.5, np.full(T, np.nan), g() + 1e6,
            np.where(rng.random(T) < 0.5, -0.0, 0.0)]
    for run in (w - 1, w, w + 5):                   # missing runs shorter than, equal to and longer than w
        r = g()
        at = min(w // 2 + 3, max(T - run - 2, 0))
        r[at:at + run] = np.nan
        rows.append(r)
    r = g()
    r[rng.random(T) < 0.1] = np.inf
    r[rng.random(T) < 0.1] = -np.inf
    rows.append(r)
    r = g()
    r[min(w // 3 + 1, T - 1)] = 1e30                  # one huge outlier enters and leaves
    rows.append(r)
    r = g()
    r[rng.random(T) < 0.3] = np.nan
    rows += [r, np.round(g()), np.abs(g()) * 1e-3 - 5.0]
    return np.array(rows, np.float32)


def _bits(a):
    """fp32 bit patterns, a zero's sign aside: numpy's sort leaves the order of
    -0.0 and 0.0, and with it the sign of a zero median, open."""
    return (np.asarray(a, np.float32) + np.float32(0)).view(np.int32).astype(np.int64)


def _check(got, x, w, mc=1):
    """center, n: equal as bits; sigma: as bits where the definition's MAD > 0 (fewer than
    half the window equal the centre), within 1 fp32 ulp in the fallback."""
    c, s, n = got
    rc, rs, rn = MI.ref_rolling_robust_stats(x, w, mc)
    assert np.array_equal(n, rn)
    assert np.array_equal(np.isnan(c), np.isnan(rc)) and np.array_equal(np.isnan(s), np.isnan(rs))
    ok = ~np.isnan(rc)
    assert np.array_equal(_bits(c[ok]), _bits(rc[ok])), np.argwhere(ok & (c != rc))[:5]
    pad = np.concatenate([np.full((x.shape[0], w - 1), np.nan, np.float32), x], axis=1)
    at_centre = (np.lib.stride_tricks.sliding_window_view(pad, w, axis=1) == rc[..., None]).sum(-1)
    exact = ok & (at_centre <= rn // 2)
    ulps = np.abs(_bits(s[ok]) - _bits(rs[ok]))
    assert ulps[exact[ok]].max(initial=0) == 0 and ulps.max(initial=0) <= 1, np.argwhere(ok & (s != rs))[:5]


@pytest.mark.parametrize("w", [1, 2, 5, 64])
def test_reference_is_robust_stats_per_window(w):
    x = _batch(200, w)
    c, s, n = MI.ref_rolling_robust_stats(x, w, 2)
    for r in range(x.shape[0]):
        for t in range(x.shape[1]):
            seg = x[r:r + 1, max(0, t - w + 1): t + 1]
            lc, ls, ln = MI.ref_robust_stats(seg, seg.shape[1])
            assert n[r, t] == ln[0]
            want = (lc[0], ls[0]) if ln[0] >= 2 else (np.float32(np.nan),) * 2
            assert np.array_equal(_bits([c[r, t], s[r, t]]), _bits(want)), (r, t)


def test_rolling_bands_robust_rules_and_default():
    from foremast_amd.config import BrainConfig
    from foremast_amd.models import zoo
    cfg = BrainConfig()
    aliases = ["error5xx", "latency"]
    tables = zoo.make_tables(aliases, cfg, "cpu")
    x = torch.from_numpy(_batch(300, 30)[:4] + np.float32(5))
    for model in ("robust", "robust_moving_average"):
        center, up, lo = zoo.rolling_bands(x, 300, 2, tables, window=30, min_count=5, model=model)
        m, s, _ = MI.ref_rolling_robust_stats(x.numpy(), 30, 5)
        assert np.array_equal(center.numpy(), m, equal_nan=True)
        for r in range(4):
            rule = cfg.rule_for(aliases[r % 2])
            want_up = m[r] + np.float32(rule.threshold) * s[r] if rule.bound & 1 else np.full(300, np.nan)
            want_lo = (np.maximum(m[r] - np.float32(rule.threshold) * s[r], np.float32(rule.min_lower_bound))
                       if rule.bound & 2 else np.full(300, np.nan))
            np.testing.assert_allclose(up[r].numpy(), want_up, rtol=1e-6, equal_nan=True)
            np.testing.assert_allclose(lo[r].numpy(), want_lo, rtol=1e-6, equal_nan=True)
    # the default is the mean / std band it has always been (tests/test_rolling.py holds its rules)
    got = zoo.rolling_bands(x, 300, 2, tables, window=30, min_count=5)
    named = zoo.rolling_bands(x, 300, 2, tables, window=30, min_count=5, model="moving_average")
    assert torch.equal(got[0].view(torch.int32), MI.rolling_stats(x, 300, 30, 5)[0].view(torch.int32))
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(got, named))
    with pytest.raises(ValueError):
        zoo.rolling_bands(x, 300, 2, tables, model="median")


def test_robust_band_stays_narrow_behind_a_spike():
    w, at = 60, 400
    x = np.random.default_rng(3).normal(10, 1, (1, 600)).astype(np.float32)
    x[0, at:at + 10] += 50
    t = at + 10 + w // 2
    _, rs, _ = MI.ref_rolling_robust_stats(x, w)
    _, sd = MI.ref_rolling_stats(x, w)
    robust, plain = rs[0, t] / rs[0, at - 1], sd[0, t] / sd[0, at - 1]
    assert plain > 4 * robust, (robust, plain)


def _gpu(x, cuda, w, mc=1, T=None):
    got = MI.rolling_robust_stats(x, x.shape[1] if T is None else T, w, mc)
    torch.cuda.synchronize()
    return [t.cpu().numpy() for t in got]


@pytest.mark.gpu
@pytest.mark.parametrize("w,T", [(w, T) for w in (1, 2, 3, 63, 64, 65, 128, 1023, 1024)
                                 for T in sorted({1, w - 1, w, w + 1, C - 1, C, C + 1, 2 * C + 7} - {0})])
def test_gpu_matches_definition(cuda, w, T):
    x = _batch(T, w)
    _check(_gpu(torch.from_numpy(x).to(cuda), cuda, w), x, w)


@pytest.mark.gpu
@pytest.mark.parametrize("w,mc,view", [(65, 1, True), (7, 5, False), (200, 150, True)])
def test_gpu_column_view_and_min_count(cuda, w, mc, view):
    x = _batch(C + 70, w, seed=1)
    xg = torch.from_numpy(x).to(cuda)
    if view:                                         # rows 4-byte aligned only, stride T + 1
        x, xg = x[:, 1:], xg[:, 1:]
    _check(_gpu(xg, cuda, w, mc), np.ascontiguousarray(x), w, mc)


@pytest.mark.gpu
@pytest.mark.parametrize("w,T", [(0, 100), (1025, 100), (5, 0), (5, 101)])
def test_gpu_rejects_bad_arguments(cuda, w, T):
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    x = torch.zeros((3, 100), device=cuda)
    with pytest.raises(ValueError):
        MI.rolling_robust_stats(x, T, w)
    o = torch.empty((3, 3, 128), device=cuda)
    with pytest.raises(RuntimeError, match="hipError 1"):        # the entry point itself: hipErrorInvalidValue
        LIB.call("fm_rolling_robust_stats", ptr(x), 100, T, 3, w, 1, ptr(o[0]), ptr(o[1]), ptr(o[2]), 128, stream_of(x))
