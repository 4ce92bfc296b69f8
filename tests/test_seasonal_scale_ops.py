"""K22 seasonal scale robust model (K14's per-phase median profile with a sigma
per phase), the band decision with a sigma per point it needs, and the zoo
model ``seasonal_scale_robust`` built on them: the numpy contract against a
direct per-row loop, the traffic-shaped history whose noise grows with the
level that the model exists for, and the kernels against the contracts on
every row type and on every shape that takes another path through them."""
import math

import numpy as np
import pytest
import torch

from foremast_amd.config import BOUND_BOTH, BrainConfig
from foremast_amd.models import zoo
from foremast_amd.ops import canary as C
from foremast_amd.ops import misc as MI
from foremast_amd.ops import smoothing as SM

F32 = np.float32
ALGO = "seasonal_scale_robust"
FLOOR = 0.1


# ------------------------------------------------------------------ contract
def _middle(v):
    c = len(v)
    return F32(0.5) * v[(c - 1) // 2] + F32(0.5) * v[c // 2]


def _loop_ref(x, T, m, H, smooth, scale_smooth, floor):
    """The contract of the issue written as plain loops over one row at a time."""
    J = min(T // m, 16, 13312 // m - 2)
    k = min(smooth, m // 24)
    w = max(0, min(scale_smooth, m // 8))
    start = T - J * m
    R = x.shape[0]
    nan = F32(np.nan)
    fc, sh = np.full((R, H), nan, F32), np.full((R, H), nan, F32)
    sigma0, kappa = np.full(R, nan, F32), np.full(R, nan, F32)
    n = np.zeros(R, np.int32)
    profile, scale = np.full((R, m), nan, F32), np.full((R, m), nan, F32)
    for r in range(R):
        span = x[r, start:T]
        raw = []
        for p in range(m):
            v = sorted(F32(s) for s in span[p::m] if np.isfinite(s))
            raw.append(_middle(v) if v else nan)
        for p in range(m):
            nb = [float(raw[(p + d) % m]) for d in range(-k, k + 1) if np.isfinite(raw[(p + d) % m])]
            if nb:
                tot = 0.0
                for v in nb:
                    tot += v
                profile[r, p] = F32(tot / len(nb))
        idx = [i for i in range(J * m) if np.isfinite(span[i])]
        res = {i: np.abs(F32(span[i]) - profile[r, i % m]) for i in idx}
        n[r] = len(idx)
        for h in range(H):
            fc[r, h] = profile[r, h % m]
        if not idx:
            continue
        s = sorted(res.values())
        mad = _middle(s)
        sigma0[r] = F32(1.4826) * mad if mad > 0 else F32(1.2533) * F32(math.fsum(float(v) for v in s) / len(s))
        if sigma0[r] == 0:
            scale[r], sh[r] = 0, 0
            continue
        raw_s = []
        for p in range(m):
            v = sorted(res[i] for i in idx if i % m == p)
            raw_s.append(_middle(v) if v else nan)
        f = F32(floor) * F32(sigma0[r] / F32(1.4826))
        gp = []
        for p in range(m):
            nb = [float(raw_s[(p + d) % m]) for d in range(-w, w + 1) if np.isfinite(raw_s[(p + d) % m])]
            if nb:
                tot = 0.0
                for v in nb:
                    tot += v
                gp.append(max(F32(tot / len(nb)), f))
            else:
                gp.append(f)
        u = sorted(F32(res[i] / gp[i % m]) for i in idx)
        mid = _middle(u)
        kappa[r] = F32(1.4826) * mid if mid > 0 else F32(1.2533) * F32(math.fsum(float(v) for v in u) / len(u))
        for p in range(m):
            scale[r, p] = kappa[r] * gp[p]
        for h in range(H):
            sh[r, h] = scale[r, h % m]
    return fc, sh, n, sigma0, kappa, profile, scale


def _span_start(T, m):
    return T - MI.seasonal_cycles(T, m) * m


NKINDS = 8


def _row(kind, T, m, rng):
    """One history row of length T with period m: the row types of the K14 tests."""
    nan, inf = np.nan, np.inf
    t = np.arange(T)
    wave = np.sin(2 * np.pi * t / m)
    x = (100 + 40 * wave + rng.standard_normal(T) * 2).astype(F32)
    if kind == 0:                                             # negative values
        return (-(50 + 20 * wave) + rng.standard_normal(T)).astype(F32)
    if kind == 1:                                             # heavy ties: integer counts, mostly zero
        return rng.poisson(0.3, T).astype(F32)
    if kind == 2:                                             # NaN runs, one of them at the left end
        x[:max(1, T // 7)] = nan
        for s in rng.integers(0, T, 4):
            x[s:s + max(1, m // 3)] = nan
        return x
    if kind == 3:                                             # one phase missing in every cycle
        s0 = _span_start(T, m)
        x[s0 + (m // 2) % m::m] = nan
        return x
    if kind == 4:                                             # all missing
        return np.full(T, nan, F32)
    if kind == 5:                                             # constant: sigma 0
        return np.full(T, 42.0, F32)
    if kind == 6:                                             # +-inf samples
        x[rng.random(T) < 0.05] = inf
        x[rng.random(T) < 0.05] = -inf
        x[-1] = -inf
        return x
    return (rng.standard_normal(T) * 3 + 2 * wave).astype(F32)  # mixed sign


def _batch(R, T, m, seed, kinds=tuple(range(NKINDS))):
    rng = np.random.default_rng(seed)
    return np.stack([_row(kinds[r % len(kinds)], T, m, rng) for r in range(R)])


def _same(a, b):
    """Equal bit for bit, NaN in the same places."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    na, nb = np.isnan(a), np.isnan(b)
    return a.shape == b.shape and np.array_equal(na, nb) and np.array_equal(a.view(np.uint32)[~na],
                                                                           b.view(np.uint32)[~nb])


NAMES = ("forecast", "sigma_h", "n", "sigma0", "kappa", "profile", "scale")


@pytest.mark.parametrize("smooth,scale_smooth,H", [(5, 30, 3), (0, 0, 29)])
def test_ref_matches_direct_loop(smooth, scale_smooth, H):
    T, m = 203, 24
    x = _batch(5, T, m, 11, kinds=(2, 3, 4, 5, 1))
    x[0, 100:140] = np.nan                                    # a run longer than a cycle
    got = MI.ref_seasonal_scale_robust(x, T, m, H, smooth, scale_smooth, FLOOR)
    want = _loop_ref(x, T, m, H, smooth, scale_smooth, FLOOR)
    assert [g.dtype for g in got] == [F32, F32, np.int32, F32, F32, F32, F32]
    assert np.array_equal(got[2], want[2])
    for g, w, what in zip(got, want, NAMES):
        if what != "n":
            assert _same(g, w), what
    fc, sh, n, sigma0, kappa, profile, scale = got
    assert n[2] == 0 and all(np.isnan(v[2]).all() for v in (fc, sh, sigma0, kappa, profile, scale))   # the all-NaN row
    assert sigma0[3] == 0 and np.isnan(kappa[3]) and (scale[3] == 0).all() and (sh[3] == 0).all()       # the constant row
    assert (scale[[0, 1, 4]] > 0).all() and np.isfinite(kappa[[0, 1, 4]]).all()
    # the phase missing in every cycle has a NaN centre without smoothing, and a sigma all the same: the floor
    assert np.isnan(profile[1]).sum() == (0 if smooth else 1) and np.isfinite(scale[1]).all()
    assert _same(sh, scale[:, np.arange(H) % m])
    # the op on CPU tensors is the contract
    tt = MI.seasonal_scale_robust(torch.from_numpy(x), T, m, H, smooth, scale_smooth, FLOOR, want_profile=True)
    assert len(tt) == 7 and all(_same(a.numpy(), b) for a, b in zip(tt, got)) and tt[2].dtype == torch.int32
    assert len(MI.seasonal_scale_robust(torch.from_numpy(x), T, m, H)) == 5
    with pytest.raises(ValueError):
        MI.seasonal_scale_robust(torch.from_numpy(x), 40, m, H)   # J < 2
    with pytest.raises(ValueError):
        MI.seasonal_scale_robust(torch.from_numpy(x), T, m, H, floor=0.0)


@pytest.mark.parametrize("smooth", [5, 0])
def test_centre_is_seasonal_robust(smooth):
    T, m, H = 203, 24, 29
    x = _batch(8, T, m, 13)
    fc, _, n, sigma0, _, profile, _ = MI.ref_seasonal_scale_robust(x, T, m, H, smooth)
    rf, rs, rn, rp = MI.ref_seasonal_robust(x, T, m, H, smooth)
    assert _same(fc, rf) and _same(sigma0, rs) and np.array_equal(n, rn) and _same(profile, rp)


@pytest.mark.parametrize("m,cap", [(9, 1), (24, 3), (1440, 180)])
def test_scale_halfwidth_cap(m, cap):
    assert MI.scale_halfwidth(m, 30) == min(30, cap) and MI.scale_halfwidth(m, m) == cap
    assert MI.scale_halfwidth(m, 0) == 0 and MI.scale_halfwidth(m, -3) == 0
    assert 2 * MI.scale_halfwidth(m, 10 ** 6) + 1 <= m
    assert all(2 * MI.scale_halfwidth(q, 10 ** 6) + 1 <= q for q in range(1, 200))


def test_edge_rules():
    m, J = 24, 8
    T = m * J
    rng = np.random.default_rng(5)
    t = np.arange(T)
    periodic = (50 + 10 * np.sin(2 * np.pi * t / m)).astype(F32)           # the same cycle eight times
    # counts: busy by day, exactly zero in the eight night phases
    night = np.arange(m) < 8
    counts = rng.poisson(20, T).astype(F32)
    counts[np.tile(night, J)] = 0
    sparse = np.where(t % 7 == 0, 1 + t % 3, 0).astype(F32)                # six samples in seven are zero
    x = np.stack([periodic, np.full(T, 7.0, F32), counts, sparse])
    fc, sh, n, sigma0, kappa, profile, scale = MI.ref_seasonal_scale_robust(x, T, m, m, 0, 0, FLOOR)
    # perfectly periodic and constant rows: sigma 0 in every phase
    assert (sigma0[:2] == 0).all() and (scale[:2] == 0).all() and np.isnan(kappa[:2]).all() and (n[:2] == T).all()
    # the night phases never moved: their raw scale is 0 and they get the floor, a share of the pooled MAD
    f = F32(FLOOR) * (sigma0[2] / F32(1.4826))
    assert sigma0[2] > 0 and f > 0 and kappa[2] > 0
    assert (scale[2, night] == kappa[2] * f).all() and (scale[2, ~night] > scale[2, 0]).all()
    # with the default smoothing the nights next to the day are lifted, none falls below the floor
    sm = MI.ref_seasonal_scale_robust(x, T, m, m, 0)
    assert sm[3][2] == sigma0[2]
    assert (sm[6][2] >= sm[4][2] * f).all() and sm[6][2, 3] == sm[4][2] * f and sm[6][2, 7] > sm[4][2] * f
    # more than half of the residuals are zero: MAD 0, the middle of u 0, both sigmas from the mean
    r = np.abs(x[3] - np.tile(profile[3], J))
    assert (profile[3] == 0).all() and np.median(r) == 0
    raw_s = np.array([_middle(np.sort(r[p::m])) for p in range(m)], F32)
    gp = np.maximum(raw_s, F32(FLOOR) * (sigma0[3] / F32(1.4826)))
    u = (r / np.tile(gp, J)).astype(F32)
    assert np.median(u) == 0
    assert sigma0[3] == F32(1.2533) * F32(r.astype(np.float64).sum() / T)
    assert kappa[3] == F32(1.2533) * F32(u.astype(np.float64).sum() / T) and kappa[3] > 0
    assert _same(scale[3], kappa[3] * gp)


# ---------------------------------------------------------------------- zoo
M_D, J_D, R_D = 1440, 7, 64
PEAK, TROUGH = slice(300, 420), slice(1020, 1140)


def _traffic():
    """64 rows, 7 days of history plus one clean day of 100 + 80 sin(2 pi t /
    1440) with Gaussian noise of 5 % of the level; three 70-sample incidents
    at x 3 in each row's history, and 2 % of its samples NaN."""
    rng = np.random.default_rng(22)
    t = np.arange((J_D + 1) * M_D)
    level = 100 + 80 * np.sin(2 * np.pi * t / M_D)
    x = (level[None, :] * (1 + 0.05 * rng.standard_normal((R_D, t.size)))).astype(F32)
    hist, cur = x[:, :J_D * M_D].copy(), x[:, J_D * M_D:].copy()
    for r in range(R_D):
        for s in rng.integers(0, J_D * M_D - 70, 3):
            hist[r, s:s + 70] *= 3
    hist[rng.random(hist.shape) < 0.02] = np.nan
    return hist, cur, level[:M_D]


@pytest.fixture(scope="module")
def traffic():
    return _traffic()


def _decide(algo, device, hist, cur, cfg=None, period=None):
    if cfg is None:
        cfg = BrainConfig()
        cfg.threshold, cfg.bound = 3.0, BOUND_BOTH
    R, n = cur.shape
    tables = zoo.make_tables(["requests"] * R, cfg, device)
    hor = torch.arange(1, n + 1, dtype=torch.int64, device=device)[None, :].expand(R, -1).contiguous()
    dec = zoo.decide(algo, torch.from_numpy(hist).to(device), hist.shape[1], torch.from_numpy(cur).to(device), hor, R,
                     tables, period=period or cfg.seasonal_period_for(60.0), smooth=cfg.seasonal_smooth,
                     scale_smooth=cfg.seasonal_scale_smooth, scale_floor=cfg.seasonal_scale_floor)
    return dec, C.unpack_flags(dec.flags, n)


def test_noise_that_grows_with_the_level(traffic):
    """Threshold 3, both bounds, 64 rows scored against a clean day and against
    the same day with a 30 % drop over the trough (phases 1,020-1,139; the peak
    is phases 300-419).  Measured here: seasonal_robust flags 20.72 % of the
    clean peak points and 0.00 % of the drop's; seasonal_scale_robust 0.25 %
    and 100.00 %, with 0.51 % of the clean trough points flagged; its sigma
    runs from 0.83 to 13.39 (seasonal_robust's: 3.83 everywhere), within 4.5 %
    (median) and 18.9 % (95th percentile) of the true one, with kappa 1.42."""
    hist, cur, level = traffic
    assert BOUND_BOTH == 3
    _, f14 = _decide("seasonal_robust", "cpu", hist, cur)
    dec, f22 = _decide(ALGO, "cpu", hist, cur)
    print("clean peak: K14 %.4f, K22 %.4f; clean trough: K14 %.4f, K22 %.4f" % (
        f14[:, PEAK].mean(), f22[:, PEAK].mean(), f14[:, TROUGH].mean(), f22[:, TROUGH].mean()))
    assert f14[:, PEAK].mean() > 0.10 and f22[:, PEAK].mean() < 0.02
    assert f22[:, TROUGH].mean() < 0.02
    bad = cur.copy()
    bad[:, TROUGH] *= F32(0.7)
    _, b14 = _decide("seasonal_robust", "cpu", hist, bad)
    _, b22 = _decide(ALGO, "cpu", hist, bad)
    print("drop: K14 %.4f, K22 %.4f" % (b14[:, TROUGH].mean(), b22[:, TROUGH].mean()))
    assert b14[:, TROUGH].mean() < 0.05 and b22[:, TROUGH].mean() > 0.95
    # the band is the contract's: centre +/- 3 sigma of the point's own phase
    fc, sh, n, sigma0, kappa, _, scale = MI.ref_seasonal_scale_robust(hist, hist.shape[1], M_D, M_D)
    np.testing.assert_allclose(dec.upper.numpy(), fc + F32(3) * sh, rtol=1e-6)
    np.testing.assert_allclose(dec.lower.numpy(), np.maximum(fc - F32(3) * sh, 0), rtol=1e-6, atol=1e-4)
    err = np.abs(scale / (0.05 * level)[None, :] - 1)
    print("sigma: %.2f .. %.2f, flat %.2f; relative error median %.4f, p95 %.4f; kappa %.3f" % (
        scale.min(), scale.max(), np.median(sigma0), np.median(err), np.percentile(err, 95), np.median(kappa)))
    assert np.median(err) < 0.1 and np.percentile(err, 95) < 0.3
    assert 1.2 < np.median(kappa) < 1.7                      # the median of 7 half-normal values -> sigma


def test_aliases_forecast_and_config(traffic):
    for a in (ALGO, "seasonal_hetero_robust", "robust_seasonal_scale", "seasonal_mad_profile", " Seasonal_Scale_Robust "):
        assert zoo.canonical(a) == ALGO
    assert ALGO in zoo.ALGORITHMS and ALGO in zoo.FORECASTERS
    hist = np.ascontiguousarray(traffic[0][:4])
    T, H = hist.shape[1], 25
    fc, sh = zoo.forecast("seasonal_mad_profile", torch.from_numpy(hist), T, H, period=96, scale_smooth=4,
                          scale_floor=0.2)
    ref = MI.ref_seasonal_scale_robust(hist, T, 96, H, 5, 4, 0.2)
    assert sh.shape == (4, H) and _same(fc.numpy(), ref[0]) and _same(sh.numpy(), ref[1])
    assert not _same(sh.numpy(), MI.ref_seasonal_scale_robust(hist, T, 96, H)[1])
    cfg = BrainConfig.from_env({"SEASONAL_PERIOD": "96", "SEASONAL_SMOOTH": "2", "SEASONAL_SCALE_SMOOTH": "12",
                                "SEASONAL_SCALE_FLOOR": "0.25", "metric_type_threshold_count": "1",
                                "metric_type0": "latency", "threshold0": "4", "ml_algorithm0": "seasonal_hetero_robust",
                                "HPA_FORECAST_ALGORITHM": "robust_seasonal_scale"})
    assert (cfg.seasonal_scale_smooth, cfg.seasonal_scale_floor, cfg.seasonal_smooth) == (12, 0.25, 2)
    assert zoo.canonical(cfg.algorithm_for("latency")) == ALGO and cfg.algorithm_for("cpu") == "moving_average_all"
    assert zoo.canonical(cfg.hpa_forecast_algorithm) == ALGO
    d = BrainConfig()
    assert (d.seasonal_scale_smooth, d.seasonal_scale_floor) == (30, 0.1)
    assert BrainConfig.from_env({"SEASONAL_SCALE_FLOOR": "0"}).seasonal_scale_floor == 1e-3
    assert BrainConfig.from_env({"SEASONAL_SCALE_FLOOR": "-2"}).seasonal_scale_floor == 1e-3


def test_brain_passes_the_settings():
    from foremast_amd.engine.brain import Brain
    from foremast_amd.service.store import MemoryStore
    cfg = BrainConfig.from_env({"SEASONAL_PERIOD": "96", "SEASONAL_SCALE_SMOOTH": "12", "SEASONAL_SCALE_FLOOR": "0.25"})
    b = Brain(MemoryStore(), cfg, device="cpu")
    assert b._seasonal_scale_args("seasonal_mad_profile") == {"period": 96, "smooth": 5, "scale_smooth": 12,
                                                              "scale_floor": 0.25}
    assert b._seasonal_scale_args("seasonal_robust") == {} and b._seasonal_args(ALGO) == {}
    assert b._model_args(ALGO) == b._seasonal_scale_args(ALGO)


def test_short_history_falls_back_to_the_flat_robust_band(traffic):
    hist, cur, _ = traffic
    short = np.ascontiguousarray(hist[:, :2000])              # fewer than two periods
    a, fa = _decide(ALGO, "cpu", short, cur[:, :10])
    b, fb = _decide("robust_moving_average_all", "cpu", short, cur[:, :10])
    assert np.array_equal(fa, fb) and torch.equal(a.upper, b.upper) and torch.equal(a.lower, b.lower)
    assert a.valid.tolist() == b.valid.tolist() and a.count.tolist() == b.count.tolist()
    fc, sigma = zoo.forecast(ALGO, torch.from_numpy(short), 2000, 7, period=M_D)
    c, s, _ = MI.ref_robust_stats(short, 2000)
    assert sigma.dim() == 1 and _same(fc.numpy(), np.broadcast_to(c[:, None], (R_D, 7))) and _same(sigma.numpy(), s)
    # a period beyond the kernel's budget (m > 3328) falls back too
    fc, sigma = zoo.forecast(ALGO, torch.from_numpy(hist[:4, :7000].copy()), 7000, 2, period=3400)
    c, s, _ = MI.ref_robust_stats(hist[:4, :7000], 7000)
    assert _same(fc.numpy()[:, 0], c) and _same(sigma.numpy(), s)


def test_history_gate_uses_the_span_count(traffic):
    hist, cur, _ = traffic
    hist, cur = hist[:4, -868:].copy(), cur[:4, :96].copy()
    assert MI.seasonal_cycles(868, 128) == 6                  # the span is the last 768 columns
    hist[1, :-5] = np.nan                                     # 5 finite samples < MIN_HISTORICAL_DATA_POINT_TO_MEASURE
    hist[2, 100:] = np.nan                                    # 100 finite samples, none of them in the span
    hist[3, :100] = np.nan
    cur[:, 3] += 1000
    dec, flags = _decide(ALGO, "cpu", hist, cur, period=128)
    assert dec.valid.tolist() == [3, 2, 2, 3]
    assert flags[0, 3] and flags[3, 3] and not flags[1:3].any() and dec.count[1:3].tolist() == [0, 0]


# ------------------------------------------------------------ band decision
BAND_MARGIN = 1e-3
BAND_N = (1, 63, 64, 65, 130)


def _band_case(n, with_diff, R=23, M=4, const=False):
    """Points at multiples of a quarter of their own sigma from the centre
    (thresholds 2.1 / 1.3 / 2.9 / 1.7 and 0.8 of them: no band within 0.04
    sigma of a point), every bound code, lower bands clamped for metrics 0 and
    2, sigma entries 0, NaN and inf, NaN / inf points and NaN centres."""
    rng = np.random.default_rng(300 + n)
    ctr = rng.normal(0, 0.2, (R, n)).astype(F32)
    sig = (rng.uniform(0.3, 1.0, (R, 1)) * np.ones((1, n))).astype(F32) if const else \
        rng.uniform(0.3, 1.0, (R, n)).astype(F32)
    k = rng.integers(-24, 25, (R, n))
    if const:
        sig[2], sig[5], sig[6] = 0.0, np.nan, np.inf
    else:
        sig[rng.random((R, n)) < 0.08] = 0.0
        sig[rng.random((R, n)) < 0.08] = np.nan
        sig[rng.random((R, n)) < 0.08] = np.inf
        sig[2, 0], sig[5, n - 1], sig[6, n // 2] = 0.0, np.nan, np.inf
    k[(sig == 0) & (k == 0)] = 3                      # sigma = 0: every point off its centre
    step = np.where(np.isfinite(sig) & (sig > 0), sig, 1.0).astype(np.float64)
    cur = (ctr.astype(np.float64) + k * 0.25 * step).astype(F32)
    thr = np.array([2.1, 1.3, 2.9, 1.7], F32)
    bound = np.array([3, 1, 2, 0], np.int32)
    mlb = np.array([-0.37, -10.0, 0.113, -10.0], F32)
    diff = None
    if with_diff:
        diff = np.zeros(R, np.int8)
        diff[[1, 4, 6, 11]] = 1
    near = np.abs(cur - mlb[np.arange(R) % M][:, None]) < 0.01
    cur[near] += F32(0.02)                            # no point within 0.01 of a clamped lower band either
    hole = rng.random((R, n)) < 0.1
    cur[hole & (rng.random((R, n)) < 0.5)] = np.nan
    cur[hole & ~np.isnan(cur) & (rng.random((R, n)) < 0.5)] = np.inf
    ctr[rng.random((R, n)) < 0.05] = np.nan
    return cur, ctr, sig, M, thr, bound, mlb, diff, 0.8


def _np(v):
    return v.cpu().numpy()


def _band_margin(cur, ref):
    """No judged point within BAND_MARGIN of a band: a flag does not hang on the last bit."""
    for band in ref[:2]:
        ok = np.isfinite(cur) & np.isfinite(band)
        assert (np.abs(cur[ok] - band[ok]) > BAND_MARGIN).all()
    assert cur.size < 64 or (np.isfinite(cur) & np.isfinite(ref[0]) & np.isfinite(ref[1])).any()


def _t(v, dev="cpu"):
    return None if v is None else torch.from_numpy(v).to(dev)


@pytest.mark.parametrize("n", BAND_N)
@pytest.mark.parametrize("with_diff", [False, True])
def test_ref_band_decide_pp_with_constant_columns_is_ref_band_decide(n, with_diff):
    cur, ctr, sig, M, thr, bound, mlb, diff, pf = _band_case(n, with_diff, const=True)
    a = SM.ref_band_decide_pp(cur, ctr, sig, M, thr, bound, mlb, diff, pf)
    b = SM.ref_band_decide(cur, ctr, np.ascontiguousarray(sig[:, 0]), M, thr, bound, mlb, diff, pf)
    for x, y in zip(a, b):
        assert x.dtype == y.dtype and np.array_equal(x.numpy(), y.numpy(), equal_nan=x.dtype.is_floating_point)
    flag = C.unpack_flags(a[2], n)
    assert flag.any() and not flag[5].any() and not flag[np.arange(23) % 4 == 3].any()    # NaN sigma, bound 0
    # the op on CPU tensors is the reference, and a sigma per row is refused
    c = SM.band_decide_pp(_t(cur), _t(ctr), _t(sig), M, _t(thr), _t(bound), _t(mlb), _t(diff), pf)
    assert all(torch.equal(x, y) or x.dtype.is_floating_point for x, y in zip(a, c))
    with pytest.raises(ValueError):
        SM.band_decide_pp(_t(cur), _t(ctr), _t(sig[:, 0].copy()), M, _t(thr), _t(bound), _t(mlb), _t(diff), pf)


@pytest.mark.parametrize("n", BAND_N)
@pytest.mark.parametrize("with_diff", [False, True])
def test_band_cases_keep_their_margin_and_cover_the_entries(n, with_diff):
    cur, ctr, sig, M, thr, bound, mlb, diff, pf = _band_case(n, with_diff)
    ref = tuple(_np(v) for v in SM.ref_band_decide_pp(cur, ctr, sig, M, thr, bound, mlb, diff, pf))
    _band_margin(cur, ref)
    assert (sig == 0).any() and np.isnan(sig).any() and np.isinf(sig).any()
    flag = C.unpack_flags(torch.from_numpy(ref[2]), n)
    assert not flag[np.isnan(sig)].any() and not flag[np.arange(23) % 4 == 3].any()
    if n >= 63:
        assert flag.any() and (ref[1] == mlb[np.arange(23) % 4][:, None]).any() and (ref[4] == F32(1e30)).any()


def test_ref_band_decide_pp_scores_in_units_of_the_points_own_sigma():
    cur = np.array([[10.0, 10.0, 10.0, 2.0, np.nan, 10.0]], F32)
    ctr = np.full((1, 6), 5.0, F32)
    sig = np.array([[1.0, 2.0, np.nan, 0.5, 1.0, 0.0]], F32)
    one = lambda v, dt: np.array([v], dt)   # noqa: E731
    up, lo, flags, cnt, score = SM.ref_band_decide_pp(cur, ctr, sig, 1, one(2.0, F32), one(3, np.int32), one(0.0, F32),
                                                      None, 0.8)
    assert up.numpy()[0, :2].tolist() == [7.0, 9.0] and lo.numpy()[0, [0, 1, 3]].tolist() == [3.0, 1.0, 4.0]
    assert C.unpack_flags(flags, 6)[0].tolist() == [True, True, False, True, False, True] and int(cnt[0]) == 4
    assert float(score[0]) == F32(1e30)                       # the sigma = 0 point
    sig[0, 5] = 10.0
    score = SM.ref_band_decide_pp(cur, ctr, sig, 1, one(2.0, F32), one(3, np.int32), one(0.0, F32), None, 0.8)[4]
    assert float(score[0]) == 4.0                             # (4 - 2) / 0.5 beats (10 - 7) / 1 and (10 - 9) / 2


# ---------------------------------------------------------------------- GPU
SHAPES = [(2, 9, 37), (24, 203, 37), (96, 96 * 7 + 50, 37), (100, 2000, 37), (50, 100, 37), (1440, 10080, 8),
          (3328, 6656, 37)]


def _mid_rows(v, ok, cnt):
    s = np.sort(np.where(ok, v, F32(np.inf)), axis=1)
    lo = np.take_along_axis(s, ((np.maximum(cnt, 1) - 1) // 2)[:, None], 1)[:, 0]
    up = np.take_along_axis(s, (np.maximum(cnt, 1) // 2)[:, None], 1)[:, 0]
    return F32(0.5) * lo + F32(0.5) * up


def _scale_from_profile(span, profile, sigma0, J, m, w, floor):
    """(raw scale, floored scale g', kappa, whether kappa is a middle) of each
    row in numpy from a given profile and sigma0: steps 2-6 of the contract."""
    R = span.shape[0]
    fin = np.isfinite(span)
    n = fin.sum(1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = np.abs(span - np.tile(profile, (1, J))).astype(F32)
        fin3 = fin.reshape(R, J, m)
        c = fin3.sum(1)
        s = np.sort(np.where(fin3, r.reshape(R, J, m), F32(np.inf)), axis=1)
        lo = np.take_along_axis(s, ((np.maximum(c, 1) - 1) // 2)[:, None, :], 1)[:, 0]
        up = np.take_along_axis(s, (np.maximum(c, 1) // 2)[:, None, :], 1)[:, 0]
        raw = np.where(c > 0, F32(0.5) * lo + F32(0.5) * up, F32(np.nan)).astype(F32)
        tot, cnt = np.zeros((R, m), np.float64), np.zeros((R, m), np.int64)
        for d in range(-w, w + 1):
            nb = np.roll(raw, -d, axis=1)
            ok = np.isfinite(nb)
            tot += np.where(ok, nb, 0).astype(np.float64)
            cnt += ok
        g = np.where(cnt > 0, tot / np.maximum(cnt, 1), np.nan).astype(F32)
        f = (F32(floor) * (sigma0 / F32(1.4826)).astype(F32)).astype(F32)
        gp = np.where(np.isfinite(g), np.maximum(g, f[:, None]), f[:, None]).astype(F32)
        u = (r / np.tile(gp, (1, J))).astype(F32)
        mid = _mid_rows(u, fin, n)
        mean = (np.where(fin, u, 0).astype(np.float64).sum(1) / np.maximum(n, 1)).astype(F32)
        kappa = np.where(mid > 0, F32(1.4826) * mid, F32(1.2533) * mean).astype(F32)
    return raw, gp, kappa, mid > 0


def _check(got, k14, x, T, m, H, smooth, scale_smooth, what):
    fc, sh, n, sigma0, kappa, profile, scale = (t.cpu().numpy() for t in got)
    J = MI.seasonal_cycles(T, m)
    w = MI.scale_halfwidth(m, scale_smooth)
    span = x[:, T - J * m:T]
    rn = np.isfinite(span).sum(1)
    assert np.array_equal(n, rn), what
    # the centre is K14's on the same device tensor, bit for bit
    for a, b, name in zip((fc, sigma0, n, profile), k14, ("forecast", "sigma0", "n", "profile")):
        assert _same(a, b.cpu().numpy()), (what, name)
    live = (rn > 0) & (sigma0 != 0)
    assert np.isnan(kappa[~live]).all() and np.isnan(scale[rn == 0]).all(), what
    assert (scale[(rn > 0) & (sigma0 == 0)] == 0).all(), what
    assert _same(sh, scale[:, np.arange(H) % m]), what        # sigma_h is the kernel's own scale, wrapped
    raw, gp, kap, mid = _scale_from_profile(span, profile, sigma0, J, m, w, FLOOR)
    assert live.any() and np.isfinite(kappa[live]).all() and (kappa[live] > 0).all(), what
    assert _same(kappa[live & mid], kap[live & mid]), (what, "kappa from the exact selection")
    np.testing.assert_allclose(kappa[live], kap[live], rtol=1e-6, atol=0, err_msg=str(what))
    # g' from the kernel's kappa: exact without smoothing (scale is one fp32 product); with it an fp64 sum
    # of at most 2 w + 1 fp32 values rounded once, one fp32 ulp of the row's largest raw scale, then the product
    with np.errstate(invalid="ignore"):
        want = (kappa[:, None] * gp).astype(F32)
        if w == 0:
            assert _same(scale[live], want[live]), what
        else:
            top = np.nanmax(np.where(np.isnan(raw), 0, raw), axis=1)
            err = np.abs(scale.astype(np.float64) - kappa[:, None].astype(np.float64) * gp.astype(np.float64))
            lim = kappa.astype(np.float64)[:, None] * 2.0 ** -23 * top[:, None] + 2.0 ** -24 * np.abs(want)
            assert np.all(err[live] <= lim[live]), (what, (err[live] / lim[live]).max())
        np.testing.assert_allclose(sh[live], (kap[:, None] * gp)[:, np.arange(H) % m][live], rtol=1e-6, atol=0,
                                   err_msg=str(what))


@pytest.mark.gpu
@pytest.mark.parametrize("m,T,R", SHAPES)
def test_gpu_seasonal_scale_robust_matches_oracle(cuda, m, T, R):
    """Kernel == contract at (smooth, scale_smooth, H) = (5, 30, 3), (0, 0, m +
    5) and (5, m, m + 5), the last with the window at its cap: n exact;
    forecast, sigma0 and profile those of K14 on the same tensor bit for bit;
    kappa and the scale, recomputed from the kernel's own profile, bit for bit
    where kappa is a middle and the scale is not smoothed, else within the
    rounding of their sums.  Rows cycle through: negative values, integer
    counts that are mostly zero, NaN runs, a phase missing in every cycle,
    all-NaN, constant, +-inf samples, mixed sign.  Each batch also runs on
    views that start at columns 0-3 of an odd-stride buffer."""
    x = _batch(R, T, m, 2000 + T + m)
    d = torch.from_numpy(x).to(cuda)
    first = None
    for smooth, ss, H in ((5, 30, 3), (0, 0, m + 5), (5, m, m + 5)):
        k14 = MI.seasonal_robust(d, T, m, H, smooth, want_profile=True)
        got = MI.seasonal_scale_robust(d, T, m, H, smooth, ss, FLOOR, want_profile=True)
        _check(got, k14, x, T, m, H, smooth, ss, ("dense", smooth, ss, H))
        first = first or got
    out5 = MI.seasonal_scale_robust(d, T, m, 3)               # without the profile and scale outputs
    assert len(out5) == 5 and all(_same(a.cpu().numpy(), b.cpu().numpy()) for a, b in zip(out5, first))
    ld = T + 5 + T % 2                                        # odd
    for off in range(4):
        buf = np.full((R, ld), 1e9, F32)
        buf[:, off:off + T] = x
        view = torch.from_numpy(buf).to(cuda)[:, off:]
        assert view.stride(0) % 2 == 1 and view.data_ptr() % 16 == 4 * off
        H = 3 if off % 2 else m + 5
        k14 = MI.seasonal_robust(view, T, m, H, 5, want_profile=True)
        got = MI.seasonal_scale_robust(view, T, m, H, 5, 30, FLOOR, want_profile=True)
        _check(got, k14, x, T, m, H, 5, 30, ("view", off))


BAD = [(100, 150, 1, 0, FLOOR), (100, 2000, 17, 0, FLOOR), (3329, 6658, 2, 0, FLOOR), (100, 250, 3, 0, FLOOR),
       (100, 2000, 16, 0, 0.0), (100, 2000, 16, 0, -1.0), (100, 2000, 16, 0, float("nan")), (100, 2000, 16, -1, FLOOR),
       (100, 2000, 16, 50, FLOOR)]


@pytest.mark.gpu
@pytest.mark.parametrize("m,T,J,w,floor", BAD)
def test_gpu_seasonal_scale_robust_entry_rejects_bad_arguments(cuda, m, T, J, w, floor):
    """K14's bad shapes (J = 1, J = 17, (J + 2) m > 13312, J m > T), a floor
    that is not > 0, w < 0 and a window longer than the period: an error from
    the entry point, and no launch (the outputs keep their fill)."""
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    R, H = 3, 4
    hist = torch.zeros((R, T), device=cuda)
    outs = [torch.full(s, 7.0, device=cuda) for s in ((R, H), (R, H), (R, 3), (R, m), (R, m))]
    fc, sh, stats, prof, scale = outs
    with pytest.raises(RuntimeError):
        LIB.call("fm_seasonal_scale_robust", ptr(hist), hist.stride(0), T, R, m, J, 0, w, floor, H, ptr(fc), ptr(sh), H,
                 ptr(stats), ptr(prof), ptr(scale), stream_of(hist))
    torch.cuda.synchronize()
    assert all((o == 7).all() for o in outs)


@pytest.mark.gpu
@pytest.mark.parametrize("n", BAND_N)
@pytest.mark.parametrize("with_diff", [False, True])
def test_gpu_band_decide_pp(cuda, n, with_diff):
    """Kernel == reference: a partial last workgroup (R = 23), one to three
    flag words, every bound code, clamped lower bands, the pairwise factor,
    sigma entries 0 / NaN / inf, NaN and inf points, NaN centres, and sigma as
    a column view of a wider buffer.  The score divides a distance of at
    least 1e-3 from a band that is right to 1e-6: rtol 1e-3, as for
    band_decide.  With constant columns it is band_decide, bit for bit."""
    cur, ctr, sig, M, thr, bound, mlb, diff, pf = _band_case(n, with_diff)
    ref = tuple(_np(v) for v in SM.ref_band_decide_pp(cur, ctr, sig, M, thr, bound, mlb, diff, pf))
    _band_margin(cur, ref)
    wide = np.full((23, n + 3), 5.0, F32)
    wide[:, 2:2 + n] = sig
    for s in (_t(sig, cuda), _t(wide, cuda)[:, 2:2 + n]):
        g = tuple(_np(v) for v in SM.band_decide_pp(_t(cur, cuda), _t(ctr, cuda), s, M, _t(thr, cuda), _t(bound, cuda),
                                                    _t(mlb, cuda), _t(diff, cuda), pf))
        np.testing.assert_allclose(g[0], ref[0], rtol=1e-6)
        np.testing.assert_allclose(g[1], ref[1], rtol=1e-6)
        np.testing.assert_array_equal(g[2], ref[2])
        np.testing.assert_array_equal(g[3], ref[3])
        np.testing.assert_allclose(g[4], ref[4], rtol=1e-3)
    cur, ctr, sig, M, thr, bound, mlb, diff, pf = _band_case(n, with_diff, const=True)
    args = (M, _t(thr, cuda), _t(bound, cuda), _t(mlb, cuda), _t(diff, cuda), pf)
    a = SM.band_decide_pp(_t(cur, cuda), _t(ctr, cuda), _t(sig, cuda), *args)
    b = SM.band_decide(_t(cur, cuda), _t(ctr, cuda), _t(np.ascontiguousarray(sig[:, 0]), cuda), *args)
    for x, y, name in zip(a, b, ("upper", "lower", "flags", "count", "score")):
        assert np.array_equal(_np(x), _np(y), equal_nan=x.dtype.is_floating_point), name
    assert _np(a[3])[5] == 0 and (_np(a[3])[2] == 0 or _np(a[4])[2] == F32(1e30))     # NaN sigma; sigma 0, when flagged
    assert n < 63 or _np(a[3])[2] > 0


@pytest.mark.gpu
def test_gpu_seasonal_scale_zoo_equals_cpu_zoo(cuda, traffic):
    hist, cur, _ = traffic
    hist, cur = hist[:16].copy(), cur[:16, :130].copy()
    hist[7, :-5] = np.nan                                     # too little history: no verdict
    cur[:, 40:60] *= F32(1.3)
    a, fa = _decide(ALGO, "cpu", hist, cur)
    b, fb = _decide(ALGO, cuda, hist, cur)
    assert fa[:7, 40:60].mean() > 0.9 and not fa[7].any() and np.array_equal(fa, fb)
    for k in ("upper", "lower"):
        np.testing.assert_allclose(getattr(b, k).cpu().numpy(), getattr(a, k).numpy(), rtol=1e-6, err_msg=k)
    assert b.count.cpu().tolist() == a.count.tolist() and b.valid.cpu().tolist() == a.valid.tolist()
    short = np.ascontiguousarray(hist[:, :2000])              # the fallback runs K13 and the one-sigma band decision
    a, fa = _decide(ALGO, "cpu", short, cur[:, :10])
    b, fb = _decide(ALGO, cuda, short, cur[:, :10])
    assert np.array_equal(fa, fb)
    np.testing.assert_allclose(b.upper.cpu().numpy(), a.upper.numpy(), rtol=1e-6)
