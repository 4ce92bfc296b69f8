"""K20 seasonal trend robust model (repeated-median line over the cycle
medians, per-phase median profile and MAD of the residuals about it) and the
zoo model ``seasonal_trend_robust`` built on it: the numpy contract against a
direct per-row loop and against the two contracts it composes, the drifting
seasonal history with earlier incidents the model exists for, and the kernel
against the contract on every row type and on every shape that takes another
path through it."""
import functools

import numpy as np
import pytest
import torch

from foremast_amd.config import BOUND_BOTH, BrainConfig
from foremast_amd.engine.brain import Brain
from foremast_amd.engine.sources import SourceRouter
from foremast_amd.models import zoo
from foremast_amd.ops import canary as C
from foremast_amd.ops import misc as MI
from foremast_amd.service.store import MemoryStore

from test_seasonal_ops import _loop_ref as _seasonal_loop
from test_seasonal_ops import _middle, _same, _sigma_from_profile

F32 = np.float32
ALGO = "seasonal_trend_robust"


# ------------------------------------------------------------------ contract
def _loop_ref(x, T, m, H, smooth, mb):
    """The contract of the model written as plain loops over one row at a time."""
    J = min(T // m, 16, 13312 // m - 2)
    N = J * m
    R = x.shape[0]
    fc = np.full((R, H), np.nan, F32)
    sigma = np.full(R, np.nan, F32)
    n = np.zeros(R, np.int32)
    slope = np.zeros(R, F32)
    nblocks = np.zeros(R, np.int32)
    profile = np.full((R, m), np.nan, F32)
    with np.errstate(invalid="ignore", over="ignore"):
        for r in range(R):
            span = x[r, T - N:T]
            b, q = [], []
            for j in range(J):
                v = sorted(F32(s) for s in span[j * m:(j + 1) * m] if np.isfinite(s))
                if len(v) >= max(1, m // 4):
                    b.append(_middle(v))
                    q.append(j)
            B = len(b)
            nblocks[r] = B
            sl = F32(0)
            if B >= mb:
                si = []
                for i in range(B):
                    si.append(_middle(sorted(F32(b[j] - b[i]) / F32((q[j] - q[i]) * m) for j in range(B) if j != i)))
                s = _middle(sorted(si))
                if np.isfinite(s):
                    sl = F32(s)
            slope[r] = sl
            res = np.array([F32(F32(span[i]) - F32(sl * F32(i - (N - 1)))) for i in range(N)], F32)
            f0, sg, nn, pr = _seasonal_loop(res[None, :], N, m, H, smooth)
            sigma[r], n[r], profile[r] = sg[0], nn[0], pr[0]
            for h in range(H):
                fc[r, h] = F32(pr[0, h % m] + F32(sl * F32(h + 1)))
    return fc, sigma, n, slope, nblocks, profile


def _span_start(T, m):
    return T - MI.seasonal_cycles(T, m) * m


NKINDS = 10


def _row(kind, T, m, rng):
    """One history row of length T with period m (the list in
    ``test_gpu_seasonal_trend_robust_matches_oracle``)."""
    nan, inf = np.nan, np.inf
    t = np.arange(T)
    wave = np.sin(2 * np.pi * t / m)
    x = (100 + 100 * t / T + 40 * wave + rng.standard_normal(T) * 2).astype(F32)
    s0, J = _span_start(T, m), MI.seasonal_cycles(T, m)
    if kind == 0:                                             # a ramp plus a cycle
        return x
    if kind == 1:                                             # negative values, falling
        return (-(50 + 30 * t / T + 20 * wave) + rng.standard_normal(T)).astype(F32)
    if kind == 2:                                             # heavy ties: integer counts, mostly zero
        return rng.poisson(0.3, T).astype(F32)
    if kind == 3:                                             # NaN runs, one of them at the left end
        x[:max(1, T // 7)] = nan
        for s in rng.integers(0, T, 4):
            x[s:s + max(1, m // 3)] = nan
        return x
    if kind == 4:                                             # one phase missing in every cycle
        x[s0 + (m // 2) % m::m] = nan
        return x
    if kind == 5:                                             # a whole cycle missing: gapped block indices
        j = J // 2
        x[s0 + j * m:s0 + (j + 1) * m] = nan
        return x
    if kind == 6:                                             # all missing
        return np.full(T, nan, F32)
    if kind == 7:                                             # constant: slope 0, sigma 0
        return np.full(T, 42.0, F32)
    if kind == 8:                                             # +-inf samples
        x[rng.random(T) < 0.05] = inf
        x[rng.random(T) < 0.05] = -inf
        x[-1] = -inf
        return x
    # +-3e38: a line from one end of the range to the other, so pair slopes and residuals overflow
    cyc = np.clip((t - s0) // m, 0, max(J - 1, 1))
    return (F32(3e38) * (2 * cyc / max(J - 1, 1) - 1) * (0.9 + 0.1 * rng.random(T))).astype(F32)


def _batch(R, T, m, seed, kinds=tuple(range(NKINDS))):
    rng = np.random.default_rng(seed)
    return np.stack([_row(kinds[r % len(kinds)], T, m, rng) for r in range(R)])


@pytest.mark.parametrize("T,m,smooth,H,mb", [(203, 24, 5, 3, 3), (203, 24, 0, 29, 2), (99, 6, 5, 4, 3), (52, 8, 5, 9, 3)])
def test_ref_matches_direct_loop(T, m, smooth, H, mb):
    x = _batch(13, T, m, 11 + T, kinds=(0, 2, 3, 4, 5, 6, 7, 8, 9, 1, 9, 3, 3))
    x[10] = np.where(np.arange(T) % 2 == 0, F32(3e38), F32(-3e38))    # +-3e38 alternating
    x[11, :T // 2 + 3] = np.nan                               # a half-empty row
    x[12, np.random.default_rng(5).random(T) < 0.3] = np.nan  # 30 % NaN
    got = MI.ref_seasonal_trend_robust(x, T, m, H, smooth, mb)
    want = _loop_ref(x, T, m, H, smooth, mb)
    assert [g.dtype for g in got] == [F32, F32, np.int32, F32, np.int32, F32]
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[4], want[4])
    assert got[2][5] == 0 and got[4][5] == 0 and got[3][5] == 0                       # the all-NaN row
    assert np.isnan(got[1][5]) and np.isnan(got[5][5]).all() and np.isnan(got[0][5]).all()
    assert got[1][6] == 0 and got[3][6] == 0 and (got[5][6] == 42).all()              # the constant row
    J = MI.seasonal_cycles(T, m)
    assert got[4][0] == J and got[4][4] == J - 1                                      # a missing cycle is no block
    if J >= 3:
        assert got[2][8] < got[4][8] * m                      # the +-3e38 line: some residuals overflowed
    for g, w, what in zip(got, want, ("forecast", "sigma", "n", "slope", "nblocks", "profile")):
        if what not in ("n", "nblocks"):
            assert _same(g, w), what
    # the op on CPU tensors is the contract
    tf, ts_, tn, tsl, tp = MI.seasonal_trend_robust(torch.from_numpy(x), T, m, H, smooth, mb, want_profile=True)
    assert _same(tf.numpy(), got[0]) and _same(ts_.numpy(), got[1]) and tn.tolist() == got[2].tolist()
    assert _same(tsl.numpy(), got[3]) and _same(tp.numpy(), got[5]) and tn.dtype == torch.int32
    assert len(MI.seasonal_trend_robust(torch.from_numpy(x), T, m, H, smooth, mb)) == 4
    with pytest.raises(ValueError):
        MI.seasonal_trend_robust(torch.from_numpy(x), m + m // 2, m, H)   # J < 2
    with pytest.raises(ValueError):
        MI.seasonal_trend_robust(torch.from_numpy(x), T, m, H, min_blocks=1)


@pytest.mark.parametrize("T,m,mb", [(30, 12, 3), (203, 24, 9), (99, 6, 17)])
def test_rows_without_a_slope_equal_the_seasonal_model(T, m, mb):
    """J = 2 under min_blocks 3, and min_blocks above J: slope 0, and forecast,
    sigma and n are ref_seasonal_robust's of the span, as floats (x - (-0)
    turns -0.0 into +0.0)."""
    x = _batch(10, T, m, 21 + T)
    H = m + 3
    fc, sigma, n, slope, nb, profile = MI.ref_seasonal_trend_robust(x, T, m, H, 5, mb)
    assert (slope == 0).all() and (nb < mb).all()
    rf, rs, rn, rp = MI.ref_seasonal_robust(x, T, m, H, 5)
    np.testing.assert_array_equal(fc, rf)
    np.testing.assert_array_equal(sigma, rs)
    np.testing.assert_array_equal(profile, rp)
    assert np.array_equal(n, rn)
    # a constant and an all-NaN row have slope 0 under any min_blocks
    fc, sigma, n, slope, nb, _ = MI.ref_seasonal_trend_robust(x[6:8], T, m, H, 5, 2)
    assert (slope == 0).all()
    np.testing.assert_array_equal(fc, rf[6:8])
    np.testing.assert_array_equal(sigma, rs[6:8])
    assert np.array_equal(n, rn[6:8])


@pytest.mark.parametrize("m,J,lead", [(16, 4, 3), (8, 16, 0), (32, 3, 5)])
def test_exactly_representable_ramp(m, J, lead):
    """Multiples of 1/8 on a period that is a power of two: the exact slope,
    sigma 0, and a forecast that continues the series."""
    T = J * m + lead
    rng = np.random.default_rng(m)
    cyc = rng.integers(-40, 40, m) / 8.0

    def series(i):
        return (i / 8.0 + cyc[(i - lead) % m] + 7).astype(F32)
    x = np.stack([series(np.arange(T)), (-series(np.arange(T))).astype(F32)])
    H = m + 3
    fc, sigma, n, slope, nb, profile = MI.ref_seasonal_trend_robust(x, T, m, H, 0, 3)
    assert slope.tolist() == [0.125, -0.125] and nb.tolist() == [J, J] and n.tolist() == [J * m] * 2
    assert sigma.tolist() == [0, 0]
    nxt = series(np.arange(T, T + H))
    assert np.array_equal(fc[0], nxt) and np.array_equal(fc[1], -nxt)
    assert np.array_equal(profile[0], series(np.arange(T - m, T)) + F32(0.125) * (m - 1 - np.arange(m, dtype=F32)))


# ------------------------------------------------------------------ quality
M_Q, J_Q, R_Q = 96, 7, 64
SLOPE_Q = 100.0 / (J_Q * M_Q)
THR_Q = 5.0


@functools.lru_cache(maxsize=None)
def _quality(seed=7):
    """64 rows, 7 cycles of history plus one healthy cycle of 100 + 100 t /
    (7 m) + 40 sin + N(0, 2) at period 96; two +60 incidents of m // 16
    samples in every history, and one whole cycle raised by 300 on rows 0-15.
    The arrays are shared: copy before writing."""
    rng = np.random.default_rng(seed)
    t = np.arange((J_Q + 1) * M_Q)
    truth = 100 + SLOPE_Q * t + 40 * np.sin(2 * np.pi * t / M_Q)
    x = (truth[None, :] + rng.normal(0, 2, (R_Q, t.size))).astype(F32)
    w = M_Q // 16
    for s in (2 * M_Q + M_Q // 3, 5 * M_Q + M_Q // 2):
        x[:, s:s + w] += 60
    x[:16, 3 * M_Q:4 * M_Q] += 300
    hist, cur = x[:, :J_Q * M_Q].copy(), x[:, J_Q * M_Q:].copy()
    hist.setflags(write=False)
    cur.setflags(write=False)
    return hist, cur


def _cfg():
    cfg = BrainConfig()
    cfg.threshold, cfg.bound, cfg.seasonal_period = THR_Q, BOUND_BOTH, M_Q
    return cfg


def _decide(algo, device, hist, cur, cfg=None, **kw):
    cfg = cfg or _cfg()
    R, n = cur.shape
    tables = zoo.make_tables(["requests"] * R, cfg, device)
    hor = torch.arange(1, n + 1, dtype=torch.int64, device=device)[None, :].expand(R, -1).contiguous()
    dec = zoo.decide(algo, torch.from_numpy(np.array(hist)).to(device), hist.shape[1],
                     torch.from_numpy(np.array(cur)).to(device), hor, R, tables, period=cfg.seasonal_period_for(60.0),
                     smooth=cfg.seasonal_smooth, block=M_Q, trend_min_blocks=cfg.trend_min_blocks, **kw)
    return dec, C.unpack_flags(dec.flags, n)


@pytest.mark.parametrize("seed", [7, 8, 9])
def test_drifting_seasonal_history_with_incidents(seed):
    hist, cur = _quality(seed)
    T = hist.shape[1]
    fc, sigma, n, slope, nb, _ = MI.ref_seasonal_trend_robust(hist, T, M_Q, M_Q)
    z = np.abs(cur - fc) / sigma[:, None]
    print(f"seed {seed}: sigma {sigma.min():.3f}-{sigma.max():.3f}, slope error "
          f"{np.abs(slope / SLOPE_Q - 1).max():.4f}, healthy z max {z.max():.3f}")
    assert np.all(n == T) and np.all(nb == J_Q)
    assert sigma.max() <= 4.4
    assert np.abs(slope / SLOPE_Q - 1).max() <= 0.10
    # a healthy cycle: nothing flagged, either side
    dec, flags = _decide(ALGO, "cpu", hist, cur)
    assert not flags.any() and z.max() < THR_Q
    np.testing.assert_allclose(dec.upper.numpy(), fc + F32(THR_Q) * sigma[:, None], rtol=1e-6)
    np.testing.assert_allclose(dec.lower.numpy(), np.maximum(fc - F32(THR_Q) * sigma[:, None], 0), rtol=1e-6, atol=1e-4)
    # + 30 at the daily trough: flagged on every row
    ph = 3 * M_Q // 4
    bad = cur.copy()
    bad[:, ph] += 30
    dec, flags = _decide(ALGO, "cpu", hist, bad)
    zf = (bad[:, ph] - fc[:, ph]) / sigma
    assert flags[:, ph].all() and zf.min() > THR_Q
    # the cycle stays in the sigma of the two models this one composes: the same fault hides in both
    f14, s14, _, _ = MI.ref_seasonal_robust(hist, T, M_Q, M_Q)
    c16, s16, _, sl16, _ = MI.ref_trend_robust(hist, T, M_Q)
    z14 = np.abs(bad[:, ph] - f14[:, ph]) / s14
    z16 = np.abs(bad[:, ph] - (c16 + sl16 * F32(ph + 1))) / s16
    print(f"seed {seed}: fault z {zf.min():.3f}; seasonal_robust z <= {z14.max():.3f}, trend_robust z <= {z16.max():.3f}")
    for other, zo in (("seasonal_robust", z14), ("trend_robust", z16)):
        _, fo = _decide(other, "cpu", hist, bad)
        assert not fo[:, ph].any() and zo.max() < THR_Q, other


# ---------------------------------------------------------------------- zoo
def test_aliases_forecast_and_config():
    for a in (ALGO, "trend_seasonal_robust", "robust_seasonal_trend", "robust_stl", " Robust_STL "):
        assert zoo.canonical(a) == ALGO
    assert ALGO in zoo.ALGORITHMS and ALGO in zoo.FORECASTERS
    hist, _ = _quality()
    T = hist.shape[1]
    H = M_Q + 5
    th = torch.from_numpy(np.array(hist))
    fc, sigma = zoo.forecast("robust_stl", th, T, H, period=M_Q)
    rf, rs, _, rsl, _, rp = MI.ref_seasonal_trend_robust(hist, T, M_Q, H)
    assert _same(fc.numpy(), rf) and _same(sigma.numpy(), rs)
    assert _same(rf[:, M_Q:], rp[:, :5] + (rsl[:, None] * np.arange(M_Q + 1, H + 1, dtype=F32)).astype(F32))   # H > m wraps
    fc0, _ = zoo.forecast(ALGO, th, T, 4, period=M_Q, smooth=0, trend_min_blocks=8)
    want = MI.ref_seasonal_trend_robust(hist, T, M_Q, 4, smooth=0, min_blocks=8)
    assert _same(fc0.numpy(), want[0]) and (want[3] == 0).all() and not torch.equal(fc0, fc[:, :4])
    assert zoo.seasonal_start(T + 50, M_Q) == 50
    cfg = BrainConfig.from_env({"SEASONAL_PERIOD": "96", "SEASONAL_SMOOTH": "2", "TREND_MIN_BLOCKS": "4",
                                "metric_type_threshold_count": "1", "metric_type0": "memory", "threshold0": "4",
                                "ml_algorithm0": "robust_stl", "HPA_FORECAST_ALGORITHM": "trend_seasonal_robust"})
    assert zoo.canonical(cfg.algorithm_for("memory")) == ALGO and zoo.canonical(cfg.hpa_forecast_algorithm) == ALGO
    brain = Brain(MemoryStore(), cfg, device="cpu", sources=SourceRouter.synthetic_only(), worker_id="w0")
    args = {"period": 96, "smooth": 2, "trend_min_blocks": 4}
    assert brain._seasonal_trend_args("robust_stl") == args and brain._model_args(cfg.algorithm_for("memory")) == args
    for other in ("seasonal_robust", "trend_robust", "shift_robust", "moving_average_all"):
        assert brain._seasonal_trend_args(other) == {}
    assert brain._seasonal_args(ALGO) == {} and brain._trend_args(ALGO) == {} and brain._shift_args(ALGO) == {}
    assert Brain(MemoryStore(), BrainConfig(), device="cpu", sources=SourceRouter.synthetic_only(),
                 worker_id="w0")._model_args(ALGO) == {"period": 1440, "smooth": 5, "trend_min_blocks": 3}


def test_short_history_falls_back_to_the_flat_robust_band():
    hist, cur = _quality()
    short = np.ascontiguousarray(hist[:, :150])               # fewer than two periods
    a, fa = _decide(ALGO, "cpu", short, cur[:, :10])
    b, fb = _decide("robust_moving_average_all", "cpu", short, cur[:, :10])
    assert np.array_equal(fa, fb) and torch.equal(a.upper, b.upper) and torch.equal(a.lower, b.lower)
    assert a.valid.tolist() == b.valid.tolist() and a.count.tolist() == b.count.tolist()
    fc, sigma = zoo.forecast(ALGO, torch.from_numpy(short), 150, 7, period=M_Q)
    c, s, _ = MI.ref_robust_stats(short, 150)
    assert _same(fc.numpy(), np.broadcast_to(c[:, None], (R_Q, 7))) and _same(sigma.numpy(), s)
    # a period beyond the kernel's budget (m > 3328) falls back too
    long_ = np.tile(hist, (1, 11))[:4, :7000].copy()
    fc, sigma = zoo.forecast(ALGO, torch.from_numpy(long_), 7000, 2, period=3400)
    c, s, _ = MI.ref_robust_stats(long_, 7000)
    assert _same(fc.numpy()[:, 0], c) and _same(sigma.numpy(), s)


def test_history_gate_uses_the_residual_count():
    hist, cur = (a.copy() for a in _quality())
    hist[1, :-5] = np.nan                                     # 5 finite samples < MIN_HISTORICAL_DATA_POINT_TO_MEASURE
    cur[:2, 3] += 100
    dec, flags = _decide(ALGO, "cpu", hist, cur)
    assert dec.valid.tolist() == [3, 2] + [3] * (R_Q - 2)
    assert flags[0, 3] and not flags[1].any() and int(dec.count[1]) == 0


# ---------------------------------------------------------------------- GPU
SHAPES = [(2, 9, 37), (12, 30, 37), (6, 99, 37), (24, 203, 37), (96, 722, 37), (100, 2000, 37), (1440, 10080, 8),
          (2100, 6300, 20), (3328, 6656, 20)]


def _k20(d, T, m, H, smooth, mb):
    """The op's five outputs, and nblocks from a second launch of the entry
    point without forecast and profile (whose stats equal the op's)."""
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    fc, sigma, n, slope, profile = MI.seasonal_trend_robust(d, T, m, H, smooth, mb, want_profile=True)
    R = d.shape[0]
    stats = torch.full((R, 4), 7.0, device=d.device)
    LIB.call("fm_seasonal_trend_robust", ptr(d), d.stride(0), T, R, m, MI.seasonal_cycles(T, m),
             MI.seasonal_halfwidth(m, smooth), mb, 0, None, 1, ptr(stats), None, stream_of(d))
    out = [t.cpu().numpy() for t in (fc, sigma, n, slope, stats, profile)]
    assert _same(out[4][:, 0], out[1]) and _same(out[4][:, 2], out[3]) and np.array_equal(out[4][:, 1], out[2])
    out[4] = out[4][:, 3]
    return out


def _check(got, x, T, m, H, smooth, mb, what):
    fc, sigma, n, slope, nblocks, profile = got
    J = MI.seasonal_cycles(T, m)
    N = J * m
    span = x[:, T - N:T]
    rf, rs, rn, rsl, rnb, rp = MI.ref_seasonal_trend_robust(x, T, m, H, smooth, mb)
    raw = rp if smooth == 0 else MI.ref_seasonal_trend_robust(x, T, m, 0, 0, mb)[5]
    assert np.array_equal(n, rn), what
    assert _same(slope, rsl), (what, np.nonzero(slope != rsl)[0])
    assert nblocks.dtype == F32 and np.array_equal(nblocks, rnb.astype(F32)), what
    assert np.array_equal(np.isnan(profile), np.isnan(rp)), what
    if MI.seasonal_halfwidth(m, smooth) == 0:
        assert _same(profile, rp), what                       # the selection is exact
    else:
        # an fp64 sum of at most 11 fp32 values rounded once: one fp32 ulp of the largest term
        with np.errstate(invalid="ignore"):
            top = np.nanmax(np.abs(np.where(np.isnan(raw), 0, raw)), axis=1)
        err = np.abs(np.nan_to_num(profile.astype(np.float64) - rp.astype(np.float64)))
        assert np.all(err <= 2.0 ** -23 * top[:, None]), (what, err.max())
    with np.errstate(invalid="ignore", over="ignore"):
        # the forecast is the kernel's own profile, wrapped, plus the line: a product and a sum, each rounded
        h = np.arange(1, H + 1, dtype=np.int64).astype(F32)
        assert _same(fc, (profile[:, np.arange(H) % m] + (slope[:, None] * h[None, :]).astype(F32)).astype(F32)), what
        # sigma from the kernel's own slope and profile
        t = (np.arange(N, dtype=np.int64) - (N - 1)).astype(F32)
        res = (span - (slope[:, None] * t[None, :]).astype(F32)).astype(F32)
        exact, want, cnt = _sigma_from_profile(res, profile, J)
    assert np.array_equal(cnt, rn), what
    assert _same(sigma[exact], want[exact]), (what, np.nonzero(exact & (sigma != want))[0])
    rest = ~exact & (rn > 0)
    np.testing.assert_allclose(sigma[rest], want[rest], rtol=1e-6, atol=0, err_msg=str(what))
    assert np.isnan(sigma[rn == 0]).all(), what


@pytest.mark.gpu
@pytest.mark.parametrize("m,T,R", SHAPES)
def test_gpu_seasonal_trend_robust_matches_oracle(cuda, m, T, R):
    """Kernel == contract with smooth 0 and 5, H in {0, 3, m + 5} and
    min_blocks 2 and 3: n, slope and nblocks exact; the profile bit for bit
    without smoothing and within one fp32 ulp of the row's largest raw value
    with it; the forecast bit for bit the kernel's own profile, wrapped, plus
    fl(slope h); sigma, recomputed from the kernel's own slope and profile,
    bit for bit where MAD > 0 and within rtol 1e-6 on the fp64-mean fallback.
    Rows cycle through: a ramp plus a cycle, negative values, integer counts
    that are mostly zero, NaN runs, a phase missing in every cycle, a whole
    cycle missing, all-NaN, constant, +-inf samples, +-3e38.  Each batch also
    runs on views that start at columns 0-3 of an odd-stride buffer (every
    4-byte alignment of a row and of its span)."""
    x = _batch(R, T, m, 2000 + T + m)
    d = torch.from_numpy(x).to(cuda)
    for smooth, H, mb in ((5, 3, 3), (0, m + 5, 2), (5, m + 5, 2), (0, 0, 3), (5, 0, 2), (0, 3, 3)):
        _check(_k20(d, T, m, H, smooth, mb), x, T, m, H, smooth, mb, ("dense", smooth, H, mb))
    fc3, s3, n3, sl3 = MI.seasonal_trend_robust(d, T, m, 3)   # without the profile output
    ref = MI.ref_seasonal_trend_robust(x, T, m, 3)
    assert np.array_equal(n3.cpu().numpy(), ref[2]) and fc3.shape == (R, 3) and _same(sl3.cpu().numpy(), ref[3])
    ld = T + 5 + T % 2                                        # odd
    for off in range(4):
        buf = np.full((R, ld), 1e9, F32)
        buf[:, off:off + T] = x
        view = torch.from_numpy(buf).to(cuda)[:, off:]
        assert view.stride(0) % 2 == 1 and view.data_ptr() % 16 == 4 * off
        H = 3 if off % 2 else m + 5
        mb = 2 + off // 2
        _check(_k20(view, T, m, H, 5, mb), x, T, m, H, 5, mb, ("view", off))


@pytest.mark.gpu
@pytest.mark.parametrize("m,T,J,mb,skew", [(100, 150, 1, 3, 0), (100, 2000, 17, 3, 0), (3329, 6658, 2, 3, 0),
                                           (100, 250, 3, 3, 0), (100, 700, 7, 1, 0), (100, 700, 7, 3, 1)])
def test_gpu_seasonal_trend_robust_entry_rejects_bad_calls(cuda, m, T, J, mb, skew):
    """J = 1, J = 17, (J + 2) m > 13312, J m > T, min_blocks = 1 and a stats
    pointer off its 16-byte alignment: an error from the entry point, and no
    launch (the outputs keep their fill)."""
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    R, H = 3, 4
    hist = torch.zeros((R, T), device=cuda)
    fc = torch.full((R, H), 7.0, device=cuda)
    stats = torch.full((R * 4 + 4,), 7.0, device=cuda)
    prof = torch.full((R, m), 7.0, device=cuda)
    assert stats.data_ptr() % 16 == 0
    with pytest.raises(RuntimeError):
        LIB.call("fm_seasonal_trend_robust", ptr(hist), hist.stride(0), T, R, m, J, 0, mb, H, ptr(fc), H,
                 ptr(stats[skew:]), ptr(prof), stream_of(hist))
    torch.cuda.synchronize()
    assert (fc == 7).all() and (stats == 7).all() and (prof == 7).all()


@pytest.mark.gpu
def test_gpu_seasonal_trend_zoo_equals_cpu_zoo(cuda):
    hist, cur = (a.copy() for a in _quality())
    hist[7, :-5] = np.nan                                     # too little history: no verdict
    cur[:, 3 * M_Q // 4] += 30
    a, fa = _decide(ALGO, "cpu", hist, cur)
    b, fb = _decide(ALGO, cuda, hist, cur)
    assert fa[:7, 3 * M_Q // 4].all() and np.array_equal(fa, fb)
    for k in ("upper", "lower"):
        np.testing.assert_allclose(getattr(b, k).cpu().numpy(), getattr(a, k).numpy(), rtol=1e-6, err_msg=k)
    assert b.count.cpu().tolist() == a.count.tolist() and b.valid.cpu().tolist() == a.valid.tolist()
    assert a.valid[7] == 2
    short = np.ascontiguousarray(hist[:, :150])               # the fallback runs K13
    a, fa = _decide(ALGO, "cpu", short, cur[:, :10])
    b, fb = _decide(ALGO, cuda, short, cur[:, :10])
    assert np.array_equal(fa, fb) and b.valid.cpu().tolist() == a.valid.tolist()
    assert b.count.cpu().tolist() == a.count.tolist()
    np.testing.assert_allclose(b.upper.cpu().numpy(), a.upper.numpy(), rtol=1e-6)
    np.testing.assert_allclose(b.lower.cpu().numpy(), a.lower.numpy(), rtol=1e-6)
