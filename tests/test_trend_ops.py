"""K16 trend robust model (repeated-median slope over the block medians, median
/ MAD of the residuals): the numpy contract against a direct per-row loop and
on hand-built rows, the drifting history the model exists for, and the kernel
against the contract on every shape that takes another path through it."""
import functools

import numpy as np
import pytest
import torch

from foremast_amd.config import BrainConfig
from foremast_amd.models import zoo
from foremast_amd.ops import canary as C
from foremast_amd.ops import misc as MI

NAN, INF = np.nan, np.inf
F = np.float32


# ------------------------------------------------------------------ contract
def _mid(v):
    """K13's median rule over a 1-D fp32 array (not empty)."""
    s = np.sort(np.asarray(v, F))
    return F(0.5) * s[(s.size - 1) // 2] + F(0.5) * s[s.size // 2]


def _loop_row(x, T, L, mb):
    """The contract for one row, written out: sort each block, the pair
    slopes, two medians, the residuals, their median and MAD."""
    x = np.asarray(x, F)[:T]
    J = MI.shift_blocks(T, L)
    q, b = [], []
    for j in range(J):
        blk = x[T - (J - j) * L:T - (J - j - 1) * L]
        f = blk[np.isfinite(blk)]
        if f.size >= max(1, L // 4):
            q.append(j)
            b.append(_mid(f))
    slope = F(0)
    with np.errstate(invalid="ignore", over="ignore"):
        if len(q) >= mb:
            s = [_mid([F(F(b[j] - b[i]) / F((q[j] - q[i]) * L)) for j in range(len(q)) if j != i])
                 for i in range(len(q))]
            slope = _mid(s)
            if not np.isfinite(slope):
                slope = F(0)
        r = np.array([F(x[i] - F(slope * F(i - (T - 1)))) for i in range(T)], F)
    f = r[np.isfinite(r)]
    if f.size == 0:
        return F(NAN), F(NAN), 0, slope, len(q)
    with np.errstate(over="ignore"):
        c = _mid(f)
        d = np.abs(f - c)
        mad = _mid(d)
        sigma = F(1.4826) * mad if mad > 0 else F(1.2533) * F(d.astype(np.float64).sum() / f.size)
    return c, sigma, f.size, slope, len(q)


def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


def test_ref_equals_a_direct_per_row_loop():
    rng = np.random.default_rng(3)
    for T, L, mb in ((19, 1, 3), (50, 3, 3), (64, 4, 2), (97, 6, 3), (47, 12, 3), (30, 12, 3), (200, 24, 4)):
        R = 24
        t = np.arange(T)
        x = (rng.standard_normal((R, T)) * 2 + 100 + rng.uniform(-0.5, 0.5, (R, 1)) * t).astype(F)
        x[4:8] = rng.integers(0, 4, (4, T)) + (t // max(1, T // 5))            # ties
        x[8:12][rng.random((4, T)) < 0.3] = NAN
        x[12:14][rng.random((2, T)) < 0.1] = INF
        x[12:14][rng.random((2, T)) < 0.1] = -INF
        x[14, T // 2:] = NAN
        x[15] = NAN
        x[16, :] = 7.0
        x[17][rng.random(T) < 0.05] = 3e38                                   # pair slopes and residuals overflow
        x[18][rng.random(T) < 0.5] = -3e38
        out = MI.ref_trend_robust(x, T, L, mb)
        assert [a.dtype for a in out] == [F, F, np.int32, F, np.int32]
        for r in range(R):
            want = _loop_row(x[r], T, L, mb)
            for k, name in enumerate(("center", "sigma", "n", "slope", "nblocks")):
                assert _eq(out[k][r], want[k]), ((T, L, mb), r, name, out[k][r], want[k])


def test_ref_rows_without_a_slope_are_robust_stats_bit_for_bit():
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((6, 64)) * 2 + 100 + 0.3 * np.arange(64)).astype(F)
    # J < min_blocks: two blocks, or min_blocks above the blocks there are
    for T, L, mb in ((30, 12, 3), (64, 40, 3), (64, 16, 5), (10, 12, 3)):
        c, s, n, slope, nb = MI.ref_trend_robust(x, T, L, mb)
        rc, rs, rn = MI.ref_robust_stats(x, T)
        assert not slope.any() and (nb == MI.shift_blocks(T, L)).all()
        assert np.array_equal(c, rc) and np.array_equal(s, rs) and np.array_equal(n, rn)
    y = x.copy()
    y[0] = 42.0                                                # constant
    y[1] = NAN                                                 # all missing
    y[2, 16:] = NAN                                            # one block left of four
    y[3] = -0.0
    c, s, n, slope, nb = MI.ref_trend_robust(y, 64, 16, 3)
    rc, rs, rn = MI.ref_robust_stats(y, 64)
    rows = [0, 1, 2, 3]
    assert not slope[rows].any() and nb[rows].tolist() == [4, 0, 1, 4]
    assert _eq(c[rows], rc[rows]) and _eq(s[rows], rs[rows]) and np.array_equal(n[rows], rn[rows])
    assert np.isnan(c[1]) and np.isnan(s[1]) and n[1] == 0 and slope[1] == 0
    assert c[0] == 42 and s[0] == 0 and slope[4] != 0
    with pytest.raises(ValueError):
        MI.ref_trend_robust(x, 64, 16, 1)


def test_ref_recovers_an_exactly_representable_slope():
    """Multiples of 1/8 and L a power of two: every block median, every
    difference of two and every quotient is exact, so the slope is, and the
    residuals are one constant."""
    T, L = 64, 8
    x = np.stack([np.arange(T) / 8.0, 5.0 - np.arange(T) / 4.0, (np.arange(T) - 20) * 0.5]).astype(F)
    c, s, n, slope, nb = MI.ref_trend_robust(x, T, L)
    assert slope.tolist() == [0.125, -0.25, 0.5] and nb.tolist() == [8, 8, 8] and n.tolist() == [T] * 3
    assert c.tolist() == [63 / 8.0, 5.0 - 63 / 4.0, 21.5] and s.tolist() == [0, 0, 0]
    # in front of the blocks too (T = 70: six columns the slope does not read), and with a missing block
    x = (np.arange(70) / 8.0).astype(F)[None, :].copy()
    x[0, 6 + 16:6 + 24] = NAN
    c, s, n, slope, nb = MI.ref_trend_robust(x, 70, L)
    assert slope[0] == 0.125 and nb[0] == 7 and n[0] == 62 and c[0] == 69 / 8.0 and s[0] == 0


def _pair_slopes(b, L):
    J = b.size
    return np.array([(b[j] - b[i]) / ((j - i) * L) for i in range(J) for j in range(J) if i != j])


def test_two_whole_bad_blocks_of_seven_do_not_move_the_slope():
    """Two day-long incidents in a week: 11 of the 21 pair slopes are wrong,
    which breaks Theil-Sen.  Every inner median of a good block is taken over
    four good and two wild slopes, and the outer one over five good and two
    wild inner medians, so the dirty slope is an order statistic of the good
    blocks' pair slopes, as the clean one is: they differ by at most the
    spread of the clean ramp's pair slopes."""
    T, L = 448, 64
    rng = np.random.default_rng(9)
    t = np.arange(T)
    clean = (100 + 100 * t / (T - 1) + rng.standard_normal((64, T)) * 2).astype(F)
    c0, s0, _, sl0, _ = MI.ref_trend_robust(clean, T, L)
    true = 100 / (T - 1)
    assert np.abs(sl0 - true).max() < 0.1 * true
    worst = 0.0
    for a, b in ((0, 1), (2, 5), (5, 6), (0, 6), (3, 4)):
        dirty = clean.copy()
        dirty[:, a * L:(a + 1) * L] += 300
        dirty[:, b * L:(b + 1) * L] += 300
        c1, s1, _, sl1, _ = MI.ref_trend_robust(dirty, T, L)
        for r in range(clean.shape[0]):
            bm = np.median(clean[r].reshape(7, L).astype(np.float64), axis=1)
            ps = _pair_slopes(bm, L)
            assert abs(float(sl1[r]) - float(sl0[r])) <= ps.max() - ps.min() + 1e-6, (a, b, r)
        worst = max(worst, float(np.abs(sl1 - sl0).max()))
        # and the band still shows a +30 fault on today's level of 200 at 3 sigma (2 / 7 of the row is off the
        # line, so the median and the MAD of the residuals move up, but stay far from the flat model's 150 and 37)
        assert (c1 + 3 * s1).max() < 230 and (c1 - 3 * s1).min() > 170
    # the least-squares slope of the block medians moves by a third of itself on the same rows
    bm = np.median(dirty.reshape(64, 7, L).astype(np.float64), axis=2)
    ls = np.polyfit(np.arange(7) * L, bm.T, 1)[0]
    assert worst < 0.1 * true < np.abs(ls - true).min()


# ---------------------------------------------------------------------- zoo
T_FIX, L_FIX, N_CUR, THR, FAULT = 2000, 200, 10, 3.0, (2, 5, 8)


def _fixture():
    """8 rows x 2000: a ramp 100 -> 250 with N(0, 2) noise and 3 % incidents
    at 1000 (every 33rd sample).  The current window continues the line at
    horizons 1..10 within +-1, with +30 (15 sigma of the noise) at three
    points.

    Judged at 3 sigma: the trend band is the line +- 6.  The flat median /
    MAD model has centre 175 and sigma 55, an upper bound of 340 against
    faults at 280; the mean / std model's sigma is the incidents' (140)."""
    rng = np.random.default_rng(21)
    t = np.arange(T_FIX)
    step = 150.0 / (T_FIX - 1)
    hist = (100 + step * t + rng.standard_normal((8, T_FIX)) * 2).astype(F)
    hist[:, 5::33] = 1000.0
    h = np.arange(1, N_CUR + 1)
    cur = (250 + step * h + np.linspace(-1, 1, N_CUR))[None, :].repeat(8, 0).astype(F)
    cur[:, FAULT] += 30
    return hist, cur


def _decide(algo, device, hist, cur, **kw):
    cfg = BrainConfig()
    cfg.threshold = THR
    tables = zoo.make_tables(["requests"] * hist.shape[0], cfg, device)
    h = torch.from_numpy(hist).to(device)
    c = torch.from_numpy(cur).to(device)
    hor = torch.arange(1, cur.shape[1] + 1, dtype=torch.int64, device=device)[None, :].repeat(cur.shape[0], 1)
    dec = zoo.decide(algo, h, hist.shape[1], c, hor, hist.shape[0], tables, block=L_FIX, **kw)
    return dec, C.unpack_flags(dec.flags, cur.shape[1])


def test_drift_hides_a_fault_from_the_flat_models_but_not_from_trend_robust():
    hist, cur = _fixture()
    c, s, n, slope, nb = MI.ref_trend_robust(hist, T_FIX, L_FIX)
    assert nb.tolist() == [10] * 8 and n.tolist() == [T_FIX] * 8
    assert np.abs(c - 250).max() < 1 and np.abs(slope - 150 / (T_FIX - 1)).max() < 2e-3 and s.min() > 1.8
    assert s.max() < 2.4
    fault = np.zeros(N_CUR, bool)
    fault[list(FAULT)] = True
    # the margins of the fixture, on the reference: nothing sits on an edge
    h = np.arange(1, N_CUR + 1, dtype=F)
    line = c[:, None] + slope[:, None] * h[None, :]
    up, lo = line + F(THR) * s[:, None], line - F(THR) * s[:, None]
    assert (cur[:, ~fault] <= (up - s[:, None])[:, ~fault]).all()
    assert (cur[:, ~fault] >= (lo + s[:, None])[:, ~fault]).all()
    assert (cur[:, fault] >= (up + 2 * s[:, None])[:, fault]).all()
    fc, fs, _ = MI.ref_robust_stats(hist, T_FIX)
    assert (cur[:, fault] <= (fc + F(THR) * fs - fs)[:, None]).all()          # >= 1 sigma inside the flat band
    mean, std = hist.mean(1, dtype=np.float64), hist.std(1, dtype=np.float64)
    assert (cur[:, fault] <= (mean + THR * std - std)[:, None]).all()
    # the decisions
    dec, flags = _decide("trend_robust", "cpu", hist, cur)
    assert np.array_equal(flags, np.broadcast_to(fault, flags.shape))
    assert dec.count.tolist() == [3] * 8 and dec.valid.tolist() == [3] * 8
    np.testing.assert_allclose(dec.upper.numpy(), up, rtol=1e-6)
    np.testing.assert_allclose(dec.center.numpy(), line, rtol=1e-6)
    for flat in ("robust_moving_average_all", "moving_average_all"):
        d2, f2 = _decide(flat, "cpu", hist, cur)
        assert not f2[:, fault].any(), flat
    assert not _decide("robust_moving_average_all", "cpu", hist, cur)[1].any()


def test_aliases_config_and_forecaster():
    for a in ("trend_robust", "robust_trend", "trend_median", "repeated_median", " Trend_Robust "):
        assert zoo.canonical(a) == "trend_robust"
    assert "trend_robust" in zoo.ALGORITHMS and "trend_robust" in zoo.FORECASTERS
    cfg = BrainConfig()
    assert (cfg.trend_block, cfg.trend_min_blocks) == (0, 3)
    assert cfg.trend_block_for(60.0) == 1440 and cfg.trend_block_for(300.0) == 288
    cfg = BrainConfig.from_env({"ML_ALGORITHM": "repeated_median", "TREND_BLOCK": "720", "TREND_MIN_BLOCKS": "4",
                                "HPA_FORECAST_ALGORITHM": "trend_median"})
    assert zoo.canonical(cfg.algorithm_for("memory")) == "trend_robust"
    assert zoo.canonical(cfg.hpa_forecast_algorithm) == "trend_robust"
    assert (cfg.trend_block, cfg.trend_min_blocks) == (720, 4) and cfg.trend_block_for(60.0) == 720
    assert BrainConfig.from_env({"TREND_MIN_BLOCKS": "1"}).trend_min_blocks == 2          # floored
    assert BrainConfig.from_env({}).trend_min_blocks == 3


def test_forecast_is_the_extrapolated_line():
    hist, _ = _fixture()
    c, s, n, slope, _ = MI.ref_trend_robust(hist, T_FIX, L_FIX)
    H = 15
    fc, sigma = zoo.forecast("trend_median", torch.from_numpy(hist), T_FIX, H, block=L_FIX)
    h = np.arange(1, H + 1, dtype=F)
    assert fc.shape == (8, H) and fc.dtype == torch.float32
    assert np.array_equal(fc.numpy(), c[:, None] + slope[:, None] * h[None, :]) and np.array_equal(sigma.numpy(), s)
    assert (np.diff(fc.numpy(), axis=1) > 0).all()
    # min_blocks above the blocks there are: a constant forecast of the whole-history median
    fc, sigma = zoo.forecast("trend_robust", torch.from_numpy(hist), T_FIX, H, block=L_FIX, trend_min_blocks=11)
    rc, rs, _ = MI.ref_robust_stats(hist, T_FIX)
    assert np.array_equal(fc.numpy(), np.broadcast_to(rc[:, None], (8, H))) and np.array_equal(sigma.numpy(), rs)
    # the op on CPU tensors is the contract
    got = MI.trend_robust(torch.from_numpy(hist), T_FIX, L_FIX)
    assert len(got) == 4 and got[2].dtype == torch.int32
    for g, w in zip(got, (c, s, n, slope)):
        assert np.array_equal(g.numpy(), w)
    with pytest.raises(ValueError):                           # the row has to fit the LDS
        MI.trend_robust(torch.zeros((1, MI.ROBUST_LDS_KEYS + 1)), MI.ROBUST_LDS_KEYS + 1, 832)
    with pytest.raises(ValueError):
        MI.trend_robust(torch.zeros((1, 64)), 64, 8, 1)


def test_history_gate_is_the_kernels_count_and_a_long_history_reads_its_tail():
    cfg = BrainConfig()
    tables = zoo.make_tables(["requests"] * 2, cfg, "cpu")
    # row 0: 9 finite samples (below MIN_HISTORICAL_DATA_POINT_TO_MEASURE = 10), row 1: 10
    short = np.full((2, 64), NAN, F)
    short[0, 1:64:7] = 10.0 + 0.01 * np.arange(9)
    short[1, 1:64:7] = 10.0 + 0.01 * np.arange(9)
    short[1, 63] = 10.1
    n = MI.ref_trend_robust(short, 64, 4)[2]
    assert n.tolist() == [9, 10]
    dec = zoo.decide("trend_robust", torch.from_numpy(short), 64, torch.full((2, 4), 500.0),
                     torch.ones((2, 4), dtype=torch.int64), 2, tables, block=4)
    assert dec.valid.tolist() == [2, 3] and dec.count.tolist() == [0, 4]
    # a history longer than the kernel's LDS budget: the last ROBUST_LDS_KEYS columns
    assert zoo.trend_start(100) == 0 and zoo.trend_start(MI.ROBUST_LDS_KEYS + 7) == 7
    rng = np.random.default_rng(2)
    T = MI.ROBUST_LDS_KEYS + 7
    long = (rng.standard_normal((2, T)) * 5 + 100 + 0.01 * np.arange(T)).astype(F)
    long[:, :7] = 1e6
    dec = zoo.decide("trend_robust", torch.from_numpy(long), T, torch.full((2, 4), 100.0),
                     torch.ones((2, 4), dtype=torch.int64), 2, tables)
    c, s, _, slope, nb = MI.ref_trend_robust(long[:, 7:], T - 7, 1440)
    assert nb.tolist() == [9, 9] and (slope > 0.009).all()
    assert np.array_equal(dec.center.numpy()[:, 0], c + slope * F(1))


# ---------------------------------------------------------------------- GPU
SHAPES = [(19, 1), (50, 3), (32, 4), (64, 4), (97, 6), (77, 8), (47, 12), (30, 12), (200, 24), (10080, 1440),
          (MI.ROBUST_LDS_KEYS, 832)]
KINDS = 16
NOISE = 2.0


def _gpu_row(kind, T, L, rng):
    J = MI.shift_blocks(T, L)
    off = T - J * L
    t = np.arange(T)
    ramp = 100.0 * t / max(T - 1, 1)
    x = (rng.standard_normal(T) * NOISE + 100).astype(F)
    blk = lambda j: slice(off + j * L, off + (j + 1) * L)     # noqa: E731
    if kind == 0:                                             # clean flat
        pass
    elif kind == 1:                                           # ramp up
        x += ramp.astype(F)
    elif kind == 2:                                           # ramp down
        x -= ramp.astype(F)
    elif kind == 3:                                           # ramp across zero: keys cross the sign bit inside a block
        x = (rng.standard_normal(T) * NOISE + ramp - 50).astype(F)
    elif kind == 4:                                           # constant
        x[:] = 42.0
    elif kind == 5:                                           # heavy ties with a ramp
        x = (rng.integers(0, 4, T) + (8 * t // max(T, 1))).astype(F)
    elif kind == 6:                                           # a count row, mostly zero: MAD = 0, the fallback sigma
        x = np.where(rng.random(T) < 0.85, 0.0, rng.integers(1, 4, T)).astype(F)
    elif kind == 7:                                           # 5 % incidents on a ramp
        x += ramp.astype(F)
        x[rng.random(T) < 0.05] = 1000.0
    elif kind == 8:                                           # empty blocks
        x += ramp.astype(F)
        for j in (0, 2, J - 1):
            if 0 <= j < J:
                x[blk(j)] = NAN
    elif kind == 9:                                           # a block with one finite sample (empty unless L < 8)
        x += ramp.astype(F)
        if J > 1:
            x[blk(1)] = NAN
            x[off + L + L // 2] = 77.0
    elif kind == 10:                                          # even and odd finite counts side by side
        x += ramp.astype(F)
        for j in range(0, J, 2):
            x[off + j * L + (j % L)] = NAN
    elif kind == 11:                                          # missing values of every kind, at both ends too
        x += ramp.astype(F)
        x[rng.random(T) < 0.2] = NAN
        x[rng.random(T) < 0.05] = INF
        x[rng.random(T) < 0.05] = -INF
        x[0], x[-1] = -INF, NAN
        if T > 2:
            x[1], x[-2] = NAN, INF
    elif kind == 12:                                          # all missing
        x[:] = NAN
    elif kind == 13:                                          # one finite sample
        x[:] = NAN
        x[rng.integers(T)] = -12.5
    elif kind == 14:                                          # a 30 sigma step: the blocks' key ranges are disjoint
        x[T // 2:] += 30 * NOISE
    else:                                                     # 1 % missing on a shallow negative ramp of large values
        x = (1e6 - 3.0 * t + rng.standard_normal(T) * 50).astype(F)
        x[rng.random(T) < 0.01] = NAN
    return x


@functools.lru_cache(maxsize=None)
def _gpu_batch(T, L):
    """Two rows of every kind, and the reference of the batch, computed once."""
    rows = [_gpu_row(kind, T, L, np.random.default_rng([T, L, kind, rep])) for kind in range(KINDS) for rep in range(2)]
    x = np.stack(rows)
    x.setflags(write=False)
    return x, MI.ref_trend_robust(x, T, L)


def _mad_positive(x, T, slope, center):
    """Which branch sigma took, per row: the fp32 MAD of the residuals about
    the fp32 centre is > 0."""
    t = (np.arange(T, dtype=np.int64) - (T - 1)).astype(F)
    out = np.zeros(x.shape[0], bool)
    with np.errstate(invalid="ignore", over="ignore"):
        r = x - (slope[:, None] * t[None, :]).astype(F)
        for i in range(x.shape[0]):
            f = r[i][np.isfinite(r[i])]
            out[i] = f.size > 0 and _mid(np.abs(f - center[i])) > 0
    return out


def _check(got, x, T, ref, what):
    c, s, n, slope = (g.cpu().numpy() for g in got)
    rc, rs, rn, rslope, _ = ref
    bad = lambda a, b: np.nonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))[0]       # noqa: E731
    assert np.array_equal(n, rn), (what, bad(n, rn))
    assert _eq(slope, rslope), (what, bad(slope, rslope), slope, rslope)
    assert _eq(c, rc), (what, bad(c, rc))
    exact = _mad_positive(x, T, rslope, rc)
    assert np.array_equal(s[exact], rs[exact]), (what, np.nonzero(exact & (s != rs))[0])
    rest = ~exact & (rn > 0)
    np.testing.assert_allclose(s[rest], rs[rest], rtol=1e-6, atol=0, err_msg=str(what))
    assert np.isnan(s[rn == 0]).all() and np.isnan(c[rn == 0]).all(), what


@pytest.mark.parametrize("T,L", SHAPES)
def test_gpu_inputs_take_every_path(T, L):
    """On the CPU: what the batches below are meant to hold, they hold."""
    x, (c, s, n, slope, nb) = _gpu_batch(T, L)
    J = MI.shift_blocks(T, L)
    assert x.shape[0] == 2 * KINDS
    k = lambda kind: slice(2 * kind, 2 * kind + 2)             # noqa: E731
    assert (n[k(12)] == 0).all() and (n[k(13)] == 1).all() and not slope[k(12)].any() and not slope[k(13)].any()
    assert not slope[k(4)].any() and (s[k(4)] == 0).all()
    if J >= 3:
        assert (slope[k(1)] > 0).all() and (slope[k(2)] < 0).all() and (nb[k(0)] == J).all()
        assert (nb[k(8)] == J - len({0, 2, J - 1})).all()
        assert (nb[k(9)] == (J if L < 8 else J - 1)).all()
    else:
        assert not slope.any()                                 # J = 2: no slope, robust_stats of the row
        rc, rs, rn = MI.ref_robust_stats(x, T)
        assert _eq(c, rc) and _eq(s, rs) and np.array_equal(n, rn)
    exact = _mad_positive(x, T, slope, c)
    assert not exact[k(6)].any() and (s[k(6)] > 0).all() and exact[k(1)].all()
    fin = np.isfinite(x[:, T - J * L:].reshape(-1, J, L)).sum(2)
    assert (fin[k(10)] % 2 == 0).any() and (fin[k(10)] % 2 == 1).any() or J < 2


@pytest.mark.gpu
@pytest.mark.parametrize("T,L", SHAPES)
def test_gpu_trend_robust_matches_oracle(cuda, T, L):
    """Kernel == contract: n, slope and centre equal as floats (-0 == +0, NaN
    == NaN), sigma equal where the residuals' MAD > 0 and within rtol 1e-6 on
    the fp64-mean fallback (the kernel sums in another order).  Each batch
    runs contiguous, with ld > T and 1e9 past column T, and on a view that
    starts at column 1 of an odd-stride buffer (4-byte alignment only: the row
    starts at every word of a quad, and no block bound is 16-byte aligned)."""
    x, ref = _gpu_batch(T, L)
    R = x.shape[0]
    _check(MI.trend_robust(torch.from_numpy(x.copy()).to(cuda), T, L), x, T, ref, ("dense", T, L))
    wide = np.full((R, T + 5), 1e9, F)
    wide[:, :T] = x
    _check(MI.trend_robust(torch.from_numpy(wide).to(cuda), T, L), x, T, ref, ("ld > T", T, L))
    ld = T + 2 + (T + 1) % 2                                    # odd stride: row starts at every 4-byte phase
    buf = np.full((R, ld), 1e9, F)
    buf[:, 1:1 + T] = x
    view = torch.from_numpy(buf).to(cuda)[:, 1:]
    assert view.data_ptr() % 16 == 4 and view.stride(0) % 2 == 1
    _check(MI.trend_robust(view, T, L), x, T, ref, ("view", T, L))


@pytest.mark.gpu
def test_gpu_trend_robust_min_blocks_two(cuda):
    """min_blocks = 2 on two blocks: one pair slope is the slope."""
    x, _ = _gpu_batch(30, 12)
    ref = MI.ref_trend_robust(x, 30, 12, 2)
    assert ref[3][2:4].all()
    _check(MI.trend_robust(torch.from_numpy(x.copy()).to(cuda), 30, 12, 2), x, 30, ref, "min_blocks = 2")


@pytest.mark.gpu
def test_gpu_trend_robust_entry_rejects_what_it_cannot_hold(cuda):
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    big = MI.ROBUST_LDS_KEYS + 1
    h = torch.zeros((1, big), device=cuda)
    out = torch.full((1, 4), 7.0, device=cuda)
    for T, L, J, mb in ((big, 832, 16, 3),                     # T > 13312
                        (64, 2, 17, 3),                        # J > 16
                        (64, 8, 9, 3),                         # J L > T
                        (64, 8, 8, 1)):                        # min_blocks < 2
        with pytest.raises(RuntimeError, match="hipError 1"):
            LIB.call("fm_trend_robust", ptr(h), h.stride(0), T, 1, L, J, mb, ptr(out), stream_of(h))
    torch.cuda.synchronize()
    assert (out.cpu() == 7.0).all()                            # nothing was launched
    with pytest.raises(ValueError):
        MI.trend_robust(h, big, 832)


@pytest.mark.gpu
def test_gpu_trend_zoo_equals_cpu_zoo(cuda):
    hist, cur = _fixture()
    hist[7, 9:] = np.nan                                      # a short row: not judged
    a, fa = _decide("trend_robust", "cpu", hist, cur)
    b, fb = _decide("trend_robust", cuda, hist, cur)
    assert fa[:7].sum() == 21 and fa[:7][:, list(FAULT)].all() and not fa[7].any()
    assert np.array_equal(fa, fb)
    for k in ("upper", "lower"):
        np.testing.assert_allclose(getattr(b, k).cpu().numpy(), getattr(a, k).numpy(), rtol=1e-6, err_msg=k)
    assert b.count.cpu().tolist() == a.count.tolist() and b.valid.cpu().tolist() == a.valid.tolist()
    assert a.valid.tolist() == [3] * 7 + [2]
