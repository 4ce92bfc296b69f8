"""K15 level-shift robust model (median / MAD behind the latest persistent
level shift): the numpy contract on hand-built rows, the stepped-history case
the model exists for, and the kernel against the contract on every shape that
takes another path through it."""
import functools

import numpy as np
import pytest
import torch

from foremast_amd.config import BrainConfig
from foremast_amd.models import zoo
from foremast_amd.ops import canary as C
from foremast_amd.ops import misc as MI

NAN, INF = np.nan, np.inf
K, MB = 4.0, 2


# ------------------------------------------------------------------ contract
def _base(T=32):
    """A level of 10 with a small deterministic wiggle (MAD > 0)."""
    return (10 + 0.1 * np.sin(1.7 * np.arange(T))).astype(np.float32)


def _same(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w, equal_nan=True)


def _equals_robust(x, T, out, rows):
    c, s, n = MI.ref_robust_stats(x[rows], T)
    assert np.array_equal(out[0][rows], c, equal_nan=True) and np.array_equal(out[1][rows], s, equal_nan=True)
    assert np.array_equal(out[2][rows], n)
    assert not out[3][rows].any() and not out[4][rows].any()


def test_shift_blocks():
    assert MI.shift_blocks(32, 4) == 8 and MI.shift_blocks(64, 4) == 16 and MI.shift_blocks(1000, 4) == 16
    assert MI.shift_blocks(97, 6) == 16 and MI.shift_blocks(47, 12) == 3 and MI.shift_blocks(10080, 1440) == 7
    assert MI.shift_blocks(3, 4) == 0 and MI.shift_blocks(32, 0) == 0


def test_ref_step_cases():
    """L = 4, T = 32: eight blocks, candidates j = 6, 5, 4, 3."""
    T, L = 32, 4
    x = np.stack([_base() for _ in range(5)])
    x[0, 20:] += 50                                           # a step on the boundary of block 5
    x[1, 18:] += 50                                           # a step in the middle of block 4
    x[2, 26:] += 50                                           # a step inside the last min_blocks blocks
    x[3, 20:] -= 50                                           # downward
    x[4, [3, 9, 17, 22, 30]] = 1000.0                         # incidents without a step
    out = MI.ref_shift_robust(x, T, L, K, MB)
    c, s, n, start, delta, score = out
    assert [a.dtype for a in out] == [np.float32, np.float32, np.int32, np.int32, np.float32, np.float32]
    # row 0: candidate 6 (transition block 5 already on the new level): the start includes the boundary block
    assert start[0] == 20 and n[0] == 12 and abs(delta[0] - 50) < 0.2 and score[0] > 25
    # row 1: block 4 is half old, half new; it belongs to neither side and the segment starts behind it
    assert start[1] == 20 and n[1] == 12 and abs(delta[1] - 50) < 0.2 and score[1] > 25
    assert start[3] == 20 and abs(delta[3] + 50) < 0.2 and score[3] > 25
    for r in (0, 1, 3):
        rc, rs, rn = MI.ref_robust_stats(x[r:r + 1, start[r]:], T - start[r])
        assert c[r] == rc[0] and s[r] == rs[0] and n[r] == rn[0] and 0 < s[r] < 0.5
    assert abs(c[0] - 60) < 0.2 and abs(c[3] + 40) < 0.2
    # rows 2 and 4: no shift, robust_stats bit for bit; the score seen stays below k
    _equals_robust(x, T, out, [2, 4])
    assert 0 < score[2] < K and 0 < score[4] < 1
    # the candidate table: the shift of row 0 is the LARGEST j above k, although 5 scores as high
    valid, sc, d, den, edge, b = MI.shift_candidates(x, T, L, MB)
    assert valid[0].tolist() == [False] * 3 + [True] * 4 + [False] * 2
    assert sc[0, 6] > 25 and sc[0, 5] > 25 and sc[0, 4] < 1.5 and sc[0, 3] < 1.5
    assert edge[0, 6] <= den[0, 6] and edge[1, 5] > den[1, 5]
    assert abs(b[1, 4] - 35) < 0.2                            # the transition block's median is halfway


def test_ref_constant_row_with_step():
    """More than half of the row on one value: MAD = 0, so s_all is the mean
    deviation fallback and the standard-error floor alone is the spread.  At
    ordinary magnitudes that keeps den > 0 and the score finite; den == 0
    with d != 0 needs a step so small that the floor rounds to zero."""
    T, L = 32, 4
    x = np.full((2, T), 42.0, np.float32)
    x[0, 24:] = 50.0
    tiny = np.float32(4.2e-45)                                # 3 denormal units
    x[1] = 0.0
    x[1, 20:] = tiny
    c, s, n, start, delta, score = MI.ref_shift_robust(x, T, L, K, MB)
    s_all = MI.ref_robust_stats(x, T)[1]
    assert s_all[0] == np.float32(1.2533) * np.float32(8 * 8 / 32)
    se = np.float32(1.2533) * s_all[0] / np.sqrt(np.float32(L))
    assert score[0] == np.float32(8) / se and score[0] > K
    assert start[0] == 24 and delta[0] == 8 and c[0] == 50 and s[0] == 0 and n[0] == 8
    assert s_all[1] > 0 and np.float32(1.2533) * s_all[1] / np.sqrt(np.float32(L)) == 0     # the floor underflows
    assert delta[1] != 0 and score[1] == INF
    assert start[1] == 20 and n[1] == 12 and c[1] == np.float32(0.5) * tiny + np.float32(0.5) * tiny


def test_ref_all_nan_count_row_empty_blocks_and_inf():
    T, L = 32, 4
    x = np.stack([_base() for _ in range(6)])
    x[0] = NAN                                                # all missing
    x[1, :24] = [0, 0, 0, 1] * 6                              # a count row, mostly zero ...
    x[1, 24:] = [8, 9, 8, 7] * 2                              # ... whose rate steps up: MAD = 0 over the row
    x[2, 20:] += 50                                           # a step with an empty transition block
    x[2, 20:24] = NAN
    x[3, 20:] += 50                                           # empty blocks on both sides
    x[3, 4:8] = NAN
    x[3, 24:28] = NAN
    x[4, 20:] += 50                                           # +-inf are missing samples
    x[4, [2, 21, 30]] = [INF, -INF, INF]
    x[5] = x[4]
    x[5, [2, 21, 30]] = NAN
    out = MI.ref_shift_robust(x, T, L, K, MB)
    c, s, n, start, delta, score = out
    assert np.isnan(c[0]) and np.isnan(s[0]) and n[0] == 0 and start[0] == 0 and delta[0] == 0 and score[0] == 0
    s_all = MI.ref_robust_stats(x[1:2], T)[1][0]
    assert s_all == np.float32(1.2533) * np.float32((6 + 64) / 32)          # the fallback
    assert start[1] == 24 and delta[1] == 8 and c[1] == 8 and n[1] == 8 and score[1] > K
    assert s[1] == np.float32(1.4826) * np.float32(0.5)
    # row 2: blocks 6 and 7 are the post side of candidate 6, the empty block 5 cannot join them
    assert start[2] == 24 and n[2] == 8 and abs(delta[2] - 50) < 0.2
    # row 3: post of candidate 6 has one block only; candidate 5 (post = 5, 7) finds it, block 4 is old
    valid = MI.shift_candidates(x, T, L, MB)[0]
    assert not valid[3, 6] and valid[3, 5] and start[3] == 20 and n[3] == 8
    for a in out:
        assert a[4] == a[5] or (np.isnan(a[4]) and np.isnan(a[5]))
    assert start[4] == 20 and n[4] == 10


def test_ref_short_histories_and_op():
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((4, 40)) * 2 + 100).astype(np.float32)
    x[:, 28:] += 60
    for T, L in ((16, 4), (19, 4), (32, 40), (32, 8)):        # J = 4, 4, 0, 4: below 3 + min_blocks
        out = MI.ref_shift_robust(x, T, L, K, MB)
        assert MI.shift_blocks(T, L) < 5
        _equals_robust(x, T, out, [0, 1, 2, 3])
        assert not out[5].any()
    out = MI.ref_shift_robust(x, 40, 4, K, MB)
    assert (out[3] == 28).all() and (out[2] == 12).all()
    # the op on CPU tensors is the contract
    got = MI.shift_robust(torch.from_numpy(x), 40, 4, K, MB)
    _same([g.numpy() for g in got], out)
    assert got[2].dtype == torch.int32 and got[3].dtype == torch.int32
    with pytest.raises(ValueError):                           # the row has to fit the LDS
        MI.shift_robust(torch.zeros((1, MI.ROBUST_LDS_KEYS + 1)), MI.ROBUST_LDS_KEYS + 1, 832, K, MB)


# ---------------------------------------------------------------------- zoo
T_FIX, L_FIX, N_CUR, THR = 2000, 200, 10, 1.0


def _fixture():
    """8 rows x 2000: N(100, 5).  Rows 0-5 step to 140 at column 1100 and
    carry incidents (every 20th sample, 5 %, at 1000); rows 6-7 are clean.  The
    current window sits inside 140 +- 3, with 200 injected at point 3 of every
    row.

    Judged at 1 sigma (``THR``): with 45 % of a row on the new level the
    whole-row MAD reaches up into it, so ``robust_moving_average_all`` has
    centre 108 and sigma 25 here; its band tops out near 134 at 1 sigma (and
    near 184 at 3, where it would judge nothing at all).  The model behind the
    shift has centre 140 and sigma 5: a band of 135..145."""
    rng = np.random.default_rng(11)
    hist = (rng.standard_normal((8, T_FIX)) * 5 + 100).astype(np.float32)
    hist[:6, 1100:] += 40
    hist[:6, 7::20] = 1000.0
    cur = np.tile(140 + np.linspace(-3, 3, N_CUR, dtype=np.float32), (8, 1))
    cur[:, 3] = 200.0
    return hist, cur


def _decide(algo, device, hist, cur):
    cfg = BrainConfig()
    cfg.threshold = THR
    tables = zoo.make_tables(["requests"] * hist.shape[0], cfg, device)
    h = torch.from_numpy(hist).to(device)
    c = torch.from_numpy(cur).to(device)
    hor = torch.ones(cur.shape, dtype=torch.int64, device=device)
    dec = zoo.decide(algo, h, hist.shape[1], c, hor, hist.shape[0], tables, block=L_FIX)
    return dec, C.unpack_flags(dec.flags, cur.shape[1])


def test_level_shift_is_an_anomaly_to_median_mad_but_the_new_normal_to_shift_robust():
    hist, cur = _fixture()
    old, fold = _decide("robust_moving_average_all", "cpu", hist, cur)
    assert fold[:6].all()                                     # every point of the new level is flagged
    dec, flags = _decide("shift_robust", "cpu", hist, cur)
    c, s, n, start, delta, score = MI.ref_shift_robust(hist, T_FIX, L_FIX)
    assert start.tolist() == [1200] * 6 + [0, 0] and n.tolist() == [800] * 6 + [2000] * 2
    assert np.all(np.abs(c[:6] - 140) < 1) and np.all((s > 4) & (s < 7)) and np.all(score[:6] > 3 * K)
    assert np.all(score[6:] < 1)
    upper = c + np.float32(THR) * s
    np.testing.assert_allclose(dec.upper.numpy(), np.broadcast_to(upper[:, None], cur.shape), rtol=1e-6)
    want = np.zeros(cur.shape, bool)
    want[:6, 3] = True                                        # only the injected 200
    assert np.array_equal(flags[:6], want[:6])
    # the clean rows: the same decisions under both models
    assert np.array_equal(flags[6:], fold[6:]) and flags[6:].all()
    assert np.array_equal(dec.upper.numpy()[6:], old.upper.numpy()[6:])
    assert dec.count.tolist() == [1] * 6 + [N_CUR] * 2 and dec.valid.tolist() == [3] * 8


def test_short_segment_is_not_judged_and_long_history_reads_its_tail():
    # a segment below MIN_HISTORICAL_DATA_POINT_TO_MEASURE: bit 0 clear, nothing flagged
    short = np.full((1, 64), np.nan, np.float32)
    short[0, :40:2] = 10.0 + 0.01 * np.arange(20)
    short[0, 40::5] = 60.0 + 0.01 * np.arange(5)              # 5 samples behind the step, 1 or 2 per block of 4
    c, s, n, start, delta, score = MI.ref_shift_robust(short, 64, 4)
    assert start[0] >= 36 and n[0] < 10
    cfg = BrainConfig()
    tables = zoo.make_tables(["requests"], cfg, "cpu")
    cur1 = torch.full((1, 4), 500.0)
    dec = zoo.decide("shift_robust", torch.from_numpy(short), 64, cur1, torch.ones((1, 4), dtype=torch.int64), 1,
                     tables, block=4)
    assert dec.valid.tolist() == [2] and int(dec.count[0]) == 0
    # a history longer than the kernel's LDS budget: the last ROBUST_LDS_KEYS columns
    assert zoo.shift_start(100) == 0 and zoo.shift_start(MI.ROBUST_LDS_KEYS + 7) == 7
    rng = np.random.default_rng(2)
    T = MI.ROBUST_LDS_KEYS + 7
    long = (rng.standard_normal((2, T)) * 5 + 100).astype(np.float32)
    long[:, :7] = 1e6
    dec = zoo.decide("shift_robust", torch.from_numpy(long), T, torch.full((2, 4), 100.0),
                     torch.ones((2, 4), dtype=torch.int64), 2, zoo.make_tables(["requests"] * 2, cfg, "cpu"))
    c, s, n = MI.ref_robust_stats(long[:, 7:], T - 7)
    np.testing.assert_allclose(dec.center.numpy()[:, 0], c, rtol=0)


def test_aliases_config_and_not_a_forecaster():
    for a in ("shift_robust", "level_shift", "robust_shift", "shift_mad", " Shift_Robust "):
        assert zoo.canonical(a) == "shift_robust"
    assert "shift_robust" in zoo.ALGORITHMS and "shift_robust" not in zoo.FORECASTERS
    with pytest.raises(ValueError, match="not a forecasting model"):
        zoo.forecast("shift_robust", torch.zeros((1, 64)), 64, 4)
    cfg = BrainConfig()
    assert (cfg.shift_block, cfg.shift_threshold, cfg.shift_min_blocks) == (0, 4.0, 2)
    assert cfg.shift_block_for(60.0) == 1440 and cfg.shift_block_for(300.0) == 288
    cfg = BrainConfig.from_env({"ML_ALGORITHM": "level_shift", "SHIFT_BLOCK": "720", "SHIFT_THRESHOLD": "5.5",
                                "SHIFT_MIN_BLOCKS": "3"})
    assert zoo.canonical(cfg.algorithm_for("cpu")) == "shift_robust"
    assert (cfg.shift_block, cfg.shift_threshold, cfg.shift_min_blocks) == (720, 5.5, 3)
    assert cfg.shift_block_for(60.0) == 720


# ---------------------------------------------------------------------- GPU
STEP, NOISE = 60.0, 2.0                                       # a 30 sigma step
SHAPES = [(32, 4), (64, 4), (97, 6), (77, 8), (200, 24), (47, 12), (10080, 1440), (MI.ROBUST_LDS_KEYS, 832),
          (19, 1), (50, 3), (30, 12)]                          # blocks narrower than a quad (J = 16); J = 2: no candidate
SPECIAL = 12


def _noise(T, rng, level=100.0):
    return (rng.standard_normal(T) * NOISE + level).astype(np.float32)


def _gpu_row(slot, T, L, rng):
    """One history row; ``slot`` < SPECIAL picks a special kind, a larger one
    a step whose block position and in-block offset it encodes."""
    J = MI.shift_blocks(T, L)
    off = T - J * L
    late = off + max(J - 3, 0) * L                            # a boundary a shift can be found at
    last = off + max(J - 2, 0) * L                            # the latest one
    x = _noise(T, rng)
    if slot == 0:                                             # all missing
        x[:] = NAN
    elif slot == 1:                                           # clean
        pass
    elif slot == 2:                                           # a constant row with a step
        x[:] = 42.0
        x[last:] = 50.0                                       # (one block earlier and (32, 4) scores 3.4: on the edge)
    elif slot == 3:                                           # incidents without a step
        x[rng.random(T) < 0.05] = 1000.0
    elif slot == 4:                                           # a count row, mostly zero, whose rate steps up
        x[:] = np.where(rng.random(T) < 0.7, 0.0, rng.integers(1, 4, T))
        x[late:] = rng.integers(6, 12, T - late)
    elif slot == 5:                                           # empty blocks and a thin one
        x[late:] += STEP
        for j in (1, J - 4, J - 1):
            if 0 <= j < J:
                x[off + j * L:off + (j + 1) * L] = NAN
        if J > 2:
            x[off + 2 * L + 1:off + 3 * L] = NAN              # one sample left: empty unless L < 8
    elif slot == 6:                                           # missing values of every kind, at both ends too
        x[late:] += STEP
        x[rng.random(T) < 0.2] = NAN
        x[rng.random(T) < 0.05] = INF
        x[rng.random(T) < 0.05] = -INF
        x[0], x[-1] = NAN, -INF
    elif slot == 7:                                           # one finite sample
        x[:] = NAN
        x[rng.integers(T)] = -12.5
    elif slot == 8:                                           # heavy ties with a step
        x[:] = rng.integers(0, 4, T)
        x[late:] += 10
    elif slot == 9:                                           # negative levels, a step across zero
        x[:] = _noise(T, rng, -30.0)
        x[late:] += STEP
    elif slot == 10:                                          # 5 % incidents and 1 % missing around a step
        x[late:] += STEP
        x[rng.random(T) < 0.05] = 1000.0
        x[rng.random(T) < 0.01] = NAN
    elif slot == 11:                                          # a downward step inside the last min_blocks blocks
        x[T - L - L // 2:] -= STEP
    else:                                                     # a step at block bp, offset q of (0, 1, L/4, L/2, 3L/4, L-1)
        s = slot - SPECIAL
        bp, q = s % (J + 1), (s // (J + 1)) % 6
        at = off + bp * L + (0, 1, L // 4, L // 2, 3 * L // 4, L - 1)[q]
        x[min(at, T):] += STEP if s % 2 == 0 else -STEP
    return x


def _near_edge(x, T, L):
    """[R, J + 1] bool: the valid candidates whose score lies inside (0.8 k,
    1.25 k), and those above k (the ones whose transition block is ever
    compared) whose |b[j-1] - p1| / den lies inside (0.8, 1.25).

    The second test cannot cover the candidates below k as well: behind a
    clean step the next candidate down has an old block on its post side and
    an old transition block, so its den and its |b[j-1] - p1| are both the
    step and their ratio is 1 on every stepped row.  Neither implementation
    reads that ratio."""
    valid, sc, d, den, edge, b = MI.shift_candidates(x, T, L, MB)
    with np.errstate(invalid="ignore", divide="ignore"):
        ratio = edge / den
        return valid & (((sc > 0.8 * K) & (sc < 1.25 * K)) | ((sc > K) & (ratio > 0.8) & (ratio < 1.25)))


@functools.lru_cache(maxsize=None)
def _gpu_batch(T, L):
    """The rows of one shape, each drawn again (a new seed, the same kind and
    step position) until the reference's decisions sit off every knife edge;
    with them the reference of the batch, computed once."""
    J = MI.shift_blocks(T, L)
    steps = 6 * (J + 1) if T < 1000 else (12 if T == 10080 else 2 * (J + 1))
    rows = []
    for slot in range(SPECIAL + steps):
        for attempt in range(8):
            rng = np.random.default_rng([T, L, slot, attempt])
            tries = np.stack([_gpu_row(slot, T, L, rng) for _ in range(32)])
            ok = np.nonzero(~_near_edge(tries, T, L).any(1))[0]
            if ok.size:
                rows.append(tries[ok[0]])
                break
        else:
            raise AssertionError(f"no row off the knife edge for slot {slot} of {(T, L)}")
    x = np.stack(rows)
    x.setflags(write=False)
    return x, MI.ref_shift_robust(x, T, L, K, MB)


def _mad(x, c):
    """fp32 MAD of one row about the fp32 centre c (which branch sigma took)."""
    f = x[np.isfinite(x)]
    if f.size == 0:
        return np.float32(np.nan)
    d = np.sort(np.abs(f - np.float32(c)))
    return np.float32(0.5) * d[(f.size - 1) // 2] + np.float32(0.5) * d[f.size // 2]


def _check(got, x, ref, what):
    c, s, n, start, delta, score = (t.cpu().numpy() for t in got)
    rc, rs, rn, rstart, rdelta, rscore = ref
    bad = lambda a, b: np.nonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))[0]
    assert np.array_equal(start, rstart), (what, bad(start, rstart))
    assert np.array_equal(n, rn), (what, bad(n, rn))
    assert np.array_equal(c, rc, equal_nan=True), (what, bad(c, rc))
    assert np.array_equal(delta, rdelta, equal_nan=True), (what, bad(delta, rdelta))
    with np.errstate(invalid="ignore"):
        exact = np.array([_mad(x[r, rstart[r]:], rc[r]) > 0 for r in range(x.shape[0])])
    assert np.array_equal(s[exact], rs[exact]), (what, np.nonzero(exact & (s != rs))[0])
    rest = ~exact & (rn > 0)
    np.testing.assert_allclose(s[rest], rs[rest], rtol=1e-6, atol=0, err_msg=str(what))
    assert np.isnan(s[rn == 0]).all(), what
    np.testing.assert_allclose(score, rscore, rtol=1e-6, atol=0, err_msg=str(what))


@pytest.mark.parametrize("T,L", SHAPES)
def test_gpu_inputs_sit_off_every_knife_edge(T, L):
    """The kernel decides on rounded quantities (the fallback sigma's sum
    order differs), so the comparison below is only meaningful where the
    reference's decisions have room: asserted here, on the CPU, for every row
    and every valid candidate of every shape.  The batches hold every kind of
    row: with and without a shift, and a step at every block position."""
    x, ref = _gpu_batch(T, L)
    J = MI.shift_blocks(T, L)
    R = x.shape[0]
    assert R == (24 if T == 10080 else R) and R >= SPECIAL + J + 1
    assert not _near_edge(x, T, L).any()
    start = ref[3]
    if J >= 3 + MB:
        blocks = {int(J - (T - s) // L) for s in start if s > 0}
        assert blocks >= set(range(3, J - MB + 1)), blocks    # a shift found at every block it can be found at
        assert (start == 0).sum() >= 6 and np.isinf(ref[5]).sum() == 0
    else:
        assert not start.any() and not ref[5].any()           # J = 3: no candidate
    assert np.array_equal(ref[0][start == 0], MI.ref_robust_stats(x[start == 0], T)[0], equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("T,L", SHAPES)
def test_gpu_shift_robust_matches_oracle(cuda, T, L):
    """Kernel == contract: n, start, centre and delta equal as floats (-0 ==
    +0, NaN == NaN), sigma equal where the segment's MAD > 0 and within rtol
    1e-6 on the fp64-mean fallback, score within rtol 1e-6.  Each batch runs
    contiguous, with ld > T and 1e9 past column T, and on a view that starts at
    column 1 of an odd-stride buffer (4-byte alignment only: the row starts at
    every word of a quad, and no block bound is 16-byte aligned)."""
    x, ref = _gpu_batch(T, L)
    R = x.shape[0]
    _check(MI.shift_robust(torch.from_numpy(x.copy()).to(cuda), T, L, K, MB), x, ref, ("dense", T, L))
    wide = np.full((R, T + 5), 1e9, np.float32)
    wide[:, :T] = x
    _check(MI.shift_robust(torch.from_numpy(wide).to(cuda), T, L, K, MB), x, ref, ("ld > T", T, L))
    ld = T + 2 + (T + 1) % 2                                    # odd stride: row starts at every 4-byte phase
    buf = np.full((R, ld), 1e9, np.float32)
    buf[:, 1:1 + T] = x
    view = torch.from_numpy(buf).to(cuda)[:, 1:]
    assert view.data_ptr() % 16 == 4 and view.stride(0) % 2 == 1
    _check(MI.shift_robust(view, T, L, K, MB), x, ref, ("view", T, L))


@pytest.mark.gpu
def test_gpu_shift_robust_rejects_a_row_beyond_the_lds(cuda):
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    T = MI.ROBUST_LDS_KEYS + 1
    h = torch.zeros((1, T), device=cuda)
    out = torch.zeros((1, 6), device=cuda)
    with pytest.raises(RuntimeError, match="hipError 1"):
        LIB.call("fm_shift_robust", ptr(h), h.stride(0), T, 1, 832, 16, 4.0, 2, ptr(out), stream_of(h))
    with pytest.raises(ValueError):
        MI.shift_robust(h, T, 832, K, MB)


@pytest.mark.gpu
def test_gpu_shift_zoo_equals_cpu_zoo(cuda):
    hist, cur = _fixture()
    hist[7, 40:] = np.nan                                     # a short row
    a, fa = _decide("shift_robust", "cpu", hist, cur)
    b, fb = _decide("shift_robust", cuda, hist, cur)
    assert fa[:6].sum() == 6 and fa[:6, 3].all()
    assert np.array_equal(fa, fb)
    for k in ("upper", "lower"):
        np.testing.assert_allclose(getattr(b, k).cpu().numpy(), getattr(a, k).numpy(), rtol=1e-6, err_msg=k)
    assert b.count.cpu().tolist() == a.count.tolist() and b.valid.cpu().tolist() == a.valid.tolist()
