"""K24 quantile robust statistics (median and a sigma per side from tail order
statistics), the band decision with two sigmas and the zoo model built on
them: the numpy contract against an independent computation and on its edge
cases, the skewed histories the model exists for, and the kernels against the
contracts on every row type and length that takes another path through them."""
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
Z0S = (0.5, 2.0, 3.0)


def _ulp(v):
    return np.spacing(np.abs(np.asarray(v, np.float32))).astype(np.float64)


def _phi(z):
    return 0.5 * (1.0 + math.erf(z / math.sqrt(2.0)))


def _ranks(n, z0):
    k_up = min(int(math.ceil(_phi(z0) * (n - 1))), n - 1)
    return (n - 1) - k_up, k_up


def _ds(row, c, z0):
    """(d_lo, d_up) in fp32 of one row about the fp32 centre c: which branch
    either sigma took."""
    f = np.sort(row[np.isfinite(row)])
    if f.size == 0:
        return F32(np.nan), F32(np.nan)
    k_lo, k_up = _ranks(f.size, z0)
    with np.errstate(over="ignore"):
        return F32(F32(c) - f[k_lo]), F32(f[k_up] - F32(c))


# ------------------------------------------------------------------ contract
@pytest.mark.parametrize("z0", [0.5, 0.6745, 2.0, 3.0])
def test_ref_matches_fp64_sort_within_2_ulp(z0):
    """Centre, d_lo and d_up (sigma * z0) against an fp64 computation over
    np.sort of the finite samples, within 2 fp32 ulp of the compared value.
    The d are differences of a sample and the fp32 centre, so they are taken
    about the contract's own centre (its definition), and about the fp64
    median where the centre is a sample or tiny against the spread."""
    rng = np.random.default_rng(11)
    for loc, scale, T, own_center in ((0.0, 1.0, 500, False), (0.0, 1.0, 501, False), (100.0, 5.0, 777, True),
                                      (100.0, 60.0, 778, True), (-3e4, 40.0, 64, True)):
        x = (rng.standard_normal((6, T)) * scale + loc).astype(F32)
        x[rng.random(x.shape) < 0.02] = np.nan
        c, sl, su, n = MI.ref_quantile_robust_stats(x, T, z0)
        assert c.dtype == F32 and sl.dtype == F32 and su.dtype == F32 and n.dtype == np.int32
        for r in range(x.shape[0]):
            f = np.sort(x[r][np.isfinite(x[r])].astype(np.float64))
            assert n[r] == f.size
            med = 0.5 * f[(f.size - 1) // 2] + 0.5 * f[f.size // 2]
            assert abs(float(c[r]) - med) <= 2 * _ulp(med), (loc, T, r)
            k_lo, k_up = _ranks(f.size, z0)
            about = float(c[r]) if own_center else med
            for got, want in ((sl[r], about - f[k_lo]), (su[r], f[k_up] - about)):
                assert want > 0
                want = want * float(F32(1.0 / z0))
                assert abs(float(got) - want) <= 2 * _ulp(want), (loc, T, r, z0)


def test_ref_contract_cases():
    nan, inf = np.nan, np.inf
    iz = F32(1.0 / 2.0)
    x = np.full((8, 10), nan, F32)
    x[1, 4] = 7.5                                             # n = 1
    x[2, 2], x[2, 7] = 1.0, 4.0                               # n = 2
    x[3, 1], x[3, 5], x[3, 9] = 9.0, 1.0, 3.0                 # n = 3
    x[4] = 3.25                                               # constant
    x[5] = [1, 2, 3, inf, -inf, nan, 4, 5, nan, inf]          # +-inf and NaN are missing: 1..5
    x[6] = [0, 1, 5, 5, 5, 5, 5, 5, 9, 20]                    # k_lo, the middles and k_up inside one run of ties
    x[7] = [-2, -1, 1, 2, nan, nan, nan, nan, nan, nan]       # even n
    c, sl, su, n = MI.ref_quantile_robust_stats(x, 10, 2.0)
    assert n.tolist() == [0, 1, 2, 3, 10, 5, 10, 4]
    assert np.isnan(c[0]) and np.isnan(sl[0]) and np.isnan(su[0])
    assert c[1] == 7.5 and sl[1] == 0 and su[1] == 0          # one sample: no deviation on either side
    assert c[2] == 2.5 and sl[2] == F32(1.5) * iz and su[2] == F32(1.5) * iz
    assert c[3] == 3 and sl[3] == F32(2) * iz and su[3] == F32(6) * iz
    assert c[4] == 3.25 and sl[4] == 0 and su[4] == 0
    assert c[5] == 3 and sl[5] == F32(2) * iz and su[5] == F32(2) * iz
    assert c[7] == 0 and sl[7] == F32(2) * iz and su[7] == F32(2) * iz
    # Phi(2) * 9 = 8.8 -> k_up = 9, k_lo = 0 at z0 = 2; z0 = 0.5: Phi = 0.69, k_up = 7, k_lo = 2, all in the run of 5s
    assert _ranks(10, 0.5) == (2, 7)
    c5, sl5, su5, _ = MI.ref_quantile_robust_stats(x, 10, 0.5)
    assert c5[6] == 5
    assert su5[6] == F32(1.2533) * F32((4 + 15) / 8) and sl5[6] == F32(1.2533) * F32((5 + 4) / 8)
    assert c[6] == 5 and sl[6] == F32(5) * iz and su[6] == F32(15) * iz
    # z0 = 0.5 and 3.0 at small n: k_up = n - 1 wherever ceil(p (n - 1)) reaches it
    for z0 in (0.5, 3.0):
        for nn in (1, 2, 3):
            assert _ranks(nn, z0) == (0, nn - 1)
        cz, slz, suz, _ = MI.ref_quantile_robust_stats(x, 10, z0)
        assert slz[3] == F32(2) * F32(1.0 / z0) and suz[3] == F32(6) * F32(1.0 / z0)
    assert _ranks(1000, 3.0) == (1, 998) and _ranks(100, 3.0) == (0, 99)
    # only the first T columns count
    c2, sl2, su2, n2 = MI.ref_quantile_robust_stats(x, 7, 2.0)
    assert n2.tolist() == [0, 1, 1, 2, 7, 4, 7, 4] and c2[5] == 2.5 and c2[2] == 1.0 and su2[2] == 0
    # the op on CPU tensors is the contract
    got = MI.quantile_robust_stats(torch.from_numpy(x), 10, 2.0)
    for g, w in zip(got, (c, sl, su, n)):
        assert np.array_equal(g.numpy(), w, equal_nan=True)
    assert got[3].dtype == torch.int32


def _zeros_row(T, rng):
    """99 % zeros, the rest positive: the upper quantile at z0 = 2 is the
    median itself."""
    x = np.zeros(T, F32)
    k = max(1, T // 100)
    x[rng.choice(T, k, replace=False)] = rng.exponential(50.0, k).astype(F32) + 1
    return x


def test_ref_mostly_zero_row_falls_back_to_the_one_sided_mean():
    rng = np.random.default_rng(5)
    x = _zeros_row(1000, rng)[None, :]
    c, sl, su, n = MI.ref_quantile_robust_stats(x, 1000, 2.0)
    assert c[0] == 0 and n[0] == 1000
    assert _ds(x[0], c[0], 2.0) == (0, 0)                      # Phi(2) = 0.977 < 0.99
    want = F32(1.2533) * F32(x[0].astype(np.float64).sum() / 1000)
    assert su[0] == want and want > 0
    assert sl[0] == 0                                          # nothing lies below the centre
    # at z0 = 3 the upper rank reaches the positive samples: no fallback
    c3, _, su3, _ = MI.ref_quantile_robust_stats(x, 1000, 3.0)
    assert su3[0] == np.sort(x[0])[_ranks(1000, 3.0)[1]] * F32(1.0 / 3.0) and su3[0] > 0


# ---------------------------------------------------------------------- zoo
T_CAL, N_CAL, R_CAL = 10080, 2000, 8


def _skewed(seed):
    rng = np.random.default_rng(seed)
    hist = (100 * np.exp(0.8 * rng.standard_normal((R_CAL, T_CAL)))).astype(F32)
    cur = (100 * np.exp(0.8 * rng.standard_normal((R_CAL, N_CAL)))).astype(F32)
    return hist, cur


_SKEWED = _skewed(20261020)


def _decide(algo, device, hist, cur, thr=2.0, **kw):
    cfg = BrainConfig()
    cfg.threshold, cfg.bound, cfg.min_lower_bound = thr, BOUND_BOTH, 0.0
    tables = zoo.make_tables(["requests"] * hist.shape[0], cfg, device)
    h = torch.from_numpy(hist).to(device)
    c = torch.from_numpy(cur).to(device)
    hor = torch.ones(cur.shape, dtype=torch.int64, device=device)
    dec = zoo.decide(algo, h, hist.shape[1], c, hor, hist.shape[0], tables, **kw)
    return dec, C.unpack_flags(dec.flags, cur.shape[1])


def test_band_at_tail_z_flags_the_nominal_share_of_clean_skewed_points():
    """8 rows of 100 exp(0.8 N), 10,080 samples, 2,000 clean current points
    each, thr = z0 = 2, both bounds: Phi(-2) = 0.0228 of the points lie beyond
    either end of the band; [0.017, 0.029] is +-4.5 standard deviations of the
    pooled binomial count plus the quantile's own error.  The median / MAD
    band flags several times that, all of it above."""
    hist, cur = _SKEWED
    dec, flags = _decide("quantile_robust", "cpu", hist, cur, tail_z=2.0)
    up, lo = dec.upper.numpy(), dec.lower.numpy()
    above, below = float((cur > up).mean()), float((cur < lo).mean())
    print("quantile_robust above", above, "below", below)
    assert 0.017 <= above <= 0.029 and 0.017 <= below <= 0.029
    assert np.array_equal(flags, (cur > up) | (cur < lo)) and int(dec.count.sum()) == int(flags.sum())
    assert np.all(lo[:, 0] > 0) and np.all(dec.valid.numpy() == 3)
    ctr = MI.ref_quantile_robust_stats(hist, T_CAL, 2.0)[0]
    assert np.all(up[:, 0] - ctr > 2 * (ctr - lo[:, 0]))       # the band is asymmetric, wider above
    dec2, flags2 = _decide("robust_moving_average_all", "cpu", hist, cur)
    print("robust_moving_average_all flagged", float(flags2.mean()))
    assert float(flags2.mean()) > 0.08


def test_collapse_of_a_skewed_metric_is_flagged():
    """The metric falls to 0.15 of itself (median 15): the quantile band's
    lower edge is about 20 and flags more than half of the points; the median
    / MAD band reaches below zero, is clamped at minlb = 0 and can flag none
    of them below.  (Of 16,000 such points three or four, those beyond 3.5
    sigma of the log-normal, still lie above its upper edge of about 250; they
    are no sign of the collapse and are counted apart.)"""
    hist, _ = _SKEWED
    rng = np.random.default_rng(77)
    cur = (0.15 * 100 * np.exp(0.8 * rng.standard_normal((R_CAL, N_CAL)))).astype(F32)
    dec, flags = _decide("quantile_robust", "cpu", hist, cur)
    print("collapse flagged", float(flags.mean()), "lower", dec.lower.numpy()[:, 0])
    assert float(flags.mean()) > 0.5
    assert np.all(np.abs(dec.lower.numpy()[:, 0] - 20) < 3) and abs(float(np.median(cur)) - 15) < 0.5
    dec2, flags2 = _decide("robust_moving_average_all", "cpu", hist, cur)
    print("median / MAD flagged", int(flags2.sum()), "of", flags2.size)
    assert np.all(dec2.lower.numpy() == 0)                     # the band reaches below zero: clamped at minlb
    assert not (flags2 & (cur < dec2.upper.numpy())).any()      # nothing is flagged below
    assert flags2.sum() <= 16                                  # 0.001 of the points, all above the upper edge


def test_history_gate_is_the_finite_count():
    hist, cur = _SKEWED
    hist, cur = hist[:, :200].copy(), cur[:, :10].copy()
    hist[1, 5:] = np.nan
    cur[:, 3] = 1e6
    dec, flags = _decide("skew_robust", "cpu", hist, cur)
    assert dec.valid.tolist() == [3, 2] + [3] * 6 and not flags[1].any() and int(dec.count[1]) == 0
    assert flags[[0, 2, 3, 4, 5, 6, 7], 3].all()


def test_aliases_and_config():
    for a in ("quantile_robust", "skew_robust", "asymmetric_robust", "tail_quantile", " Quantile_Robust "):
        assert zoo.canonical(a) == "quantile_robust"
    assert "quantile_robust" in zoo.ALGORITHMS and "quantile_robust" not in zoo.AUTO_CANDIDATES
    with pytest.raises(ValueError):
        zoo.canonical("quantile")
    assert BrainConfig().quantile_tail_z == 2.0
    for given, want in (("0.1", 0.5), ("0.6745", 0.6745), ("2.5", 2.5), ("7", 3.0), ("x", 2.0), ("", 2.0)):
        assert BrainConfig.from_env({"QUANTILE_TAIL_Z": given}).quantile_tail_z == want
    assert MI.quantile_tail_z(0.0) == 0.5 and MI.quantile_tail_z(10) == 3.0 and MI.quantile_tail_z(1.5) == 1.5
    cfg = BrainConfig.from_env({"ML_ALGORITHM": "moving_average_all", "metric_type_threshold_count": "1",
                                "metric_type0": "latency", "threshold0": "2", "ml_algorithm0": "tail_quantile"})
    assert zoo.canonical(cfg.algorithm_for("cpu")) == "moving_average_all"
    assert zoo.canonical(cfg.algorithm_for("latency")) == "quantile_robust"


# ------------------------------------------------------------ band decision
def _band_case(R, n, with_diff, seed=0):
    rng = np.random.default_rng(1000 * R + n + seed)
    M = 3 if R >= 3 else 1
    cur = (rng.standard_normal((R, n)) * 10 + 50).astype(F32)
    cur[rng.random((R, n)) < 0.05] = np.nan
    ctr = (rng.standard_normal((R, n)) * 2 + 50).astype(F32)
    ctr[rng.random((R, n)) < 0.02] = np.nan
    sl = rng.uniform(0.5, 4, R).astype(F32)
    su = rng.uniform(2, 9, R).astype(F32)
    for r, (a, b) in zip(range(R), ((0, 0), (np.nan, 3), (2, np.nan), (0, 5), (3, 0))):
        sl[r], su[r] = a, b
    thr = rng.uniform(1, 3, M).astype(F32)
    bound = np.array([3, 1, 2][:M], np.int32)
    mlb = np.array([45.0, -1e30, 0.0][:M], F32)
    diff = (rng.random(R) < 0.4).astype(np.int8) if with_diff else None
    return cur, ctr, sl, su, M, thr, bound, mlb, diff, 0.8


def _t(a, device="cpu"):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(device)


def _np(t):
    return t.detach().cpu().numpy()


@pytest.mark.parametrize("n", [1, 64, 65, 130])
@pytest.mark.parametrize("with_diff", [False, True])
def test_ref_band_decide_2s_with_equal_sigmas_is_ref_band_decide(n, with_diff):
    cur, ctr, sl, su, M, thr, bound, mlb, diff, pf = _band_case(40, n, with_diff)
    with np.errstate(invalid="ignore"):
        a = SM.ref_band_decide_2s(cur, ctr, su, su, M, thr, bound, mlb, diff, pf)
        b = SM.ref_band_decide(cur, ctr, su, M, thr, bound, mlb, diff, pf)
    for x, y, k in zip(a, b, ("upper", "lower", "flags", "count", "score")):
        assert x.dtype == y.dtype and np.array_equal(_np(x), _np(y), equal_nan=True), k
    # the op on CPU tensors is the reference, and it wants one sigma per row on either side
    c = SM.band_decide_2s(_t(cur), _t(ctr), _t(sl), _t(su), M, _t(thr), _t(bound), _t(mlb), _t(diff), pf)
    with np.errstate(invalid="ignore"):
        d = SM.ref_band_decide_2s(cur, ctr, sl, su, M, thr, bound, mlb, diff, pf)
    for x, y in zip(c, d):
        assert np.array_equal(_np(x), _np(y), equal_nan=True)
    with pytest.raises(ValueError):
        SM.band_decide_2s(_t(cur), _t(ctr), _t(sl[:-1].copy()), _t(su), M, _t(thr), _t(bound), _t(mlb), _t(diff), pf)


def test_ref_band_decide_2s_scores_in_units_of_the_side_it_left():
    one = lambda v, dt: np.array([v], dt)
    cur = np.array([[100, 130, 80, np.nan, 101]], F32)
    ctr = np.full((1, 5), 100, F32)
    up, lo, flags, cnt, score = SM.ref_band_decide_2s(cur, ctr, one(2.0, F32), one(10.0, F32), 1, one(2.0, F32),
                                                      one(3, np.int32), one(0.0, F32), None, 0.8)
    assert np.all(_np(up) == 120) and np.all(_np(lo) == 96)
    assert C.unpack_flags(flags, 5).tolist() == [[False, True, True, False, False]] and cnt.tolist() == [2]
    assert float(score[0]) == 8.0                              # (96 - 80) / 2 beats (130 - 120) / 10
    # a NaN sigma flags nothing on its side; a zero sigma scores 1e30
    _, _, flags, cnt, score = SM.ref_band_decide_2s(cur, ctr, one(np.nan, F32), one(0.0, F32), 1, one(2.0, F32),
                                                    one(3, np.int32), one(0.0, F32), None, 0.8)
    assert C.unpack_flags(flags, 5).tolist() == [[False, True, False, False, True]] and float(score[0]) == F32(1e30)


# ---------------------------------------------------------------------- GPU
NTYPES = 14


def _row(kind, T, rng):
    """One history row of length T of the given type (see the list in
    ``test_gpu_quantile_robust_stats_matches_contract``)."""
    nan, inf = np.nan, np.inf
    x = np.full(T, nan, F32)
    if kind == 0:                                             # all missing
        return x
    if kind == 1:                                             # one finite sample
        x[rng.integers(T)] = -12.5
        return x
    if kind == 2:                                             # constant
        x[:] = 42.0
        return x
    if kind == 3:                                             # > 50 % zeros
        x[:] = np.where(rng.random(T) < 0.7, 0.0, rng.exponential(3.0, T))
        return x
    if kind == 4:                                             # heavy ties
        return rng.integers(0, 4, T).astype(F32)
    if kind == 5:                                             # all negative
        return (-np.abs(rng.standard_normal(T)) * 50 - 1).astype(F32)
    if kind == 6:                                             # mixed sign
        return (rng.standard_normal(T) * 3).astype(F32)
    if kind == 7:                                             # -0.0 next to +0.0 around the middle
        x[:] = np.where(rng.random(T) < 0.5, -0.0, 0.0)
        k = T // 5
        x[:k], x[T - k:] = -1.5, 2.5
        return rng.permutation(x)
    if kind == 8:                                             # missing values of every kind, also at both ends
        x[:] = rng.standard_normal(T) * 5 + 100
        x[rng.random(T) < 0.2] = nan
        x[rng.random(T) < 0.05] = inf
        x[rng.random(T) < 0.05] = -inf
        x[0], x[-1] = nan, -inf
        return x
    if kind == 9:                                             # 1e30 and 1e-30 in one row
        x[:] = np.where(rng.random(T) < 0.5, 1e30, 1e-30) * rng.choice([-1.0, 1.0], T) * rng.uniform(1, 2, T)
        return x
    if kind == 10:                                            # differ in the last mantissa bits only
        return (F32(1.0).view(np.uint32) + rng.integers(0, 4, T).astype(np.uint32)).view(F32)
    if kind == 11:                                            # even n, middles differ in the top byte of the key
        v = np.concatenate([-(1 + rng.random(T // 2)), 1 + rng.random(T // 2)]).astype(F32)
        x[:v.size] = v                                        # an odd T leaves one missing sample
        return rng.permutation(x)
    if kind == 12:                                            # 99 % zeros: d_up = 0 at z0 = 2, a positive fallback
        return _zeros_row(T, rng)
    x[:] = 5.0                                                # k_lo, the middles and k_up inside one run of ties
    k = T // 200                                              # (0.5 % a side: inside every z0's tail)
    x[:k] = -rng.random(k) * 3
    x[T - k:] = 9 + rng.random(k) * 20
    return rng.permutation(x)


def _batch(R, T, seed):
    rng = np.random.default_rng(seed)
    off = 6 if R == 1 else 0
    return np.stack([_row((r + off) % NTYPES, T, rng) for r in range(R)])


def _check(got, ref, exact_lo, exact_up, what):
    c, sl, su, n = (_np(t) for t in got)
    rc, rsl, rsu, rn = ref
    assert np.array_equal(n, rn), what
    assert np.array_equal(c, rc, equal_nan=True), (what, np.nonzero(~((c == rc) | (np.isnan(c) & np.isnan(rc))))[0])
    for s, rs, exact, side in ((sl, rsl, exact_lo, "lo"), (su, rsu, exact_up, "up")):
        assert np.array_equal(s[exact], rs[exact]), (what, side, np.nonzero(exact & (s != rs))[0])
        rest = ~exact & (rn > 0)
        np.testing.assert_allclose(s[rest], rs[rest], rtol=1e-6, atol=0, err_msg=str((what, side)))
        assert np.isnan(s[rn == 0]).all(), (what, side)


SHAPES = [(1, 37), (2, 37), (3, 37), (63, 37), (64, 37), (65, 37), (255, 37), (256, 37), (257, 37), (1000, 37),
          (4099, 37), (10080, 37), (MI.ROBUST_LDS_KEYS, 5), (MI.ROBUST_LDS_KEYS + 3, 5), (1000, 1), (257, 700)]


@pytest.mark.gpu
@pytest.mark.parametrize("z0", Z0S)
@pytest.mark.parametrize("T,R", SHAPES)
def test_gpu_quantile_robust_stats_matches_contract(cuda, T, R, z0):
    """Kernel == contract: n and centre equal as floats (-0 == +0), either
    sigma equal where its d > 0 and within rtol 1e-6 on the fp64-mean
    fallback.  Rows cycle through the twelve kinds of test_robust_ops.py
    (all-NaN, single finite, constant, > 50 % zeros, integers 0..3,
    all-negative, mixed sign, -0.0 / +0.0, NaN and +-inf scattered, 1e30 with
    1e-30, last-mantissa-bit differences, an even-n row whose middles differ in
    the key's top byte), a 99 %-zeros row and a row whose three ranks lie in
    one run of ties.  Each batch also runs with ld > T and 1e9 past column T,
    and on a view that starts at column 1 of an odd-stride buffer (4-byte
    alignment only, every peel)."""
    x = _batch(R, T, 100 + T)
    ref = MI.ref_quantile_robust_stats(x, T, z0)
    with np.errstate(invalid="ignore"):
        d = np.array([_ds(x[r, :T], ref[0][r], z0) for r in range(R)])
        exact_lo, exact_up = d[:, 0] > 0, d[:, 1] > 0
    _check(MI.quantile_robust_stats(torch.from_numpy(x).to(cuda), T, z0), ref, exact_lo, exact_up, ("dense", T, R))
    wide = np.full((R, T + 5), 1e9, F32)
    wide[:, :T] = x
    _check(MI.quantile_robust_stats(torch.from_numpy(wide).to(cuda), T, z0), ref, exact_lo, exact_up,
           ("ld > T", T, R))
    ld = T + 2 + (T + 1) % 2                                    # odd stride: row starts at every 4-byte phase
    buf = np.full((R, ld), 1e9, F32)
    buf[:, 1:1 + T] = x
    view = torch.from_numpy(buf).to(cuda)[:, 1:]
    assert view.data_ptr() % 16 == 4 and view.stride(0) % 2 == 1
    _check(MI.quantile_robust_stats(view, T, z0), ref, exact_lo, exact_up, ("view", T, R))


def test_row_kinds_reach_both_branches():
    """The batches of the GPU test hold rows with d > 0 and rows on the
    fallback, on either side."""
    x = _batch(37, 1000, 1100)
    ref = MI.ref_quantile_robust_stats(x, 1000, 2.0)
    d = np.array([_ds(x[r], ref[0][r], 2.0) for r in range(37)])
    with np.errstate(invalid="ignore"):
        for side in (0, 1):
            assert (d[:, side] > 0).sum() >= 10 and (d[:, side] == 0).sum() >= 4
    assert d[12, 1] == 0 and ref[2][12] > 0                    # 99 % zeros: a positive fallback above
    assert tuple(d[13]) == (0, 0) and ref[1][13] > 0 and ref[2][13] > 0    # one run of ties


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 65, 130])
@pytest.mark.parametrize("R", [1, 4, 5, 1000])
def test_gpu_band_decide_2s(cuda, R, n):
    """Kernel == reference: bounds, flags and counts equal, the score within
    the rounding of its reciprocal; with equal sigmas it is fm_band_decide bit
    for bit; too few flag words are refused."""
    for with_diff in (False, True):
        cur, ctr, sl, su, M, thr, bound, mlb, diff, pf = _band_case(R, n, with_diff)
        with np.errstate(invalid="ignore"):
            ref = tuple(_np(v) for v in SM.ref_band_decide_2s(cur, ctr, sl, su, M, thr, bound, mlb, diff, pf))
        args = (M, _t(thr, cuda), _t(bound, cuda), _t(mlb, cuda), _t(diff, cuda), pf)
        got = tuple(_np(v) for v in SM.band_decide_2s(_t(cur, cuda), _t(ctr, cuda), _t(sl, cuda), _t(su, cuda), *args))
        for k, g, w in zip(("upper", "lower", "flags", "count"), got, ref):
            assert np.array_equal(g, w, equal_nan=True), (k, R, n, with_diff)
        # the kernel multiplies by 1 / sigma where the reference divides: 1.5 ulp (a rounded reciprocal, a rounded
        # product) -> rtol 2e-7 at most; 1e-6 is the suite's bound for fm_band_decide's score
        np.testing.assert_allclose(got[4], ref[4], rtol=1e-6, atol=0)
        a = SM.band_decide_2s(_t(cur, cuda), _t(ctr, cuda), _t(su, cuda), _t(su, cuda), *args)
        b = SM.band_decide(_t(cur, cuda), _t(ctr, cuda), _t(su, cuda), *args)
        for k, x, y in zip(("upper", "lower", "flags", "count", "score"), a, b):
            assert x.dtype == y.dtype and np.array_equal(_np(x).view(np.uint8), _np(y).view(np.uint8)), (k, R, n)


@pytest.mark.gpu
def test_gpu_band_decide_2s_rejects_too_few_flag_words(cuda):
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    cur, ctr, sl, su, M, thr, bound, mlb, diff, pf = _band_case(4, 65, False)
    d = {k: _t(v, cuda) for k, v in dict(cur=cur, ctr=ctr, sl=sl, su=su, thr=thr, bound=bound, mlb=mlb).items()}
    up, lo = torch.empty((4, 65), device=cuda), torch.empty((4, 65), device=cuda)
    flags = torch.zeros((4, 2), dtype=torch.int64, device=cuda)
    cnt = torch.zeros((4,), dtype=torch.int32, device=cuda)
    sc = torch.zeros((4,), dtype=torch.float32, device=cuda)
    with pytest.raises(RuntimeError):
        LIB.call("fm_band_decide_2s", ptr(d["cur"]), 65, 65, ptr(d["ctr"]), 65, ptr(d["sl"]), ptr(d["su"]), 4, M,
                 ptr(d["thr"]), ptr(d["bound"]), ptr(d["mlb"]), None, pf, ptr(up), ptr(lo), ptr(flags), 1, ptr(cnt),
                 ptr(sc), stream_of(d["cur"]))
    torch.cuda.synchronize()
    assert int(flags.abs().sum()) == 0 and int(cnt.sum()) == 0      # nothing was launched


@pytest.mark.gpu
def test_gpu_quantile_zoo_equals_cpu_zoo(cuda):
    hist, cur = _SKEWED
    hist, cur = hist[:, :2000].copy(), cur[:, :70].copy()
    hist[7, 40:] = np.nan                                     # a short row
    hist[6, 5:] = np.nan                                      # fewer than MIN_HISTORICAL_DATA_POINT_TO_MEASURE
    cur[:, 3], cur[:, 9] = 5000.0, 1.0
    a, fa = _decide("quantile_robust", "cpu", hist, cur, tail_z=2.0)
    b, fb = _decide("quantile_robust", cuda, hist, cur, tail_z=2.0)
    assert fa[:6, 3].all() and fa[:6, 9].all() and not fa[6].any()
    assert np.array_equal(fa, fb)
    for k in ("upper", "lower"):
        np.testing.assert_allclose(getattr(b, k).cpu().numpy(), getattr(a, k).numpy(), rtol=1e-6, err_msg=k)
    assert b.count.cpu().tolist() == a.count.tolist() and b.valid.cpu().tolist() == a.valid.tolist()
