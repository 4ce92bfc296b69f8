"""K23 hold-out score and the zoo model ``auto_robust`` built on it: the numpy
contracts (ref_holdout_score, ref_auto_pick) against plain per-row loops, the
six row shapes the six candidate models exist for, each of which must pick its
own model, the row-by-row equality of an ``auto_robust`` decision with the
chosen model's own, and the kernel against the contract on every shape, stride
mix and row kind that takes another path through it."""
import math

import numpy as np
import pytest
import torch

from foremast_amd.models import zoo
from foremast_amd.ops import misc as MI

F32 = np.float32
ZCAP, MARGIN = 8.0, 0.05
M96 = 96
ARGS = dict(period=M96, holdout=M96, block=M96)


# ------------------------------------------------------------------ contracts as loops
def _at(a, r, t):
    return a[r, t if a.shape[1] > 1 else 0]


def _loop_score(x, fc, sigma, zcap):
    R, L = x.shape
    C = len(fc)
    score = np.full((R, C), np.inf, F32)
    n = np.zeros((R, C), np.int32)
    nx = np.zeros(R, np.int32)
    with np.errstate(over="ignore", invalid="ignore"):
        for r in range(R):
            nx[r] = sum(1 for t in range(L) if np.isfinite(x[r, t]))
            for c in range(C):
                terms = []
                for t in range(L):
                    xv, f, s = F32(x[r, t]), F32(_at(fc[c], r, t)), F32(_at(sigma[c], r, t))
                    if not (np.isfinite(xv) and np.isfinite(f) and np.isfinite(s) and s > 0):
                        continue
                    z = min(F32(np.abs(F32(xv - f)) / s), F32(zcap))
                    terms.append(float(F32(math.log(float(s)))) + float(z))
                n[r, c] = len(terms)
                if terms:
                    score[r, c] = F32(math.fsum(terms) / len(terms))
    return score, n, nx


def _loop_pick(score, n, nx, margin):
    out = np.zeros(score.shape[0], np.int32)
    for r in range(score.shape[0]):
        elig = [c for c in range(score.shape[1]) if n[r, c] >= 1 and 2 * n[r, c] >= nx[r]]
        if elig:
            lim = F32(min(score[r, c] for c in elig) + F32(margin))
            out[r] = next(c for c in elig if score[r, c] <= lim)
    return out


def _flip_distance(score, n, nx, margin, choice):
    """How far, in nats, the scores of each row are from another choice: the
    chosen candidate and every eligible one in front of it against the limit
    ``best + margin``, and every eligible one behind it against pushing the
    chosen one out (``score + margin`` against the chosen score).  Rows without
    an eligible candidate are decided by counts alone: +inf."""
    d = np.full(score.shape[0], np.inf)
    s = score.astype(np.float64)
    for r in range(score.shape[0]):
        elig = [c for c in range(score.shape[1]) if n[r, c] >= 1 and 2 * n[r, c] >= nx[r]]
        if not elig:
            continue
        k = int(choice[r])
        lim = min(s[r, c] for c in elig) + margin
        for c in elig:
            d[r] = min(d[r], abs(s[r, c] - lim) if c <= k else s[r, c] + margin - s[r, k])
    return d


def _rand_case(rng, R, L, C, nan_share=0.1):
    x = (100 + 5 * rng.standard_normal((R, L))).astype(F32)
    x[rng.random((R, L)) < nan_share] = np.nan
    fc, sg = [], []
    for c in range(C):
        wide_f, wide_s = bool(c & 1), bool(c & 2)
        f = (100 + rng.standard_normal((R, L if wide_f else 1))).astype(F32)
        s = np.exp(rng.uniform(-2, 3, (R, L if wide_s else 1))).astype(F32)
        fc.append(f)
        sg.append(s)
    return x, fc, sg


def test_contracts_equal_plain_loops():
    rng = np.random.default_rng(0)
    x, fc, sg = _rand_case(rng, 12, 37, 6)
    x[0] = np.nan                                             # all missing: n = 0 -> +inf everywhere, choice 0
    x[1, :5] = [np.inf, -np.inf, 3e38, -3e38, 1e6]            # +-inf samples, a difference that overflows, the cap
    fc[1][1, :5] = [100, 100, -3e38, 3e38, 100]
    sg[0][2] = 0.0                                            # sigma 0, NaN, inf and negative do not count
    sg[2][3, ::2] = np.nan
    sg[2][3, 1] = np.inf
    sg[2][3, 3] = -1.0
    fc[1][4, :30] = np.nan                                    # scores 7 points of ~33: not eligible
    fc[3][4, :12] = np.nan                                    # scores more than half: eligible
    fc[5][5] = fc[1][5]                                       # a tie: the first of the two is taken
    sg[5][5] = sg[1][5]
    score, n, nx = MI.ref_holdout_score(x, fc, sg, ZCAP)
    ls, ln, lnx = _loop_score(x, fc, sg, ZCAP)
    np.testing.assert_array_equal(n, ln)
    np.testing.assert_array_equal(nx, lnx)
    assert np.isinf(score[0]).all() and (n[0] == 0).all() and np.isinf(score[2, 0])
    assert (score[5, 5] == score[5, 1]) and n[4, 1] * 2 < nx[4] <= n[4, 3] * 2
    np.testing.assert_allclose(score, ls, rtol=1.2e-7, atol=0)
    for margin in (0.0, MARGIN, 10.0):
        choice = MI.ref_auto_pick(score, n, nx, margin)
        np.testing.assert_array_equal(choice, _loop_pick(score, n, nx, margin))
        assert choice[0] == 0 and choice[4] != 1
    assert MI.ref_auto_pick(score, n, nx, 10.0)[5] <= 1       # a wide margin takes the simplest eligible model
    # the cap bounds a point's influence: a miss of 1e6 sigmas adds zcap
    one = MI.ref_holdout_score(np.array([[1e6]], F32), [np.zeros((1, 1), F32)], [np.ones((1, 1), F32)], ZCAP)
    assert one[0][0, 0] == F32(ZCAP)
    # ties go to the first candidate; the second must win by more than the margin
    sc = np.array([[1.0, 1.0], [1.0, 0.96], [1.0, 0.94], [np.inf, np.inf]], F32)
    cnt = np.array([[4, 4], [4, 4], [4, 4], [0, 0]], np.int32)
    np.testing.assert_array_equal(MI.ref_auto_pick(sc, cnt, np.full(4, 4, np.int32), MARGIN), [0, 0, 1, 0])
    np.testing.assert_array_equal(MI.ref_auto_pick(sc, cnt, np.full(4, 9, np.int32), MARGIN), [0, 0, 0, 0])


def test_wrapper_refuses_what_the_kernel_does_not_take():
    x = torch.zeros((2, 4))
    one = [torch.zeros((2, 1))]
    with pytest.raises(ValueError):
        MI.holdout_score(x, one * 9, [torch.ones((2, 1))] * 9)
    with pytest.raises(ValueError):
        MI.holdout_score(torch.zeros((1, MI.ROBUST_LDS_KEYS + 1)), one[:1], [torch.ones((1, 1))])
    with pytest.raises(ValueError):
        MI.holdout_score(x, one, [torch.ones((2, 3))])
    with pytest.raises(ValueError):
        MI.holdout_score(x, one, [torch.ones((2, 1))], zcap=0.0)


# ------------------------------------------------------------------ the six shapes
def six_rows(seed, m=M96, days=7, incident=False, tile=1):
    """The six histories the candidates exist for, in candidate order: flat,
    a level shift that held, drift, a daily cycle, a daily cycle whose noise
    grows with the level, drift plus a daily cycle, over one draw of noise;
    ``tile`` > 1: that many copies of the six (row ``6 k + i`` has shape
    ``i``), every row with noise of its own.  ``incident`` puts +60 on a tenth
    of the last day of every row."""
    T = m * days
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    w = np.sin(2 * np.pi * t / m)
    rows = []
    for _ in range(tile):
        e = rng.standard_normal((6, T)) if tile > 1 else np.tile(rng.standard_normal(T), (6, 1))
        lvl = 100 + 80 * w
        rows += [100 + 2 * e[0], 100 + 2 * e[1] + 40 * (t >= 3 * m + m // 3), 100 + 10 * t / m + 2 * e[2],
                 100 + 40 * w + 2 * e[3], lvl + 0.08 * lvl * e[4], 100 + 40 * w + 10 * t / m + 2 * e[5]]
    x = np.stack(rows).astype(F32)
    if incident:
        a = T - m + m // 4
        x[:, a:a + m // 10 + 1] += 60
    return x


def _cpu_selection(x):
    T = x.shape[1]
    choice, score, n = zoo.auto_select(torch.from_numpy(x), T, **ARGS)
    nx = np.isfinite(x[:, T - M96:]).sum(1)
    return choice.numpy(), score.numpy(), _flip_distance(score.numpy(), n.numpy(), nx, MARGIN, choice.numpy())


@pytest.mark.parametrize("incident", [False, True])
def test_each_shape_picks_its_model(incident):
    x = six_rows(0, incident=incident)
    choice, score, dist = _cpu_selection(x)
    print("scores", np.round(score, 4).tolist(), "distance to flipping", np.round(dist, 4).tolist())
    assert (dist >= 1e-3).all(), dist                         # every row: no choice hangs on the last bits
    np.testing.assert_array_equal(choice, np.arange(6))


def test_short_history_is_not_back_tested():
    x = torch.from_numpy(six_rows(0)[:, :2 * M96 - 1].copy())
    choice, score, n = zoo.auto_select(x, x.shape[1], **ARGS)
    assert (choice == 0).all() and torch.isinf(score).all() and (n == 0).all()
    assert (zoo.auto_select(x, x.shape[1], candidates="seasonal_robust,trend_robust", **ARGS)[0] == 2).all()


def test_candidate_subset_keeps_the_table_order():
    assert zoo.auto_candidates(None) == tuple(range(6)) and zoo.auto_candidates("") == tuple(range(6))
    assert zoo.auto_candidates("seasonal_robust, median_mad") == (0, 3)
    with pytest.raises(ValueError):
        zoo.auto_candidates("seasonal_robust,holt_winters")
    x = six_rows(0)
    choice, score, _ = zoo.auto_select(torch.from_numpy(x), x.shape[1], candidates=["trend_robust", "mad"], **ARGS)
    assert score.shape == (6, 2) and set(choice.tolist()) <= {0, 2} and choice[2] == 2 and choice[0] == 0


def _tables(R, dev="cpu", min_hist=10):
    return zoo.Tables(torch.full((R,), 3.0, device=dev), torch.full((R,), 3, dtype=torch.int32, device=dev),
                      torch.zeros((R,), device=dev), 0.5, min_hist)


def _current(x, n=12):
    """A current window after each history: its last ``n`` samples again (the
    same phase is ``n`` steps on), with an excursion in the middle."""
    cur = x[:, -n:].copy()
    cur[:, n // 2] += 150
    cur[:, 1] = np.nan
    return cur


def _decision_equal(a, b, rows=None):
    for k in ("upper", "lower", "flags", "count", "score", "valid"):
        va = getattr(a, k).cpu().numpy()
        np.testing.assert_array_equal(va if rows is None else va[rows], getattr(b, k).cpu().numpy(), err_msg=k)


SINGLE = {k: v for k, v in ARGS.items() if k != "holdout"}      # what a candidate gets as the configured model


@pytest.mark.parametrize("incident", [False, True])
def test_decision_is_the_chosen_models_own(incident):
    x = six_rows(0, incident=incident)
    x[2, 40:60] = np.nan
    R, T = x.shape
    hist, cur = torch.from_numpy(x), torch.from_numpy(_current(x))
    n = cur.shape[1]
    hor = torch.arange(1, n + 1).repeat(R, 1)
    diff = torch.tensor([0, 1, 0, 0, 1, 0], dtype=torch.int8)
    tb = _tables(R)
    dec = zoo.decide("auto_robust", hist, T, cur, hor, R, tb, diff, **ARGS)
    np.testing.assert_array_equal(dec.choice.numpy(), np.arange(6))
    assert (dec.count.numpy() >= 1).all()                     # the excursion is seen under every model
    for r in range(R):
        one = zoo.Tables(tb.thr[r:r + 1], tb.bound[r:r + 1], tb.minlb[r:r + 1], tb.pair_factor, tb.min_hist)
        own = zoo.decide(zoo.AUTO_CANDIDATES[r], hist[r:r + 1].clone(), T, cur[r:r + 1], hor[r:r + 1], 1, one,
                         diff[r:r + 1], **SINGLE)
        _decision_equal(dec, own, slice(r, r + 1))


def test_given_choices_are_kept_and_the_rest_selected():
    x = six_rows(0)
    hist = torch.from_numpy(x)
    T, H = x.shape[1], 7
    given = torch.tensor([5, -1, 0, -1, 2, -1], dtype=torch.int32)
    fc, sigma, nfin, choice = zoo._auto_robust(hist, T, H, choice=given, **ARGS)
    np.testing.assert_array_equal(choice.numpy(), [5, 1, 0, 3, 2, 5])
    assert fc.shape == (6, H) and sigma.shape == (6, H) and nfin.dtype == torch.int32
    f5, s5, n5 = zoo._seasonal_trend_robust(hist[[0, 5]], T, H, M96, 5, 3)
    np.testing.assert_array_equal(fc[[0, 5]].numpy(), f5.numpy())
    np.testing.assert_array_equal(sigma[[0, 5]].numpy(), s5[:, None].expand(-1, H).numpy())
    f0, s0, n0 = MI.robust_stats(hist[2:3], T)
    assert (fc[2] == f0).all() and (sigma[2] == s0).all() and nfin[2] == n0
    with pytest.raises(ValueError):
        zoo._auto_robust(hist, T, H, choice=torch.tensor([6, 0, 0, 0, 0, 0]), **ARGS)
    # forecast() serves the HPA load forecast with the same numbers
    fc2, sigma2 = zoo.forecast("auto_robust", hist, T, H, **ARGS)
    np.testing.assert_array_equal(fc2[[1, 3]].numpy(), fc[[1, 3]].numpy())


def test_auto_robust_is_registered():
    for name in ("auto_robust", "auto", "robust_auto", "auto_select", " AUTO "):
        assert zoo.canonical(name) == "auto_robust"
    assert "auto_robust" in zoo.ALGORITHMS and "auto_robust" in zoo.FORECASTERS
    assert zoo.AUTO_CANDIDATES == ("robust_moving_average_all", "shift_robust", "trend_robust", "seasonal_robust",
                                   "seasonal_scale_robust", "seasonal_trend_robust")


# ------------------------------------------------------------------ K23 against the contract
NKINDS = 10


def _kernel_case(L, C, R, seed):
    """Held-out rows of every kind (row r is kind r % NKINDS) and C candidates
    in every stride mix (candidate c: forecast per point when c & 1, sigma per
    point when c & 2) -> (x, fc list, sigma list) as numpy arrays."""
    rng = np.random.default_rng(seed)
    nan, inf = np.nan, np.inf
    t = np.arange(L)
    x = np.empty((R, L), F32)
    fc = [np.empty((R, L if c & 1 else 1), F32) for c in range(C)]
    sg = [np.empty((R, L if c & 2 else 1), F32) for c in range(C)]
    for r in range(R):
        kind = r % NKINDS
        base = (100 + 30 * np.sin(2 * np.pi * t / 97) + 3 * rng.standard_normal(L)).astype(F32)
        for c in range(C):
            fc[c][r] = 100 + 30 * np.sin(2 * np.pi * t[:fc[c].shape[1]] / 97) * (c & 1) + rng.uniform(-2, 2)
            sg[c][r] = np.exp(rng.uniform(0.5, 2.5)) * (1 + 0.3 * rng.random(sg[c].shape[1]))
        if kind == 0:                                         # negative values
            base = -base
            for c in range(C):
                fc[c][r] = -fc[c][r]
        elif kind == 1:                                       # heavy ties: integer counts, mostly zero
            base = rng.poisson(0.3, L).astype(F32)
            for c in range(C):
                fc[c][r] = rng.uniform(0, 1)
                sg[c][r] = np.exp(rng.uniform(-2.5, -0.2))    # sigma < 1: negative logarithms
        elif kind == 2:                                       # NaN runs, at either end too
            base[:max(1, L // 9)] = nan
            base[L - max(1, L // 11):] = nan
            for s in rng.integers(0, L, 3):
                base[s:s + max(1, L // 13)] = nan
        elif kind == 3:                                       # all missing: +inf everywhere, choice 0
            base[:] = nan
        elif kind == 4:                                       # +-inf samples do not count
            base[rng.integers(0, L, max(1, L // 8))] = inf
            base[rng.integers(0, L, max(1, L // 8))] = -inf
        elif kind == 5:                                       # a constant row some model gives sigma 0, others NaN
            base[:] = 42.0
            for c in range(C):
                fc[c][r] = 42.0 + rng.uniform(-1, 1)
                if c % 3 == 0:
                    sg[c][r] = 0.0
                elif c % 3 == 1:
                    sg[c][r] = nan
        elif kind == 6:                                       # misses far beyond the cap
            base[rng.integers(0, L, max(1, L // 5))] += 1e6
            base[rng.integers(0, L, max(1, L // 7))] = 3e38
        elif kind == 7:                                       # forecasts missing on some columns, either side of 2 n >= nx
            for c in range(C):
                if c & 1:
                    share = (0.3, 0.7)[(c >> 1) & 1] if L > 1 else 1.0
                    fc[c][r, rng.random(L) < share] = nan
                elif c & 2:
                    sg[c][r, rng.random(L) < 0.2] = nan
        elif kind == 8:                                       # tiny and huge sigmas
            for c in range(C):
                sg[c][r] = F32(10.0) ** rng.integers(-30, 30)
        x[r] = base
    return x, fc, sg


def _views(arrs, dev, offs):
    """Each [R, w] array as a column view at offset ``offs[i]`` of a wider
    tensor of odd width, so rows and operands differ in their 16-B alignment."""
    out = []
    for a, off in zip(arrs, offs):
        R, w = a.shape
        buf = torch.full((R, w + off + 5 - (w + off) % 2), float("nan"), device=dev)
        buf[:, off:off + w] = torch.from_numpy(a)
        out.append(buf[:, off:off + w])
    return out


def _kernel_check(L, C, R, off, dev, seed):
    x, fc, sg = _kernel_case(L, C, R, seed)
    score, n, nx = MI.ref_holdout_score(x, fc, sg, ZCAP)
    choice = MI.ref_auto_pick(score, n, nx, MARGIN)
    with np.errstate(divide="ignore", invalid="ignore"):
        maxln = np.stack([np.nanmax(np.where(np.isfinite(s) & (s > 0), np.abs(np.log(s.astype(np.float64))), 0), 1)
                          for s in sg], 1)
    tol = 4 * 2.0 ** -23 * np.maximum(1, np.maximum(np.where(np.isfinite(score), np.abs(score), 0), maxln))
    dist = _flip_distance(score, n, nx, MARGIN, choice)
    assert (dist > 2 * tol.max(1)).all(), (L, C, R, off, np.nonzero(dist <= 2 * tol.max(1))[0])
    # candidates 0-3 keep forecast and sigma at one alignment, the others differ: both read paths
    xs = _views([x], dev, [off])[0]
    fcs = _views(fc, dev, [(off + c) % 4 for c in range(C)])
    sgs = _views(sg, dev, [(off + c + (c >= 4)) % 4 for c in range(C)])
    g_score, g_n, g_nx, g_choice = (t.cpu().numpy() for t in MI.holdout_score(xs, fcs, sgs, ZCAP, MARGIN))
    np.testing.assert_array_equal(g_n, n)
    np.testing.assert_array_equal(g_nx, nx)
    np.testing.assert_array_equal(np.isinf(g_score), np.isinf(score))
    fin = np.isfinite(score)
    err = np.abs(g_score[fin].astype(np.float64) - score[fin])
    print(f"L {L} C {C} R {R} off {off}: max score error / tolerance {np.max(err / tol[fin], initial=0):.3f}")
    assert (err <= tol[fin]).all(), (L, C, R, off, float(np.max(err / tol[fin])))
    np.testing.assert_array_equal(g_choice, choice)


KERNEL_SHAPES = [(1, 6, 257), (3, 8, 257), (255, 6, 257), (256, 8, 257), (257, 1, 257), (257, 6, 1), (1441, 8, 257),
                 (1441, 6, 1), (1441, 1, 257)]


@pytest.mark.gpu
@pytest.mark.parametrize("L,C,R", KERNEL_SHAPES)
def test_gpu_holdout_score_matches_contract(cuda, L, C, R):
    for off in range(4):                                      # the held-out view starts at any column mod 4
        _kernel_check(L, C, R, off, cuda, seed=1000 * L + 10 * C + off)


@pytest.mark.gpu
def test_gpu_holdout_score_longest_row_and_refusals(cuda):
    _kernel_check(MI.ROBUST_LDS_KEYS, 6, 1, 1, cuda, seed=5)
    x = torch.zeros((1, MI.ROBUST_LDS_KEYS + 1), device=cuda)
    one = torch.ones((1, 1), device=cuda)
    with pytest.raises(ValueError):
        MI.holdout_score(x, [one], [one])
    with pytest.raises(ValueError):
        MI.holdout_score(x[:, :8], [one] * 9, [one] * 9)
    # an expanded tensor is one value per row, and no held-out sample at all is a row without a choice to make
    s, n, nx, ch = MI.holdout_score(x[:, :8], [one.expand(-1, 8)], [one[:, 0]])
    assert s.item() == 1.0 and n.item() == 8                  # ln 1 + |0 - 1| / 1 and nx.item() == 8 and ch.item() == 0
    s, n, nx, ch = MI.holdout_score(x[:, :0], [one], [one])
    assert math.isinf(s.item()) and n.item() == 0 and nx.item() == 0 and ch.item() == 0


@pytest.fixture(scope="module")
def fleet48():
    """Eight noisy copies of the six shapes, every second one with the
    incident, and the CPU reference's selection of them."""
    x = np.concatenate([six_rows(1, tile=4), six_rows(2, tile=4, incident=True)])
    choice, score, dist = _cpu_selection(x)
    return x, choice, dist


def test_fleet_of_six_shapes_picks_six_models(fleet48):
    x, choice, dist = fleet48
    assert (dist >= 1e-3).all(), dist
    np.testing.assert_array_equal(choice, np.arange(48) % 6)


@pytest.mark.gpu
def test_gpu_auto_select_matches_cpu(cuda, fleet48):
    x, choice, _ = fleet48
    got = zoo.auto_select(torch.from_numpy(x).to(cuda), x.shape[1], **ARGS)[0]
    np.testing.assert_array_equal(got.cpu().numpy(), choice)


@pytest.mark.gpu
def test_gpu_decision_is_the_chosen_models_own(cuda, fleet48):
    x, choice, _ = fleet48
    R, T = x.shape
    hist, cur = torch.from_numpy(x).to(cuda), torch.from_numpy(_current(x)).to(cuda)
    hor = torch.arange(1, cur.shape[1] + 1, device=cuda).repeat(R, 1)
    diff = (torch.arange(R, device=cuda) % 5 == 0).to(torch.int8)
    tb = _tables(R, cuda)
    dec = zoo.decide("auto_robust", hist, T, cur, hor, R, tb, diff, **ARGS)
    np.testing.assert_array_equal(dec.choice.cpu().numpy(), choice)
    assert (dec.count.cpu().numpy() >= 1).all()
    for ci, name in enumerate(zoo.AUTO_CANDIDATES):
        idx = torch.from_numpy(np.nonzero(choice == ci)[0]).to(cuda)
        sub = zoo.Tables(tb.thr[idx], tb.bound[idx], tb.minlb[idx], tb.pair_factor, tb.min_hist)
        own = zoo.decide(name, hist[idx].contiguous(), T, cur[idx].contiguous(), hor[idx], int(idx.numel()), sub,
                         diff[idx], **SINGLE)
        _decision_equal(dec, own, idx.cpu().numpy())
