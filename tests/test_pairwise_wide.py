"""The pairwise rank tests beyond the wave kernel's 1,024 pooled points: the
sufficient-statistics contract in numpy (``ref.pairwise_suff``), K21
(``fm_pairwise_suff_wide``) against it, the three-tier routing of
``C.pairwise_tests`` and the resident scorer over an 800 + 800 window."""
import functools

import numpy as np
import pytest
import torch

from foremast_amd.engine.resident import ResidentHistory
from foremast_amd.engine.scorer import CanaryScorer
from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref
from foremast_amd.ops._lib import LIB, ptr, stream_of

from boundary import diff_boundary
from test_robust_tick import ALIASES, T, _clear_of_edges, _history

SHAPES = [(513, 512), (1, 1100), (1100, 1), (1025, 1024), (3000, 2049), (4096, 4096), (8191, 1)]
R = 9
INT_COLS = [0, 1, 2, 3, 4, 6, 7, 12, 13]     # counts, rank sums (half-integers), tie terms, npos, nzero


@functools.lru_cache(maxsize=None)
def _rows(n_cur, n_base):
    """R rows of rounded normals (ties, and both zeros: round(-0.04, 1) is
    -0.0); row 2 an error count 0..3, row 3 constant, row 4 with 3 % NaN,
    row 5 without a baseline, row 6 unrounded."""
    rng = np.random.default_rng(21)
    cur = np.round(rng.normal(0, 1, (R, n_cur)), 1)
    base = np.round(rng.normal(0.3, 1.2, (R, n_base)), 1)
    cur[2], base[2] = rng.integers(0, 4, n_cur), rng.integers(0, 4, n_base)
    cur[3], base[3] = 7.0, 7.0
    cur[4, rng.random(n_cur) < 0.03] = np.nan
    base[4, rng.random(n_base) < 0.03] = np.nan
    base[5] = np.nan
    cur[6], base[6] = rng.normal(0, 1, n_cur), rng.normal(0.3, 1.2, n_base)
    cur, base = cur.astype(np.float32), base.astype(np.float32)
    cur.setflags(write=False)
    base.setflags(write=False)
    return cur, base


@functools.lru_cache(maxsize=None)
def _suff(n_cur, n_base):
    s = ref.pairwise_suff(*_rows(n_cur, n_base))
    s.setflags(write=False)
    return s


@functools.lru_cache(maxsize=None)
def _oracle(n_cur, n_base, min_points):
    mins = (min_points,) * 3 if min_points else (20, 20, 5)
    return ref.pairwise_tests(*_rows(n_cur, n_base), 63, 0, 0.05, *mins)


# ---------------------------------------------------------------------- CPU
@pytest.mark.parametrize("n_cur,n_base", SHAPES)
def test_reference_suff_reproduces_the_oracle_statistics(n_cur, n_base):
    """What the 14 numbers imply equals the oracle's statistics (rtol 1e-6:
    ``S`` is rounded to fp32), with every gate at one point so that each
    statistic exists wherever its sample does; the gates' counts are exact."""
    cur, base = _rows(n_cur, n_base)
    s = _suff(n_cur, n_base)
    assert s.shape == (R, 14) and s.dtype == np.float64
    _, S, _ = _oracle(n_cur, n_base, 1)
    n1, n2, nw, r1, rplus, npos, nzero = s[:, 0], s[:, 1], s[:, 2], s[:, 3], s[:, 6], s[:, 12], s[:, 13]
    fc, fb = np.isfinite(cur), np.isfinite(base)
    npair = min(n_cur, n_base)
    ok = fc[:, :npair] & fb[:, :npair]
    d = cur[:, :npair] - base[:, :npair]
    np.testing.assert_array_equal(n1, fc.sum(1))
    np.testing.assert_array_equal(n2, fb.sum(1))
    np.testing.assert_array_equal(nw, (ok & (d != 0)).sum(1))
    np.testing.assert_array_equal(nw + nzero, ok.sum(1))
    both = (n1 > 0) & (n2 > 0)
    np.testing.assert_array_equal(np.isfinite(S[:, 0]), both)
    np.testing.assert_allclose((r1 - n1 * (n1 + 1) / 2)[both], S[both, 0], rtol=1e-6)
    np.testing.assert_allclose(s[both, 5], S[both, 3], rtol=1e-6)
    has = nw > 0
    np.testing.assert_array_equal(np.isfinite(S[:, 1]), has)
    np.testing.assert_allclose(np.minimum(rplus, nw * (nw + 1) / 2 - rplus)[has], S[has, 1], rtol=1e-6)
    blocks = nw + nzero > 0
    np.testing.assert_array_equal(np.isfinite(S[:, 5]), blocks)
    q = np.where(has, (2 * npos - nw) ** 2 / np.maximum(nw, 1), 0.0)
    np.testing.assert_allclose(q[blocks], S[blocks, 5], rtol=1e-6, atol=1e-12)
    # the rows built to stress the integers
    n = n1 + n2
    assert s[3, 4] == n[3] ** 3 - n[3] and s[3, 5] == 0.0 and s[3, 10] == 0.0     # one tie run of n
    assert s[5, 1] == 0 and s[5, 5] == 0.0 and s[5, 9] == 0.0 and s[5, 2] == 0      # no baseline
    assert s[2, 4] > (n[2] / 4) ** 3                                               # four huge runs


def test_reference_suff_signed_zeros_tie():
    cur = np.array([[-0.0, 1.0, 2.0, 5.0]], np.float32)
    base = np.array([[0.0, 3.0, 4.0]], np.float32)
    s = ref.pairwise_suff(cur, base)[0]
    assert s[4] == 6.0                                   # the two zeros are one run of 2: 2^3 - 2
    assert s[3] == 1.5 + 3 + 4 + 7                       # the current sample's ranks
    assert (s[2], s[12], s[13]) == (2, 0, 1)             # d = -0.0 counts as a zero pair
    assert s[6] == 0.0 and s[7] == 6.0                   # |d| = 2, 2: both negative, one run
    np.testing.assert_allclose(s[5], 5 / 12, rtol=1e-15)  # |a1/4 - a2/3| is largest behind x = 2: 3/4 - 1/3
    cpu = C.pairwise_suff_wide(torch.from_numpy(cur), torch.from_numpy(base))
    np.testing.assert_array_equal(cpu.numpy()[0], s)


def _wide_batch():
    """Left-packed rows padded to 5000 + 5000 columns."""
    rng = np.random.default_rng(7)
    widths = [(50, 50)] * 4 + [(400, 300)] * 2 + [(700, 700)] * 2 + [(3000, 3000)] * 2 + [(5000, 5000)]
    cur = np.full((len(widths), 5000), np.nan, np.float32)
    base = np.full((len(widths), 5000), np.nan, np.float32)
    for r, (a, b) in enumerate(widths):
        cur[r, :a] = np.round(rng.normal(0, 1, a), 1)
        base[r, :b] = np.round(rng.normal(0.2, 1.1, b), 1)
    cur[7, 10] = np.nan                      # a gap inside a row stays a gap
    return cur, base, widths


def test_routing_tiers_on_the_host():
    """The tier of every row of the routed batch, from the used widths alone,
    and the half-the-cap rule of a bucket whose common width breaks the cap."""
    _, _, widths = _wide_batch()
    lc = torch.tensor([w[0] for w in widths])
    lb = torch.tensor([w[1] for w in widths])
    every = torch.ones(len(widths), dtype=torch.bool)
    fit = C._bucket(lc, lb, every, C.PAIRWISE_MAX)
    wide = C._bucket(lc, lb, ~fit, C.PAIRWISE_WIDE_MAX)
    assert fit.tolist() == [True] * 6 + [False] * 5
    assert wide.tolist() == [False] * 6 + [True] * 4 + [False]
    # a bucket whose common width breaks the cap keeps the rows within half of it per side
    lc2, lb2 = torch.tensor([8000, 100, 4096, 4000]), torch.tensor([100, 8000, 4096, 100])
    assert C._bucket(lc2, lb2, torch.ones(4, dtype=torch.bool), C.PAIRWISE_WIDE_MAX).tolist() == [False, False, True, True]
    assert C.PAIRWISE_WIDE_MAX == 8192 and set(C.route_rows()) == {"wave", "wide", "oracle"}


# ---------------------------------------------------------------------- GPU
def _check_suff(got, want, cur, base):
    """Every integer equal, D the same quotient (rtol 1e-12), the fp64 moments
    to rtol 1e-9 (means: atol 1e-9 max|x|)."""
    print("max |diff| per column:", np.abs(got - want).max(0))
    np.testing.assert_array_equal(got[:, INT_COLS], want[:, INT_COLS])
    np.testing.assert_allclose(got[:, 5], want[:, 5], rtol=1e-12, atol=0)
    amax = [np.nanmax(np.abs(np.where(np.isfinite(x), x, np.nan)), initial=0.0) for x in (cur, base)]
    np.testing.assert_allclose(got[:, 8], want[:, 8], rtol=1e-9, atol=1e-9 * amax[0])
    np.testing.assert_allclose(got[:, 9], want[:, 9], rtol=1e-9, atol=1e-9 * amax[1])
    np.testing.assert_allclose(got[:, 10:12], want[:, 10:12], rtol=1e-9, atol=0)


@pytest.mark.gpu
@pytest.mark.parametrize("n_cur,n_base", SHAPES)
def test_gpu_suff_wide_is_exact(cuda, n_cur, n_base):
    """K21 against the numpy contract: every integer equal, D the same quotient
    (rtol 1e-12), the fp64 moments to rtol 1e-9 (means: atol 1e-9 max|x|)."""
    cur, base = _rows(n_cur, n_base)
    want = _suff(n_cur, n_base)
    got = C.pairwise_suff_wide(torch.tensor(cur, device=cuda), torch.tensor(base, device=cuda)).cpu().numpy()
    _check_suff(got, want, cur, base)


@pytest.mark.gpu
def test_gpu_suff_wide_from_an_unaligned_view(cuda):
    """Rows that start at column 1 of odd-stride buffers: 4-byte alignment only."""
    n_cur, n_base = 3000, 2049
    cur, base = _rows(n_cur, n_base)
    views = []
    for x in (cur, base):
        n = x.shape[1]
        buf = torch.full((R, n + 2 + (n + 1) % 2), float("nan"), device=cuda)
        view = buf[:, 1:1 + n]
        view.copy_(torch.tensor(x))
        assert view.data_ptr() % 16 == 4 and view.stride(0) % 2 == 1
        views.append(view)
    got = C.pairwise_suff_wide(*views).cpu().numpy()
    want = _suff(n_cur, n_base)
    _check_suff(got, want, cur, base)


@pytest.mark.gpu
@pytest.mark.parametrize("n_cur,n_base", SHAPES)
def test_gpu_wide_pvalues_match_the_oracle(cuda, n_cur, n_base):
    """K21 + the p-value kernel through ``C.pairwise_tests`` at the edge
    shapes (every row on the wide route): NaN pattern, p-values at the
    tolerance of test_gpu_pairwise_matches_reference, decisions equal (no row
    of the oracle's lies at the decision boundary)."""
    cur, base = _rows(n_cur, n_base)
    P0, S0, d0 = _oracle(n_cur, n_base, 0)
    assert diff_boundary(P0, 63, 0.05).sum() == 0
    C.reset_route_rows()
    pv, st, d = C.pairwise_tests(torch.tensor(cur, device=cuda), torch.tensor(base, device=cuda))
    pv, st, d = pv.cpu().numpy(), st.cpu().numpy(), d.cpu().numpy()
    # (row 5 has no baseline and row 4 may end in a gap: their used widths can fit the wave kernel)
    routes = C.route_rows()
    assert routes["oracle"] == 0 and routes["wide"] >= R - 2 and routes["wide"] + routes["wave"] == R
    np.testing.assert_array_equal(np.isnan(pv), np.isnan(P0))
    np.testing.assert_allclose(np.nan_to_num(pv), np.nan_to_num(P0), rtol=2e-4, atol=2e-6)
    np.testing.assert_allclose(np.nan_to_num(st[:, [0, 1, 3, 5]]), np.nan_to_num(S0[:, [0, 1, 3, 5]]), rtol=1e-5,
                               atol=1e-5)
    np.testing.assert_array_equal(d, d0)


@pytest.mark.gpu
def test_gpu_suff_wide_rejects_more_than_the_cap(cuda):
    """8,193 pooled columns: an error from the op and from the entry point,
    and nothing launched (the output keeps its fill)."""
    cur = torch.zeros((2, 8192), device=cuda)
    base = torch.ones((2, 1), device=cuda)
    with pytest.raises(ValueError):
        C.pairwise_suff_wide(cur, base)
    suff = torch.full((2, C.SUFF), -1.0, dtype=torch.float64, device=cuda)
    fn = LIB.load().fm_pairwise_suff_wide
    rc = fn(ptr(cur), cur.stride(0), 8192, ptr(base), base.stride(0), 1, 2, ptr(suff), stream_of(cur))
    assert rc == 1                                        # hipErrorInvalidValue
    torch.cuda.synchronize()
    assert bool((suff == -1.0).all())
    with pytest.raises(RuntimeError):
        LIB.call("fm_pairwise_suff_wide", ptr(cur), cur.stride(0), 8192, ptr(base), base.stride(0), 1, 2, ptr(suff),
                 stream_of(cur))
    # one column fewer is the cap, any split
    got = C.pairwise_suff_wide(cur[:, :8191], base)
    assert got[:, 0].tolist() == [8191.0, 8191.0] and got[:, 1].tolist() == [1.0, 1.0]


@pytest.mark.gpu
def test_gpu_routing_and_values(cuda, monkeypatch):
    """Rows of five used widths in one batch padded to 5000 + 5000: the first
    two widths on the wave kernel, 700 + 700 and 3000 + 3000 on K21, only
    5000 + 5000 on the oracle, and every row's values equal the oracle's."""
    cur, base, widths = _wide_batch()
    cfg = C.PairwiseConfig("ALL")
    P0, S0, d0 = ref.pairwise_tests(cur, base, *cfg.mask_and_combine(), cfg.p_threshold, 20, 20, 5)
    assert diff_boundary(P0, 63, 0.05).sum() == 0
    seen = []
    oracle = ref.pairwise_tests

    def recording(c, b, *a):
        seen.append((np.array(c), np.array(b)))
        return oracle(c, b, *a)

    monkeypatch.setattr(ref, "pairwise_tests", recording)
    C.reset_route_rows()
    pv, st, d = C.pairwise_tests(torch.from_numpy(cur).to(cuda), torch.from_numpy(base).to(cuda), cfg)
    assert C.route_rows() == {"wave": 6, "wide": 4, "oracle": 1}
    assert len(seen) == 1 and seen[0][0].shape == (1, 5000) and seen[0][1].shape == (1, 5000)
    np.testing.assert_array_equal(seen[0][0][0], cur[-1])
    np.testing.assert_array_equal(seen[0][1][0], base[-1])
    pv, d = pv.cpu().numpy(), d.cpu().numpy()
    np.testing.assert_array_equal(np.isnan(pv), np.isnan(P0))
    np.testing.assert_allclose(np.nan_to_num(pv), np.nan_to_num(P0), rtol=2e-4, atol=2e-6)
    np.testing.assert_array_equal(d, d0)
    # the wide tier switched off: the parent's two routes
    monkeypatch.setattr(C, "PAIRWISE_WIDE_MAX", C.PAIRWISE_MAX)
    C.reset_route_rows()
    C.pairwise_tests(torch.from_numpy(cur).to(cuda), torch.from_numpy(base).to(cuda), cfg)
    assert C.route_rows() == {"wave": 6, "wide": 0, "oracle": 5}


N_WIDE = 800


def _wide_windows(hist, M, model, seed):
    """test_robust_tick's windows at 800 + 800 points: ordinary points within
    0.9 sigma of the row's centre, anomalies 2 to 3 thresholds out in every 3rd
    row, the baseline the current window itself (every test p = 1 or not
    applicable), shifted by 4 sigma on the rows of odd services (p tiny)."""
    from foremast_amd.config import BrainConfig
    from foremast_amd.ops import misc as MI
    rng = np.random.default_rng(seed)
    Rr = hist.shape[0]
    if model == "robust_moving_average_all":
        c, s, _ = MI.ref_robust_stats(hist, T)
    else:
        c, s = np.nanmean(hist.astype(np.float64), 1), np.nanstd(hist.astype(np.float64), 1)
    c, s = c.astype(np.float32), s.astype(np.float32)
    thr = np.array([BrainConfig().rule_for(ALIASES[r % M]).threshold for r in range(Rr)], np.float32)
    cur = (c[:, None] + rng.uniform(-0.9, 0.9, (Rr, N_WIDE)) * s[:, None]).astype(np.float32)
    hot = np.arange(Rr) % 3 == 0
    out = (2 + rng.random(Rr)) * thr * s
    cur[hot, 3] = (c + out)[hot]
    cur[hot, 707] = (c - out)[hot]
    cur[1::5, 9] = np.nan
    base = cur.copy()
    odd = (np.arange(Rr) // M) % 2 == 1
    base[odd] += 4 * s[odd, None]
    return cur, base


@pytest.mark.gpu
@pytest.mark.parametrize("model", ["moving_average_all", "robust_moving_average_all"])
def test_gpu_resident_tick_with_a_wide_window(cuda, monkeypatch, model):
    """``score_resident`` over a static store with an 800 + 800 window equals
    the same scorer on CPU tensors (test_robust_tick's comparisons), and the
    GPU tick never calls the host oracle: the rows run K21."""
    M, S = 8, 2
    Rr = S * M
    aliases = ALIASES[:M]
    st = ResidentHistory(T, cuda)
    prow, _ = st.rows_for([("k", i) for i in range(Rr)], owner=("ns", "app"))
    hist = _history(Rr, 808)
    st.write_static(prow, list(hist), np.zeros(Rr))
    rm = torch.from_numpy(prow.astype(np.int32)).to(cuda)
    cur, base = _wide_windows(hist, M, model, 8)
    sc = CanaryScorer(aliases, device=cuda, model=model)
    cpu = CanaryScorer(aliases, device="cpu", model=model)
    ref_o = cpu.score(torch.from_numpy(hist), torch.from_numpy(base), torch.from_numpy(cur), T)
    assert _clear_of_edges(cur, ref_o.decide.stats.numpy())
    assert int(ref_o.decide.count.sum()) > 0 and bool(ref_o.diff.any()) and not bool(ref_o.diff.all())
    assert diff_boundary(ref_o.pvals.numpy(), 63, 0.05).sum() == 0

    def no_oracle(*a, **k):
        raise AssertionError("the host oracle was called for an 800 + 800 window")

    C.reset_route_rows()
    with monkeypatch.context() as m:
        m.setattr(ref, "pairwise_tests", no_oracle)
        o = sc.score_resident(st.view(), rm, torch.from_numpy(cur).to(cuda), torch.from_numpy(base).to(cuda))
        torch.cuda.synchronize()
    assert C.route_rows() == {"wave": 0, "wide": Rr, "oracle": 0}
    np.testing.assert_array_equal(np.isnan(o.pvals.cpu().numpy()), np.isnan(ref_o.pvals.numpy()))
    np.testing.assert_allclose(np.nan_to_num(o.pvals.cpu().numpy()), np.nan_to_num(ref_o.pvals.numpy()), rtol=2e-4,
                               atol=2e-6)
    np.testing.assert_array_equal(o.diff.cpu().numpy(), ref_o.diff.numpy())
    np.testing.assert_allclose(o.decide.stats.cpu().numpy(), ref_o.decide.stats.numpy(), rtol=2e-5, atol=1e-5)
    np.testing.assert_array_equal(o.decide.count.cpu().numpy(), ref_o.decide.count.numpy())
    np.testing.assert_array_equal(o.decide.flags.cpu().numpy(), ref_o.decide.flags.numpy())
    np.testing.assert_array_equal(o.decide.valid.cpu().numpy(), ref_o.decide.valid.numpy())
    np.testing.assert_array_equal(o.packed.cpu().numpy()[:, [0, 2, 3]], ref_o.packed.numpy()[:, [0, 2, 3]])
