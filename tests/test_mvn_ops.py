"""multivariate_normal (K12, csrc/kernels/mvn.hip): the cut table, the fp64
oracle against numpy, the contract's edge cases, the zoo entry point, the
case the joint model exists for, and the kernel against the oracle."""
import numpy as np
import pytest
import torch

from foremast_amd.models import zoo
from foremast_amd.ops import misc as MI

CUT_TABLE = {2: [2.0, 2.486, 2.8328, 3.117, 3.3636, 3.5845, 3.7864, 3.9735],
             3: [3.0, 3.4394, 3.7625, 4.0313, 4.2668, 4.4791, 4.674, 4.8554],
             10: [10.0, 10.2507, 10.4564, 10.6388, 10.8055, 10.9608, 11.107, 11.2459]}


def _rows(G, K, first=0):
    r = np.full((G, 8), -1, np.int32)
    r[:, :K] = first + np.arange(G * K).reshape(G, K)
    return r


def _unpack(words, n):
    w = np.ascontiguousarray(words).view(np.uint64)
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")
    return bits[:, :n].astype(bool)


def _correlated(rng, K, T, mean=None, scale=None):
    """K correlated Gaussian rows, mixed mildly enough that the correlation
    matrix stays well conditioned (smallest eigenvalue around 0.1 or more)."""
    A = rng.normal(size=(K, K)) * (0.5 / np.sqrt(K)) + np.eye(K)
    x = A @ rng.normal(size=(K, T))
    scale = np.ones(K) if scale is None else scale
    mean = np.zeros(K) if mean is None else mean
    return (x * scale[:, None] + mean[:, None]), A


# --------------------------------------------------------------------------- 1
def test_mvn_cuts_table():
    for thr, want in CUT_TABLE.items():
        c = MI.mvn_cuts(thr, 0.8)
        assert c.shape == (2, 9) and c.dtype == np.float32
        np.testing.assert_allclose(c[0, 1:], want, atol=1e-3)
        assert c[0, 1] == np.float32(thr) and c[1, 1] == np.float32(thr * 0.8)
        assert c[0, 0] == 0 and c[1, 0] == 0
        assert (np.diff(c[0]) > 0).all() and (np.diff(c[1]) > 0).all() and np.isfinite(c).all()
        np.testing.assert_allclose(c[1], MI.mvn_cuts(thr * 0.8, 1.0)[0], rtol=1e-6)


# --------------------------------------------------------------------------- 2
@pytest.mark.parametrize("K", [2, 3, 5, 8])
def test_ref_mvn_matches_numpy_cov_solve(K):
    rng = np.random.default_rng(10 + K)
    G, T, n = 6, 400, 12
    hist = np.zeros((G * K, T), np.float32)
    cur = np.zeros((G * K, n), np.float32)
    for g in range(G):
        mean, scale = rng.normal(5, 2, K), rng.uniform(0.5, 3, K)
        hist[g * K:(g + 1) * K] = _correlated(rng, K, T, mean, scale)[0]
        cur[g * K:(g + 1) * K] = mean[:, None] + scale[:, None] * rng.normal(0, 2, (K, n))
    cuts = MI.mvn_cuts(3.0, 0.8)
    params, dist, flags, cnt, valid = MI.ref_mvn(hist, cur, _rows(G, K), K, cuts, np.zeros(G, np.uint8), 10)
    iu = np.triu_indices(K)
    for g in range(G):
        h = hist[g * K:(g + 1) * K].astype(np.float64)
        x = cur[g * K:(g + 1) * K].astype(np.float64)
        mu, Cv = h.mean(1), np.cov(h)
        dx = x - mu[:, None]
        want = np.sqrt((dx * np.linalg.solve(Cv, dx)).sum(0))
        # the ridge shrinks d by at most ridge / (2 lambda_min(R)) relative: 2.5e-5 here, inside the rtol
        assert np.linalg.eigvalsh(np.corrcoef(h)).min() >= 0.02
        np.testing.assert_allclose(dist[g], want, rtol=1e-4)
        np.testing.assert_allclose(params[g, 2:2 + K], mu, rtol=1e-6, atol=1e-6)
        np.testing.assert_allclose(params[g, 2 + K:], Cv[iu], rtol=1e-5, atol=1e-6)
        assert params[g, 0] == T and params[g, 1] == K and valid[g] == 3
        np.testing.assert_array_equal(_unpack(flags, n)[g], dist[g] > cuts[0, K])
        assert cnt[g] == (dist[g] > cuts[0, K]).sum()
    if K == 2:
        bv = MI.ref_bivariate(hist[0::2], hist[1::2], cur[0::2], cur[1::2], 3.0)
        np.testing.assert_allclose(dist, bv[1], rtol=1e-4)


# --------------------------------------------------------------------------- 3
def _contract_case(K=3, T=60, n=4, seed=0):
    rng = np.random.default_rng(seed)
    hist = _correlated(rng, K, T, np.full(K, 10.0))[0].astype(np.float32)
    cur = np.full((K, n), 10.0, np.float32)
    return hist, cur, MI.mvn_cuts(3.0, 0.5)


def test_contract_nan_removes_the_column_for_all_members():
    hist, cur, cuts = _contract_case()
    hist[1, 5] = np.nan
    hist[2, 9] = np.inf
    p = MI.ref_mvn(hist, cur, _rows(1, 3), 3, cuts, np.zeros(1, np.uint8), 10)[0]
    keep = np.ones(60, bool)
    keep[[5, 9]] = False
    assert p[0, 0] == 58
    np.testing.assert_allclose(p[0, 2:5], hist[:, keep].astype(np.float64).mean(1), rtol=1e-6)
    np.testing.assert_allclose(p[0, 5:], np.cov(hist[:, keep].astype(np.float64))[np.triu_indices(3)], rtol=1e-5)


def test_contract_too_few_complete_columns_is_invalid():
    hist, cur, cuts = _contract_case(K=3, T=4)                       # N = K + 1
    cur[0, 0] = 1e6
    p, dist, flags, cnt, valid = MI.ref_mvn(hist, cur, _rows(1, 3), 3, cuts, np.zeros(1, np.uint8), 1)
    assert p[0, 0] == 4 and np.isnan(dist).all() and cnt[0] == 0 and not flags.any() and (valid[0] & 1) == 0
    hist5 = _contract_case(K=3, T=5)[0]                              # N = K + 2: just enough
    _, dist, _, cnt, valid = MI.ref_mvn(hist5, cur, _rows(1, 3), 3, cuts, np.zeros(1, np.uint8), 1)
    assert (valid[0] & 1) == 1 and np.isfinite(dist).all() and cnt[0] == 1
    _, dist, _, cnt, valid = MI.ref_mvn(hist5, cur, _rows(1, 3), 3, cuts, np.zeros(1, np.uint8), 6)   # min_hist
    assert (valid[0] & 1) == 0 and np.isnan(dist).all()


def test_contract_constant_member_is_dropped_and_may_not_move():
    hist, cur, cuts = _contract_case(K=3, T=200, n=3)
    hist[1] = 0.25
    cur[1] = 0.25
    sd = hist[[0, 2]].astype(np.float64).std(1, ddof=1)
    # point 0 sits between the cut for 2 live members and the cut for 3, along the first axis alone
    Cv = np.cov(hist[[0, 2]].astype(np.float64))
    mu = hist[[0, 2]].astype(np.float64).mean(1)
    mid = 0.5 * (cuts[0, 2] + cuts[0, 3])
    unit = np.sqrt(np.linalg.inv(Cv)[0, 0])                          # distance of a unit step on axis 0
    cur[0, 0] = mu[0] + mid / unit
    cur[2, 0] = mu[1]
    cur[1, 2] = 0.2500005                                            # the constant moved (2e-6 relative)
    p, dist, flags, cnt, valid = MI.ref_mvn(hist, cur, _rows(1, 3), 3, cuts, np.zeros(1, np.uint8), 10)
    assert p[0, 1] == 2 and sd.min() > 0
    np.testing.assert_allclose(dist[0, 0], mid, rtol=1e-4)
    f = _unpack(flags, 3)[0]
    assert f[0] and cuts[0, 2] < dist[0, 0] < cuts[0, 3]             # flagged by the cut for k = 2
    assert not f[1] and dist[0, 1] < cuts[0, 2]
    assert f[2] and np.isposinf(dist[0, 2]) and cnt[0] == 2
    hist[:] = 7.0                                                    # every member constant: k = 0, d = 0
    cur[:] = 7.0
    p, dist, flags, cnt, _ = MI.ref_mvn(hist, cur, _rows(1, 3), 3, cuts, np.zeros(1, np.uint8), 10)
    assert p[0, 1] == 0 and (dist == 0).all() and cnt[0] == 0


def test_contract_missing_current_member_and_lowered_row():
    hist, cur, cuts = _contract_case(K=3, T=200, n=3)
    mu = hist.astype(np.float64).mean(1)
    unit = np.sqrt(np.linalg.inv(np.cov(hist.astype(np.float64)))[0, 0])
    cur[:] = mu[:, None].astype(np.float32)
    cur[0, 0] = mu[0] + 0.75 * cuts[0, 3] / unit                     # between the lowered cut (x 0.5) and the cut
    cur[0, 1] = 1e6
    cur[2, 1] = np.nan                                               # far out, but a member is missing
    rows = np.concatenate([_rows(1, 3), _rows(1, 3)])
    _, dist, flags, cnt, valid = MI.ref_mvn(hist, cur, rows, 3, cuts, np.array([0, 1], np.uint8), 10)
    f = _unpack(flags, 3)
    assert np.isnan(dist[:, 1]).all() and not f[:, 1].any()
    assert not f[0].any() and cnt[0] == 0
    assert f[1, 0] and cnt[1] == 1 and cuts[1, 3] < dist[1, 0] < cuts[0, 3]
    assert (valid == 3).all()


def test_wrapper_rejects_bad_group_size():
    hist, cur, cuts = torch.zeros(18, 64), torch.zeros(18, 4), MI.mvn_cuts(3.0)
    rows = torch.from_numpy(_rows(2, 8))
    with pytest.raises(ValueError):
        MI.mvn(hist, 64, cur, rows, 9, cuts, torch.zeros(2, dtype=torch.uint8), 10)
    with pytest.raises(ValueError):
        MI.mvn(hist, 64, cur, rows, 1, cuts, torch.zeros(2, dtype=torch.uint8), 10)
    with pytest.raises(ValueError):
        MI.mvn(hist, 64, cur, rows + 100, 8, cuts, torch.zeros(2, dtype=torch.uint8), 10)


# --------------------------------------------------------------------------- 4
def _tables(M, thr=3.0, min_hist=10):
    return zoo.Tables(torch.full((M,), thr), torch.full((M,), 3, dtype=torch.int32), torch.full((M,), -1e30), 0.8,
                      min_hist)


def _fleet(S, M, T=300, n=8, seed=0):
    rng = np.random.default_rng(seed)
    hist = np.concatenate([_correlated(rng, M, T, rng.normal(5, 1, M))[0] for _ in range(S)]).astype(np.float32)
    cur = (hist[:, :n] + rng.normal(0, 1.5, (S * M, n))).astype(np.float32)
    return torch.from_numpy(hist), torch.from_numpy(cur), torch.ones((S * M, n), dtype=torch.int64)


def test_zoo_canonical_names():
    for name in ("mvn", "multivariate", "multivariate_normal", " MVN "):
        assert zoo.canonical(name) == "multivariate_normal"
    assert "multivariate_normal" in zoo.ALGORITHMS


def test_zoo_decide_rows_of_a_service_share_the_decision():
    S, M, n = 5, 4, 8
    hist, cur, hor = _fleet(S, M, n=n)
    dec = zoo.decide("mvn", hist, hist.shape[1], cur, hor, M, _tables(M))
    assert dec.count.sum() > 0
    for s in range(S):
        sl = slice(s * M, (s + 1) * M)
        assert (dec.flags[sl] == dec.flags[s * M]).all() and (dec.count[sl] == dec.count[s * M]).all()
        assert (dec.score[sl] == dec.score[s * M]).all() and (dec.valid[sl] == 3).all()
    cut = MI.mvn_cuts(3.0, 0.8)[0, M]
    assert (dec.upper == cut).all() and (dec.lower == 0).all()
    # a differing canary lowers the whole group's cut; an explicit joint threshold replaces the table's
    diff = torch.zeros(S * M, dtype=torch.int8)
    diff[5] = 1
    low = zoo.decide("mvn", hist, hist.shape[1], cur, hor, M, _tables(M), diff)
    assert (low.upper[4:8] == MI.mvn_cuts(3.0, 0.8)[1, M]).all() and (low.upper[:4] == cut).all()
    assert (low.count >= dec.count).all()
    wide = zoo.decide("mvn", hist, hist.shape[1], cur, hor, M, _tables(M), mvn_threshold=10.0)
    assert (wide.upper == MI.mvn_cuts(10.0, 0.8)[0, M]).all() and wide.count.sum() < dec.count.sum()


def test_zoo_decide_nine_metrics_is_eight_plus_a_single():
    S, M, n = 2, 9, 8
    hist, cur, hor = _fleet(S, M, n=n, seed=1)
    T = hist.shape[1]
    dec = zoo.decide("mvn", hist, T, cur, hor, M, _tables(M))
    for s in range(S):
        first, last = s * M, s * M + 8
        assert (dec.flags[first:last] == dec.flags[first]).all()
        assert (dec.upper[first:last] == MI.mvn_cuts(3.0, 0.8)[0, 8]).all()
        one = zoo.decide("moving_average_all", hist[last:last + 1], T, cur[last:last + 1], hor[last:last + 1], 1,
                         _tables(1))
        for k in ("flags", "count", "score", "upper", "lower"):
            torch.testing.assert_close(getattr(dec, k)[last:last + 1], getattr(one, k), equal_nan=True, rtol=0,
                                       atol=0)
    # a one-metric job is a single too
    h1, c1, o1 = hist[:3], cur[:3], hor[:3]
    a = zoo.decide("mvn", h1, T, c1, o1, 1, _tables(1))
    b = zoo.decide("moving_average_all", h1, T, c1, o1, 1, _tables(1))
    torch.testing.assert_close(a.flags, b.flags)
    torch.testing.assert_close(a.upper, b.upper)


# --------------------------------------------------------------------------- 5
def test_broken_relation_inside_every_band_is_caught_only_jointly():
    rng = np.random.default_rng(5)
    T, n = 2000, 5
    x1 = rng.normal(100, 4, T)
    hist = np.stack([x1, x1 + rng.normal(0, 0.4, T), rng.normal(0.5, 0.05, T), rng.normal(20, 2, T)]).astype(
        np.float32)
    mu, sd = hist.astype(np.float64).mean(1), hist.astype(np.float64).std(1)
    cur = np.repeat(mu[:, None], n, 1)
    cur[0, 2] = mu[0] + 1.5 * sd[0]                                  # both inside their own 3-sigma band,
    cur[1, 2] = mu[1] - 1.5 * sd[1]                                  # moving against their relation
    hist_t, cur_t = torch.from_numpy(hist), torch.from_numpy(cur.astype(np.float32))
    hor = torch.ones((4, n), dtype=torch.int64)
    ma = zoo.decide("moving_average_all", hist_t, T, cur_t, hor, 4, _tables(4))
    assert ma.count.sum() == 0
    mv = zoo.decide("multivariate_normal", hist_t, T, cur_t, hor, 4, _tables(4))
    f = _unpack(mv.flags.numpy(), n)
    assert f[:, 2].all() and f.sum() == 4 and (mv.count == 1).all()


# --------------------------------------------------------------------------- GPU: kernel vs oracle
G_GPU, MIN_N = 37, 4
GPU_K, GPU_T, GPU_N = (2, 3, 5, 8), (7, 259, 1027), (1, 30, 65)
STRIP = 2e-3


def _gpu_case(K, T, n, G=G_GPU, seed=3):
    """hist [Rb, ld] (ld padded past T, the padding finite garbage), cur
    [Rb, n], rows a random permutation of the larger buffer, 5 % NaN, and the
    special groups of the issue: 0 a fully-NaN member, 1 a constant member,
    2 a constant member that moves, 3 offset 1e4 / sigma 1, 4 a 10-sigma
    linear trend."""
    rng = np.random.default_rng(1000 * K + T + 7 * n + seed)
    Rb, ld = G * K + 13, (T + 3) // 4 * 4 + 8
    hist = rng.normal(0, 1, (Rb, ld)).astype(np.float32) * 1e6        # rows no group uses, and the padding
    cur = rng.normal(0, 1, (Rb, n)).astype(np.float32)
    perm = rng.permutation(Rb)[:G * K].reshape(G, K).astype(np.int32)
    rows = np.full((G, 8), -1, np.int32)
    rows[:, :K] = perm
    scales = np.array([100.0, 0.1, 1.0, 30.0, 0.01, 5.0, 1.0, 1000.0])[:K]
    for g in range(G):
        mean = rng.normal(0, 3, K) * scales + 5 * scales
        sc = scales
        if g == 3:
            mean, sc = np.full(K, 1e4), np.ones(K)
        h, A = _correlated(rng, K, T, mean, sc)
        if g == 4:
            h[0] += np.linspace(0, 10 * h[0].std(), T)
        # current points well inside the cut, one in four far outside: few land next to it
        spread = np.where(rng.random(n) < 0.25, 6.0, 0.6)
        x = mean[:, None] + sc[:, None] * (A @ (rng.normal(0, 1, (K, n)) * spread))
        if g == 4:
            x[0] += 10 * h[0].std() / 2
        if g in (1, 2):
            j = 0 if g == 1 else K - 1
            c = 0.0 if g == 1 else 3.5
            h[j], x[j] = c, c
            if g == 2:
                x[j, 0] = 4.0
        h = h.astype(np.float32)
        x = x.astype(np.float32)
        h[rng.random((K, T)) < 0.05] = np.nan
        x[rng.random((K, n)) < 0.03] = np.nan
        if g == 0:
            h[1] = np.nan
        hist[perm[g], :T] = h
        cur[perm[g]] = x
    lowered = (rng.random(G) < 0.3).astype(np.uint8)
    return hist, ld, cur, rows, lowered


def _strip_mask(dist, params, lowered, cuts):
    used = cuts[lowered.astype(int), params[:, 1].astype(int)][:, None]
    present = np.isfinite(dist)
    with np.errstate(invalid="ignore"):
        near = present & (np.abs(dist - used) <= STRIP * used)
    return present, near


@pytest.mark.parametrize("K", GPU_K)
def test_reference_distances_keep_clear_of_the_cut(K):
    """The seeds of the GPU cases, checked with the oracle alone: at most 1 %
    of the present points lie within 2e-3 x cut of the cut, and the cases do
    exercise what they are for."""
    cuts = MI.mvn_cuts(3.0, 0.8)
    for T in GPU_T:
        for n in GPU_N:
            hist, ld, cur, rows, lowered = _gpu_case(K, T, n)
            p, dist, flags, cnt, valid = MI.ref_mvn(hist[:, :T], cur, rows, K, cuts, lowered, MIN_N)
            present, near = _strip_mask(dist, p, lowered, cuts)
            assert near.sum() <= 0.01 * max(present.sum(), 1), (K, T, n, near.sum(), present.sum())
            assert (valid[0] & 1) == 0
            if T == 7:
                assert ((valid & 1) == 0).all() if K == 8 else True
                if K == 5:
                    ok = (valid & 1) == 1
                    assert ok.any() and (p[ok, 0] == 7).all()            # valid only with every column complete
            else:
                assert ((valid[1:] & 1) == 1).all()
                assert p[1, 1] == K - 1 and p[2, 1] == K - 1 and (p[3:, 1] == K).all()
                if n > 1 and np.isfinite(cur[rows[2, :K], 0]).all():
                    assert np.isposinf(dist[2, 0])
                if n >= 30:
                    assert 0 < cnt.sum() < present.sum()


def _compare_gpu(K, T, n, cuda, G=G_GPU):
    cuts = MI.mvn_cuts(3.0, 0.8)
    hist, ld, cur, rows, lowered = _gpu_case(K, T, n, G)
    t = lambda a: torch.from_numpy(a)
    ref = MI.mvn(t(hist), T, t(cur), t(rows), K, cuts, t(lowered), MIN_N)
    got = MI.mvn(t(hist).to(cuda), T, t(cur).to(cuda), t(rows).to(cuda), K, cuts, t(lowered).to(cuda), MIN_N)
    rp, rd, rf, rc, rv = (a.numpy() for a in ref)
    gp, gd, gf, gc, gv = (a.cpu().numpy() for a in got)
    np.testing.assert_array_equal(gp[:, :2], rp[:, :2])               # N and k
    np.testing.assert_array_equal(gv, rv)
    has = rp[:, 0] > 1
    np.testing.assert_allclose(gp[has, 2:], rp[has, 2:], rtol=1e-4, atol=1e-5)
    if G > 3 and has[3]:
        # offset 1e4, sigma 1: the sums run on x - shift, which fp32 forms exactly for |x - shift| << |x|,
        # so the covariance error does not grow with the offset; the mean is off by at most the rounding
        # of the fp32 output, one ulp = 2^-23 |mu| (1.2e-7 |mu|), on top of the atol above
        mu = rp[3, 2:2 + K]
        assert (np.abs(gp[3, 2:2 + K] - mu) <= 2.0 ** -23 * np.abs(mu) + 1e-5).all()
        np.testing.assert_allclose(gp[3, 2 + K:], rp[3, 2 + K:], rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(np.isnan(gd), np.isnan(rd))
    np.testing.assert_array_equal(np.isposinf(gd), np.isposinf(rd))
    fin = np.isfinite(rd)
    np.testing.assert_allclose(gd[fin], rd[fin], rtol=1e-3, atol=1e-3)
    present, near = _strip_mask(rd, rp, lowered, cuts)
    assert near.sum() <= 0.01 * max(present.sum(), 1)
    gfl, rfl = _unpack(gf, n), _unpack(rf, n)
    np.testing.assert_array_equal(gfl[~near], rfl[~near])
    assert np.abs(gc - rc).sum() <= near.sum()
    np.testing.assert_array_equal(gc, gfl.sum(1))


@pytest.mark.gpu
@pytest.mark.parametrize("T", GPU_T)
@pytest.mark.parametrize("K", GPU_K)
def test_gpu_mvn_matches_reference(cuda, K, T):
    for n in GPU_N:
        _compare_gpu(K, T, n, cuda)


@pytest.mark.gpu
def test_gpu_mvn_production_row_length(cuda):
    _compare_gpu(8, 10080, 10, cuda, G=4)


@pytest.mark.gpu
@pytest.mark.parametrize("K,T,n", [(3, 259, 30), (8, 1027, 65), (5, 7, 30)])
def test_gpu_mvn_tail_shift_form_matches_reference(cuda, monkeypatch, K, T, n):
    """The kernel's other moment form (shift from the row tails, one centred
    sweep) holds the same bounds; group 0's tail has no complete column and
    takes the mean sweep."""
    monkeypatch.setattr(MI, "MVN_FORM", 1 - MI.MVN_FORM)
    _compare_gpu(K, T, n, cuda)
    _compare_gpu(8, 10080, 10, cuda, G=4)


@pytest.mark.gpu
def test_gpu_mvn_wrapper_rejects_misaligned_rows(cuda):
    """Bad arguments stop in the wrapper: nothing is launched."""
    hist = torch.zeros((16, 66), device=cuda)                         # row stride not a multiple of 4
    cur = torch.zeros((16, 4), device=cuda)
    rows = torch.from_numpy(_rows(2, 8)).to(cuda)
    low = torch.zeros(2, dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError):
        MI.mvn(hist, 64, cur, rows, 8, MI.mvn_cuts(3.0), low, 10)
    with pytest.raises(ValueError):
        MI.mvn(torch.zeros((16, 68), device=cuda)[:, 1:], 64, cur, rows, 8, MI.mvn_cuts(3.0), low, 10)
    with pytest.raises(ValueError):
        MI.mvn(torch.zeros((16, 64), device=cuda), 64, cur, rows, 9, MI.mvn_cuts(3.0), low, 10)
