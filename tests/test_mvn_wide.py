"""The joint detector's wide tier (K37, csrc/kernels/mvn_wide.hip): groups of
9 to 32 member rows against the fp64 definitions ref_mvn / ref_mvn_robust, the
zoo's routing, and the wrapper's argument checks."""
import functools

import numpy as np
import pytest
import torch

from foremast_amd.models import zoo
from foremast_amd.ops import misc as MI

CUTS = MI.mvn_cuts(3.0, 0.8, MI.MVN_WIDE_MAX_K)
MIN_N = 4
WIDE_K, WIDE_T, WIDE_N = (9, 16, 31, 32), (37, 259, 1027), (1, 30, 65)
# member scales over three decades; the largest product of two is 100, so that the rounding of an fp32 product
# sum (2^-24 of 100 = 6e-6) stays inside the covariance's atol of 1e-5
SCALES = np.array([10.0, 0.1, 1.0, 3.0, 0.01, 5.0, 1.0, 0.3])


def _unpack(words, n):
    w = np.ascontiguousarray(words).view(np.uint64)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :n].astype(bool)


@functools.lru_cache(maxsize=None)
def _case(K, T, n, incidents=False):
    """Two groups on scattered rows of a larger buffer (the other rows and the
    padding past T hold finite garbage).  Members are mixtures of independent
    noise with cond(R) <= 100; member 1 is constant; about 5 % of the columns
    have a NaN in a random member; with n >= 30 current point 1 moves the
    constant member and point 2 misses member 3.  ``incidents``: group 0 has
    three incident columns, group 1 has them in two thirds of its columns.
    Returns the inputs and the reference's outputs."""
    rng = np.random.default_rng(100 * K + T + 7 * n)
    G, Rb, ld = 2, 2 * K + 7, (T + 3) // 4 * 4 + 8
    hist = (rng.normal(size=(Rb, ld)) * 1e6).astype(np.float32)
    cur = rng.normal(size=(Rb, n)).astype(np.float32)
    rows = np.full((G, 32), -1, np.int32)
    rows[:, :K] = rng.permutation(Rb)[:G * K].reshape(G, K)
    sc = np.resize(SCALES, K)
    for g in range(G):
        A = np.eye(K) + rng.normal(size=(K, K)) * (0.3 / np.sqrt(K))
        Rp = A @ A.T
        assert np.linalg.cond(Rp / np.sqrt(np.outer(np.diag(Rp), np.diag(Rp)))) <= 100
        mean = 5 * sc + rng.normal(0, 3, K) * sc
        h = mean[:, None] + sc[:, None] * (A @ rng.normal(size=(K, T)))
        # current points well inside the cut, one in four far outside: few land next to it
        x = mean[:, None] + sc[:, None] * (A @ (rng.normal(size=(K, n)) * np.where(rng.random(n) < 0.25, 6.0, 0.6)))
        h[1], x[1] = mean[1], mean[1]
        if n >= 30:
            x[1, 1] = mean[1] + 1.0
            x[3, 2] = np.nan
        if incidents and g == 0:
            h[2, [5, T // 2, T - 2]] += 50 * sc[2]
        if incidents and g == 1:                             # each a minority of its member, together a majority
            h[0, 0::3] += 50 * sc[0]
            h[2, 1::3] -= 50 * sc[2]
        cols = rng.choice(T, max(1, round(0.05 * T)), replace=False)
        h[rng.integers(0, K, len(cols)), cols] = np.nan
        hist[rows[g, :K], :T] = h.astype(np.float32)
        cur[rows[g, :K]] = x.astype(np.float32)
    lowered = np.array([0, 1], np.uint8)
    if incidents:
        ref = MI.ref_mvn_robust(hist[:, :T], cur, rows, K, CUTS, lowered, MIN_N, MI.MVN_REJECT, 32)
    else:
        ref = MI.ref_mvn(hist[:, :T], cur, rows, K, CUTS, lowered, MIN_N)
    return hist, cur, rows, lowered, ref


def _compare(K, T, n, cuda, robust):
    """K12's GPU-against-host tolerances (tests/test_mvn_ops.py): N, k, count
    and valid exact, mean / covariance rtol 1e-4 atol 1e-5, distances rtol
    1e-3 atol 1e-3, flags exact away from the cut."""
    hist, cur, rows, lowered, ref = _case(K, T, n, robust)
    dev = [torch.from_numpy(a).to(cuda) for a in (hist, cur, rows, lowered)]
    if robust:
        got = MI.mvn_wide_robust(dev[0], T, dev[1], dev[2], K, CUTS, dev[3], MIN_N)
        assert ref[5][0] >= 3 and ref[5][1] == 0              # the planted columns; the breakdown guard
        np.testing.assert_array_equal(got[5].cpu().numpy(), ref[5])
    else:
        got = MI.mvn_wide(dev[0], T, dev[1], dev[2], K, CUTS, dev[3], MIN_N)
    rp, rd, rf, rc, rv = ref[:5]
    gp, gd, gf, gc, gv = (a.cpu().numpy() for a in got[:5])
    assert (rp[:, 0] >= K + 2).all() and (rp[:, 1] == K - 1).all() and (rv == 3).all()
    np.testing.assert_array_equal(gp[:, :2], rp[:, :2])
    np.testing.assert_array_equal(gv, rv)
    np.testing.assert_allclose(gp[:, 2:], rp[:, 2:], rtol=1e-4, atol=1e-5)
    np.testing.assert_array_equal(np.isnan(gd), np.isnan(rd))
    np.testing.assert_array_equal(np.isposinf(gd), np.isposinf(rd))
    if n >= 30:
        assert np.isposinf(rd[:, 1]).all() and np.isnan(rd[:, 2]).all()
    fin = np.isfinite(rd)
    np.testing.assert_allclose(gd[fin], rd[fin], rtol=1e-3, atol=1e-3)
    used = CUTS[lowered.astype(int), rp[:, 1].astype(int)][:, None]
    with np.errstate(invalid="ignore"):
        near = fin & (np.abs(rd - used) <= 1e-3 * np.abs(rd) + 1e-3)
    assert near.sum() <= 0.02 * rd.size
    gfl, rfl = _unpack(gf, n), _unpack(rf, n)
    np.testing.assert_array_equal(gfl[~near], rfl[~near])
    np.testing.assert_array_equal(gc, gfl.sum(1))
    assert np.abs(gc - rc).sum() <= near.sum()


@pytest.mark.gpu
@pytest.mark.parametrize("n", WIDE_N)
@pytest.mark.parametrize("T", WIDE_T)
@pytest.mark.parametrize("K", WIDE_K)
def test_gpu_mvn_wide_matches_reference(cuda, K, T, n):
    _compare(K, T, n, cuda, robust=False)


@pytest.mark.gpu
@pytest.mark.parametrize("n", WIDE_N)
@pytest.mark.parametrize("T", (259, 1027))
@pytest.mark.parametrize("K", (9, 32))
def test_gpu_mvn_wide_robust_matches_reference(cuda, K, T, n):
    _compare(K, T, n, cuda, robust=True)


def test_zoo_routes_jobs_of_more_than_eight_metrics_to_one_group():
    rows, ks, singles = zoo.mvn_groups([range(0, 9), range(9, 42), range(42, 76)], max_k=32)
    assert rows.shape == (4, 32) and ks.tolist() == [9, 32, 32, 2] and singles.tolist() == [41]
    assert rows[0, :9].tolist() == list(range(9)) and (rows[0, 9:] == -1).all() and rows[3, :2].tolist() == [74, 75]
    # a 12-metric job; the current point 1 is 1.5 sigma per metric (rms) off along the first principal direction.
    # With independent metrics d^2 = 27 / lambda_1 jointly (5.10 against the cut 4.97 for 12 members at 2.4 sigma)
    # and about 27 w / lambda within a chunk that holds the share w of the direction: the seed is one that
    # spreads it 59 % / 41 % over the chunks of 8 and 4 (3.94 against 4.33, 3.32 against 3.48).
    rng = np.random.default_rng(12)
    M, T, n, thr = 12, 20000, 3, 2.4
    sc = np.resize(SCALES, M)
    hist = (5 * sc[:, None] + sc[:, None] * rng.normal(size=(M, T))).astype(np.float32)
    h = hist.astype(np.float64)
    mu, sd = h.mean(1), h.std(1, ddof=1)
    u1 = np.linalg.eigh(np.corrcoef(h))[1][:, -1]
    cur = np.repeat(mu[:, None], n, 1)
    cur[:, 1] += 1.5 * np.sqrt(M) * u1 * sd
    tables = zoo.Tables(torch.full((M,), 3.0), torch.full((M,), 3, dtype=torch.int32), torch.full((M,), -1e30), 0.8, 10)
    args = ("multivariate_normal", torch.from_numpy(hist), T, torch.from_numpy(cur.astype(np.float32)),
            torch.ones((M, n), dtype=torch.int64), M, tables)
    joint = zoo.decide(*args, mvn_threshold=thr, mvn_max_members=32)
    assert (joint.flags == joint.flags[0]).all() and (joint.score == joint.score[0]).all()
    assert (joint.upper == MI.mvn_cuts(thr, 0.8, 32)[0, M]).all() and (joint.valid == 3).all()
    assert _unpack(joint.flags.numpy(), n).tolist() == [[False, True, False]] * M
    split = zoo.decide(*args, mvn_threshold=thr)                      # 8 + 4: neither chunk sees enough of it
    assert split.count.sum() == 0 and (split.upper[:8] == MI.mvn_cuts(thr, 0.8)[0, 8]).all()
    by_groups = zoo.decide(*args, mvn_threshold=thr, groups=zoo.mvn_groups([range(M)], max_k=32))
    assert torch.equal(by_groups.flags, joint.flags)


@pytest.mark.parametrize("K,width,ncut", [(8, 32, 33), (33, 32, 33), (16, 8, 33), (16, 32, 9)])
def test_mvn_wide_rejects_bad_arguments(K, width, ncut):
    hist, cur, low = torch.zeros(40, 64), torch.zeros(40, 4), torch.zeros(1, dtype=torch.uint8)
    rows = torch.arange(width, dtype=torch.int32)[None, :]
    cuts = MI.mvn_cuts(3.0, 1.0, ncut - 1)
    for fn in (MI.mvn_wide, MI.mvn_wide_robust):
        with pytest.raises(ValueError):
            fn(hist, 64, cur, rows, K, cuts, low, 10)
