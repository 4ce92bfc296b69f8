"""K18 (fm_robust_stats_cached): K13's median / MAD statistics over the rows
of a resident history store, kept per physical row in a row-statistics cache.
Cold launches equal K13 bit for bit in both launch forms; hits copy the cache
and read no history; a wrong hint or another view length costs time, never
correctness."""
import numpy as np
import pytest
import torch

from foremast_amd.engine.resident import RowStatsCache
from foremast_amd.ops import misc as MI

from test_robust_ops import _check


def _rows(P, T, seed):
    """P physical rows of length T: row 0 all NaN, 1 constant (the MAD = 0
    fallback), 2 NaN / +-inf scattered, 3 two-valued, 4 all negative, then
    mixed-sign noise with every 7th row carrying missing samples."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((P, T)) * 5).astype(np.float32)
    x[0] = np.nan
    if P > 1:
        x[1] = 42.0
    if P > 2:
        x[2, rng.random(T) < 0.3] = np.nan
        x[2, rng.random(T) < 0.1] = np.inf
        x[2, rng.random(T) < 0.1] = -np.inf
    if P > 3:
        x[3] = np.where(rng.random(T) < 0.6, -1.5, 2.5)
    if P > 4:
        x[4] = -np.abs(x[4]) - 1
    x[7::7][rng.random(x[7::7].shape) < 0.1] = np.nan
    return x


def _rowmap(P, R, seed):
    """R logical rows over P physical ones: every physical row at least once
    when R >= P, the rest duplicates, shuffled."""
    rng = np.random.default_rng(seed)
    rm = np.concatenate([rng.permutation(P)[:min(P, R)], rng.integers(0, P, max(0, R - P))])
    return rng.permutation(rm).astype(np.int32)


def _store(x, off, dev, pad=1e9):
    """The rows on the device with their base ``off`` floats past a 16-B
    boundary (K18, like K13, peels up to 3 samples) and garbage past column T."""
    P, T = x.shape
    ld = T + 4
    flat = torch.full((P * ld + 8,), pad, dtype=torch.float32, device=dev)
    assert flat.data_ptr() % 16 == 0
    h = flat[off:off + P * ld].view(P, ld)
    h[:, :T] = torch.from_numpy(x).to(dev)
    return h


def _k13(h, rm, T):
    g = h.index_select(0, rm.long()).contiguous()
    c, s, n = MI.robust_stats(g, T)
    return torch.stack([c, s, n.float()], 1)


def _k18(h, T, rm, cache, miss):
    c, s, n = MI.robust_stats_cached(h, T, rm, cache, expect_miss=miss)
    return torch.stack([c, s, n.float()], 1)


def _same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


# ---------------------------------------------------------------------- CPU
def test_cpu_op_is_the_contract_over_the_mapped_rows():
    x = _rows(9, 37, 1)
    rm = np.array([3, 3, 0, 8, 1, 7, 2, 2, 2, 5, 4, 6], np.int32)
    cache = RowStatsCache(9, "cpu")
    c, s, n = MI.robust_stats_cached(torch.from_numpy(x), 37, torch.from_numpy(rm), cache)
    rc, rs, rn = MI.ref_robust_stats(x[rm], 37)
    assert np.array_equal(c.numpy(), rc, equal_nan=True) and np.array_equal(s.numpy(), rs, equal_nan=True)
    assert n.dtype == torch.int32 and n.tolist() == rn.tolist()
    assert not cache.valid.any()                              # the CPU path ignores the cache
    c2, _, _ = MI.robust_stats_cached(torch.from_numpy(x), 37, None, None)
    assert np.array_equal(c2.numpy(), MI.ref_robust_stats(x, 37)[0], equal_nan=True)
    with pytest.raises(Exception):
        MI.robust_stats_cached(torch.from_numpy(x), 37, torch.tensor([9], dtype=torch.int32), None)


# ---------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 5, 37, 1000])
@pytest.mark.parametrize("R", [1, 7, 513, 1100])
def test_gpu_cold_equals_k13_bit_for_bit(cuda, T, R):
    """An empty cache, both hints: out == fm_robust_stats of the gathered
    rows as bits, and every mapped entry carries the tag T afterwards.  R = 513
    is more than one 512-thread scan pass of a workgroup when the grid is one
    workgroup (blocks = 1 below), 1100 spreads over several workgroups."""
    P = max(1, min(R, 300))
    x = _rows(P, T, 10 * T + R)
    rm_h = _rowmap(P, R, R)
    rm = torch.from_numpy(rm_h).to(cuda)
    for off in range(4):
        h = _store(x, off, cuda)
        want = _k13(h, rm, T)
        for miss in (False, True):
            cache = RowStatsCache(P, cuda)
            got = _k18(h, T, rm, cache, miss)
            assert _same_bits(got, want), (T, R, off, miss)
            v = cache.valid.cpu().numpy()
            assert (v[np.unique(rm_h)] == T).all() and (np.delete(v, np.unique(rm_h)) == 0).all()
    # one workgroup scanning every row: R = 513 takes a second pass, R = 1100 a third
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    cache = RowStatsCache(P, cuda)
    out = torch.empty((R, 3), dtype=torch.float32, device=cuda)
    LIB.call("fm_robust_stats_cached", ptr(h), h.stride(0), T, R, ptr(out), ptr(rm), ptr(cache.stats),
             ptr(cache.valid), 0, 1, stream_of(h))
    assert _same_bits(out, want)


@pytest.mark.gpu
def test_gpu_global_memory_path(cuda):
    T, P = MI.ROBUST_LDS_KEYS + 4, 3
    x = _rows(P, T, 5)
    x[0, 17] = 3.0                                            # (not all missing: three rows, three kinds)
    h = _store(x, 1, cuda)
    rm = torch.tensor([2, 0, 1], dtype=torch.int32, device=cuda)
    want = _k13(h, rm, T)
    for miss in (False, True):
        cache = RowStatsCache(P, cuda)
        assert _same_bits(_k18(h, T, rm, cache, miss), want), miss
        assert (cache.valid == T).all()
    assert _same_bits(_k18(h, T, rm, cache, False), want)     # and the hits


@pytest.mark.gpu
def test_gpu_longest_lds_row(cuda):
    """T = ROBUST_LDS_KEYS, the launch with the most LDS in the family, on a
    view that starts at column 1 of an odd-stride buffer (the key array takes
    its extra quad): cold in the scan form (every row a miss) and with no
    cache, against ref_robust_stats."""
    T, R = MI.ROBUST_LDS_KEYS, 3
    x = _rows(R, T, 6)
    x[0, 17] = 3.0                                            # (not all missing: three rows, three kinds)
    buf = np.full((R, T + 3), 1e9, np.float32)
    buf[:, 1:1 + T] = x
    view = torch.from_numpy(buf).to(cuda)[:, 1:]
    assert view.data_ptr() % 16 == 4 and view.stride(0) % 2 == 1
    _check(MI.robust_stats_cached(view, T, None, RowStatsCache(R, cuda), expect_miss=False), x, T, "scan form")
    _check(MI.robust_stats_cached(view, T, None, None), x, T, "no cache")


@pytest.mark.gpu
def test_gpu_hits_do_not_read_history(cuda):
    P, T, R = 40, 37, 90
    x = _rows(P, T, 2)
    h = _store(x, 0, cuda)
    rm_h = _rowmap(P, R, 4)
    rm = torch.from_numpy(rm_h).to(cuda)
    cache = RowStatsCache(P, cuda)
    want = _k18(h, T, rm, cache, None)                        # cold (the cache's own hint: miss)
    assert _same_bits(want, _k13(h, rm, T))
    times = np.bincount(rm_h, minlength=P)
    sent = np.flatnonzero(times > 1)[:2].tolist() + np.flatnonzero(times == 1)[:1].tolist()
    assert len(sent) == 3                                     # two physical rows mapped twice or more, one once
    keep = cache.stats.clone()
    for p in sent:
        cache.stats[p] = torch.tensor([1000.0 + p, -7.0, 3.0], device=cuda)
    got = _k18(h, T, rm, cache, False)
    hit = np.isin(rm_h, sent)
    exp = want.clone()
    exp[torch.from_numpy(hit).to(cuda)] = cache.stats[rm.long()[torch.from_numpy(hit).to(cuda)]]
    assert _same_bits(got, exp)                               # the sentinels, on exactly those logical rows
    assert (got[torch.from_numpy(hit).to(cuda), 1] == -7.0).all()
    cache.touch(torch.tensor(sent, device=cuda))
    assert cache.dirty == 3
    assert _same_bits(_k18(h, T, rm, cache, None), want)      # recomputed ...
    assert _same_bits(cache.stats[torch.from_numpy(np.unique(rm_h)).to(cuda)],
                      keep[torch.from_numpy(np.unique(rm_h)).to(cuda)])   # ... and the cache repaired
    assert (cache.valid[torch.tensor(sent, device=cuda)] == T).all()


@pytest.mark.gpu
def test_gpu_wrong_hints_and_tags(cuda):
    P, T, R = 300, 37, 1100
    x = _rows(P, T + 3, 8)
    h = _store(x, 2, cuda)
    rm = torch.from_numpy(_rowmap(P, R, 9)).to(cuda)
    cache = RowStatsCache(P, cuda)
    cold = _k18(h, T, rm, cache, True)
    assert _same_bits(cold, _k13(h, rm, T))
    assert _same_bits(_k18(h, T, rm, cache, True), cold)      # "miss" over a fully valid cache
    cache.invalidate()
    torch.cuda.synchronize()
    assert not cache.valid.any()
    assert _same_bits(_k18(h, T, rm, cache, False), cold)     # "hit" over a fully invalid cache
    assert (cache.valid == T).all()
    # another view length: every tag differs, every row is selected again
    cache.stats.fill_(-1.0)
    got = _k18(h, T + 3, rm, cache, False)
    assert _same_bits(got, _k13(h, rm, T + 3)) and (cache.valid == T + 3).all()
    assert not (cache.stats[:, 2] == -1.0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("T,R", [(37, 513), (1000, 37)])
def test_gpu_against_numpy(cuda, T, R):
    """The bounds tests/test_robust_ops.py holds K13 to, against
    ref_robust_stats: centre and n equal, sigma equal where MAD > 0 and within
    rtol 1e-6 on the fp64-mean fallback; cold, then from the cache."""
    P = min(R, 100)
    x = _rows(P, T, T + R)
    rm_h = _rowmap(P, R, 3)
    h = _store(x, 3, cuda)
    cache = RowStatsCache(P, cuda)
    for miss in (True, False):
        got = MI.robust_stats_cached(h, T, torch.from_numpy(rm_h).to(cuda), cache, expect_miss=miss)
        _check(got, x[rm_h], T, ("k18", T, R, miss))
