"""CanaryScorer(model="robust_moving_average_all"): the resident tick with
median / MAD history statistics.  On the CPU the scorer equals the zoo's robust
op path; on the GPU the cached resident tick equals the uncached ``score`` and
K13 over several ticks with writes in between, and the CPU scorer on inputs
that keep every current point clear of the band edges."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from foremast_amd.config import BrainConfig
from foremast_amd.engine.resident import ResidentHistory
from foremast_amd.engine.scorer import CanaryScorer
from foremast_amd.models import zoo
from foremast_amd.ops import canary as C
from foremast_amd.ops import misc as MI

ROBUST = "robust_moving_average_all"
ALIASES = ["error5xx", "latency", "traffic", "error4xx", "cpu", "memory", "tomcat_threads", "jvm_heap"]
T = 300
N_CUR = 10


def _history(P, seed):
    """P rows of N(1000, 5) with 2 % missing samples: far from the
    min_lower_bound clamp at every threshold in use (<= 10 sigma, doubled)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((P, T)) * 5 + 1000).astype(np.float32)
    x[rng.random(x.shape) < 0.02] = np.nan
    return x


def _windows(hist, M, n_base, seed):
    """Current and baseline windows for the logical rows ``hist`` [R, T].
    Ordinary points lie within 0.9 sigma of the row's median (every band is at
    least 0.8 * 2 sigma wide); the anomalies injected into every 3rd row sit
    2 to 3 thresholds out, above and below, so no point comes near a band edge
    whichever threshold applies.  The baseline holds the current window's own
    samples repeated (every test: p = 1 or not applicable), shifted by
    4 sigma on the rows of odd services (p tiny; a lone service: on its odd
    rows): no p-value sits near the pairwise threshold, so CPU and GPU lower
    the same rows' thresholds."""
    rng = np.random.default_rng(seed)
    R = hist.shape[0]
    c, s, _ = MI.ref_robust_stats(hist, T)
    c = np.where(np.isfinite(c), c, np.float32(1000)).astype(np.float32)
    s = np.where(np.isfinite(s), s, np.float32(5)).astype(np.float32)
    thr = np.array([BrainConfig().rule_for(ALIASES[r % M]).threshold for r in range(R)], np.float32)
    cur = (c[:, None] + rng.uniform(-0.9, 0.9, (R, N_CUR)) * s[:, None]).astype(np.float32)
    hot = np.arange(R) % 3 == 0
    out = (2 + rng.random(R)) * thr * s
    cur[hot, 3] = (c + out)[hot]
    cur[hot, 7] = (c - out)[hot]
    cur[1::5, 9] = np.nan                                     # a missing current sample
    base = None
    if n_base:
        reps = -(-n_base // N_CUR)
        base = np.tile(cur, (1, reps))[:, :n_base].copy()
        odd = ((np.arange(R) // M) if R > M else np.arange(R)) % 2 == 1   # (one service: its odd rows)
        base[odd] += 4 * s[odd, None]
    return cur, base


def _clear_of_edges(cur, stats):
    """No current point within relative 1e-4 of either bound (a NaN bound --
    a row without history -- has no edge to be near)."""
    up, lo = stats[:, 2:3], stats[:, 3:4]
    with np.errstate(invalid="ignore"):
        near = (np.abs(cur - up) <= 1e-4 * np.abs(up)) | (np.abs(cur - lo) <= 1e-4 * np.abs(lo))
    return not near.any()


# ---------------------------------------------------------------------- CPU
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("n_base", [0, 50])
def test_cpu_robust_score_equals_the_zoo_path(S, M, n_base):
    aliases = ALIASES[:M]
    hist = _history(S * M, 10 * S + M)
    cur, base = _windows(hist, M, n_base, 3)
    h, c_ = torch.from_numpy(hist), torch.from_numpy(cur)
    b = torch.from_numpy(base) if base is not None else None
    sc = CanaryScorer(aliases, device="cpu", model=ROBUST)
    o = sc.score(h, b, c_, T)
    diff = C.pairwise_tests(c_, b, sc.pcfg)[2] if b is not None else None
    tables = zoo.make_tables(aliases, sc.cfg, "cpu")
    hor = torch.ones(cur.shape, dtype=torch.int64)
    dec = zoo.decide(ROBUST, h, T, c_, hor, M, tables, diff)
    packed = C.service_reduce(dec.count, dec.score, dec.valid.to(torch.int32), M)
    assert torch.equal(o.decide.flags, dec.flags) and int(dec.count.sum()) > 0
    assert torch.equal(o.decide.count, dec.count)
    assert torch.equal(o.decide.valid, dec.valid.to(torch.int32))
    assert torch.equal(o.packed, packed)
    if diff is not None:
        assert torch.equal(o.diff, diff) and (S == 1 or bool(diff.any()))
    np.testing.assert_array_equal(o.decide.stats[:, 2].numpy(), dec.upper[:, 0].numpy())
    np.testing.assert_array_equal(o.decide.stats[:, 3].numpy(), dec.lower[:, 0].numpy())


def test_cpu_history_gate_and_empty_rows():
    hist = _history(4, 1)
    hist[1] = np.nan                                          # no history at all
    hist[2, 5:] = np.nan                                      # fewer samples than min_historical_points
    cur, _ = _windows(hist, 1, 0, 2)
    cfg = BrainConfig()
    cfg.min_historical_points = 10
    cur[:, 0] = 5000.0
    o = CanaryScorer(["cpu"], cfg, device="cpu", model=ROBUST).score(torch.from_numpy(hist), None,
                                                                      torch.from_numpy(cur), T)
    assert o.decide.valid.tolist() == [3, 2, 2, 3]
    assert o.decide.count.tolist()[1:3] == [0, 0] and o.decide.count[0] > 0
    assert o.decide.score.tolist()[1:3] == [0.0, 0.0]
    assert o.packed[:, 0].tolist() == [1.0, 2.0, 2.0, 1.0]
    assert np.isnan(o.decide.stats[1].numpy()).all()


def test_unknown_model_and_unsupported_mode():
    with pytest.raises(ValueError):
        CanaryScorer(["cpu"], device="cpu", model="nonsense")
    with pytest.raises(ValueError):
        CanaryScorer(["cpu"], device="cpu", model=ROBUST, mode="fused")
    assert CanaryScorer(["cpu"], device="cpu").model == "moving_average_all"


# ------------------------------------------------------- second-cache bookkeeping
def _cpu_store(n):
    st = ResidentHistory(40, "cpu")
    rows, _ = st.rows_for([("k", i) for i in range(n)], owner=("ns", "app"))
    rng = np.random.default_rng(1)
    st.write_static(rows, [rng.normal(size=40).astype(np.float32) for _ in rows], np.zeros(len(rows)))
    return st, rows


def _mark(cache, tag):
    cache.valid.fill_(tag)
    cache.ticked(tag)


def _cleared(cache):
    return torch.nonzero(cache.valid == 0).flatten().tolist()


def test_second_cache_follows_every_writer():
    st, rows = _cpu_store(12)
    assert st.rcache is not None and st.rcache is not st.cache
    assert len(st.rcache) == st.buf.shape[0] and _cleared(st.rcache) == list(range(len(st.rcache)))
    v = st.view()
    assert v.rcache is st.rcache and v.cache is st.cache and st.view_until(None).rcache is st.rcache
    # separate bookkeeping: the two caches are ticked by different models
    _mark(st.rcache, 40)
    assert not st.rcache.expect_miss(40, 12) and st.cache.expect_miss(40, 12)
    _mark(st.cache, 40)
    w = rows[[2, 5, 7]]
    st.write_static(w, [np.ones(40, np.float32)] * 3, np.zeros(3))
    assert _cleared(st.rcache) == sorted(int(r) for r in w) == _cleared(st.cache)
    assert st.rcache.dirty == 3 and st.cache.dirty == 3
    st.rcache.ticked(40)
    assert st.rcache.dirty == 0 and st.cache.dirty == 3
    _mark(st.rcache, 40)
    assert st.release([("k", 3), ("k", 9)]) == 2
    assert _cleared(st.rcache) == sorted(int(rows[i]) for i in (3, 9))
    # growing keeps the words and the statistics
    _mark(st.rcache, 40)
    st.rcache.stats.copy_(torch.arange(len(st.rcache) * 3, dtype=torch.float32).reshape(-1, 3))
    n0, keep_v, keep_s = len(st.rcache), st.rcache.valid.clone(), st.rcache.stats.clone()
    st.rows_for([("g", i) for i in range(n0 + 50)])
    assert len(st.rcache) == st.buf.shape[0] > n0
    assert torch.equal(st.rcache.valid[:n0], keep_v) and torch.equal(st.rcache.stats[:n0], keep_s)
    assert not st.rcache.valid[n0:].any()
    # a sliding store has neither cache
    sl = ResidentHistory(40, "cpu", sliding=True, slack=8, capacity=16)
    assert sl.rcache is None and sl.view().rcache is None


def test_second_cache_cleared_by_checkpoint_restore():
    from foremast_amd.engine.fp_history import load_history
    st, rows = _cpu_store(12)
    _mark(st.rcache, 40)
    vals = torch.arange(3 * 40, dtype=torch.float32).reshape(3, 40)
    t = {"static.values": vals, "static.last_t": torch.zeros(3, dtype=torch.float64),
         "static.nlen": torch.full((3,), 40, dtype=torch.int64)}
    meta = {"static.keys": [["k", 1], ["k", 4], ["r", 0]], "static.owners": [["ns", "app"]] * 3}
    fp = SimpleNamespace(static=st, sliding=None, cycle=0, history_s=0.0)
    assert load_history(fp, t, meta, now=0.0) == 3
    assert _cleared(st.rcache) == sorted([int(rows[1]), int(rows[4]), st.slot[("r", 0)]])


def test_invalidate_history_reaches_the_robust_cache_only():
    st, rows = _cpu_store(6)
    sc = CanaryScorer(["cpu", "memory"], device="cpu", model=ROBUST)
    cur = torch.zeros((6, 4))
    o = sc.score_resident(st.view(), torch.from_numpy(rows.astype(np.int32)), cur, None)
    want = MI.ref_robust_stats(st.buf.numpy()[rows], st.view().T)
    np.testing.assert_array_equal(o.decide.stats[:, 0].numpy(), want[0])
    _mark(st.rcache, 40)
    _mark(st.cache, 40)
    sc.invalidate_history()
    assert not st.rcache.valid.any() and st.rcache.dirty >= len(st.rcache)
    assert st.rcache.expect_miss(40, 6)
    assert bool(st.cache.valid.all()) and st.cache.dirty == 0  # the mean/std cache is another scorer's


# ---------------------------------------------------------------------- GPU
def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _k13(buf, rm, Tv):
    g = buf.index_select(0, rm.long()).contiguous()
    c, s, n = MI.robust_stats(g, Tv)
    return torch.stack([c, s, n.float()], 1)


def _rows_for(M, target):
    return -(-target // M) * M                                # the smallest multiple of M >= target


@pytest.mark.gpu
@pytest.mark.parametrize("M", [1, 3, 8])
@pytest.mark.parametrize("target", [8, 520])
def test_gpu_resident_robust_ticks(cuda, M, target):
    """Four ticks over a static store: cold, all hits, after ``write_static``
    on 3 rows and a ``release`` (n_cur + n_base = 60), then a wide one (310
    pooled points).  R is the smallest multiple of M that reaches 8 or 520
    (M = 3: 9 and 522); two logical rows repeat physical ones.

    After every tick ``hs`` and the cache entries of the mapped rows are K13
    of those rows as bits -- nothing but K18 may write the robust cache, in
    particular no mean / std of a launch handed the wrong cache -- and packed /
    count / flags equal the uncached ``score``; against the CPU scorer: stats
    to rtol 2e-5, atol 1e-5, counts, flags and service status equal, on inputs
    asserted clear of the band edges on the CPU oracle."""
    aliases = ALIASES[:M]
    R = _rows_for(M, target)
    S = R // M
    P = R + 3
    st = ResidentHistory(T, cuda)
    keys = [("k", i) for i in range(P)]
    prow, _ = st.rows_for(keys, owner=("ns", "app"))
    hist = _history(P, 100 * M + target)
    st.write_static(prow, list(hist), np.zeros(P))
    lg = np.random.default_rng(5).permutation(P)[:R]          # logical row -> key
    lg[-2:] = lg[:2]
    rm_h = prow[lg].astype(np.int32)
    rm = torch.from_numpy(rm_h).to(cuda)
    sc = CanaryScorer(aliases, device=cuda, model=ROBUST)
    cold = CanaryScorer(aliases, device=cuda, model=ROBUST)
    off = CanaryScorer(aliases, device=cuda, model=ROBUST, hist_cache=False)
    cpu = CanaryScorer(aliases, device="cpu", model=ROBUST)

    def tick(k, n_base, want_miss):
        cur, base = _windows(hist[lg], M, n_base, 50 + k)
        cd, bd = torch.from_numpy(cur).to(cuda), torch.from_numpy(base).to(cuda)
        view = st.view()
        assert view.T == T and view.rcache is st.rcache
        assert st.rcache.expect_miss(T, R) == want_miss, k
        o = sc.score_resident(view, rm, cd, bd)
        torch.cuda.synchronize()
        assert st.rcache.dirty == 0 and st.rcache.T == T
        assert _bits(o.hs, _k13(st.buf, rm, T)), k
        assert (st.rcache.valid[rm.long()] == T).all()
        assert _bits(st.rcache.stats[rm.long()], o.hs), k     # what the cache holds is the robust triple
        g = st.buf.index_select(0, rm.long()).contiguous()
        u = cold.score(g, bd, cd, T)
        for name in ("packed",):
            assert _bits(getattr(o, name), getattr(u, name)), (k, name)
        assert torch.equal(o.decide.count, u.decide.count) and torch.equal(o.decide.flags, u.decide.flags), k
        torch.testing.assert_close(o.pvals, u.pvals, equal_nan=True)
        w = off.score_resident(view, rm, cd, bd)
        assert _bits(w.hs, o.hs) and _bits(w.packed, o.packed) and torch.equal(w.decide.flags, o.decide.flags), k
        assert torch.equal(w.diff, o.diff)
        ref = cpu.score(torch.from_numpy(hist[lg]), torch.from_numpy(base), torch.from_numpy(cur), T)
        assert _clear_of_edges(cur, ref.decide.stats.numpy()), k
        assert int(ref.decide.count.sum()) > 0 and bool(ref.diff.any()) and not bool(ref.diff.all())
        np.testing.assert_array_equal(o.diff.cpu().numpy(), ref.diff.numpy())
        np.testing.assert_allclose(o.decide.stats.cpu().numpy(), ref.decide.stats.numpy(), rtol=2e-5, atol=1e-5)
        np.testing.assert_array_equal(o.decide.count.cpu().numpy(), ref.decide.count.numpy())
        np.testing.assert_array_equal(o.decide.flags.cpu().numpy(), ref.decide.flags.numpy())
        np.testing.assert_array_equal(o.decide.valid.cpu().numpy(), ref.decide.valid.numpy())
        np.testing.assert_array_equal(o.packed.cpu().numpy()[:, [0, 2, 3]], ref.packed.numpy()[:, [0, 2, 3]])

    tick(1, 50, True)                                         # cold
    tick(2, 50, False)                                        # every row cached
    # three rows rewritten (one of them mapped twice), one mapped row released
    w = [int(lg[0]), int(lg[5]), int(lg[R // 2])]
    new = _history(3, 77)
    st.write_static(prow[w], list(new), np.zeros(3))
    hist[w] = new
    gone = int(lg[3])
    assert st.release([keys[gone]]) == 1
    hist[gone] = np.nan
    assert st.rcache.dirty == 4
    assert (st.rcache.valid[torch.from_numpy(prow[w + [gone]].astype(np.int64)).to(cuda)] == 0).all()
    tick(3, 50, R < 64)                                       # 4 stale rows: a miss-shaped launch only when R is small
    assert int(st.rcache.valid.count_nonzero()) == len(np.unique(rm_h))   # the rows no one maps stay invalid
    tick(4, 300, False)                                       # wider than a wave-sorted 256


@pytest.mark.gpu
def test_gpu_invalidate_and_unsupported_forms(cuda):
    M, R = 3, 9
    aliases = ALIASES[:M]
    st = ResidentHistory(T, cuda)
    prow, _ = st.rows_for([("k", i) for i in range(R)], owner=("ns", "app"))
    hist = _history(R, 4)
    st.write_static(prow, list(hist), np.zeros(R))
    rm = torch.from_numpy(prow.astype(np.int32)).to(cuda)
    cur, base = _windows(hist, M, 50, 6)
    cd, bd = torch.from_numpy(cur).to(cuda), torch.from_numpy(base).to(cuda)
    sc = CanaryScorer(aliases, device=cuda, model=ROBUST)
    a = sc.score_resident(st.view(), rm, cd, bd).packed.clone()
    # a write behind the store's back, then invalidate_history: recomputed
    st.buf[int(prow[0])] -= 500.0
    sc.invalidate_history()
    assert st.rcache.expect_miss(T, R)
    o = sc.score_resident(st.view(), rm, cd, bd)
    assert _bits(o.hs, _k13(st.buf, rm, T)) and float(o.hs[0, 0]) < 600
    assert not _bits(o.packed, a)                             # row 0's window now sits far above its band
    g = st.buf.index_select(0, rm.long()).contiguous()
    for call in (lambda: sc.capture(g, bd, cd, T), lambda: sc.split_launchers(g, bd, cd, T),
                 lambda: sc.capture_front(g, bd, cd, T), lambda: sc.front_only(g, bd, cd, T)):
        with pytest.raises(ValueError):
            call()
