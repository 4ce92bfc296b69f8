"""Baseline cache of the front kernel's pairwise role (fm_tick_front_bc,
csrc/include/fm_pairwise.h PwBaseCache): whether a row hits its entry, misses
it or the launch has no cache at all, the outputs are what the separate
kernels give without any cache -- fm_pairwise_suff (all 14 ``suff`` columns
as raw fp64 bits) and fm_pvalues_only (``pvals``, ``pstats``).  They run the
same pw_compute / eval_test code, so every comparison is rtol = atol = 0.
Every output is NaN-filled before each launch, and every word of the pairwise
row queue and of the history queue must be zero again after each launch.

The entries themselves are checked too: what a launch may and may not write
(hits write nothing, a miss rewrites its own row, shapes without a cache
kernel touch no word), and -- by corrupting ``sorted`` -- that a hit really
takes the sorted baseline from the cache."""
import ctypes
import gc

import pytest
import torch

from foremast_amd.ops import canary as C

T, RMAX = 64, 1030
WINDOWS = {"50x50": (50, 50), "64x64": (64, 64), "1x64": (1, 64), "64x1": (64, 1), "10x3": (10, 3),
           "k1": (10, 10), "k4": (130, 100)}
SPLIT = ("50x50", "64x64", "1x64", "64x1")       # the shapes the cache serves: both <= 64, more than 64 together
ROWS = (1, 5, 203, 1030)
NPS = (0, 2, 8)
QS = (0, 8, 64)
MIN = 2                                          # min_mw / min_wil / min_kru
ALIASES = ["error5xx", "latency", "traffic", "error4xx"]
# baseline rows with a content of their own
ROW_NAN, ROW_CONST, ROW_INF, ROW_ZEROS = 9, 10, 11, 12


def _inputs(n_cur, n_base, seed):
    """As test_front_dynamic's: rounded samples (ties within and across the
    samples, zero differences), a few NaNs, plus the special baseline rows."""
    g = torch.Generator().manual_seed(seed)
    cur = torch.round(torch.randn(RMAX, n_cur, generator=g) * 4.0) / 2.0
    base = torch.round(torch.randn(RMAX, n_base, generator=g) * 4.0) / 2.0 + 0.5 * (torch.arange(RMAX) % 3)[:, None]
    cur[2, : n_cur // 2] = float("nan")
    base[4, n_base // 2] = float("nan")
    cur[7] = base[7, :n_cur] if n_cur <= n_base else cur[7]
    base[ROW_NAN] = float("nan")                 # n2 = 0
    base[ROW_CONST] = 1.5
    base[ROW_INF, 0] = float("inf")
    base[ROW_INF, n_base - 1] = float("-inf")
    base[ROW_ZEROS, 0] = 0.0
    if n_base > 1:
        base[ROW_ZEROS, 1] = -0.0
    return cur, base


def _oracle(cur, base, n_cur, n_base):
    """The separate kernels over RMAX rows of (cur, base), no cache anywhere."""
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    dev, st = cur.device, stream_of(cur)
    suff = torch.full((RMAX, C.SUFF), float("nan"), dtype=torch.float64, device=dev)
    pvals = torch.full((RMAX, C.N_TESTS), float("nan"), device=dev)
    pstats = torch.full((RMAX, C.N_TESTS), float("nan"), device=dev)
    LIB.call("fm_pairwise_suff", ptr(cur), cur.stride(0), n_cur, ptr(base), base.stride(0), n_base, RMAX, ptr(suff), 0,
             st)
    LIB.call("fm_pvalues_only", ptr(suff), RMAX, MIN, MIN, MIN, ptr(pvals), ptr(pstats), st)
    torch.cuda.synchronize()
    return suff, pvals, pstats


class _Cache:
    def __init__(self, dev, rows=RMAX):
        self.raw = torch.zeros((rows, 64), dtype=torch.int32, device=dev)
        self.sorted = torch.zeros((rows, 64), dtype=torch.int32, device=dev)
        self.stats = torch.zeros((rows, 4), dtype=torch.int32, device=dev)

    def tensors(self):
        return self.raw, self.sorted, self.stats

    def clear(self):
        for t in self.tensors():
            t.zero_()

    def snap(self):
        return tuple(t.clone() for t in self.tensors())

    def changed_rows(self, snap):
        """Rows with any word of their entry different from ``snap``."""
        ch = torch.zeros(self.raw.shape[0], dtype=torch.bool, device=self.raw.device)
        for t, s in zip(self.tensors(), snap):
            ch |= (t != s).any(dim=1)
        return set(ch.nonzero().flatten().tolist())


class _Data:
    """One window shape: inputs for RMAX rows, the oracle's outputs (computed
    once; rows are independent, so R rows are the first R of them), work
    buffers and queues."""

    def __init__(self, dev, n_cur, n_base, seed):
        from foremast_amd.engine.resident import RowStatsCache
        g = torch.Generator().manual_seed(seed + 100)
        self.h = (torch.randn(RMAX, T, generator=g) * 3.0 + 10.0).to(dev)
        cur, base = _inputs(n_cur, n_base, seed)
        self.cur, self.base = cur.to(dev), base.to(dev)
        self.n_cur, self.n_base = n_cur, n_base
        self.suff, self.pvals, self.pstats = _oracle(self.cur, self.base, n_cur, n_base)
        self.o_suff = torch.empty_like(self.suff)
        self.o_pvals, self.o_pstats = torch.empty_like(self.pvals), torch.empty_like(self.pstats)
        self.o_hs = torch.empty((RMAX, 3), device=dev)
        self.queue = torch.zeros(8 * 32 + 64, dtype=torch.int32, device=dev)
        self.pq = torch.zeros(64 * 32, dtype=torch.int32, device=dev)
        self.hcache = RowStatsCache(RMAX, dev)
        self.bc = _Cache(dev)


_DATA = {}


def _data(dev, key):
    if key not in _DATA:
        _DATA[key] = _Data(dev, *WINDOWS[key], seed=31 + len(_DATA))
    return _DATA[key]


def _launch(d, R, n_p, q, miss, bc, entry="fm_tick_front_bc", n_base=None):
    """One front launch into NaN-filled outputs; ``bc``: a _Cache or None (null pointers)."""
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    for t in (d.o_suff, d.o_pvals, d.o_pstats, d.o_hs):
        t.fill_(float("nan"))
    args = [ptr(d.h), d.h.stride(0), T, R, ptr(d.o_hs), ptr(d.cur), d.cur.stride(0), d.n_cur, ptr(d.base),
            d.base.stride(0), d.n_base if n_base is None else n_base, ptr(d.o_suff), n_p, 0, MIN, MIN, MIN,
            ptr(d.o_pvals), ptr(d.o_pstats), ptr(d.queue), None, ptr(d.hcache.stats), ptr(d.hcache.valid), miss,
            ptr(d.pq), q]
    if entry == "fm_tick_front_bc":
        args += [ptr(t) for t in bc.tensors()] if bc is not None else [None, None, None]
    LIB.call(entry, *args, stream_of(d.h))
    torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _check(d, R, what, ref=None):
    suff, pvals, pstats = ref if ref is not None else (d.suff, d.pvals, d.pstats)
    assert torch.equal(_bits(d.o_suff[:R]), _bits(suff[:R])), f"suff {what}"
    torch.testing.assert_close(d.o_pvals[:R], pvals[:R], rtol=0, atol=0, equal_nan=True, msg=f"pvals {what}")
    torch.testing.assert_close(d.o_pstats[:R], pstats[:R], rtol=0, atol=0, equal_nan=True, msg=f"pstats {what}")
    assert torch.isnan(d.o_suff[R:]).all(), f"rows past R {what}"
    assert not d.pq.any(), f"pqueue not reset {what}"
    assert not d.queue[:256].any(), f"history queue not reset {what}"


def _filled(d, R, n_base=None):
    """Entries [0, R) carry the tag n_base, entries past R are empty."""
    nb = d.n_base if n_base is None else n_base
    assert (d.bc.stats[:R, 3] == nb).all() and not d.bc.stats[R:].any()
    assert not d.bc.raw[R:].any() and not d.bc.sorted[R:].any()


@pytest.mark.gpu
@pytest.mark.parametrize("win", SPLIT + ("10x3",))
def test_gpu_empty_cache_then_hits(cuda, win):
    """Case 1, every (R, nP, q_ranges, expect_miss): static rows, the pool and
    the raised nP (R = 1030, nP = 2 in the scan shape).  A launch over an
    empty cache, then the same launch twice more: each equals the oracle, the
    first fills exactly the entries of its rows and the other two (all hits)
    change no word.  (10, 3) pools 13 points: K = 1, no cache kernel -- the
    launch is the oracle's and the cache stays empty."""
    d = _data(cuda, win)
    for R in ROWS:
        for n_p in NPS:
            for q in QS:
                for miss in (0, 1):
                    what = f"{win} R={R} nP={n_p} q={q} miss={miss}"
                    d.bc.clear()
                    _launch(d, R, n_p, q, miss, d.bc)
                    _check(d, R, f"{what} empty")
                    if win in SPLIT:
                        _filled(d, R)
                    else:
                        assert not any(t.any() for t in d.bc.tensors()), what
                    snap = d.bc.snap()
                    for k in (1, 2):
                        _launch(d, R, n_p, q, miss, d.bc)
                        _check(d, R, f"{what} hit {k}")
                        assert d.bc.changed_rows(snap) == set(), f"{what} hit {k}"


@pytest.mark.gpu
@pytest.mark.parametrize("win", ["50x50", "1x64"])
def test_gpu_changing_current_window(cuda, win):
    """Case 2: ``cur`` replaced before each of three launches, ``base``
    untouched: every launch equals the oracle recomputed for that ``cur`` and,
    past the first, writes no word of the cache."""
    d = _data(cuda, win)
    d.bc.clear()
    keep = d.cur.clone()
    snap = None
    try:
        for k in range(3):
            cur, _ = _inputs(d.n_cur, d.n_base, 500 + k)
            d.cur.copy_(cur)
            ref = _oracle(d.cur, d.base, d.n_cur, d.n_base)
            _launch(d, RMAX, 8, 64, 0, d.bc)
            _check(d, RMAX, f"{win} cur {k}", ref)
            if snap is None:
                _filled(d, RMAX)
                snap = d.bc.snap()
            assert d.bc.changed_rows(snap) == set(), f"{win} cur {k}"
    finally:
        d.cur.copy_(keep)


@pytest.mark.gpu
@pytest.mark.parametrize("n_p,q,miss", [(8, 64, 0), (2, 0, 1)])
def test_gpu_changed_baseline_rows(cuda, n_p, q, miss):
    """Case 3: between two launches a tenth of the baseline rows is rewritten,
    among them one row where a single +0.0 becomes -0.0, one where only a
    NaN's payload changes and one permuted in place.  The launch equals the
    oracle of the new baseline, and exactly the rewritten rows' entries
    changed."""
    d = _data(cuda, "50x50")
    keep = d.base.clone()
    try:
        r_zero, r_nan, r_perm = 23, 33, 43
        d.base[r_zero, 5] = 0.0
        _bits(d.base)[r_nan, 7] = 0x7FC00000
        d.bc.clear()
        _launch(d, RMAX, n_p, q, miss, d.bc)
        _check(d, RMAX, "before", _oracle(d.cur, d.base, d.n_cur, d.n_base))
        _filled(d, RMAX)
        snap = d.bc.snap()
        g = torch.Generator().manual_seed(77)
        rows = list(range(3, RMAX, 10))
        assert {r_zero, r_nan, r_perm} <= set(rows)
        fresh = (torch.round(torch.randn(len(rows), d.n_base, generator=g) * 4.0) / 2.0 + 100.0).to(cuda)
        for i, r in enumerate(rows):
            if r == r_zero:
                d.base[r, 5] = -0.0
            elif r == r_nan:
                _bits(d.base)[r, 7] = 0x7FC00001
            elif r == r_perm:
                assert not torch.equal(d.base[r], d.base[r].flip(0))
                d.base[r] = d.base[r].flip(0)
            else:
                d.base[r] = fresh[i]
        ref = _oracle(d.cur, d.base, d.n_cur, d.n_base)
        _launch(d, RMAX, n_p, q, miss, d.bc)
        _check(d, RMAX, "after", ref)
        assert d.bc.changed_rows(snap) == set(rows)
        raw_changed = (d.bc.raw != snap[0]).any(dim=1).nonzero().flatten().tolist()
        assert raw_changed == rows
        # and the refreshed entries hit
        snap = d.bc.snap()
        _launch(d, RMAX, n_p, q, miss, d.bc)
        _check(d, RMAX, "after, hits", ref)
        assert d.bc.changed_rows(snap) == set()
    finally:
        d.base.copy_(keep)


@pytest.mark.gpu
def test_gpu_changed_n_base_misses_every_row(cuda):
    """Case 4: one cache launched with n_base 64, then 50 on the same storage:
    the tag tells the entries apart, every row misses and is rewritten."""
    d = _data(cuda, "64x64")
    ref50 = _oracle(d.cur, d.base, 64, 50)
    for R, n_p, q in ((RMAX, 8, 64), (203, 2, 0)):
        d.bc.clear()
        _launch(d, R, n_p, q, 0, d.bc)
        _check(d, R, f"n_base 64 R={R}")
        _filled(d, R, 64)
        snap = d.bc.snap()
        _launch(d, R, n_p, q, 0, d.bc, n_base=50)
        _check(d, R, f"n_base 50 R={R}", ref50)
        _filled(d, R, 50)
        assert d.bc.changed_rows(snap) == set(range(R))


@pytest.mark.gpu
@pytest.mark.parametrize("n_p,q,miss", [(8, 64, 0), (8, 0, 0), (2, 0, 1)])
def test_gpu_hits_read_the_cache(cuda, n_p, q, miss):
    """Case 5, the only check that a hit takes the cache's word for it: after
    a fill, ``sorted`` of three rows is overwritten with another finite
    sequence (raw, stats and tag intact).  The next launch differs from the
    oracle in ``suff`` on exactly those rows; with their tags cleared the rows
    miss, and the launch after that equals the oracle again.  (Dynamic rows,
    static rows in the scan shape, static rows in the streaming shape.)"""
    d = _data(cuda, "50x50")
    d.bc.clear()
    _launch(d, RMAX, n_p, q, miss, d.bc)
    _check(d, RMAX, "fill")
    rows = [20, 500, RMAX - 1]
    # larger than every sample, descending like the register's second half
    wrong = (2000.0 - torch.arange(64, dtype=torch.float32)).to(cuda)
    for r in rows:
        d.bc.sorted[r] = _bits(wrong)
    _launch(d, RMAX, n_p, q, miss, d.bc)
    differs = (_bits(d.o_suff) != _bits(d.suff)).any(dim=1).nonzero().flatten().tolist()
    assert differs == rows
    assert not d.pq.any() and not d.queue[:256].any()
    d.bc.stats[rows, 3] = 0
    _launch(d, RMAX, n_p, q, miss, d.bc)
    _check(d, RMAX, "tags cleared")
    _filled(d, RMAX)
    _launch(d, RMAX, n_p, q, miss, d.bc)
    _check(d, RMAX, "refilled, hits")


@pytest.mark.gpu
@pytest.mark.parametrize("win", ["k1", "k4"])
def test_gpu_unused_shapes_leave_the_cache_alone(cuda, win):
    """Case 6: (10, 10) -> K = 1 and (130, 100) -> K = 4 with cache pointers
    passed: the oracle's outputs, and no word of the cache changes."""
    d = _data(cuda, win)
    for t in d.bc.tensors():
        t.fill_(0x5A5A5A5A)
    snap = d.bc.snap()
    for R, n_p, q, miss in ((RMAX, 8, 64, 0), (203, 2, 8, 0), (203, 0, 0, 1), (5, 2, 0, 0)):
        _launch(d, R, n_p, q, miss, d.bc)
        _check(d, R, f"{win} R={R} nP={n_p} q={q} miss={miss}")
        assert d.bc.changed_rows(snap) == set()
    d.bc.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("win", ["50x50", "k1", "k4"])
def test_gpu_nulls_equal_the_old_entry_point(cuda, win):
    """Case 7: the same inputs through fm_tick_front and through
    fm_tick_front_bc with null cache pointers: identical bits."""
    d = _data(cuda, win)
    for R, n_p, q, miss in ((RMAX, 8, 64, 0), (203, 2, 8, 0), (203, 0, 0, 1), (5, 2, 0, 0)):
        _launch(d, R, n_p, q, miss, None, entry="fm_tick_front")
        _check(d, R, f"{win} old entry")
        old = [_bits(t).clone() for t in (d.o_suff, d.o_pvals, d.o_pstats, d.o_hs)]
        _launch(d, R, n_p, q, miss, None)
        _check(d, R, f"{win} nulls")
        new = [_bits(t) for t in (d.o_suff, d.o_pvals, d.o_pstats, d.o_hs)]
        assert all(torch.equal(a, b) for a, b in zip(old, new))


@pytest.mark.gpu
def test_gpu_scorer_ticks_with_the_cache_equal_ticks_without(cuda):
    """CanaryScorer: score_resident, split_launchers and capture_front (three
    ticks each: a fill, then hits) give what a scorer with ``base_cache=False``
    gives; a rewritten baseline row is seen without any call."""
    from foremast_amd.engine.resident import HistView, RowStatsCache
    from foremast_amd.engine.scorer import CanaryScorer
    S, M, TH = 150, 4, 10080                     # (the history length of the flagship tick: its kernel)
    R = S * M
    h, b, c = C.synth_fleet(S, M, TH, 5, 10, 0, device=cuda, fault_rate=0.2)
    sc = CanaryScorer(ALIASES, device=cuda)
    ref_sc = CanaryScorer(ALIASES, device=cuda, base_cache=False)
    assert sc.base_cache and not ref_sc.base_cache
    rm = torch.arange(R, dtype=torch.int32, device=cuda)

    def reference():
        o = ref_sc.score_resident(HistView(h, h.stride(0), TH, RowStatsCache(R, cuda)), rm, c, b)
        torch.cuda.synchronize()
        return [t.clone() for t in (o.suff, o.pvals, o.pstats, o.packed)]

    def same(o, ref, what):
        torch.cuda.synchronize()
        assert torch.equal(_bits(o.suff), _bits(ref[0])), what
        for t, r in zip((o.pvals, o.pstats, o.packed), ref[1:]):
            torch.testing.assert_close(t, r, rtol=0, atol=0, equal_nan=True, msg=what)

    ref = reference()
    assert not ref_sc._base_caches
    view = HistView(h, h.stride(0), TH, RowStatsCache(R, cuda))
    for k in range(3):
        same(sc.score_resident(view, rm, c, b), ref, f"score_resident {k}")
    assert len(sc._base_caches) == 1
    bc = sc._base_cache_of(b, c)
    assert (bc.stats[:, 3] == b.shape[1]).all()
    front, decide, o_s = sc.split_launchers(h, b, c, TH)
    assert front.keep[1] is bc
    for k in range(3):
        front()
        decide()
        same(o_s, ref, f"split_launchers {k}")
    replay, o_g = sc.capture_front(h, b, c, TH, slot=1)
    assert replay.keep[1] is bc
    for k in range(3):
        replay()
        sc.decide_only(c, o_g)
        same(o_g, ref, f"capture_front {k}")
    b[17] = b[17].flip(0) + 1.0
    ref = reference()
    front()
    decide()
    same(o_s, ref, "after a baseline write")


# ---- CPU: the scorer's bookkeeping -----------------------------------------
def _cpu_pair(rows=8, n_cur=50, n_base=50):
    return torch.zeros(rows, n_cur), torch.zeros(rows, n_base)


def test_scorer_one_cache_per_baseline_tensor():
    from foremast_amd.engine.scorer import CanaryScorer
    sc = CanaryScorer(ALIASES)
    cur, base = _cpu_pair()
    bc = sc._base_cache_of(base, cur)
    assert bc is not None and len(bc) == 8
    assert bc.raw.shape == (8, 64) and bc.sorted.shape == (8, 64) and bc.stats.shape == (8, 4)
    assert all(t.dtype == torch.int32 and not t.any() for t in (bc.raw, bc.sorted, bc.stats))
    assert sc._base_cache_of(base, cur) is bc                    # the same tensor: the same cache
    assert sc._base_cache_of(base, torch.zeros(8, 40)) is bc     # whatever the current window
    other = torch.zeros(8, 50)
    assert sc._base_cache_of(other, cur) is not bc               # equal content, another tensor
    assert len(sc._base_caches) == 2
    # shapes the kernel has no cache for
    assert sc._base_cache_of(torch.zeros(8, 10), torch.zeros(8, 10)) is None
    assert sc._base_cache_of(torch.zeros(8, 100), torch.zeros(8, 130)) is None
    assert sc._base_cache_of(torch.zeros(8, 65), torch.zeros(8, 10)) is None
    assert sc._base_cache_of(torch.zeros(4, 50), cur) is None    # fewer baseline rows than rows
    assert len(sc._base_caches) == 2


def test_scorer_drops_the_cache_with_its_tensor():
    from foremast_amd.engine.scorer import CanaryScorer
    sc = CanaryScorer(ALIASES)
    cur, base = _cpu_pair()
    keep = torch.zeros(8, 50)
    sc._base_cache_of(base, cur)
    sc._base_cache_of(keep, cur)
    assert len(sc._base_caches) == 2
    del base
    gc.collect()
    assert len(sc._base_caches) == 1 and next(iter(sc._base_caches.values()))[0]() is keep


def test_scorer_passes_nulls_when_switched_off(monkeypatch):
    from foremast_amd.engine.scorer import CanaryScorer
    cur, base = _cpu_pair()
    hist = torch.zeros(8, 64)

    def tail(sc):
        o = sc._alloc(8, cur.shape[1])
        bc = sc._base_cache_of(base, cur)
        return sc._front_args(hist.data_ptr(), hist.stride(0), 64, base, cur, o, None, None, True, bc)[-3:], bc

    on, bc = tail(CanaryScorer(ALIASES))
    assert on == (bc.raw.data_ptr(), bc.sorted.data_ptr(), bc.stats.data_ptr())
    off, bc = tail(CanaryScorer(ALIASES, base_cache=False))
    assert bc is None and off == (None, None, None)
    monkeypatch.setenv("FM_BASE_CACHE", "0")
    sc = CanaryScorer(ALIASES)
    assert not sc.base_cache
    off, bc = tail(sc)
    assert bc is None and off == (None, None, None) and not sc._base_caches
    monkeypatch.setenv("FM_BASE_CACHE", "1")
    assert CanaryScorer(ALIASES).base_cache and not CanaryScorer(ALIASES, base_cache=False).base_cache


def test_cpu_scoring_ignores_the_cache():
    from foremast_amd.engine.resident import HistView
    from foremast_amd.engine.scorer import CanaryScorer
    S, M, TH = 6, 4, 200
    h, b, c = C.synth_fleet(S, M, TH, 5, 10, 0, device=torch.device("cpu"), fault_rate=0.3)
    assert b.shape[1] == 50 and c.shape[1] == 50                 # the shape a GPU tick would cache
    on, off = CanaryScorer(ALIASES), CanaryScorer(ALIASES, base_cache=False)
    rm = torch.arange(S * M, dtype=torch.int32)
    for sc in (on, off):
        sc.score(h, b, c, TH)
        sc.score_resident(HistView(h, h.stride(0), TH), rm, c, b)
        assert not sc._base_caches
    a, z = on.score(h, b, c, TH), off.score(h, b, c, TH)
    assert torch.equal(a.packed, z.packed)
    torch.testing.assert_close(a.pvals, z.pvals, rtol=0, atol=0, equal_nan=True)


def test_entry_point_is_registered():
    from foremast_amd.ops._lib import LIB
    lib = LIB.load()
    assert len(lib.fm_tick_front_bc.argtypes) == len(lib.fm_tick_front.argtypes) + 3
    assert lib.fm_tick_front_bc.argtypes[-4:-1] == [ctypes.c_void_p] * 3
