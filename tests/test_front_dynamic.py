"""Dynamic row queue of the front kernel's pairwise role (fm_tick_front with a
pqueue, csrc/kernels/tick_front.hip): whichever wave ranks a row, the launch gives
exactly what the separate kernels give -- fm_pairwise_suff (all 14 ``suff``
columns as raw fp64 bits), fm_pvalues_only (``pvals``, ``pstats``) and
fm_hist_stats (``hs``).  They run the same pw_row / eval_test /
block_row_stats code, so every comparison is rtol = atol = 0.  Every output
is NaN-filled before each launch, so a row nobody took shows, and every word
of the queue must be zero again after each launch."""
import ctypes

import numpy as np
import pytest
import torch

from foremast_amd.ops import canary as C

T, M, RMAX, CAP = 601, 4, 1030, 64
WINDOWS = {"k1": (10, 10), "k2": (50, 50), "k4": (130, 100)}
ROWS = (1, 3, 4, 5, 203, 1030)
NPS = (0, 1, 2, 8)
QS = (1, 8, 64)
MIN = 2                                          # min_mw / min_wil / min_kru
ALIASES = ["error5xx", "latency", "traffic", "error4xx"]


def _plan(R, n_p, q, scan):
    from foremast_amd.ops._lib import LIB
    out = (ctypes.c_int64 * 4)()
    LIB.call("fm_front_plan", R, n_p, q, scan, ctypes.cast(out, ctypes.c_void_p))
    return tuple(out)                            # static rows per wave, pool start, ranges, effective nP


def _check_plan(R, n_p, q, scan):
    s, pool0, qe, npe = _plan(R, n_p, q, scan)
    pmax = (R + 3) // 4
    if R == 0:
        assert qe == 0 and pool0 == 0
        return
    assert 1 <= npe <= pmax and s >= 0
    if n_p > 0 and not scan:
        assert npe == min(n_p, pmax)             # a streaming launch keeps its grid
    W = 4 * npe
    if qe == 0:                                  # static rows: wave rows 4 pb + w + i W, i < s, cover [0, R)
        assert pool0 == R and W * s >= R
        assert not scan                          # the scan shape always gets the queue
        return
    # static rows are exactly [0, pool0), the pool is [pool0, R)
    assert pool0 == W * s and 0 <= pool0 <= R
    assert 1 <= qe <= min(q, npe) and s < CAP
    assert W * CAP >= R
    pool = R - pool0
    # the longest range against the fewest workgroups a range can have ...
    assert -(-pool // qe) <= (npe // qe) * 4 * (CAP - s)
    if R > 300 and R % 11:
        return
    # ... and range by range: its rows fit what is left of the lists of its workgroups
    pb = np.arange(npe)
    nwg = np.bincount((pb + pb // qe) % qe, minlength=qe)
    x = np.arange(qe + 1, dtype=np.int64)
    bounds = pool0 + pool * x // qe
    assert bounds[0] == pool0 and bounds[-1] == R
    assert (np.diff(bounds) <= nwg * 4 * (CAP - s)).all()


def test_front_plan_partitions_the_rows():
    """Host only: static rows and pool partition [0, R), the wave lists hold
    every row (4 nP cap >= R, and range by range), the streaming shape never
    changes its grid and the scan shape always gets the queue."""
    for scan in (1, 0):
        for n_p in NPS:
            for q in QS:
                for R in range(0, 5001, 1 if scan else 3):
                    _check_plan(R, n_p, q, scan)
    assert _plan(1030, 2, 64, 1)[3] >= 5         # 129 rows per wave > cap: nP raised
    assert _plan(1030, 2, 64, 0)[2] == 0         # ... or static rows in the streaming shape
    assert _plan(80000, 1280, 64, 1) == (12, 61440, 64, 1280)   # 85 % of 15 rows per wave
    assert _plan(1000, 8, 0, 1)[2] == 0          # queue off


class _Data:
    """One window shape: inputs for RMAX rows and the separate kernels' outputs
    (computed once; rows are independent, so R rows are the first R of them)."""

    def __init__(self, dev, n_cur, n_base, seed):
        from foremast_amd.ops._lib import LIB, ptr, stream_of
        g = torch.Generator().manual_seed(seed)
        ld = (T + 3) // 4 * 4
        h = torch.full((RMAX + 3, ld), float("nan"))
        h[:, :T] = torch.randn(RMAX + 3, T, generator=g) * 3.0 + 10.0
        h[3, 100:140] = float("nan")             # the masked path
        h[5 % RMAX, :] = float("nan")            # no history at all
        # rounded samples: ties and zero differences in every row; a few NaNs
        cur = torch.round(torch.randn(RMAX, n_cur, generator=g) * 4.0) / 2.0
        base = torch.round(torch.randn(RMAX, n_base, generator=g) * 4.0) / 2.0 + 0.5 * (torch.arange(RMAX) % 3)[:, None]
        cur[2, : n_cur // 2] = float("nan")
        base[4, 1] = float("nan")
        cur[7] = base[7, :n_cur] if n_cur <= n_base else cur[7]
        self.h, self.cur, self.base = h.to(dev), cur.to(dev), base.to(dev)
        self.n_cur, self.n_base = n_cur, n_base
        st = stream_of(self.h)
        self.suff = torch.full((RMAX, C.SUFF), float("nan"), dtype=torch.float64, device=dev)
        self.pvals = torch.full((RMAX, C.N_TESTS), float("nan"), device=dev)
        self.pstats = torch.full((RMAX, C.N_TESTS), float("nan"), device=dev)
        self.hs_phys = torch.full((RMAX + 3, 3), float("nan"), device=dev)
        LIB.call("fm_pairwise_suff", ptr(self.cur), self.cur.stride(0), n_cur, ptr(self.base), self.base.stride(0),
                 n_base, RMAX, ptr(self.suff), 0, st)
        LIB.call("fm_pvalues_only", ptr(self.suff), RMAX, MIN, MIN, MIN, ptr(self.pvals), ptr(self.pstats), st)
        LIB.call("fm_hist_stats", ptr(self.h), self.h.stride(0), T, RMAX + 3, ptr(self.hs_phys), st)
        torch.cuda.synchronize()
        # work buffers
        self.o_suff = torch.empty_like(self.suff)
        self.o_pvals, self.o_pstats = torch.empty_like(self.pvals), torch.empty_like(self.pstats)
        self.o_hs = torch.empty((RMAX, 3), device=dev)
        self.queue = torch.zeros(8 * 32 + 64, dtype=torch.int32, device=dev)
        self.pq = torch.zeros(64 * 32, dtype=torch.int32, device=dev)


_DATA = {}


def _data(dev, key):
    if key not in _DATA:
        _DATA[key] = _Data(dev, *WINDOWS[key], seed=11 + len(_DATA))
    return _DATA[key]


def _launch(d, R, n_p, q, miss, cache, rowmap=None):
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    for t in (d.o_suff, d.o_pvals, d.o_pstats, d.o_hs):
        t.fill_(float("nan"))
    LIB.call("fm_tick_front", ptr(d.h), d.h.stride(0), T, R, ptr(d.o_hs), ptr(d.cur), d.cur.stride(0), d.n_cur,
             ptr(d.base), d.base.stride(0), d.n_base, ptr(d.o_suff), n_p, 0, MIN, MIN, MIN, ptr(d.o_pvals),
             ptr(d.o_pstats), ptr(d.queue), ptr(rowmap), ptr(cache.stats), ptr(cache.valid), miss, ptr(d.pq), q,
             stream_of(d.h))
    torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _check(d, R, what, rowmap=None):
    assert torch.equal(_bits(d.o_suff[:R]), _bits(d.suff[:R])), f"suff {what}"
    torch.testing.assert_close(d.o_pvals[:R], d.pvals[:R], rtol=0, atol=0, equal_nan=True, msg=f"pvals {what}")
    torch.testing.assert_close(d.o_pstats[:R], d.pstats[:R], rtol=0, atol=0, equal_nan=True, msg=f"pstats {what}")
    hs = d.hs_phys[:R] if rowmap is None else d.hs_phys[rowmap.long()]
    torch.testing.assert_close(d.o_hs[:R], hs, rtol=0, atol=0, equal_nan=True, msg=f"hs {what}")
    # nothing past the rows asked for, and the queues are ready for the next launch
    assert torch.isnan(d.o_suff[R:]).all() and torch.isnan(d.o_hs[R:]).all(), f"rows past R {what}"
    assert not d.pq.any(), f"pqueue not reset {what}"
    assert not d.queue[:256].any(), f"history queue not reset {what}"


@pytest.mark.gpu
@pytest.mark.parametrize("win", list(WINDOWS))
def test_gpu_dynamic_rows_equal_the_separate_kernels(cuda, win):
    """Every (R, nP, q_ranges) of the issue: fewer rows than waves, R no
    multiple of 4, static share 0 (R < 4 nP), more ranges than pool rows,
    several grabs per wave, 129 rows per wave at R = 1030 / nP = 2 (nP raised
    in the scan shape, static rows when streaming); both hints over a filled
    and over an empty cache.  q = 0: static rows, in the scan shape too (the
    p-value phase is one function for both row forms); pq then stays zero,
    which _check asserts after every launch."""
    from foremast_amd.engine.resident import RowStatsCache
    d = _data(cuda, win)
    cache = RowStatsCache(RMAX + 3, cuda)
    for R in ROWS:
        for n_p in NPS:
            for q in (0,) + QS:
                for miss in (0, 1):
                    for filled in (False, True):
                        if not filled:
                            cache.invalidate()
                            torch.cuda.synchronize()
                        _launch(d, R, n_p, q, miss, cache)
                        _check(d, R, f"R={R} nP={n_p} q={q} miss={miss} filled={filled}")
                        assert (cache.valid[:R].cpu().numpy() == T).all()


@pytest.mark.gpu
def test_gpu_dynamic_rows_permuted_rowmap_with_a_duplicate(cuda):
    from foremast_amd.engine.resident import RowStatsCache
    d = _data(cuda, "k2")
    cache = RowStatsCache(RMAX + 3, cuda)
    g = torch.Generator().manual_seed(3)
    for R in (5, 203, 1030):
        rm = torch.randperm(RMAX + 3, generator=g)[:R].to(torch.int32)
        rm[1] = rm[0]                            # two logical rows on one physical row
        rm = rm.to(cuda)
        for miss in (1, 0, 0):                   # fill through the map, then hit twice
            _launch(d, R, 8, 8, miss, cache, rm)
            _check(d, R, f"rowmap R={R} miss={miss}", rm)
        cache.invalidate()
        _launch(d, R, 0, 64, 0, cache, rm)       # expect hits over an empty cache
        _check(d, R, f"rowmap R={R} empty", rm)


@pytest.mark.gpu
@pytest.mark.parametrize("win", ["k1", "k4"])
def test_gpu_dynamic_rows_same_launch_three_times(cuda, win):
    """One pqueue, the same launch three times: the kernel leaves its counters
    zero, so every launch hands out every row again."""
    from foremast_amd.engine.resident import RowStatsCache
    d = _data(cuda, win)
    cache = RowStatsCache(RMAX + 3, cuda)
    _launch(d, RMAX, 8, 64, 1, cache)
    for R, n_p, q in ((1030, 8, 64), (1030, 2, 8), (203, 0, 8), (5, 1, 1)):
        outs = []
        for _ in range(3):
            _launch(d, R, n_p, q, 0, cache)
            _check(d, R, f"repeat R={R} nP={n_p} q={q}")
            outs.append((_bits(d.o_suff).clone(), _bits(d.o_pvals).clone(), _bits(d.o_hs).clone()))
        for o in outs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))


@pytest.mark.gpu
def test_gpu_scorer_ticks_with_the_queue_equal_static_rows(cuda, monkeypatch):
    """CanaryScorer: score_resident, split_launchers and capture_front
    (replayed three times) launch with the pairwise row queue and give what a scorer
    with the queue switched off gives; the scorer's pqueue is zero after each."""
    from foremast_amd.engine.resident import HistView, RowStatsCache
    from foremast_amd.engine.scorer import CanaryScorer
    S = 150
    R = S * M
    h, b, c = C.synth_fleet(S, M, T, 5, 10, 0, device=cuda, fault_rate=0.2)
    sc = CanaryScorer(ALIASES, device=cuda)
    assert sc._q_ranges > 0 and sc._pqueue.numel() == sc._q_ranges * 32
    monkeypatch.setenv("FM_FRONT_DYN_Q", "0")
    ref_sc = CanaryScorer(ALIASES, device=cuda)
    assert ref_sc._pqueue is None
    rm = torch.arange(R, dtype=torch.int32, device=cuda)
    ref = ref_sc.score_resident(HistView(h, h.stride(0), T, RowStatsCache(R, cuda)), rm, c, b)
    torch.cuda.synchronize()

    def same(o, what):
        torch.cuda.synchronize()
        assert torch.equal(_bits(o.suff), _bits(ref.suff)), what
        for name in ("hs", "pvals", "pstats"):
            torch.testing.assert_close(getattr(o, name), getattr(ref, name), rtol=0, atol=0, equal_nan=True,
                                       msg=f"{name} {what}")
        assert not sc._pqueue.any(), what

    def poison(o):
        for t in (o.suff, o.hs, o.pvals, o.pstats):
            t.fill_(float("nan"))

    view = HistView(h, h.stride(0), T, RowStatsCache(R, cuda))
    for k in range(3):                           # streams, then hits twice
        o = sc.score_resident(view, rm, c, b)
        same(o, f"score_resident {k}")
        poison(o)
    front, decide, o = sc.split_launchers(h, b, c, T)
    for k in range(3):
        poison(o)
        front()
        decide()
        same(o, f"split_launchers {k}")
    replay, o = sc.capture_front(h, b, c, T, slot=1)
    for k in range(3):
        poison(o)
        replay()
        same(o, f"capture_front replay {k}")
