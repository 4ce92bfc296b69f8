"""Row-statistics cache of the history role (csrc/include/fm_row_stats.h,
engine/resident.py RowStatsCache): a tick that reads cached (mean, std, n)
gives exactly what a tick that streams every history row gives.  Every
comparison is bit for bit (rtol = atol = 0) against a scorer with the cache
disabled on the same data."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from foremast_amd.ops import canary as C

ALIASES = ["error5xx", "latency", "traffic", "error4xx", "cpu", "memory", "tomcat_threads", "jvm_heap"]


def _same(o, ref):
    torch.cuda.synchronize()
    for name in ("hs", "pvals", "packed"):
        torch.testing.assert_close(getattr(o, name), getattr(ref, name), rtol=0, atol=0, equal_nan=True, msg=name)
    torch.testing.assert_close(o.decide.count, ref.decide.count, rtol=0, atol=0)


def _scorers(M, dev, **kw):
    from foremast_amd.engine.scorer import CanaryScorer
    return (CanaryScorer(ALIASES[:M], device=dev, **kw), CanaryScorer(ALIASES[:M], device=dev, hist_cache=False, **kw))


def _valid(cache):
    return cache.valid.cpu().numpy()


@pytest.mark.gpu
def test_gpu_mixed_hit_and_miss_equals_cold(cuda):
    """Hot tick, then rows overwritten in place and invalidated (10 %: the
    tick is shaped for streaming; 3 %: the misses are found by the scan),
    then a write nobody reported followed by invalidate_history()."""
    from foremast_amd.engine.resident import HistView, RowStatsCache
    from foremast_amd.ops._lib import LIB, ptr
    S, M, T = 150, 4, 601                        # the last float4 of a row is partial
    R = S * M
    h, b, c = C.synth_fleet(S, M, T, 5, 10, 0, device=cuda, fault_rate=0.2)
    h[3, 100:140] = float("nan")                 # NaN runs: the masked path
    h[77, :300] = float("nan")
    h[R - 1, T - 2:T] = float("nan")
    h[200, :] = float("nan")                     # no history at all
    rm = torch.arange(R, dtype=torch.int32, device=cuda)
    sc, cold = _scorers(M, cuda)
    cache = RowStatsCache(R, cuda)
    view, plain = HistView(h, h.stride(0), T, cache), HistView(h, h.stride(0), T)
    ref = cold.score_resident(plain, rm, c, b)
    _same(sc.score_resident(view, rm, c, b), ref)          # all miss, recorded
    assert (_valid(cache) == T).all()
    _same(sc.score_resident(view, rm, c, b), ref)          # all hit
    # the hit tick read the cache, not the rows: poison a row behind the cache's back and see no change
    keep = h[10].clone()
    LIB.call("fm_memcpy_sync", ptr(h[10]), ptr(torch.full_like(keep, 7.0)), keep.numel() * 4)
    _same(sc.score_resident(view, rm, c, b), ref)
    LIB.call("fm_memcpy_sync", ptr(h[10]), ptr(keep), keep.numel() * 4)

    g = torch.Generator().manual_seed(5)
    for frac in (0.10, 0.03):
        rows = torch.randperm(R, generator=g)[:int(R * frac)].to(cuda)
        h[rows] = h[rows] * 1.25 + 3.0
        cache.touch(rows)
        assert cache.expect_miss(T, R) == (frac == 0.10)
        ref = cold.score_resident(plain, rm, c, b)
        _same(sc.score_resident(view, rm, c, b), ref)
        assert (_valid(cache) == T).all()

    # a raw write the cache owner cannot see, then the scorer-wide invalidation
    LIB.call("fm_memcpy_sync", ptr(h[42]), ptr(h[43].clone()), h.shape[1] * 4)
    sc.invalidate_history()
    assert not _valid(cache).any()
    ref = cold.score_resident(plain, rm, c, b)
    _same(sc.score_resident(view, rm, c, b), ref)
    _same(sc.score_resident(view, rm, c, b), ref)


@pytest.mark.gpu
@pytest.mark.parametrize("hint_miss", [0, 1])
def test_gpu_wrong_hint_is_still_correct(cuda, hint_miss):
    """The host's expectation only shapes the launch: 'expect none' over an
    empty cache and 'expect misses' over a full one both give the cold result."""
    from foremast_amd.engine.resident import RowStatsCache
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    S, M, T = 150, 4, 601
    R = S * M
    h, b, c = C.synth_fleet(S, M, T, 5, 10, 0, device=cuda, fault_rate=0.2)
    sc, cold = _scorers(M, cuda)
    ref = cold.score(h, b, c, T)
    cache = RowStatsCache(R, cuda)
    o = sc._alloc(R, c.shape[1])

    def front(miss, n_h):
        LIB.call("fm_tick_front", ptr(h), h.stride(0), T, R, ptr(o.hs), ptr(c), c.stride(0), c.shape[1],
                 ptr(b), b.stride(0), b.shape[1], ptr(o.suff), 0, n_h, 2, 2, 2, ptr(o.pvals), ptr(o.pstats),
                 ptr(sc._queue), None, ptr(cache.stats), ptr(cache.valid), miss, None, 0, stream_of(h))
    if hint_miss:
        front(1, 0)                              # fill
    for n_h in (0, 2, 700):                      # scan: 200 rows per workgroup, 300 (two passes), one
        if not hint_miss:
            cache.invalidate()
        o.hs.fill_(-1.0)
        front(hint_miss, n_h)
        torch.cuda.synchronize()
        torch.testing.assert_close(o.hs, ref.hs, rtol=0, atol=0, equal_nan=True)
        assert (_valid(cache) == T).all()
    assert not sc._queue[:256].any()


@pytest.mark.gpu
def test_gpu_resident_rowmap_release_and_longer_row(cuda):
    """score_resident over a static ResidentHistory: permuted row map with two
    logical rows on one physical row, 12 rows (fewer than 8 history
    workgroups), release + reuse of slots, then a longer row (the view length,
    i.e. the tag, changes: every row is recomputed once)."""
    from foremast_amd.engine.resident import ResidentHistory
    S, M, T0, T1 = 3, 4, 590, 601
    R = S * M
    h, b, c = C.synth_fleet(S + 2, M, T1, 5, 10, 0, device="cpu", fault_rate=0.2)
    h = h.numpy()
    b, c = b[:R].to(cuda), c[:R].to(cuda)
    st = ResidentHistory(T1, cuda)
    keys = [("job", i) for i in range(R - 1)]
    rows, _ = st.rows_for(keys)
    st.write_static(rows, [h[i, :T0] for i in range(R - 1)], np.zeros(R - 1))
    perm = np.random.default_rng(2).permutation(R - 1)
    sc, cold = _scorers(M, cuda)

    def rowmap():
        phys = np.array([st.slot[k] for k in keys], np.int32)[perm]
        return torch.from_numpy(np.append(phys, phys[4]).astype(np.int32)).to(cuda)   # rows 4 and 11 share a slot

    def tick_equals_cold():
        rm, v = rowmap(), st.view()
        ref = cold.score_resident(v, rm, c, b)
        _same(sc.score_resident(v, rm, c, b), ref)
        return rm, v
    rm, v = tick_equals_cold()                   # cold: both duplicates compute the shared row
    assert v.T == T0 and (_valid(st.cache)[rm.cpu().numpy()] == T0).all()
    tick_equals_cold()                           # hot

    gone = [keys[1], keys[6], keys[8]]
    freed = sorted(st.slot[k] for k in gone)
    assert st.release(gone) == 3
    assert not _valid(st.cache)[freed].any()
    for j, k in enumerate(gone):
        keys[keys.index(k)] = ("new", j)
    rows, new = st.rows_for([("new", j) for j in range(3)])
    assert new.all() and sorted(rows.tolist()) == freed
    st.write_static(rows, [h[R + j, :T0] for j in range(3)], np.zeros(3))
    rm, v = tick_equals_cold()                   # 3 of 12 rows miss
    assert (_valid(st.cache)[rm.cpu().numpy()] == T0).all()
    tick_equals_cold()

    # one longer row: max_len grows, every cached entry carries the old tag
    r0 = np.array([st.slot[keys[0]]])
    st.write_static(r0, [h[0, :T1]], np.zeros(1))
    rm, v = tick_equals_cold()
    assert v.T == T1 and (_valid(st.cache)[rm.cpu().numpy()] == T1).all()
    tick_equals_cold()

    # windows wider than the front kernel's 256: the stand-alone statistics kernel, same cache
    bw = torch.cat([b, b, b, b, b], 1).contiguous()          # 50 + 250 points
    st.cache.invalidate()
    for _ in range(2):
        rm, v = rowmap(), st.view()
        _same(sc.score_resident(v, rm, c, bw), cold.score_resident(v, rm, c, bw))
    assert (_valid(st.cache)[rm.cpu().numpy()] == T1).all()


@pytest.mark.gpu
def test_gpu_xcd_balanced_all_miss_ticks_equal_serial(cuda):
    """32,768 rows (tick_front.hip kXcdMinRows): ticks after invalidate_history()
    take the dynamic queue with XCD-balanced ranges and record every row; the
    queue counters are back at zero; hot ticks follow."""
    from foremast_amd.engine.scorer import CanaryScorer
    T = 600
    h, b, c = C.synth_fleet(4096, 8, T, 5, 10, 0, device=cuda, fault_rate=0.2)
    ref = CanaryScorer(ALIASES, device=cuda, mode="serial").score(h, b, c, T)
    sc, cold = _scorers(8, cuda, xcd_balance=True)
    f0, d0, o0 = cold.split_launchers(h, b, c, T)
    f0(), d0()
    front, decide, o = sc.split_launchers(h, b, c, T)
    cache = sc._bound[id(h)].cache
    for k in range(11):
        if k < 8:
            sc.invalidate_history()
        front(), decide()
        _same(o, o0)
        torch.testing.assert_close(o.packed, ref.packed)
        torch.testing.assert_close(o.decide.count, ref.decide.count)
        assert (_valid(cache) == T).all()
        if k == 7:
            ctl = sc._queue[256:].cpu().numpy().view(np.uint32)
            assert ctl[0] == 1 and ctl[31] == 1
            f = ctl[2:11].astype(np.int64)
            assert f[0] == 0 and f[8] == 1 << 24 and (np.diff(f) > 0).all()
    assert not sc._queue[:256].any()             # the per-XCD counters are back to zero


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["direct", "graph"])
def test_gpu_bound_launchers_follow_the_tensor_version(cuda, form):
    """split_launchers / capture_front, two slots in flight, decision on a side
    stream: hist.mul_(1.5) between ticks 3 and 4 is picked up."""
    S, M, T = 77, 4, 10080
    h, b, c = C.synth_fleet(S, M, T, 5, 10, 1, device=cuda, fault_rate=0.2)
    sc, cold = _scorers(M, cuda, front_wgs=(1.0, 3.0))
    def snap(o):                                 # (the scorer reuses its output buffers)
        return SimpleNamespace(hs=o.hs.clone(), pvals=o.pvals.clone(), packed=o.packed.clone(),
                               count=o.decide.count.clone())
    ref = [snap(cold.score(h, b, c, T))]
    packed = [torch.full((S, 4), -1.0, device=cuda) for _ in range(2)]
    side = torch.cuda.Stream()
    if form == "graph":
        fr = [sc.capture_front(h, b, c, T, packed_out=packed[i], slot=i) for i in range(2)]
        fronts = [f for f, _ in fr]
        outs = [o for _, o in fr]
        decides = [lambda o=o: sc.decide_only(c, o) for o in outs]
    else:
        sl = [sc.split_launchers(h, b, c, T, packed_out=packed[i], slot=i, decide_stream=side) for i in range(2)]
        fronts, decides, outs = [x[0] for x in sl], [x[1] for x in sl], [x[2] for x in sl]
    assert outs[0].hs.data_ptr() != outs[1].hs.data_ptr()
    ev = [torch.cuda.Event() for _ in range(2)]
    done = [torch.cuda.Event() for _ in range(2)]
    got = []
    for k in range(7):
        i = k % 2
        if k == 4:
            h.mul_(1.5)                          # bumps hist._version
        if k >= 2:
            torch.cuda.current_stream().wait_event(done[i])
            got.append((k - 2, outs[i].hs.clone(), outs[i].pvals.clone(), packed[i].clone(),
                        outs[i].decide.count.clone()))
        packed[i].fill_(-1.0)
        fronts[i]()
        ev[i].record()
        side.wait_event(ev[i])
        with torch.cuda.stream(side):
            decides[i]()
        done[i].record(side)
    torch.cuda.synchronize()
    for k in (5, 6):
        i = k % 2
        got.append((k, outs[i].hs, outs[i].pvals, packed[i], outs[i].decide.count))
    ref.append(snap(cold.score(h, b, c, T)))     # the scaled history
    torch.cuda.synchronize()
    assert not torch.equal(ref[0].hs, ref[1].hs)
    for k, hs, pv, pk, cnt in got:
        r = ref[k >= 4]
        torch.testing.assert_close(hs, r.hs, rtol=0, atol=0, equal_nan=True, msg=f"hs tick {k}")
        torch.testing.assert_close(pv, r.pvals, rtol=0, atol=0, equal_nan=True, msg=f"pvals tick {k}")
        torch.testing.assert_close(pk, r.packed, rtol=0, atol=0, equal_nan=True, msg=f"packed tick {k}")
        torch.testing.assert_close(cnt, r.count, rtol=0, atol=0, msg=f"count tick {k}")
    assert (sc._bound[id(h)].cache.valid == T).all()
