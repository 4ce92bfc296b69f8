"""CanaryScorer(model="band_mix"): the resident tick of a per-metric mix of the
static band models (moving_average_all, robust_moving_average_all,
quantile_robust) over the store's band-record cache.  On the CPU the scorer
equals the zoo's decision run metric by metric; on the GPU the cached resident
tick equals the uncached ``score``, K1 / K13 / K24 over the mapped rows and
itself, tick after tick, with an invalidation and a write in between."""
import numpy as np
import pytest
import torch

from foremast_amd.engine.resident import ResidentHistory
from foremast_amd.engine.scorer import CanaryScorer
from foremast_amd.models import zoo
from foremast_amd.ops import canary as C
from foremast_amd.ops import misc as MI

from test_robust_tick import ALIASES, N_CUR, T, _clear_of_edges, _history, _windows

NAMES = {v: k for k, v in MI.BAND_CODES.items()}
TAIL_Z = 1.5


def _codes(M):
    return tuple((2, 1, 0)[m % 3] for m in range(M))


# ---------------------------------------------------------------------- CPU
@pytest.mark.parametrize("S", [1, 5])
@pytest.mark.parametrize("M", [3, 8])
@pytest.mark.parametrize("n_base", [0, 50])
def test_cpu_band_mix_equals_the_zoo_decision_metric_by_metric(S, M, n_base):
    aliases, codes = ALIASES[:M], _codes(M)
    hist = _history(S * M, 10 * S + M)
    cur, base = _windows(hist, M, n_base, 3)
    h, c_ = torch.from_numpy(hist), torch.from_numpy(cur)
    b = torch.from_numpy(base) if base is not None else None
    sc = CanaryScorer(aliases, device="cpu", model="band_mix", codes=codes, tail_z=TAIL_Z)
    o = sc.score(h, b, c_, T)
    assert _clear_of_edges(cur, o.decide.stats.numpy()) and int(o.decide.count.sum()) > 0
    diff = C.pairwise_tests(c_, b, sc.pcfg)[2] if b is not None else None
    if diff is not None:
        assert torch.equal(o.diff, diff) and (S == 1 or bool(diff.any()))
    count = torch.zeros_like(o.decide.count)
    score = torch.zeros_like(o.decide.score)
    valid = torch.zeros_like(o.decide.valid)
    for m in range(M):
        rows = slice(m, None, M)
        tables = zoo.make_tables([aliases[m]], sc.cfg, "cpu")
        hor = torch.ones(cur[rows].shape, dtype=torch.int64)
        dec = zoo.decide(NAMES[codes[m]], h[rows].contiguous(), T, c_[rows].contiguous(), hor, 1, tables,
                         None if diff is None else diff[rows].contiguous(), tail_z=TAIL_Z)
        assert torch.equal(o.decide.flags[rows], dec.flags), m
        assert torch.equal(o.decide.count[rows], dec.count), m
        assert torch.equal(o.decide.valid[rows], dec.valid.to(torch.int32)), m
        got_up, got_lo = o.decide.stats[rows, 2].numpy(), o.decide.stats[rows, 3].numpy()
        if codes[m] == 0:
            # the zoo's mean / std bounds are made in fp64 (ops/reference.py)
            np.testing.assert_allclose(got_up, dec.upper[:, 0].numpy(), rtol=2e-6)
            np.testing.assert_allclose(got_lo, dec.lower[:, 0].numpy(), rtol=2e-6)
            np.testing.assert_allclose(o.decide.score[rows].numpy(), dec.score.numpy(), rtol=1e-4)
        else:
            np.testing.assert_array_equal(got_up, dec.upper[:, 0].numpy())
            np.testing.assert_array_equal(got_lo, dec.lower[:, 0].numpy())
            np.testing.assert_array_equal(o.decide.score[rows].numpy(), dec.score.numpy())
        count[rows], score[rows], valid[rows] = dec.count, o.decide.score[rows], dec.valid.to(torch.int32)
    assert torch.equal(o.packed, C.service_reduce(count, score, valid, M))
    want, _ = MI.ref_band_stats(hist, T, codes, TAIL_Z)
    np.testing.assert_array_equal(o.bs.numpy(), want)
    assert (want[2::M, 1] == want[2::M, 2]).all() and (want[1::M, 1] == want[1::M, 2]).all()   # codes 0 and 1 ...
    assert (want[0::M, 1] != want[0::M, 2]).any()                       # ... the quantile rows have a sigma per side


def test_band_mix_arguments():
    with pytest.raises(ValueError):
        CanaryScorer(["cpu", "memory"], device="cpu", model="band_mix")                    # no codes
    with pytest.raises(ValueError):
        CanaryScorer(["cpu", "memory"], device="cpu", model="band_mix", codes=(0,))        # one per metric
    with pytest.raises(ValueError):
        CanaryScorer(["cpu", "memory"], device="cpu", model="band_mix", codes=(0, 3))
    with pytest.raises(ValueError):
        CanaryScorer(["cpu"], device="cpu", model="band_mix", codes=(2,), mode="fused")
    with pytest.raises(ValueError):
        CanaryScorer(["cpu"], device="cpu", codes=(0,))                                    # codes without the model
    with pytest.raises(ValueError):                                                        # M = 17
        CanaryScorer([f"m{i}" for i in range(17)], device="cpu", model="band_mix", codes=(2,) * 17)
    sc = CanaryScorer(["cpu"], device="cpu", model="band_mix", codes=(2,), tail_z=9.0)
    assert sc.tail_z == 3.0 and sc.codes == (2,) and sc.code_mask == 4


def test_band_cache_follows_every_writer_and_the_tail_parameter():
    st = ResidentHistory(40, "cpu")
    rows, _ = st.rows_for([("k", i) for i in range(12)], owner=("ns", "app"))
    rng = np.random.default_rng(1)
    st.write_static(rows, [rng.normal(size=40).astype(np.float32) for _ in rows], np.zeros(len(rows)))
    bc = st.bcache
    assert bc is not None and bc.stats.shape == (st.buf.shape[0], 4) and st.view().bcache is bc
    assert st.view_until(None).bcache is bc and not bc.valid.any()
    bc.valid.fill_(MI.band_tag(2, 40))
    bc.ticked(40)
    st.write_static(rows[[2, 5]], [np.ones(40, np.float32)] * 2, np.zeros(2))
    assert torch.nonzero(bc.valid == 0).flatten().tolist() == sorted(int(r) for r in rows[[2, 5]]) and bc.dirty == 2
    bc.valid.fill_(MI.band_tag(2, 40))
    assert st.release([("k", 3)]) == 1 and int(bc.valid[int(rows[3])]) == 0
    # growing keeps words and records
    bc.valid.fill_(7)
    bc.stats.copy_(torch.arange(len(bc) * 4, dtype=torch.float32).reshape(-1, 4))
    n0, keep_v, keep_s = len(bc), bc.valid.clone(), bc.stats.clone()
    st.rows_for([("g", i) for i in range(n0 + 50)])
    assert len(bc) == st.buf.shape[0] > n0 and bc is st.bcache
    assert torch.equal(bc.valid[:n0], keep_v) and torch.equal(bc.stats[:n0], keep_s) and not bc.valid[n0:].any()
    # the tail parameter: the first one is remembered, another one invalidates
    bc.ticked(40)
    bc.rekey(2.0)
    assert bc.z0 == 2.0 and bool(bc.valid[:n0].all()) and bc.dirty == 0
    bc.rekey(2.0)
    assert bool(bc.valid[:n0].all())
    bc.rekey(1.0)
    assert bc.z0 == 1.0 and not bc.valid.any() and bc.expect_miss(40, 12)
    assert ResidentHistory(40, "cpu", sliding=True, slack=8, capacity=16).view().bcache is None
    # invalidate_history of a band_mix scorer reaches the band cache only
    sc = CanaryScorer(["cpu", "memory"], device="cpu", model="band_mix", codes=(2, 0))
    sc.score_resident(st.view(), torch.from_numpy(rows[:6].astype(np.int32)), torch.zeros((6, 4)), None)
    for cch in (st.bcache, st.cache, st.rcache):
        cch.valid.fill_(5)
        cch.ticked(40)
    sc.invalidate_history()
    assert not st.bcache.valid.any() and bool(st.cache.valid.all()) and bool(st.rcache.valid.all())


# ---------------------------------------------------------------------- GPU
def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _kernels(buf, rm, Tv, codes, z0):
    """The band records of the mapped rows from K1, K13 and K24 themselves."""
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    g = buf.index_select(0, rm.long()).contiguous()
    R, M = g.shape[0], len(codes)
    hs = torch.empty((R, 3), dtype=torch.float32, device=g.device)
    LIB.call("fm_hist_stats", ptr(g), g.stride(0), Tv, R, ptr(hs), stream_of(g))
    c, s, n = MI.robust_stats(g, Tv)
    qc, ql, qu, qn = MI.quantile_robust_stats(g, Tv, z0)
    per = [torch.stack([hs[:, 0], hs[:, 1], hs[:, 1], hs[:, 2]], 1), torch.stack([c, s, s, n.float()], 1),
           torch.stack([qc, ql, qu, qn.float()], 1)]
    code = torch.tensor([codes[r % M] for r in range(R)], device=g.device)
    out = torch.empty((R, 4), dtype=torch.float32, device=g.device)
    for k in range(3):
        out[code == k] = per[k][code == k]
    return out


def _snapshot(o):
    d = o.decide
    return [t.clone() for t in (o.bs, d.stats, d.flags, d.count, d.score, d.valid, o.packed, o.diff, o.pvals)]


def _same(a, b):
    return all(_bits(x, y) if x.dtype == torch.float32 else torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.gpu
@pytest.mark.parametrize("M,target", [(3, 9), (8, 520), (1, 8)])
def test_gpu_resident_band_ticks(cuda, M, target):
    aliases, codes = ALIASES[:M], _codes(M)
    R = -(-target // M) * M
    P = R + 3
    st = ResidentHistory(T, cuda)
    keys = [("k", i) for i in range(P)]
    prow, _ = st.rows_for(keys, owner=("ns", "app"))
    hist = _history(P, 100 * M + target)
    st.write_static(prow, list(hist), np.zeros(P))
    lg = np.random.default_rng(5).permutation(P)[:R]          # logical row -> key
    for j in range(min(2, M)):
        lg[R - M + j] = lg[j]                                 # two physical rows mapped twice, in their own slots
    rm_h = prow[lg].astype(np.int32)
    rm = torch.from_numpy(rm_h).to(cuda)
    mk = lambda **kw: CanaryScorer(aliases, device=cuda, model="band_mix", codes=codes, tail_z=TAIL_Z, **kw)
    sc, cold, off = mk(), mk(), mk(hist_cache=False)
    cpu = CanaryScorer(aliases, device="cpu", model="band_mix", codes=codes, tail_z=TAIL_Z)
    tags = torch.tensor([MI.band_tag(codes[r % M], T) for r in range(R)], dtype=torch.int32, device=cuda)
    cur, base = _windows(hist[lg], M, 50, 51)
    cd, bd = torch.from_numpy(cur).to(cuda), torch.from_numpy(base).to(cuda)

    def tick(want_miss, what):
        view = st.view()
        assert view.T == T and view.bcache is st.bcache
        if want_miss is not None:
            assert st.bcache.expect_miss(T, R) == want_miss or st.bcache.z0 is None, what
        o = sc.score_resident(view, rm, cd, bd)
        torch.cuda.synchronize()
        assert st.bcache.dirty == 0 and st.bcache.T == T and st.bcache.z0 == TAIL_Z
        assert _bits(o.bs, _kernels(st.buf, rm, T, codes, TAIL_Z)), what
        assert torch.equal(st.bcache.valid[rm.long()], tags), what         # every mapped word tagged
        assert _bits(st.bcache.stats[rm.long()], o.bs), what
        assert not st.cache.valid.any() and not st.rcache.valid.any()      # the other caches are other models'
        return o

    o1 = tick(True, "cold")
    one = _snapshot(o1)
    assert int(o1.decide.count.sum()) > 0 and bool(o1.diff.any()) and not bool(o1.diff.all())
    # against the uncached score, the cache switched off, and the CPU scorer
    g = st.buf.index_select(0, rm.long()).contiguous()
    u = cold.score(g, bd, cd, T)
    assert _same(_snapshot(u), one)
    assert _same(_snapshot(off.score_resident(st.view(), rm, cd, bd)), one)
    ref = cpu.score(torch.from_numpy(hist[lg]), torch.from_numpy(base), torch.from_numpy(cur), T)
    assert _clear_of_edges(cur, ref.decide.stats.numpy())
    np.testing.assert_array_equal(o1.diff.cpu().numpy(), ref.diff.numpy())
    np.testing.assert_allclose(o1.decide.stats.cpu().numpy(), ref.decide.stats.numpy(), rtol=2e-5, atol=1e-5)
    np.testing.assert_array_equal(o1.decide.count.cpu().numpy(), ref.decide.count.numpy())
    np.testing.assert_array_equal(o1.decide.flags.cpu().numpy(), ref.decide.flags.numpy())
    np.testing.assert_array_equal(o1.decide.valid.cpu().numpy(), ref.decide.valid.numpy())
    np.testing.assert_array_equal(o1.packed.cpu().numpy()[:, [0, 2, 3]], ref.packed.numpy()[:, [0, 2, 3]])
    # tick 2: every row from the cache, array for array
    assert _same(_snapshot(tick(False, "hot")), one)
    # invalidate_history: recomputed, the same again
    sc.invalidate_history()
    torch.cuda.synchronize()
    assert not st.bcache.valid.any()
    assert _same(_snapshot(tick(True, "invalidated")), one)
    # a write to one job's rows (service 1, or the lone service's) retags only those
    s0 = 1 if R > M else 0
    w = [int(k) for k in lg[s0 * M:(s0 + 1) * M]]
    new = _history(M, 77) + 40.0
    st.write_static(prow[w], list(new), np.zeros(M))
    hist[w] = new
    wrote = torch.from_numpy(prow[w].astype(np.int64)).to(cuda)
    kept = torch.from_numpy(np.setdiff1d(rm_h, prow[w]).astype(np.int64)).to(cuda)
    assert not st.bcache.valid[wrote].any() and bool((st.bcache.valid[kept] != 0).all()) and st.bcache.dirty == M
    before = st.bcache.stats.clone()
    o4 = tick(None, "after a write")
    assert _bits(st.bcache.stats[kept], before[kept]) and not _bits(st.bcache.stats[wrote], before[wrote])
    hit = torch.from_numpy(np.isin(rm_h, prow[w])).to(cuda)
    assert _bits(o4.bs[~hit], one[0][~hit]) and bool((o4.bs[hit, 0] > 1020).all())


@pytest.mark.gpu
def test_gpu_refused_forms_and_wide_services(cuda):
    M, R = 3, 9
    aliases, codes = ALIASES[:M], _codes(M)
    st = ResidentHistory(T, cuda)
    prow, _ = st.rows_for([("k", i) for i in range(R)], owner=("ns", "app"))
    hist = _history(R, 4)
    st.write_static(prow, list(hist), np.zeros(R))
    rm = torch.from_numpy(prow.astype(np.int32)).to(cuda)
    cur, base = _windows(hist, M, 50, 6)
    cd, bd = torch.from_numpy(cur).to(cuda), torch.from_numpy(base).to(cuda)
    sc = CanaryScorer(aliases, device=cuda, model="band_mix", codes=codes)
    sc.score_resident(st.view(), rm, cd, bd)
    g = st.buf.index_select(0, rm.long()).contiguous()
    for call in (lambda: sc.capture(g, bd, cd, T), lambda: sc.split_launchers(g, bd, cd, T),
                 lambda: sc.capture_front(g, bd, cd, T), lambda: sc.front_only(g, bd, cd, T)):
        with pytest.raises(ValueError):
            call()
    with pytest.raises(ValueError):
        CanaryScorer([f"m{i}" for i in range(17)], device=cuda, model="band_mix", codes=(2,) * 17)
    # without a baseline: no p-values, no diff, the same records
    o = sc.score_resident(st.view(), rm, cd, None)
    torch.cuda.synchronize()
    assert _bits(o.bs, _kernels(st.buf, rm, T, codes, sc.tail_z)) and int(o.decide.count.sum()) > 0
