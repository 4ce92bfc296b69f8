"""K25 (fm_band_stats_cached) and the two-sigma service decision
(fm_decide_services_2s): the band records of a per-metric mix of the static
band models equal K1, K13 and K24 bit for bit in every launch form; hits copy
the cache and read no history; tags tell models and view lengths apart; the
launcher refuses what it cannot take; the decision equals fm_decide_services as
bits where both sigmas are equal and the composed CPU reference where they are
not."""
import numpy as np
import pytest
import torch

from foremast_amd.engine.resident import RowStatsCache
from foremast_amd.ops import canary as C
from foremast_amd.ops import misc as MI
from foremast_amd.ops import smoothing as SM

from boundary import B_EPS, point_boundary
from test_decide_edges import FACTOR, MIN_HIST, P_THR, _combine, _inputs
from test_decide_edges import T as DT

P = 48                                        # physical rows: a multiple of every M below
MS = (1, 3, 8, 16)
KINDS = 6
INVALID = 1                                   # hipErrorInvalidValue


def _code_vectors(M):
    cyc = tuple(m % 3 for m in range(M))
    return [(0,) * M, (1,) * M, (2,) * M] + ([cyc] if M > 1 else [])


def _kind(p):
    return (p // 3) % KINDS


def _rows(T, seed):
    """P rows of length T by kind: 0 noise with scattered NaN, 1 noise with
    NaN in the last quad, 2 constant (both fallback sigmas), 3 99 % zeros with
    a right tail (K24's one-sided fallback), 4 all NaN, 5 plain mixed-sign
    noise (K1's unmasked path)."""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((P, T)) * 5 + 1).astype(np.float32)
    for p in range(P):
        k = _kind(p)
        if k == 0:
            x[p, rng.random(T) < 0.1] = np.nan
        elif k == 1:
            x[p, max(0, T - 2):] = np.nan
        elif k == 2:
            x[p] = 42.0
        elif k == 3:
            x[p] = np.where(rng.random(T) < 0.99, 0.0, rng.exponential(20.0, T) + 1).astype(np.float32)
        elif k == 4:
            x[p] = np.nan
    return x


def _store(x, dev, pad=1e9):
    """The rows on the device, 16-byte aligned with ld % 4 == 0 (K1's rows)
    and garbage past column T."""
    n, T = x.shape
    ld = (T + 3) // 4 * 4 + 4
    h = torch.full((n, ld), pad, dtype=torch.float32, device=dev)
    assert h.data_ptr() % 16 == 0
    h[:, :T] = torch.from_numpy(x).to(dev)
    return h


def _rowmap(M, R, seed):
    """R logical rows over the P physical ones: logical row r reads a physical
    row of its own metric slot (p % M == r % M), so a physical row has one
    code; every slot's rows permuted, the rest duplicates."""
    rng = np.random.default_rng(seed)
    rm = np.empty(R, np.int32)
    for m in range(M):
        idx = np.arange(m, R, M)
        own = np.arange(m, P, M)
        pick = np.concatenate([rng.permutation(own), rng.choice(own, max(0, len(idx) - len(own)))])[:len(idx)]
        rm[idx] = rng.permutation(pick)
    return rm


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _k1(h, T):
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    hs = torch.empty((h.shape[0], 3), dtype=torch.float32, device=h.device)
    LIB.call("fm_hist_stats", ptr(h), h.stride(0), T, h.shape[0], ptr(hs), stream_of(h))
    return torch.stack([hs[:, 0], hs[:, 1], hs[:, 1], hs[:, 2]], 1)


def _per_model(h, T, z0=MI.QUANTILE_TAIL_Z):
    """[3][P, 4]: the record of every physical row under each code, from the
    project's own kernels for K1, K13 and K24."""
    c, s, n = MI.robust_stats(h, T)
    qc, ql, qu, qn = MI.quantile_robust_stats(h, T, z0)
    return [_k1(h, T), torch.stack([c, s, s, n.float()], 1), torch.stack([qc, ql, qu, qn.float()], 1)]


def _want(per, rm, codes):
    R, M = len(rm), len(codes)
    code = torch.tensor([codes[r % M] for r in range(R)], device=per[0].device)
    rows = torch.as_tensor(rm, device=per[0].device).long()
    out = torch.empty((R, 4), dtype=torch.float32, device=per[0].device)
    for k in range(3):
        out[code == k] = per[k][rows[code == k]]
    return out


def _tags(codes, rm, T):
    M = len(codes)
    want = np.zeros(P, np.int64)
    for r, p in enumerate(rm):
        want[p] = MI.band_tag(codes[r % M], T)
    return want


# ---------------------------------------------------------------------- CPU
@pytest.mark.parametrize("M", MS)
def test_cpu_ref_band_stats_is_the_three_references_row_by_row(M):
    T = 37
    x = _rows(T, M)
    codes = [m % 3 for m in range(M)]
    rec, n = MI.ref_band_stats(x, T, codes, 1.5)
    refs = [MI.ref_hist_stats(x, T), MI.ref_robust_stats(x, T), MI.ref_quantile_robust_stats(x, T, 1.5)]
    assert {(codes[p % M], _kind(p)) for p in range(P)} >= {(c, k) for c in set(codes) for k in range(KINDS)}
    for p in range(P):
        c = codes[p % M]
        if c == 2:
            want = [refs[2][0][p], refs[2][1][p], refs[2][2][p], refs[2][3][p]]
        else:
            want = [refs[c][0][p], refs[c][1][p], refs[c][1][p], refs[c][2][p]]
        np.testing.assert_array_equal(rec[p], np.array(want, np.float32), err_msg=f"row {p} code {c}")
        assert n[p] == want[3]
    # an all-NaN row: K1's zeros, the selections' NaN; T == 0: NaN, NaN, NaN, 0
    nan_rows = [p for p in range(P) if _kind(p) == 4]
    for p in nan_rows:
        assert rec[p, 3] == 0 and (np.isnan(rec[p, :3]).all() if codes[p % M] else (rec[p, :3] == 0).all())
    r0, n0 = MI.ref_band_stats(x, 0, codes)
    assert np.isnan(r0[:, :3]).all() and not r0[:, 3].any() and not n0.any()
    # the op on the CPU: the reference over the mapped rows, the cache untouched
    rm = _rowmap(M, 64, 3)
    cache = RowStatsCache(P, "cpu", width=4)
    got = MI.band_stats_cached(torch.from_numpy(x), T, torch.from_numpy(rm), codes, cache, 1.5)
    np.testing.assert_array_equal(got.numpy(), MI.ref_band_stats(x[rm], T, codes, 1.5)[0])
    assert not cache.valid.any()
    with pytest.raises(ValueError):
        MI.ref_band_stats(x, T, [0, 3])
    with pytest.raises(ValueError):
        MI.ref_band_stats(x, T, [0] * 17)


def _tables(M):
    thr = np.tile(np.array([2.0, 3.0, 2.5, 1.5, 2.0, 4.0, 1.0, 3.5], np.float32), 2)[:M]
    bound = np.tile(np.array([3, 1, 2, 3, 1, 2, 3, 1], np.int32), 2)[:M]      # 1 upper, 2 lower, 3 both
    minlb = np.tile(np.array([0.0, 0.0, 9.5, -5.0, 0.0, 9.0, 9.75, 0.0], np.float32), 2)[:M]
    return thr, bound, minlb


def _records(hist, two_sided, seed):
    """Band records of the decision cases: K1's contract of ``hist`` (rows
    below min_hist, without history and with sigma == 0 are among them), and
    for ``two_sided`` each side's sigma scaled by its own factor in [0.5, 2],
    every 5th row with one side's sigma zero."""
    m, s, n = MI.ref_hist_stats(hist, hist.shape[1])
    bs = np.stack([m, s, s, n.astype(np.float32)], 1)
    if two_sided:
        rng = np.random.default_rng(seed)
        f = rng.uniform(0.5, 2.0, (len(bs), 2)).astype(np.float32)
        bs[:, 1] *= f[:, 0]
        bs[:, 2] *= f[:, 1]
        bs[0::10, 1] = 0.0
        bs[5::10, 2] = 0.0
    return bs


def _ref_2s(bs, cur, pv, M, mask, combine_any, with_pv):
    thr, bound, minlb = _tables(M)
    return C.ref_decide_services_2s(bs, cur, M, thr, bound, minlb, FACTOR, MIN_HIST, pv if with_pv else None, mask,
                                    combine_any, P_THR)


def _placed_2s(S, M, n_cur, mask, combine_any, with_pv, two_sided=True):
    """test_decide_edges._placed for band records: every point the reference
    finds within B_EPS of an active edge (distance as boundary.point_boundary,
    the larger sigma as the scale) is moved off it; the points still near are
    returned (none may be)."""
    hist, cur, pv = _inputs(S, M, n_cur)
    bs = _records(hist, two_sided, S + M + n_cur)
    thr, bound, _ = _tables(M)
    for _ in range(2):
        dec, packed, diff = _ref_2s(bs, cur, pv, M, mask, combine_any, with_pv)
        th_rows = np.tile(thr, S) * (np.where(diff.numpy().astype(bool), FACTOR, 1.0) if diff is not None else 1.0)
        st = dec.stats.numpy()
        scale_stats = np.stack([st[:, 0], np.maximum(bs[:, 1], bs[:, 2]), st[:, 2], st[:, 3]], 1)
        near = point_boundary(cur, scale_stats, th_rows, np.tile(bound, S))
        if not near.any():
            break
        scale = np.abs(scale_stats[:, 0:1]) + th_rows[:, None] * np.abs(scale_stats[:, 1:2]) + 1e-6
        cur = np.where(near, cur + (1e3 * B_EPS * scale).astype(np.float32), cur).astype(np.float32)
    return bs, cur, pv, dec, packed.numpy(), diff, near


def test_cpu_ref_decide_services_2s():
    """Equal sigmas: the one-sigma composition CanaryScorer's robust CPU branch
    is made of (ref_band_decide, gate, service_reduce), and C.stats_decide on
    the history the records came from (its bounds are fp64: flags exact on
    placed points, bounds to the canary tests' tolerance).  Two sigmas:
    ref_band_decide_2s + gate + reduce."""
    S, M, n_cur = 5, 3, 50
    thr, bound, minlb = _tables(M)
    t = torch.from_numpy
    for two in (False, True):
        bs, cur, pv, dec, packed, diff, near = _placed_2s(S, M, n_cur, 63, 0, True, two)
        assert not near.any() and int(dec.count.sum()) > 0 and bool(diff.any()) and not bool(diff.all())
        n = bs[:, 3].astype(np.int64)
        has = t((n >= MIN_HIST) & (n > 0))
        assert not bool(has.all()) and bool((bs[:, 2] == 0).any())
        if two:
            up, lo, fl, cnt, sc = SM.ref_band_decide_2s(cur, bs[:, 0:1], bs[:, 1], bs[:, 2], M, thr, bound, minlb,
                                                         diff.numpy(), FACTOR)
            assert bool((bs[:, 1] != bs[:, 2]).any())
        else:
            up, lo, fl, cnt, sc = SM.ref_band_decide(cur, bs[:, 0:1], bs[:, 1], M, thr, bound, minlb, diff.numpy(),
                                                     FACTOR)
        cnt, sc = torch.where(has, cnt, torch.zeros_like(cnt)), torch.where(has, sc, torch.zeros_like(sc))
        fl = torch.where(has[:, None], fl, torch.zeros_like(fl))
        valid = has.to(torch.int32) | (t(np.isfinite(cur).any(1)).to(torch.int32) << 1)
        assert torch.equal(dec.flags, fl) and torch.equal(dec.count, cnt) and torch.equal(dec.valid, valid)
        assert torch.equal(dec.score, sc)
        np.testing.assert_array_equal(dec.stats.numpy(), np.stack([bs[:, 0], bs[:, 2], up[:, 0], lo[:, 0]], 1))
        np.testing.assert_array_equal(packed, C.service_reduce(cnt, sc, valid, M).numpy())
        if not two:
            hist = _inputs(S, M, n_cur)[0]
            old = C.stats_decide(t(hist), t(cur), DT, M, t(thr), t(bound), t(minlb), diff, FACTOR, MIN_HIST)
            assert torch.equal(old.flags, dec.flags) and torch.equal(old.count, dec.count)
            assert torch.equal(old.valid, dec.valid)
            np.testing.assert_allclose(dec.stats.numpy(), old.stats.numpy(), rtol=2e-5, atol=1e-5)
    # the op on CPU tensors is the reference
    o, p2, d2 = C.decide_services_2s(t(bs), t(cur), M, t(thr), t(bound), t(minlb), FACTOR, MIN_HIST, t(pv), 63, 0,
                                     P_THR)
    assert torch.equal(o.flags, dec.flags) and torch.equal(d2, diff) and np.array_equal(p2.numpy(), packed)
    np.testing.assert_array_equal(C.combine_pvalues(pv, 0b101010, 1, P_THR), _combine(pv, 0b101010, 1))


# ---------------------------------------------------------------------- GPU: K25
def _launch(h, T, rm, codes, cache, miss, blocks, z0=MI.QUANTILE_TAIL_Z):
    return MI.band_stats_cached(h, T, rm, codes, cache, z0, expect_miss=miss, blocks=blocks)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 5, 64, 1023, 1443, 10080, 13312, 13316])
def test_gpu_cold_record_equals_the_existing_kernels_as_bits(cuda, T):
    """Every M and code vector at this T; the launch forms (both hints, 1 / 3 /
    default workgroups, no cache, no row map) go round the combinations, each
    on an empty cache.  13316 takes the selections' global-memory form and is
    still within K1's row limit."""
    assert (T > MI.ROBUST_LDS_KEYS) == (T == 13316) and T <= MI.BAND_MEAN_MAX_T
    x = _rows(T, T)
    h = _store(x, cuda)
    per = _per_model(h, T)
    forms = [(True, 0), (False, 0), (False, 1), (True, 3), (False, 3), (True, 1), (None, 0)]
    k = 0
    for M in MS:
        R = 64 if T < 10000 else 48
        rm_h = _rowmap(M, R, 7 * M + T)
        rm = torch.from_numpy(rm_h).to(cuda)
        assert R <= P or len(np.unique(rm_h)) < R               # a permutation; with R > P also duplicates
        for codes in _code_vectors(M):
            want = _want(per, rm_h, codes)
            for _ in range(2 if T < 10000 else 1):
                miss, blocks = forms[k % len(forms)]
                k += 1
                what = (T, M, codes, miss, blocks)
                if miss is None:                               # no cache; also without a row map
                    assert _bits(_launch(h, T, rm, codes, None, None, blocks), want), what
                    ident = _want(per, np.arange(P), codes)
                    assert _bits(_launch(h, T, None, codes, None, None, blocks), ident), what
                    continue
                cache = RowStatsCache(P, cuda, width=4)
                assert _bits(_launch(h, T, rm, codes, cache, miss, blocks), want), what
                v = cache.valid.cpu().numpy().astype(np.int64) & 0xFFFFFFFF
                tags = _tags(codes, rm_h, T)
                assert np.array_equal(v, tags), what
                assert _bits(cache.stats[rm.long()], want), what
                # and from the cache, in the scan form
                assert _bits(_launch(h, T, rm, codes, cache, False, blocks), want), what
    assert k >= len(forms)


@pytest.mark.gpu
def test_gpu_t_zero_records_nothing(cuda):
    x = _rows(8, 1)
    h = _store(x, cuda)
    codes = (0, 1, 2)
    cache = RowStatsCache(P, cuda, width=4)
    for miss in (True, False):
        got = _launch(h, 0, None, codes, cache, miss, 0).cpu().numpy()
        assert np.isnan(got[:, :3]).all() and not got[:, 3].any()
        assert not cache.valid.any()


@pytest.mark.gpu
def test_gpu_hits_read_no_history(cuda):
    T, M, R = 37, 3, 64
    codes = (0, 1, 2)
    x = _rows(T, 11)
    h = _store(x, cuda)
    rm_h = _rowmap(M, R, 5)
    rm = torch.from_numpy(rm_h).to(cuda)
    cache = RowStatsCache(P, cuda, width=4)
    first = _launch(h, T, rm, codes, cache, None, 0).clone()       # the cache's own hint: cold
    assert _bits(first, _want(_per_model(h, T), rm_h, codes)) and cache.dirty == 0
    # new data behind the cache's back: nothing is read
    y = _rows(T, 12)[::-1].copy()
    h[:, :T] = torch.from_numpy(y).to(cuda)
    assert not cache.expect_miss(T, R)
    assert _bits(_launch(h, T, rm, codes, cache, None, 0), first)
    # one row of each code touched (rows whose record the new data changes):
    # exactly their logical rows change
    new = _want(_per_model(h, T), rm_h, codes)
    differs = (new.view(torch.int32) != first.view(torch.int32)).any(1).cpu().numpy()
    sent = [int(rm_h[next(r for r in range(R) if r % M == c and differs[r])]) for c in range(3)]
    assert [codes[p % M] for p in sent] == [0, 1, 2]
    cache.touch(torch.tensor(sent, device=cuda))
    assert cache.dirty == 3 and not cache.expect_miss(T, R)
    got = _launch(h, T, rm, codes, cache, None, 0)
    hit = torch.from_numpy(np.isin(rm_h, sent)).to(cuda)
    assert _bits(got[hit], new[hit]) and _bits(got[~hit], first[~hit])
    changed = (got.view(torch.int32) != first.view(torch.int32)).any(1)
    assert torch.equal(changed, hit)
    assert np.array_equal(cache.valid.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, _tags(codes, rm_h, T))


@pytest.mark.gpu
def test_gpu_tags_tell_view_lengths_models_and_tail_parameters_apart(cuda):
    T, M, R = 40, 3, 64
    x = _rows(T, 21)
    h = _store(x, cuda)
    rm_h = _rowmap(M, R, 6)
    rm = torch.from_numpy(rm_h).to(cuda)
    cache = RowStatsCache(P, cuda, width=4)
    codes = (0, 1, 2)
    per = _per_model(h, T)
    assert _bits(_launch(h, T, rm, codes, cache, True, 0), _want(per, rm_h, codes))
    # another view length: every tag differs
    cache.stats.fill_(-1.0)
    got = _launch(h, T - 3, rm, codes, cache, False, 0)
    assert _bits(got, _want(_per_model(h, T - 3), rm_h, codes))
    assert np.array_equal(cache.valid.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, _tags(codes, rm_h, T - 3))
    # the same physical rows under other models
    other = (2, 0, 1)
    cache.stats.fill_(-1.0)
    per3 = _per_model(h, T - 3)
    got = _launch(h, T - 3, rm, other, cache, False, 0)
    assert _bits(got, _want(per3, rm_h, other))
    assert np.array_equal(cache.valid.cpu().numpy().astype(np.int64) & 0xFFFFFFFF, _tags(other, rm_h, T - 3))
    assert not (cache.stats[rm.long()] == -1.0).any()
    # another tail parameter: the code-2 rows are made again, nothing stale
    assert cache.z0 == MI.QUANTILE_TAIL_Z and cache.dirty == 0
    cache.stats.fill_(-1.0)
    got = _launch(h, T - 3, rm, other, cache, None, 0, z0=1.0)
    assert cache.z0 == 1.0
    want = _want(_per_model(h, T - 3, 1.0), rm_h, other)
    assert _bits(got, want) and not (got == -1.0).any()
    code2 = torch.tensor([other[r % M] == 2 for r in range(R)], device=cuda)
    old = _want(per3, rm_h, other)
    assert _bits(got[~code2], old[~code2]) and not _bits(got[code2], old[code2])
    assert _bits(_launch(h, T - 3, rm, other, cache, None, 0, z0=1.0), want)      # and the hits


@pytest.mark.gpu
def test_gpu_launcher_refuses(cuda):
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    fn = LIB.load().fm_band_stats_cached
    T, R, M = 16, 6, 3
    big = torch.zeros((2, 16392), dtype=torch.float32, device=cuda)
    flat = torch.zeros((R * 24 + 8,), dtype=torch.float32, device=cuda)
    h = flat[:R * 20].view(R, 20)
    h_odd = flat[:R * 21].view(R, 21)                                  # ld % 4 != 0
    h_off = flat[1:1 + R * 20].view(R, 20)                             # 4 bytes past a 16-byte boundary
    out = torch.empty((R, 4), dtype=torch.float32, device=cuda)
    cache = RowStatsCache(R + 1, cuda, width=4)
    off_cache = cache.stats.view(-1)[1:]                               # not 16-byte aligned
    codes = torch.tensor([0, 1, 2], dtype=torch.int32, device=cuda)
    p, iz = MI.quantile_tail_params(2.0)
    st = stream_of(h)

    def call(hist=h, ld=None, T=T, R=R, M=M, mask=7, p=p, iz=float(iz), cache_p=ptr(cache.stats),
             valid_p=ptr(cache.valid), out_p=ptr(out)):
        return fn(ptr(hist), hist.stride(0) if ld is None else ld, T, R, M, ptr(codes), mask, p, iz, out_p, None,
                  cache_p, valid_p, 0, 0, st)
    assert call() == 0
    assert call(mask=8) == INVALID and call(mask=15) == INVALID and call(mask=0) == INVALID
    assert call(M=0) == INVALID and call(M=17) == INVALID
    assert call(valid_p=None) == INVALID
    assert call(cache_p=off_cache.data_ptr()) == INVALID
    assert call(hist=h_odd) == INVALID and call(hist=h_odd, mask=6) == 0       # only K1 needs the alignment
    assert call(hist=h_off) == INVALID and call(hist=h_off, mask=6) == 0
    assert call(hist=big, T=16385, R=2) == INVALID and call(hist=big, T=16385, R=2, mask=6) == 0
    assert call(T=1 << 28) == INVALID and call(T=-1) == INVALID
    for bad in (0.4, 1.5, float("nan")):
        assert call(p=bad) == INVALID and call(p=bad, mask=3) == 0             # K24's ranges, with code 2 only
    assert call(iz=0.0) == INVALID and call(iz=-1.0) == INVALID and call(iz=0.0, mask=3) == 0
    assert call(R=0, out_p=None, cache_p=None, valid_p=None) == 0              # a no-op
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        MI.band_stats_cached(h, T, None, (0, 1, 2), RowStatsCache(R, cuda))    # a 3-float cache


# ---------------------------------------------------------------------- GPU: the decision
def _gpu_decide(cuda, name, stats_in, cur, pv, S, M, mask, combine_any, with_pv):
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    thr, bound, minlb = _tables(M)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    R, n_cur = cur.shape
    s_in, c, p = t(stats_in), t(cur), (t(pv) if with_pv else None)
    thr_d, bound_d, minlb_d = t(thr), t(bound), t(minlb)
    o = C.alloc_decide(R, n_cur, cuda)
    for x in (o.stats, o.score):
        x.fill_(float("nan"))
    for x in (o.flags, o.count, o.valid):
        x.fill_(-7)
    diff = torch.full((R,), -7, dtype=torch.int8, device=cuda)
    packed = torch.full((S, 4), float("nan"), device=cuda)
    LIB.call(name, ptr(s_in), ptr(c), c.stride(0), n_cur, S, M, ptr(thr_d), ptr(bound_d), ptr(minlb_d), FACTOR,
             ptr(p), mask, combine_any, P_THR, MIN_HIST, ptr(o.stats), ptr(o.flags), o.flags.shape[1], ptr(o.count),
             ptr(o.score), ptr(o.valid), ptr(diff), ptr(packed), stream_of(c))
    torch.cuda.synchronize()
    return o, diff, packed


DECIDE_M = (1, 3, 4, 8, 9, 16)
DECIDE_N = (1, 63, 64, 65, 130)
DECIDE_CFG = ((63, 0, True), (63, 1, True), (0b101010, 0, True), (63, 0, False))


@pytest.mark.gpu
@pytest.mark.parametrize("M", DECIDE_M)
def test_gpu_decision_with_symmetric_records_is_fm_decide_services(cuda, M):
    """sigma_lo == sigma_up: every output array as bits, for every window
    width, with and without p-values, both combine modes; the cases hold rows
    below min_hist, without history, with sigma == 0 and an all-NaN window."""
    for n_cur in DECIDE_N:
        for mask, combine_any, with_pv in DECIDE_CFG:
            S = 5 if M > 1 else 12
            hist, cur, pv = _inputs(S, M, n_cur)
            bs = _records(hist, False, 0)
            n = bs[:, 3]
            assert ((n > 0) & (n < MIN_HIST)).any() and (n == 0).any() and ((bs[:, 1] == 0) & (n >= MIN_HIST)).any()
            assert (~np.isfinite(cur)).all(1).any()
            a, da, pa = _gpu_decide(cuda, "fm_decide_services", bs[:, [0, 1, 3]], cur, pv, S, M, mask, combine_any,
                                    with_pv)
            b, db, pb = _gpu_decide(cuda, "fm_decide_services_2s", bs, cur, pv, S, M, mask, combine_any, with_pv)
            what = (M, n_cur, mask, combine_any, with_pv)
            assert _bits(a.stats, b.stats) and _bits(a.score, b.score) and _bits(pa, pb), what
            assert torch.equal(a.flags, b.flags) and torch.equal(a.count, b.count), what
            assert torch.equal(a.valid, b.valid) and torch.equal(da, db), what
            assert int(a.count.sum()) > 0 and (with_pv or bool((db == -7).all())), what


def _score_tol(stats, bs, bound_rows, z):
    """test_decide_edges' bound on the score error, per side: the edge and the
    sigma of the side a point left carry tol(v) = 2e-5 |v| + 1e-5, plus the
    1-ulp reciprocal and two roundings; a row's score is the largest of its
    points', so its error is within the larger of its active sides' bounds at
    the row's own |z|.  A side whose sigma is not positive scores the constant
    1e30 on both sides."""
    tol = lambda v: 2e-5 * np.abs(v) + 1e-5
    out = np.zeros(len(z))
    for side, edge, bit in ((bs[:, 2], stats[:, 2], 1), (bs[:, 1], stats[:, 3], 2)):
        sd = side.astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            t_side = np.where(sd > 0, (tol(edge.astype(np.float64)) + np.abs(z) * tol(sd)) / sd + 1e-6 * np.abs(z), 0.0)
        out = np.maximum(out, np.where((bound_rows & bit) != 0, t_side, 0.0))
    return np.where(z >= 1e30, 0.0, out)


@pytest.mark.gpu
@pytest.mark.parametrize("M", DECIDE_M)
def test_gpu_decision_with_two_sigmas_matches_the_reference(cuda, M):
    for n_cur in DECIDE_N:
        for mask, combine_any, with_pv in DECIDE_CFG:
            S = 5 if M > 1 else 12
            what = f"M={M} n_cur={n_cur} mask={mask} any={combine_any} pvals={with_pv}"
            bs, cur, pv, dec, want_packed, want_diff, near = _placed_2s(S, M, n_cur, mask, combine_any, with_pv)
            assert not near.any(), what                       # no point near an edge: the share allowed is zero
            assert (bs[:, 1] != bs[:, 2]).any() and int(dec.count.sum()) > 0, what
            o, diff, packed = _gpu_decide(cuda, "fm_decide_services_2s", bs, cur, pv, S, M, mask, combine_any, with_pv)
            stats, want_stats = o.stats.cpu().numpy(), dec.stats.numpy()
            np.testing.assert_allclose(stats, want_stats, rtol=2e-5, atol=1e-5, err_msg=what)
            np.testing.assert_array_equal(o.flags.cpu().numpy(), dec.flags.numpy(), err_msg=what)
            np.testing.assert_array_equal(o.count.cpu().numpy(), dec.count.numpy(), err_msg=what)
            np.testing.assert_array_equal(o.valid.cpu().numpy(), dec.valid.numpy(), err_msg=what)
            if with_pv:
                np.testing.assert_array_equal(diff.cpu().numpy(), want_diff.numpy(), err_msg=what)
            else:
                assert bool((diff == -7).all()), what
            score, want_score = o.score.cpu().numpy().astype(np.float64), dec.score.numpy().astype(np.float64)
            tol = _score_tol(want_stats, bs, np.tile(_tables(M)[1], S), want_score)
            print(what, "max score error / bound", float(np.max(np.abs(score - want_score) / np.maximum(tol, 1e-30),
                                                                  where=tol > 0, initial=0.0)))
            assert (np.abs(score - want_score) <= tol).all(), what
            packed = packed.cpu().numpy()
            np.testing.assert_array_equal(packed[:, [0, 2, 3]], want_packed[:, [0, 2, 3]], err_msg=what)
            np.testing.assert_array_equal(packed[:, 1], np.maximum(score.reshape(S, M).max(1), 0).astype(np.float32),
                                          err_msg=what)
