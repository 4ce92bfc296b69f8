"""The steady front kernel's raw row statistics (tick_front_dyn_kernel,
csrc/kernels/tick_front.hip): a rank-test row leaves its 14 statistics as raw
integer / float words in the workgroup's LDS, and the workgroup converts its
rows to the doubles of ``suff`` one row per thread behind its barrier, before
the p-values.  The launch must still give exactly what the separate kernels
give -- fm_pairwise_suff (``suff``, raw fp64 bits), fm_pvalues_only (``pvals``,
``pstats``) and fm_hist_stats (``hs``): rtol = atol = 0.  Every output is
NaN-filled before each launch and the queue words must be zero afterwards
(the method of test_front_dynamic.py).

Shapes: R around the sizes at which the convert step changes -- fewer rows
than waves (R <= 3), one row per thread up to the 256 a workgroup's four wave
lists hold (R = 255 / 256 with one workgroup: every list fills to its cap),
and one past it (R = 257: the plan must add a workgroup); every sort layout
(K = 1, the split and the pooled K = 2, K = 4); rows that take every branch of
the conversion (no current sample: the D = 0 branch; one tie run; no non-zero
difference) and the tie / zero / NaN / subnormal rows of test_pairwise_lean.py's
generator."""
import ctypes

import numpy as np
import pytest
import torch

from foremast_amd.ops import canary as C

T, RMAX, CAP = 101, 257, 64
WINDOWS = {"1x1": (1, 1), "10x10": (10, 10), "50x50": (50, 50), "64x64": (64, 64), "65x63": (65, 63),
           "130x100": (130, 100)}
ROWS = (1, 2, 3, 5, 63, 64, 65, 255, 256, 257)
NPS = (0, 1)
QS = (1, 64)
MIN = 2                                          # min_mw / min_wil / min_kru
KINDS = 13


def _plan(R, n_p, q, scan):
    from foremast_amd.ops._lib import LIB
    out = (ctypes.c_int64 * 4)()
    LIB.call("fm_front_plan", R, n_p, q, scan, ctypes.cast(out, ctypes.c_void_p))
    return tuple(out)                            # static rows per wave, pool start, ranges, effective nP


def _row(kind, rng, n1, n2):
    """One (current, baseline) row; kinds 5 .. 12 re-state the patterns of
    test_pairwise_lean.py."""
    npair = min(n1, n2)
    c = rng.normal(10.0, 3.0, n1).astype(np.float32)
    b = rng.normal(10.5, 3.0, n2).astype(np.float32)
    if kind == 1:                                # rounded: ties and zero differences
        c, b = np.round(c), np.round(b)
    elif kind == 2:                              # no current sample: n1 = 0, D = 0 without a division
        c[:] = np.nan
    elif kind == 3:                              # no baseline sample
        b[:] = np.nan
    elif kind == 4:                              # all equal: one tie run, the largest tie term
        c[:], b[:] = 3.25, 3.25
    elif kind == 5:                              # every paired difference zero: nw = 0
        c[:npair] = b[:npair]
    elif kind == 6:                              # three values: long tie runs across both samples
        vals = np.array([1.5, 2.5, 7.0], np.float32)
        c, b = vals[rng.integers(0, 3, n1)], vals[rng.integers(0, 3, n2)]
    elif kind == 7:                              # signed zeros
        z = np.array([0.0, -0.0], np.float32)
        c, b = z[rng.integers(0, 2, n1)], z[rng.integers(0, 2, n2)]
    elif kind == 8:                              # NaN and both infinities
        for a in (c, b):
            a[rng.random(a.shape) < 0.1] = np.nan
            a[rng.integers(0, len(a))] = np.inf
            a[rng.integers(0, len(a))] = -np.inf
    elif kind == 9:                              # negative values
        c, b = -c, (5.0 - b).astype(np.float32)
    elif kind == 10:                             # |d| equal, signs opposite, in many pairs
        b = rng.integers(0, 50, n2).astype(np.float32)
        c = rng.integers(0, 50, n1).astype(np.float32)
        k = rng.integers(1, 4, npair).astype(np.float32) * np.where(rng.random(npair) < 0.5, -1, 1)
        c[:npair] = b[:npair] + k
    elif kind == 11:                             # differences are fp32 subnormals
        tiny = np.float32(2.0 ** -149)
        mb, mc = rng.integers(1, 1 << 12, n2), rng.integers(1, 1 << 12, n1)
        mc[:npair] = mb[:npair] + rng.integers(-40, 41, npair)
        c, b = (np.maximum(mc, 0) * tiny).astype(np.float32), (mb * tiny).astype(np.float32)
    elif kind == 12:                             # half the current window missing
        c[: (n1 + 1) // 2] = np.nan
    return c.astype(np.float32), b.astype(np.float32)


class _Data:
    """One window shape: inputs for RMAX rows and the separate kernels' outputs
    (computed once; rows are independent, so R rows are the first R of them)."""

    def __init__(self, dev, n_cur, n_base, seed):
        from foremast_amd.ops._lib import LIB, ptr, stream_of
        rng = np.random.default_rng(seed)
        ld = (T + 3) // 4 * 4
        h = np.full((RMAX, ld), np.nan, np.float32)
        h[:, :T] = rng.normal(10.0, 3.0, (RMAX, T))
        h[1, 20:60] = np.nan                     # the masked path
        h[2, :] = np.nan                         # no history at all
        cur, base = np.empty((RMAX, n_cur), np.float32), np.empty((RMAX, n_base), np.float32)
        for r in range(RMAX):                    # rows 0 .. 4 (the smallest R) start with the conversion's branches
            cur[r], base[r] = _row((2, 4, 5, 0, 3)[r] if r < 5 else r % KINDS, rng, n_cur, n_base)
        self.h, self.cur, self.base = (torch.from_numpy(a).to(dev) for a in (h, cur, base))
        self.n_cur, self.n_base = n_cur, n_base
        st = stream_of(self.h)
        self.suff = torch.full((RMAX, C.SUFF), float("nan"), dtype=torch.float64, device=dev)
        self.pvals = torch.full((RMAX, C.N_TESTS), float("nan"), device=dev)
        self.pstats = torch.full((RMAX, C.N_TESTS), float("nan"), device=dev)
        self.hs = torch.full((RMAX, 3), float("nan"), device=dev)
        LIB.call("fm_pairwise_suff", ptr(self.cur), self.cur.stride(0), n_cur, ptr(self.base), self.base.stride(0),
                 n_base, RMAX, ptr(self.suff), 0, st)
        LIB.call("fm_pvalues_only", ptr(self.suff), RMAX, MIN, MIN, MIN, ptr(self.pvals), ptr(self.pstats), st)
        LIB.call("fm_hist_stats", ptr(self.h), self.h.stride(0), T, RMAX, ptr(self.hs), st)
        torch.cuda.synchronize()
        # the rows do take the conversion's branches
        s = self.suff.cpu().numpy()
        assert s[0, 0] == 0 and s[0, 5] == 0                        # n1 = 0
        assert s[2, 2] == 0 or min(n_cur, n_base) == 0              # nw = 0
        n = n_cur + n_base
        assert s[1, 4] == n ** 3 - n                                # one tie run
        # work buffers
        self.o_suff = torch.empty_like(self.suff)
        self.o_pvals, self.o_pstats = torch.empty_like(self.pvals), torch.empty_like(self.pstats)
        self.o_hs = torch.empty((RMAX, 3), device=dev)
        self.queue = torch.zeros(8 * 32 + 64, dtype=torch.int32, device=dev)
        self.pq = torch.zeros(64 * 32, dtype=torch.int32, device=dev)


def _launch(d, R, n_p, q, cache):
    """The scan shape (a cache and no miss expected) with a pqueue."""
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    for t in (d.o_suff, d.o_pvals, d.o_pstats, d.o_hs):
        t.fill_(float("nan"))
    LIB.call("fm_tick_front", ptr(d.h), d.h.stride(0), T, R, ptr(d.o_hs), ptr(d.cur), d.cur.stride(0), d.n_cur,
             ptr(d.base), d.base.stride(0), d.n_base, ptr(d.o_suff), n_p, 0, MIN, MIN, MIN, ptr(d.o_pvals),
             ptr(d.o_pstats), ptr(d.queue), None, ptr(cache.stats), ptr(cache.valid), 0, ptr(d.pq), q,
             stream_of(d.h))
    torch.cuda.synchronize()


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _check(d, R, what):
    assert torch.equal(_bits(d.o_suff[:R]), _bits(d.suff[:R])), f"suff {what}"
    torch.testing.assert_close(d.o_pvals[:R], d.pvals[:R], rtol=0, atol=0, equal_nan=True, msg=f"pvals {what}")
    torch.testing.assert_close(d.o_pstats[:R], d.pstats[:R], rtol=0, atol=0, equal_nan=True, msg=f"pstats {what}")
    torch.testing.assert_close(d.o_hs[:R], d.hs[:R], rtol=0, atol=0, equal_nan=True, msg=f"hs {what}")
    # nothing past the rows asked for, and the queues are ready for the next launch
    assert torch.isnan(d.o_suff[R:]).all() and torch.isnan(d.o_pvals[R:]).all(), f"rows past R {what}"
    assert not d.pq.any(), f"pqueue not reset {what}"
    assert not d.queue[:256].any(), f"history queue not reset {what}"


def test_front_plan_lets_one_workgroup_fill_its_lists():
    """Host only.  R = 256 on one requested workgroup: the plan keeps nP = 1,
    so its four wave lists hold 4 x 64 = R rows and every one of them fills to
    the cap; one row more and the plan adds a workgroup."""
    for q in QS:
        s, pool0, qe, npe = _plan(256, 1, q, 1)
        assert npe == 1 and qe == 1 and 4 * npe * CAP == 256 and s < CAP and pool0 == 4 * s
        assert _plan(257, 1, q, 1)[3] >= 2
        assert _plan(255, 1, q, 1)[3] == 1


@pytest.mark.gpu
@pytest.mark.parametrize("win", list(WINDOWS))
def test_gpu_raw_stats_rows_equal_the_separate_kernels(cuda, win):
    from foremast_amd.engine.resident import RowStatsCache
    d = _Data(cuda, *WINDOWS[win], seed=100 + list(WINDOWS).index(win))
    cache = RowStatsCache(RMAX, cuda)
    for R in ROWS:
        for n_p in NPS:
            for q in QS:
                outs = []
                for k in range(3):               # the same buffers three times (the first fills the cache)
                    _launch(d, R, n_p, q, cache)
                    _check(d, R, f"{win} R={R} nP={n_p} q={q} launch {k}")
                    outs.append((_bits(d.o_suff).clone(), _bits(d.o_pvals).clone(), _bits(d.o_pstats).clone()))
                for o in outs[1:]:
                    assert all(torch.equal(a, b) for a, b in zip(o, outs[0]))
        cache.invalidate()
        torch.cuda.synchronize()
