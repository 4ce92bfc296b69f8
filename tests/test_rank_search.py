"""Search form of the pooled ranks in the front kernels with a baseline cache
(csrc/include/fm_pairwise.h pw_rank_search): a row without a tie in its pooled
sample is ranked by a binary search of each current value in the sorted
baseline instead of the tagged 128-merge; a row with any tie takes the merge.
Either way the 14 ``suff`` words, ``pvals`` and ``pstats`` are those of the
separate kernels fm_pairwise_suff (which ranks by the merge) and
fm_pvalues_only, bit for bit (rtol = atol = 0).

Unlike the rounded samples of the other front-kernel tests, most rows here are
tie-free -- a permutation of distinct values dealt to the two samples -- so
the search arm is what runs; the first rows are crafted edge cases, each
checked on the CPU to be what its name says.  Every (shape, launch form) is
ticked twice with one cache: all rows miss, then all rows hit.  The whole set
runs once more in a child process with FM_RANK_SEARCH=0 (the switch is read
once per process): the kernels compiled without the search form.

The CPU test pins the integer identities the kernel implements down against
the pooled-order definition."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

T, RMAX, MIN = 64, 1030, 2
SHAPES = {"50x50": (50, 50), "64x64": (64, 64), "1x64": (1, 64), "64x1": (64, 1)}
FORMS = {"dynamic": (8, 64, 0), "static": (2, 0, 1)}      # n_p, q_ranges, expect_miss
FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN = float(np.finfo(np.float32).tiny)


# ---- CPU: the identities ----------------------------------------------------
def _pooled(x, y):
    """r1x2, tie, dnum of finite samples x, y by the pooled-order definition
    (what the merge computes): doubled average ranks, sum t^3 - t over tie
    runs, max |a1 n2 - a2 n1| over the pooled points' "<=" counts."""
    n1, n2 = len(x), len(y)
    v = np.concatenate([x, y])
    lt = (v[None, :] < v[:, None]).sum(1)
    eq = (v[None, :] == v[:, None]).sum(1)
    r2 = 2 * lt + eq + 1
    tie = int((eq * eq - 1).sum())
    a1 = (x[None, :] <= v[:, None]).sum(1)
    a2 = (y[None, :] <= v[:, None]).sum(1)
    dnum = int(np.abs(a1 * n2 - a2 * n1).max()) if n1 > 0 and n2 > 0 else 0
    return int(r2[:n1].sum()), tie, dnum


def _counts(x, y):
    xs = np.sort(x)
    return xs, (y[None, :] < xs[:, None]).sum(1).astype(np.int64)


def _search_stated(x, y):
    """The identities as the change was specified: per current lane i the
    candidates at x_i, at the first and last baseline point of the gap below
    it (when the gap has any), and once the gap above the largest."""
    n1, n2 = len(x), len(y)
    _, c = _counts(x, y)
    i = np.arange(n1)
    r1x2 = int((2 * (i + c) + 2).sum())
    cp = np.concatenate([[0], c[:-1]])
    d = np.abs((i + 1) * n2 - c * n1)
    gap = c > cp
    d = np.maximum(d, np.where(gap, np.abs(i * n2 - c * n1), 0))
    d = np.maximum(d, np.where(gap, np.abs(i * n2 - (cp + 1) * n1), 0))
    dnum = int(d.max())
    if c[-1] < n2:
        dnum = max(dnum, abs(n1 * n2 - (c[-1] + 1) * n1))
    return r1x2, dnum


def _search_kernel(x, y):
    """The same maximum as the kernel forms it: e_i = i n2 - c_i n1, the
    candidates |e_i + n2|, |e_i| (unconditional) and |e'_i| with
    e'_i = e_(i-1) + n2 - n1 (e'_0 = -n1) where e'_i >= e_i; no candidate for
    the gap above the largest current value."""
    n1, n2 = len(x), len(y)
    _, c = _counts(x, y)
    i = np.arange(n1)
    e = i * n2 - c * n1
    e1 = np.concatenate([[-n2], e[:-1]]) + n2 - n1
    d = np.maximum(np.abs(e + n2), np.abs(e))
    d = np.maximum(d, np.where(e1 >= e, np.abs(e1), 0))
    return int((2 * (i + c) + 2).sum()), int(d.max())


def test_search_identities_equal_the_pooled_order():
    rng = np.random.default_rng(5)
    sizes = [(1, 1), (1, 64), (64, 1), (64, 64), (50, 50), (2, 63)]
    sizes += [tuple(rng.integers(1, 65, 2)) for _ in range(1500)]
    for k, (n1, n2) in enumerate(sizes):
        pool = rng.permutation(4 * (n1 + n2))[: n1 + n2].astype(np.float64)
        if k % 3 == 1:       # one sample mostly below the other
            pool = np.sort(pool)
            pool[:n1] = rng.permutation(pool[:n1])
        x, y = pool[:n1], pool[n1:]
        if k % 3 == 2:
            x, y = np.sort(x), np.sort(y)[::-1]
        r1x2, tie, dnum = _pooled(x, y)
        assert tie == 0
        assert _search_stated(x, y) == (r1x2, dnum), (n1, n2, k)
        assert _search_kernel(x, y) == (r1x2, dnum), (n1, n2, k)


# ---- inputs -----------------------------------------------------------------
def _tie_free(rows, n_cur, n_base, g):
    """Each row: a permutation of n distinct values dealt to cur and base."""
    n = n_cur + n_base
    perm = torch.rand(rows, n, generator=g).argsort(dim=1).float()
    vals = (perm - n / 2) * 0.37 + 0.01 * (torch.arange(rows) % 11)[:, None].float()
    return vals[:, :n_cur].clone(), vals[:, n_cur:].clone()


def _finite(t):
    return t[torch.isfinite(t)]


def _ties(c, b):
    """(pairs equal inside cur, inside base, across), float == on the finite values."""
    c, b = _finite(c), _finite(b)
    inside = lambda v: int(((v[:, None] == v[None, :]).sum() - len(v)) // 2)
    return inside(c), inside(b), int((c[:, None] == b[None, :]).sum())


def _bits(t):
    return t.view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _crafted(n_cur, n_base):
    """[(name, cur row, base row)], each asserted to be what it is named for.
    A case a shape cannot hold (a tie inside a one-value sample) is left out."""
    g = torch.Generator().manual_seed(99)
    fresh = lambda: tuple(t[0] for t in _tie_free(1, n_cur, n_base, g))
    n, m = n_cur + n_base, min(n_cur, n_base)
    out = []

    c, b = torch.randperm(n_cur, generator=g).float() - 1000.0, torch.randperm(n_base, generator=g).float() + 1000.0
    assert c.max() < b.min() and _ties(c, b) == (0, 0, 0)
    out.append(("cur below base", c, b))
    c, b = torch.randperm(n_cur, generator=g).float() + 1000.0, torch.randperm(n_base, generator=g).float() - 1000.0
    assert b.max() < c.min() and _ties(c, b) == (0, 0, 0)
    out.append(("base below cur", c, b))

    # strictly alternating while both samples last: cur 0, 2, 4, ..., base 1, 3, 5, ...
    c, b = 2.0 * torch.arange(n_cur).float(), 2.0 * torch.arange(n_base).float() + 1.0
    tags = torch.cat([torch.zeros(n_cur), torch.ones(n_base)])[torch.cat([c, b]).argsort()]
    assert (tags[: 2 * m : 2] == 0).all() and (tags[1 : 2 * m : 2] == 1).all() and _ties(c, b) == (0, 0, 0)
    out.append(("alternating", c.flip(0), b))

    c, b = fresh()
    c[n_cur // 2] = b[n_base // 3]
    assert _ties(c, b) == (0, 0, 1)
    out.append(("one cross tie", c, b))
    if n_cur >= 2:
        c, b = fresh()
        c[0] = c[n_cur - 1]
        assert _ties(c, b) == (1, 0, 0)
        out.append(("one tie inside cur", c, b))
    if n_base >= 2:
        c, b = fresh()
        b[n_base - 1] = b[0]
        assert _ties(c, b) == (0, 1, 0)
        out.append(("one tie inside base", c, b))

    c, b = fresh()
    c, b = c + 100.0, b + 100.0           # no other value near zero
    c[0], b[n_base - 1] = 0.0, -0.0
    assert _bits(c)[0] == 0 and _bits(b)[n_base - 1] == -2 ** 31 and _ties(c, b) == (0, 0, 1)
    out.append(("+0.0 against -0.0", c, b))

    c, b = fresh()
    c[: max(1, n_cur // 2)] = float("nan")
    assert torch.isfinite(c).sum() < n_cur and _ties(c, b) == (0, 0, 0)
    out.append(("NaNs in cur", c, b))
    c, b = fresh()
    c[:] = float("nan")
    assert not torch.isfinite(c).any()
    out.append(("all-NaN cur", c, b))
    c, b = fresh()
    b[:] = float("nan")
    assert not torch.isfinite(b).any()
    out.append(("all-NaN base", c, b))

    c, b = fresh()
    b[0] = float("inf")
    if n_base >= 2:
        b[n_base - 1] = float("-inf")
    assert torch.isinf(b).sum() == min(2, n_base) and _ties(c, b) == (0, 0, 0)
    out.append(("inf in base", c, b))

    # subnormals of both signs, built as bit patterns (700 ulp apart)
    k = torch.randperm(n, generator=g).int() + 1
    sub = (k * 700) | ((k % 2) << 31)
    v = sub.view(torch.float32)
    assert (v.abs() < FLT_MIN).all() and (v != 0).all() and len(set(sub.tolist())) == n
    c, b = v[:n_cur].clone(), v[n_cur:].clone()
    assert _ties(c, b) == (0, 0, 0)
    out.append(("subnormals", c, b))

    # within 2^-12 of FLT_MAX: cur at the top, base at the bottom of the range
    k = torch.randperm(n, generator=g).double()
    v = (FLT_MAX * (1.0 - k * 2.0 ** -20)).float()
    assert torch.isfinite(v).all() and (v > FLT_MAX * (1 - 2.0 ** -12)).all() and len(set(v.tolist())) == n
    c, b = v[:n_cur].clone(), -v[n_cur:].clone()
    assert _ties(c, b) == (0, 0, 0)
    out.append(("near FLT_MAX", c, b))
    return out


def _inputs(n_cur, n_base, seed):
    g = torch.Generator().manual_seed(seed)
    cur, base = _tie_free(RMAX, n_cur, n_base, g)
    crafted = _crafted(n_cur, n_base)
    for r, (_, c, b) in enumerate(crafted):
        cur[r], base[r] = c, b
    # a tenth of the remaining rows rounded, as in the other front-kernel tests: ties of every kind
    rows = torch.arange(len(crafted) + 5, RMAX, 13)
    cur[rows] = torch.round(cur[rows])
    base[rows] = torch.round(base[rows])
    return cur, base, [name for name, _, _ in crafted]


def _tie_free_share(cur, base):
    v = torch.cat([cur, base], dim=1).clone()
    v[~torch.isfinite(v)] = float("inf")
    s = v.sort(dim=1).values
    tied = ((s[:, 1:] == s[:, :-1]) & torch.isfinite(s[:, 1:])).any(dim=1)
    return 1.0 - tied.float().mean().item()


def test_inputs_are_mostly_tie_free():
    for k, (n_cur, n_base) in enumerate(SHAPES.values()):
        cur, base, names = _inputs(n_cur, n_base, 40 + k)
        assert _tie_free_share(cur, base) >= 0.9
        assert len(names) >= 11 and "one cross tie" in names and "alternating" in names


# ---- GPU --------------------------------------------------------------------
class _Data:
    """One window shape: inputs, the oracle's outputs (computed once), work
    buffers, queues and the baseline cache."""

    def __init__(self, dev, n_cur, n_base, seed):
        from foremast_amd.engine.resident import RowStatsCache
        from foremast_amd.ops import canary as C
        from foremast_amd.ops._lib import LIB, ptr, stream_of
        g = torch.Generator().manual_seed(seed + 100)
        self.h = (torch.randn(RMAX, T, generator=g) * 3.0 + 10.0).to(dev)
        cur, base, self.names = _inputs(n_cur, n_base, seed)
        assert _tie_free_share(cur, base) >= 0.9
        self.cur, self.base = cur.to(dev), base.to(dev)
        self.n_cur, self.n_base = n_cur, n_base
        self.suff = torch.full((RMAX, C.SUFF), float("nan"), dtype=torch.float64, device=dev)
        self.pvals = torch.full((RMAX, C.N_TESTS), float("nan"), device=dev)
        self.pstats = torch.full((RMAX, C.N_TESTS), float("nan"), device=dev)
        st = stream_of(self.cur)
        LIB.call("fm_pairwise_suff", ptr(self.cur), self.cur.stride(0), n_cur, ptr(self.base), self.base.stride(0),
                 n_base, RMAX, ptr(self.suff), 0, st)
        LIB.call("fm_pvalues_only", ptr(self.suff), RMAX, MIN, MIN, MIN, ptr(self.pvals), ptr(self.pstats), st)
        torch.cuda.synchronize()
        assert not torch.isnan(self.suff[:, :3]).any()
        self.o_suff = torch.empty_like(self.suff)
        self.o_pvals, self.o_pstats = torch.empty_like(self.pvals), torch.empty_like(self.pstats)
        self.o_hs = torch.empty((RMAX, 3), device=dev)
        self.queue = torch.zeros(8 * 32 + 64, dtype=torch.int32, device=dev)
        self.pq = torch.zeros(64 * 32, dtype=torch.int32, device=dev)
        self.hcache = RowStatsCache(RMAX, dev)
        self.bc = [torch.zeros((RMAX, w), dtype=torch.int32, device=dev) for w in (64, 64, 4)]


_DATA = {}


def _data(dev, key):
    if key not in _DATA:
        _DATA[key] = _Data(dev, *SHAPES[key], seed=40 + list(SHAPES).index(key))
    return _DATA[key]


def _launch(d, n_p, q, miss):
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    for t in (d.o_suff, d.o_pvals, d.o_pstats, d.o_hs):
        t.fill_(float("nan"))
    LIB.call("fm_tick_front_bc", ptr(d.h), d.h.stride(0), T, RMAX, ptr(d.o_hs), ptr(d.cur), d.cur.stride(0), d.n_cur,
             ptr(d.base), d.base.stride(0), d.n_base, ptr(d.o_suff), n_p, 0, MIN, MIN, MIN, ptr(d.o_pvals),
             ptr(d.o_pstats), ptr(d.queue), None, ptr(d.hcache.stats), ptr(d.hcache.valid), miss, ptr(d.pq), q,
             *[ptr(t) for t in d.bc], stream_of(d.h))
    torch.cuda.synchronize()


def _check(d, what):
    bad = (_bits(d.o_suff) != _bits(d.suff)).any(dim=1).nonzero().flatten().tolist()
    named = [d.names[r] if r < len(d.names) else r for r in bad[:8]]
    assert not bad, f"suff {what}: {len(bad)} rows differ, first {named}"
    torch.testing.assert_close(d.o_pvals, d.pvals, rtol=0, atol=0, equal_nan=True, msg=f"pvals {what}")
    torch.testing.assert_close(d.o_pstats, d.pstats, rtol=0, atol=0, equal_nan=True, msg=f"pstats {what}")
    assert not d.pq.any(), f"pqueue not reset {what}"
    assert not d.queue[:256].any(), f"history queue not reset {what}"


def _miss_then_hit(dev, win, form):
    d = _data(dev, win)
    n_p, q, miss = FORMS[form]
    for t in d.bc:
        t.zero_()
    _launch(d, n_p, q, miss)
    _check(d, f"{win} {form}, every row misses")
    assert (d.bc[2][:, 3] == d.n_base).all()
    snap = [t.clone() for t in d.bc]
    _launch(d, n_p, q, miss)
    _check(d, f"{win} {form}, every row hits")
    assert all(torch.equal(a, b) for a, b in zip(snap, d.bc)), f"{win} {form}: a hit wrote its entry"


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("win", list(SHAPES))
def test_gpu_search_rows_equal_the_merge(cuda, win, form):
    _miss_then_hit(cuda, win, form)


@pytest.mark.gpu
def test_gpu_switched_off_equals_the_merge():
    """FM_RANK_SEARCH=0 in a fresh process: the kernels without the search form."""
    env = dict(os.environ, PYTHONPATH=ROOT, FM_RANK_SEARCH="0")
    flags = ["-s"] if sys.flags.no_user_site else []
    r = subprocess.run([sys.executable, *flags, os.path.abspath(__file__)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.strip().splitlines()[-1] == f"ok {len(SHAPES) * len(FORMS)}"


if __name__ == "__main__":
    from foremast_amd.ops._lib import LIB
    LIB.load()
    _dev = torch.device("cuda", 0)
    _n = 0
    for _win in SHAPES:
        for _form in FORMS:
            _miss_then_hit(_dev, _win, _form)
            _n += 1
    print("ok", _n)
