"""Exact sufficient statistics of the pairwise rank tests (sort form) against a
numpy oracle written from the definitions, on tie-heavy and edge inputs, in
every layout of the sort: split (K = 2, each side <= 64), pooled K = 1, 2, 4,
16; and the front kernel's p-value phase (several rows per workgroup, so the
rotated chunk deal is taken) against the serial tick."""
import numpy as np
import pytest
import torch

from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref

EXACT = [0, 1, 2, 3, 4, 5, 6, 7, 12, 13]   # n1 n2 nw r1 tie dmax rplus tiew npos nzero
R = 37                                      # not a multiple of the 4 rows per workgroup
EPS32 = 2.0 ** -24


def oracle_suff(cur, base):
    """The ten exact entries of `suff`, per row, from the definitions: doubled
    average ranks 2 #(v < x) + #(v == x) + 1 as integers, sum(t^3 - t) over tie
    runs, D n1 n2 as an integer maximum over the distinct values, signed-rank
    sums over the non-zero |d| (differences formed in fp32, as on the device)."""
    cur = np.asarray(cur, dtype=np.float32)
    base = np.asarray(base, dtype=np.float32)
    out = np.zeros((cur.shape[0], len(EXACT)), dtype=np.float64)
    npair = min(cur.shape[1], base.shape[1])
    for r in range(cur.shape[0]):
        c = cur[r][np.isfinite(cur[r])].astype(np.float64)
        b = base[r][np.isfinite(base[r])].astype(np.float64)
        n1, n2 = len(c), len(b)
        v = np.concatenate([c, b])
        r1x2 = int(sum(2 * int((v < x).sum()) + int((v == x).sum()) + 1 for x in c))
        _, t = np.unique(v, return_counts=True)          # -0.0 == +0.0: one run
        tie = int((t.astype(np.int64) ** 3 - t).sum())
        dnum = 0
        if n1 > 0 and n2 > 0:
            for x in np.unique(v):
                dnum = max(dnum, abs(int((c <= x).sum()) * n2 - int((b <= x).sum()) * n1))
        dmax = dnum / (float(n1) * n2) if n1 > 0 and n2 > 0 else 0.0
        pc, pb = cur[r, :npair], base[r, :npair]
        ok = np.isfinite(pc) & np.isfinite(pb)
        with np.errstate(invalid="ignore", over="ignore"):
            d = (pc - pb).astype(np.float32)
        nz = ok & (d != 0)
        ad = np.abs(d[nz]).astype(np.float64)
        pos = d[nz] > 0
        rp2 = int(sum(2 * int((ad < x).sum()) + int((ad == x).sum()) + 1 for x in ad[pos]))
        _, tw = np.unique(ad, return_counts=True)
        tiew = int((tw.astype(np.int64) ** 3 - tw).sum())
        out[r] = [n1, n2, int(nz.sum()), 0.5 * r1x2, tie, dmax, 0.5 * rp2, tiew, int(pos.sum()),
                  int((ok & ~nz).sum())]
    return out


def _random(rng, n1, n2):
    return (rng.normal(10.0, 3.0, (R, n1)).astype(np.float32), rng.normal(10.5, 3.0, (R, n2)).astype(np.float32))


def _pattern(name, n1, n2):
    rng = np.random.default_rng(sum(map(ord, name)) * 1000 + n1 * 7 + n2)
    npair = min(n1, n2)
    if name == "three_values":          # long tie runs across both samples
        vals = np.array([1.5, 2.5, 7.0], dtype=np.float32)
        return vals[rng.integers(0, 3, (R, n1))], vals[rng.integers(0, 3, (R, n2))]
    if name == "all_equal":
        return np.full((R, n1), 3.25, np.float32), np.full((R, n2), 3.25, np.float32)
    if name == "signed_zeros":
        z = np.array([0.0, -0.0], dtype=np.float32)
        return z[rng.integers(0, 2, (R, n1))], z[rng.integers(0, 2, (R, n2))]
    if name == "nan_inf":
        c, b = _random(rng, n1, n2)
        for a in (c, b):
            a[rng.random(a.shape) < 0.05] = np.nan
            a[rng.integers(0, R, 5), rng.integers(0, a.shape[1], 5)] = np.inf
            a[rng.integers(0, R, 5), rng.integers(0, a.shape[1], 5)] = -np.inf
        return c, b
    if name == "negative":
        c, b = _random(rng, n1, n2)
        return -c, (5.0 - b).astype(np.float32)
    if name == "opposite_signs":        # |d| equal, signs opposite, in many pairs
        b = rng.integers(0, 50, (R, n2)).astype(np.float32)
        c = rng.integers(0, 50, (R, n1)).astype(np.float32)
        k = rng.integers(1, 4, (R, npair)).astype(np.float32) * np.where(rng.random((R, npair)) < 0.5, -1, 1)
        c[:, :npair] = b[:, :npair] + k
        return c, b
    if name == "all_d_zero":
        c, b = _random(rng, n1, n2)
        c[:, :npair] = b[:, :npair]
        return c, b
    if name == "subnormal_d":           # differences are fp32 subnormals, distinct as bit patterns
        tiny = np.float32(2.0 ** -149)
        mb = rng.integers(1, 1 << 12, (R, n2))
        mc = rng.integers(1, 1 << 12, (R, n1))
        mc[:, :npair] = mb[:, :npair] + rng.integers(-40, 41, (R, npair))   # some zero, some tied |d|
        c, b = (np.maximum(mc, 0) * tiny).astype(np.float32), (mb * tiny).astype(np.float32)
        d = c[:, :npair] - b[:, :npair]
        assert (np.abs(d[d != 0]) < np.finfo(np.float32).tiny).all() and len(np.unique(np.abs(d).view(np.uint32))) > 30
        return c, b
    raise KeyError(name)


SHAPES = [(1, 1), (2, 63), (50, 50), (64, 64), (65, 63), (33, 31), (130, 100), (512, 512)]
PATTERNS = ["three_values", "all_equal", "signed_zeros", "nan_inf", "negative", "opposite_signs", "all_d_zero",
            "subnormal_d"]
PATTERN_SHAPES = [(50, 50), (65, 63), (130, 100)]


def test_oracle_matches_reference():
    """U1 = r1 - n1 (n1 + 1) / 2 is the reference's Mann-Whitney statistic and
    min(R+, R-) its Wilcoxon statistic."""
    for name, (n1, n2) in (("three_values", (50, 50)), ("nan_inf", (65, 63)), ("opposite_signs", (33, 31))):
        cur, base = _pattern(name, n1, n2)
        o = oracle_suff(cur, base)
        _, S, _ = ref.pairwise_tests(cur, base, 63, False, 0.05, 1, 1, 1)
        n1r, nw, r1, rplus = o[:, 0], o[:, 2], o[:, 3], o[:, 6]
        np.testing.assert_array_equal((r1 - n1r * (n1r + 1) / 2).astype(np.float32), S[:, 0])
        np.testing.assert_array_equal(np.minimum(rplus, nw * (nw + 1) / 2 - rplus).astype(np.float32), S[:, 1])


def _suff(cuda, cur, base, variant):
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    c, b = torch.from_numpy(cur).to(cuda), torch.from_numpy(base).to(cuda)
    suff = torch.full((cur.shape[0], C.SUFF), -1.0, dtype=torch.float64, device=cuda)
    LIB.call("fm_pairwise_suff_v", ptr(c), c.stride(0), cur.shape[1], ptr(b), b.stride(0), base.shape[1],
             cur.shape[0], ptr(suff), 0, variant, stream_of(c))
    torch.cuda.synchronize()
    return suff.cpu().numpy()


def _check(cuda, cur, base):
    n1, n2 = cur.shape[1], base.shape[1]
    want = oracle_suff(cur, base)
    sort, count = _suff(cuda, cur, base, 0), _suff(cuda, cur, base, 1)
    np.testing.assert_array_equal(sort[:, EXACT], want)
    np.testing.assert_array_equal(sort[:, EXACT], count[:, EXACT])
    # Welch moments.  Both forms add the same fp32 values in the same tree when
    # they share the pooled layout: bit-identical.  The split layout (K = 2,
    # each side <= 64) holds one value per lane and sample, another order of the
    # same sum: a mean is then off by at most (K + 6 levels + the division)
    # roundings of partial sums <= n max|x|, i.e. 10 eps32 max|x| for K = 2
    # (plus one subnormal ulp, where a rounding is absolute).
    split = n1 + n2 > 64 and n1 <= 64 and n2 <= 64
    if not split:
        np.testing.assert_array_equal(sort[:, 8:12], count[:, 8:12])
    for col, a in ((8, cur), (9, base)):
        fin = np.where(np.isfinite(a), a, 0.0).astype(np.float64)
        n = np.maximum(np.isfinite(a).sum(1), 1)
        K = (n1 + n2 + 63) // 64
        tol = (K + 8) * EPS32 * np.abs(fin).max(1) + 2.0 ** -149
        assert (np.abs(sort[:, col] - fin.sum(1) / n) <= tol).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2", SHAPES)
def test_gpu_suff_matches_oracle_shapes(cuda, n1, n2):
    cur, base = _random(np.random.default_rng(n1 * 1031 + n2), n1, n2)
    cur[:, : min(n1, n2) // 3] = base[:, : min(n1, n2) // 3]          # some zero differences
    _check(cuda, cur, base)


@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2", PATTERN_SHAPES)
@pytest.mark.parametrize("name", PATTERNS)
def test_gpu_suff_matches_oracle_patterns(cuda, name, n1, n2):
    _check(cuda, *_pattern(name, n1, n2))


@pytest.mark.gpu
def test_gpu_front_rotated_pvalues_equal_serial(cuda):
    """72 rows on a few pairwise workgroups: each takes several rows per wave and
    evaluates their p-values with the chunk deal rotated by its index."""
    from foremast_amd.engine.scorer import CanaryScorer
    aliases = ["error5xx", "latency", "traffic", "error4xx", "cpu", "memory", "tomcat_threads", "jvm_heap"]
    h, b, c = C.synth_fleet(9, 8, 300, 5, 10, device=cuda)
    want = CanaryScorer(aliases, device=cuda, mode="serial").score(h, b, c, 300)
    for kw in ({}, {"front_wgs": (0.02, 0.1)}):
        sc = CanaryScorer(aliases, device=cuda, mode="front", **kw)
        for _ in range(2):                  # a tick that streams the history, then a cached one
            o = sc.score(h, b, c, 300)
            torch.cuda.synchronize()
            torch.testing.assert_close(o.pvals, want.pvals, rtol=0, atol=0, equal_nan=True)
            torch.testing.assert_close(o.pstats, want.pstats, rtol=0, atol=0, equal_nan=True)
            assert torch.equal(o.packed, want.packed)
