"""Edge shapes of the early model kernels: K5 bivariate, the band decision,
K8 HPA score, K9 downstream impact with the per-cluster maximum, and K10
least squares.

Every family has a fixture builder that returns numpy inputs, used twice: a
CPU test holds the library reference against a scalar fp64 / fp32 loop written
from the kernel's header comment and docs/BRAIN_SPEC.md, and a GPU test holds
the kernel against the library reference.  Integer outputs (flag words, counts,
reasons, scores, state, nvalid) are compared exactly.  Where a flag hangs on a
float comparison the inputs sit on a grid, and the test asserts on the
reference that every finite point keeps the stated margin from its cut.

Which GPU test enters which path:

K5   NV = 2/4/8/10/16, T % 4 != 0 (tail mask), NaN / inf in the history .. test_gpu_bivariate_dispatch_sweep
     T > 16384, the error return ............................................ test_gpu_bivariate_rejects_long_history
     n > 64 (several words), n > 256 (the i0 loop, word i0 / 64 + wave),
     NaN / inf in the current points ........................................ test_gpu_bivariate_current_shapes
     fewer than two finite pairs ............................................ test_gpu_bivariate_short_histories
     means far from zero .................................................... test_gpu_bivariate_offset_means
     singular and near-singular covariance .................................. test_gpu_bivariate_degenerate_covariance
band ``diff``, a partial last workgroup, NaN point / centre, sigma 0 / NaN,
     bound 0, n = 1, n a multiple of 64 ..................................... test_gpu_band_decide_edges
K8   reason 4, the window reset with live flips, isAbsolute, isIncrease
     false, NaN in point / bands, no SLA metric, upper == lower ............. test_gpu_hpa_score_sequence
     fm_hpa_score_slots ..................................................... test_gpu_hpa_score_slots
K9   the lane-stride loop twice and more, rows without edges, self-loops,
     NaN scores ............................................................. test_gpu_downstream_impact_edges
     segment_max K > 256, S > 2048 (several blocks), NaN, ids out of range .. test_gpu_segment_max_edges
     K > 16384, the error return ............................................ test_gpu_segment_max_rejects_too_many_segments
K10  a chunk partly past T, NaN / inf samples, a NaN first sample, R < 32,
     R % 32 = 1, T % 4 != 0, the residual tail with T % 32 != 0 ............. test_gpu_lsq_edges"""
import math

import numpy as np
import pytest
import torch

from foremast_amd.ops import lsq as LQ
from foremast_amd.ops import misc as MI
from foremast_amd.ops import smoothing as SM

F32 = np.float32


def _ceil4(T):
    return (T + 3) // 4 * 4


def _unpack(words, n):
    """int64 flag words [P, NW] -> bool [P, n]; bit i of word w is point 64 w + i."""
    w = np.ascontiguousarray(words).view(np.uint64)
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")
    assert not bits[:, n:].any()                      # no bit set past the last point
    return bits[:, :n].astype(bool)


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


# =========================================================================== K5
K5_THR = 3.0
K5_MARGIN = 0.05
# Mahalanobis distances of the built current points: steps of 0.25 with the cut itself left out
K5_GRID = np.array([0.25 * k for k in range(25) if k != 12])


def _points_at(a, b, n, rng):
    """Current points [P, n] x 2 (fp32) whose distance from the history pair
    (a, b) [P, T] lies on K5_GRID: mean + chol(cov) (r cos t, r sin t), with the
    moments taken in fp64 over the pairs that have both members finite."""
    P = a.shape[0]
    ca, cb = np.zeros((P, n), F32), np.zeros((P, n), F32)
    for p in range(P):
        ok = np.isfinite(a[p]) & np.isfinite(b[p])
        x = np.stack([a[p, ok], b[p, ok]]).astype(np.float64)
        L = np.linalg.cholesky(np.cov(x))
        r, t = rng.choice(K5_GRID, n), rng.uniform(0, 2 * np.pi, n)
        ca[p], cb[p] = x.mean(1)[:, None] + L @ (r * np.stack([np.cos(t), np.sin(t)]))
    return ca, cb


def _k5_rows(a, b, pad=4):
    """History rows as the kernel takes them: ld = ceil4(T) + pad, and the columns
    at and past T hold 1e30, so a load that escapes the tail mask ruins the moments."""
    P, T = a.shape
    ha, hb = (np.full((P, _ceil4(T) + pad), 1e30, F32) for _ in range(2))
    ha[:, :T], hb[:, :T] = a, b
    return ha, hb


def k5_sweep_case(T, n=30, P=6, seed=0):
    rng = np.random.default_rng(1000 + T + seed)
    a = rng.normal(5, 1, (P, T)).astype(F32)
    b = (0.5 * a + rng.normal(0, 0.3, (P, T))).astype(F32)
    a[rng.random((P, T)) < 0.03] = np.nan
    b[rng.random((P, T)) < 0.03] = np.nan
    a[0, T // 2] = np.inf
    ca, cb = _points_at(a, b, n, rng)
    return _k5_rows(a, b) + (T, ca, cb)


def k5_current_case(n, T=2048):
    ha, hb, T, ca, cb = k5_sweep_case(T, n=n, seed=n)
    if n == 1:
        ca[0, 0], cb[1, 0] = np.nan, np.inf
    else:
        for p in range(ca.shape[0]):
            ca[p, (3 * p) % n] = np.nan
            cb[p, (5 * p + 1) % n] = np.inf
            if p % 2:
                ca[p, n - 1] = -np.inf
    return ha, hb, T, ca, cb


def k5_short_case():
    """Rows with 0 (all NaN), 0 (disjoint holes), 1, 2 and T finite pairs, and one
    pair beside an infinite sample.  The two pairs (1, 2), (3, 6) give the moments
    (2, 4, 2, 4, 8) exactly in fp32 and in fp64, a correlation of 1; the current
    points are the mean, the point one step along the line (dist 1 / sqrt(2)) and
    points off it."""
    T, n = 8, 5
    rng = np.random.default_rng(7)
    a = rng.normal(5, 1, (6, T)).astype(F32)
    b = (0.5 * a + rng.normal(0, 0.3, (6, T))).astype(F32)
    a[0] = np.nan
    a[1, ::2], b[1, 1::2] = np.nan, np.nan
    a[2, 1:], b[2, :5] = np.nan, np.nan
    b[2, 0] = 1.5
    a[3], b[3] = np.nan, np.nan
    a[3, [2, 6]], b[3, [2, 6]] = [1.0, 3.0], [2.0, 6.0]
    a[5, 1:] = np.inf
    ca = np.tile(np.array([2.0, 3.0, 3.0, 1.0, 2.0], F32), (6, 1))
    cb = np.tile(np.array([4.0, 6.0, 3.5, 4.0, 4.5], F32), (6, 1))
    ca[4], cb[4] = _points_at(a[4:5], b[4:5], n, rng)
    return _k5_rows(a, b) + (T, ca, cb)


def k5_offset_case(T=4097, n=30, P=6):
    rng = np.random.default_rng(11)
    a64 = 1e6 + rng.normal(0, 100, (P, T))
    a = a64.astype(F32)
    b = (3e5 + 0.5 * (a64 - 1e6) + rng.normal(0, 40, (P, T))).astype(F32)
    ca, cb = _points_at(a, b, n, rng)
    return _k5_rows(a, b) + (T, ca, cb)


K5_Z = np.array([0, 1, 2, 4, 5, -4, -5], np.float64)


def k5_degenerate_case(T=2048):
    """Rows (i) b = 2a, (ii) b constant, (iii) both constant, (iv) b = fl32(0.3 a + 1)
    with current points on the line at z = K5_Z, (v) as (iv) with the points moved
    off the line by 0.1 std(b)."""
    rng = np.random.default_rng(13)
    base = rng.normal(2, 1, T).astype(F32)
    a = np.tile(base, (5, 1))
    b = np.zeros_like(a)
    b[0] = 2 * a[0]
    b[1] = 7.5
    a[2], b[2] = 3.25, 7.5
    b[3] = (0.3 * a[3].astype(np.float64) + 1).astype(F32)
    b[4] = b[3]
    ma, sa = float(base.astype(np.float64).mean()), float(base.astype(np.float64).std(ddof=1))
    n = len(K5_Z)
    ca = np.tile((ma + K5_Z * sa).astype(F32), (5, 1))
    cb = np.zeros_like(ca)
    # (i) on the line at z = 0, 1, 2, 4, then off it
    cb[0] = 2 * ca[0]
    cb[0, 4:] += np.array([0.5, -0.5, 1.0], F32)
    # (ii) the constant member stays put, then moves
    cb[1] = 7.5
    cb[1, 4:] = [7.5 + 1e-3, 7.0, 8.0]
    # (iii) nothing moves, then either member does
    ca[2], cb[2] = 3.25, 7.5
    ca[2, 3:5] = [3.5, 3.0]
    cb[2, 5:] = [7.75, 7.0]
    cb[3] = (0.3 * ca[3].astype(np.float64) + 1).astype(F32)
    sb = float(b[3].astype(np.float64).std(ddof=1))
    cb[4] = (cb[3].astype(np.float64) + 0.1 * sb).astype(F32)
    return _k5_rows(a, b) + (T, ca, cb)


def spec_bivariate(ha, hb, T, ca, cb, thr):
    """docs/BRAIN_SPEC.md, K5: a pair counts when both members are finite; fewer
    than two pairs give NaN and no flag; S = C with its diagonal scaled by
    1 + 1e-6 (plus 1e-30); d = sqrt(dx' S^-1 dx), flagged when d > thr."""
    P, n = ca.shape
    params = np.zeros((P, 5))
    dist = np.full((P, n), np.nan)
    flag = np.zeros((P, n), bool)
    for p in range(P):
        pr = [(float(x), float(y)) for x, y in zip(ha[p, :T], hb[p, :T]) if math.isfinite(x) and math.isfinite(y)]
        c = len(pr)
        ma = math.fsum(x for x, _ in pr) / c if c else 0.0
        mb = math.fsum(y for _, y in pr) / c if c else 0.0
        den = max(c - 1, 1)
        caa = math.fsum((x - ma) ** 2 for x, _ in pr) / den
        cbb = math.fsum((y - mb) ** 2 for _, y in pr) / den
        cab = math.fsum((x - ma) * (y - mb) for x, y in pr) / den
        params[p] = ma, mb, caa, cab, cbb
        if c < 2:
            continue
        saa, sbb = caa * (1 + 1e-6) + 1e-30, cbb * (1 + 1e-6) + 1e-30
        det = saa * sbb - cab * cab
        for i in range(n):
            xa, xb = float(ca[p, i]), float(cb[p, i])
            if math.isfinite(xa) and math.isfinite(xb):
                da, db = xa - ma, xb - mb
                dist[p, i] = math.sqrt(max((da * da * sbb - 2 * da * db * cab + db * db * saa) / det, 0.0))
                flag[p, i] = dist[p, i] > thr
    return params, dist, flag


def _k5_ref(case):
    ha, hb, T, ca, cb = case
    return tuple(_np(v) for v in MI.bivariate(*(torch.from_numpy(v) for v in (ha, hb)), T,
                                              *(torch.from_numpy(v) for v in (ca, cb)), K5_THR))


def _k5_margin(ref):
    d = ref[1][np.isfinite(ref[1])]
    assert (np.abs(d - K5_THR) > K5_MARGIN).all(), np.abs(d - K5_THR).min()


def _k5_ref_vs_spec(case, dist_rtol=1e-6):
    ha, hb, T, ca, cb = case
    ref = _k5_ref(case)
    params, dist, flag = spec_bivariate(ha, hb, T, ca, cb, K5_THR)
    _k5_margin(ref)
    n = ca.shape[1]
    np.testing.assert_allclose(ref[0], params, rtol=1e-6, atol=1e-9)
    np.testing.assert_array_equal(np.isnan(ref[1]), np.isnan(dist))
    if dist_rtol is not None:
        np.testing.assert_allclose(ref[1], dist, rtol=dist_rtol, atol=1e-6)
    np.testing.assert_array_equal(_unpack(ref[2], n), flag)
    np.testing.assert_array_equal(ref[3], flag.sum(1))
    assert ref[2].dtype == np.int64 and ref[2].shape == (ca.shape[0], max(1, (n + 63) // 64))
    assert ref[3].dtype == np.int32
    return ref


def _k5_gpu(cuda, case):
    ha, hb, T, ca, cb = case
    t = lambda v: torch.from_numpy(v).to(cuda)     # noqa: E731
    return tuple(_np(v) for v in MI.bivariate(t(ha), t(hb), T, t(ca), t(cb), K5_THR))


def _k5_gpu_vs_ref(cuda, case, compare_dist=True):
    ref = _k5_ref(case)
    _k5_margin(ref)
    g = _k5_gpu(cuda, case)
    n = case[3].shape[1]
    if n <= 8:
        print("K5 dist gpu", g[1].tolist(), "ref", ref[1].tolist())
    np.testing.assert_array_equal(g[2], ref[2])                      # every flag word
    np.testing.assert_array_equal(g[3], ref[3])
    np.testing.assert_array_equal(np.isnan(g[1]), np.isnan(ref[1]))
    assert not _unpack(g[2], n)[np.isnan(ref[1])].any()
    if compare_dist:
        np.testing.assert_allclose(g[0], ref[0], rtol=1e-4, atol=1e-5)
        fin = np.isfinite(ref[1])
        np.testing.assert_allclose(g[1][fin], ref[1][fin], rtol=1e-3, atol=1e-3)
        np.testing.assert_array_equal(g[1][~fin], ref[1][~fin])
    return g, ref


K5_SWEEP_T = [5, 2048, 2049, 4097, 8193, 10080, 10241, 16384]


@pytest.mark.parametrize("T", [5, 2049, 16384])
def test_ref_bivariate_sweep_matches_scalar_spec(T):
    ref = _k5_ref_vs_spec(k5_sweep_case(T))
    assert 0 < ref[3].sum() < ref[1].size


@pytest.mark.parametrize("n", [1, 65, 300])
def test_ref_bivariate_current_shapes_match_scalar_spec(n):
    case = k5_current_case(n)
    ref = _k5_ref_vs_spec(case)
    bad = ~(np.isfinite(case[3]) & np.isfinite(case[4]))
    assert bad.any() and np.isnan(ref[1][bad]).all()


def test_ref_bivariate_short_histories_give_nan():
    case = k5_short_case()
    ref = _k5_ref_vs_spec(case)
    assert np.isnan(ref[1][[0, 1, 2, 5]]).all() and not ref[2][[0, 1, 2, 5]].any()
    assert not ref[3][[0, 1, 2, 5]].any()
    np.testing.assert_array_equal(ref[0][3], [2, 4, 2, 4, 8])
    assert ref[1][3, 0] == 0 and (ref[1][3, 2:] > 100).all()
    np.testing.assert_allclose(ref[1][3, 1], math.sqrt(0.5), rtol=1e-5)
    assert np.isfinite(ref[1][4]).all()


def test_ref_bivariate_offset_matches_scalar_spec():
    _k5_ref_vs_spec(k5_offset_case())


def test_ref_bivariate_degenerate_covariance():
    case = k5_degenerate_case()
    # (i)-(iii) follow the scalar spec; (iv) and (v) hang on the rounding of b and are held by their flags
    ha, hb, T, ca, cb = case
    _k5_ref_vs_spec((ha[:3], hb[:3], T, ca[:3], cb[:3]), dist_rtol=1e-5)
    ref = _k5_ref(case)
    _k5_margin(ref)
    fl = _unpack(ref[2], len(K5_Z))
    np.testing.assert_array_equal(fl[0], [0, 0, 0, 1, 1, 1, 1])
    np.testing.assert_array_equal(fl[1], [0, 0, 0, 1, 1, 1, 1])
    np.testing.assert_array_equal(fl[2], [0, 0, 0, 1, 1, 1, 1])
    np.testing.assert_array_equal(fl[3], np.abs(K5_Z) >= 4)
    assert fl[4].all()
    np.testing.assert_array_equal(ref[3], fl.sum(1))


@pytest.mark.gpu
@pytest.mark.parametrize("T", K5_SWEEP_T)
def test_gpu_bivariate_dispatch_sweep(cuda, T):
    """NV = 2 / 4 / 8 / 10 / 16 on both sides of every boundary, T % 4 != 0, the
    1e30 tail, NaN and +inf in the history."""
    _k5_gpu_vs_ref(cuda, k5_sweep_case(T))


@pytest.mark.gpu
def test_gpu_bivariate_rejects_long_history(cuda):
    P, T, n = 2, 16385, 4
    h = torch.zeros((P, _ceil4(T) + 4), device=cuda)
    c = torch.zeros((P, n), device=cuda)
    with pytest.raises(RuntimeError):
        MI.bivariate(h, h.clone(), T, c, c.clone(), K5_THR)
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 65, 257, 300])
def test_gpu_bivariate_current_shapes(cuda, n):
    """One to five flag words, the second trip of the 256-point loop, NaN and inf
    among the current points."""
    g, ref = _k5_gpu_vs_ref(cuda, k5_current_case(n))
    assert g[2].shape[1] == max(1, (n + 63) // 64)


@pytest.mark.gpu
def test_gpu_bivariate_short_histories(cuda):
    _k5_gpu_vs_ref(cuda, k5_short_case())


@pytest.mark.gpu
def test_gpu_bivariate_offset_means(cuda):
    """Means of 1e6 and 3e5 over a spread of 100 and 64: two-pass moments about an
    fp32 mean move dist by ulp(1e6) / 2 / 100 = 3e-4 relative, inside the 1e-3."""
    _k5_gpu_vs_ref(cuda, k5_offset_case())


@pytest.mark.gpu
def test_gpu_bivariate_degenerate_covariance(cuda):
    """(i)-(iii): dist to rtol 1e-3, flags exact.  (iv), (v): flags and count
    only; the distances there are printed.  With the fp32 inverse and form and
    the conditional 1e-9 regulariser the kernel gave (iv) = [0, 4, 8, 16, 0, 16, 0]
    at z = K5_Z (flags at z = 1 and 2, none at +-5) and about 1072 in (v); with the
    ridge and the fp64 form it gives |z| to 1e-6 and 70.7 - 70.9, as the reference."""
    ha, hb, T, ca, cb = k5_degenerate_case()
    _k5_gpu_vs_ref(cuda, (ha[:3], hb[:3], T, ca[:3], cb[:3]))
    _k5_gpu_vs_ref(cuda, (ha[3:], hb[3:], T, ca[3:], cb[3:]), compare_dist=False)


# ================================================================== band_decide
BAND_MARGIN = 1e-3


def band_case(n, bound, R=7, M=3):
    rng = np.random.default_rng(100 + n)
    ctr = rng.normal(0, 0.2, (R, n)).astype(F32)
    sig = rng.uniform(0.3, 1.0, R).astype(F32)
    sig[2], sig[5] = 0.0, np.nan
    k = rng.integers(-24, 25, (R, n))
    k[2][k[2] == 0] = 3                              # the sigma = 0 row: every point off its centre
    step = np.where(sig > 0, sig, 1.0).astype(np.float64)
    cur = (ctr.astype(np.float64) + k * 0.25 * step[:, None]).astype(F32)
    thr = np.array([2.1, 1.3, 2.9], F32)
    mlb = np.array([-0.37, -10.0, 0.113], F32)       # clamps rows of metric 0 and 2
    diff = np.zeros(R, np.int8)
    diff[[1, 4]] = 1
    hole = rng.random((R, n)) < 0.1
    hole[2] = False
    cur[hole & (rng.random((R, n)) < 0.5)] = np.nan
    cur[hole & ~np.isnan(cur) & (rng.random((R, n)) < 0.5)] = np.inf
    ctr[rng.random((R, n)) < 0.05] = np.nan
    ctr[2] = np.nan_to_num(ctr[2])
    if n > 1:
        cur[0, 0], cur[1, n - 1], ctr[3, n // 2] = np.nan, np.inf, np.nan
    return cur, ctr, sig, M, thr, np.asarray(bound, np.int32), mlb, diff, 0.8


def spec_band_decide(cur, ctr, sig, M, thr, bound, mlb, diff, pf):
    """docs/BRAIN_SPEC.md 3.1 and the kernel's header, in fp32 one point at a time."""
    R, n = cur.shape
    up, lo = np.zeros((R, n), F32), np.zeros((R, n), F32)
    flag = np.zeros((R, n), bool)
    score = np.zeros(R, F32)
    for r in range(R):
        m = r % M
        th = F32(thr[m]) * F32(pf) if diff[r] else F32(thr[m])
        sd = F32(sig[r])
        with np.errstate(invalid="ignore"):
            w = F32(th * sd)
        for i in range(n):
            c, x = F32(ctr[r, i]), F32(cur[r, i])
            with np.errstate(invalid="ignore"):
                u, l = F32(c + w), F32(c - w)
            if l < mlb[m]:
                l = F32(mlb[m])
            up[r, i], lo[r, i] = u, l
            if not (np.isfinite(x) and np.isfinite(c)):
                continue
            hi = bool(bound[m] & 1) and x > u
            lw = bool(bound[m] & 2) and x < l
            if hi or lw:
                flag[r, i] = True
                z = F32((x - u if hi else l - x) / sd) if sd > 0 else F32(1e30)
                score[r] = max(score[r], z)
    return up, lo, flag, flag.sum(1), score


def _band_ref(case):
    cur, ctr, sig, M, thr, bound, mlb, diff, pf = case
    t = torch.from_numpy
    return tuple(_np(v) for v in SM.band_decide(t(cur), t(ctr), t(sig), M, t(thr), t(bound), t(mlb), t(diff), pf))


def _band_margin(case, ref):
    cur = case[0]
    for band in ref[:2]:
        ok = np.isfinite(cur) & np.isfinite(band)
        assert ok.any() and (np.abs(cur[ok] - band[ok]) > BAND_MARGIN).all()


BAND_CASES = [(n, b) for n in (1, 64, 129) for b in ([0, 1, 3], [2, 3, 1])]


@pytest.mark.parametrize("n,bound", BAND_CASES)
def test_ref_band_decide_matches_scalar_spec(n, bound):
    case = band_case(n, bound)
    ref = _band_ref(case)
    _band_margin(case, ref)
    up, lo, flag, cnt, score = spec_band_decide(*case)
    np.testing.assert_array_equal(ref[0], up)
    np.testing.assert_array_equal(ref[1], lo)
    np.testing.assert_array_equal(_unpack(ref[2], n), flag)
    np.testing.assert_array_equal(ref[3], cnt)
    np.testing.assert_allclose(ref[4], score, rtol=1e-6)
    assert ref[2].dtype == np.int64 and ref[3].dtype == np.int32 and ref[4].dtype == np.float32
    assert ref[4][5] == 0 and cnt[5] == 0            # NaN sigma: no band, no flag
    assert cnt[2] == (n if bound[2] == 3 else (case[0][2] > case[1][2]).sum())
    if cnt[2]:
        assert ref[4][2] == F32(1e30)
    if 0 in bound:                                   # bound 0 judges neither side
        assert not flag[np.arange(7) % 3 == bound.index(0)].any()


@pytest.mark.gpu
@pytest.mark.parametrize("n,bound", BAND_CASES)
def test_gpu_band_decide_edges(cuda, n, bound):
    """A partial last workgroup (R = 7), the pairwise factor, clamped lower bands,
    sigma = 0 and NaN, NaN / inf points and centres, bound 0, one to three words."""
    case = band_case(n, bound)
    cur, ctr, sig, M, thr, bd, mlb, diff, pf = case
    ref = _band_ref(case)
    _band_margin(case, ref)
    t = lambda v: torch.from_numpy(v).to(cuda)     # noqa: E731
    g = tuple(_np(v) for v in SM.band_decide(t(cur), t(ctr), t(sig), M, t(thr), t(bd), t(mlb), t(diff), pf))
    np.testing.assert_allclose(g[0], ref[0], rtol=1e-6)
    np.testing.assert_allclose(g[1], ref[1], rtol=1e-6)
    np.testing.assert_array_equal(g[2], ref[2])
    np.testing.assert_array_equal(g[3], ref[3])
    np.testing.assert_allclose(g[4], ref[4], rtol=1e-3)
    assert g[4][5] == 0
    if ref[3][2]:
        assert g[4][2] == F32(1e30)


# =========================================================================== K8
HPA_PARAMS = dict(breath_up=10.0, breath_down=20.0, max_flips=1, flip_window=100.0)
HPA_TICKS = (0.0, 5.0, 15.0, 40.0, 70.0, 95.0, 130.0)
HPA_TEMPLATES = {
    "sla": (["traffic", "cpu", "free_mem", "latency"],
            {"free_mem": {"isIncrease": False, "isAbsolute": True, "priority": 2}}),
    "no_sla": (["traffic", "cpu"], None),
}


def hpa_case(name, S=300, seed=0):
    """Bands and one ``cur`` per tick.  Each service leans up or down as a whole
    and the lean reverses from tick to tick, so the breath time, the flip limit
    and the window reset are all met."""
    aliases, cfg = HPA_TEMPLATES[name]
    tmpl = MI.HpaTemplate.from_aliases(aliases, cfg)
    Mt = len(aliases)
    rng = np.random.default_rng(40 + Mt + seed)
    up = rng.uniform(1, 2, (S, Mt)).astype(F32)
    lo = (up - rng.uniform(0.2, 1, (S, Mt))).astype(F32)
    lo[:5] = up[:5]                                   # upper == lower
    sign = np.where(np.asarray(tmpl.is_increase), 1.0, -1.0)
    lean0 = rng.choice([-1.0, 1.0], S)
    curs = []
    for k in range(len(HPA_TICKS)):
        lean = lean0 * (-1.0) ** k
        quiet = rng.random(S) < 0.15                  # some services sit inside their bands
        mid, half = (up + lo) / 2, (up - lo) / 2 + 0.05
        x = mid + (lean[:, None] * sign[None, :]) * half * rng.uniform(0.6, 3.0, (S, Mt))
        x = np.where(quiet[:, None], mid, x)
        x[rng.random((S, Mt)) < 0.1] = np.nan
        curs.append(x.astype(F32))
    up[rng.random((S, Mt)) < 0.1] = np.nan
    lo[rng.random((S, Mt)) < 0.1] = np.nan
    return tmpl, curs, up, lo


def spec_hpa_tick(cur, up, lo, tmpl, st, now, breath_up, breath_down, max_flips, flip_window):
    """docs/BRAIN_SPEC.md 7, one service at a time in fp32; ``st`` = dict of numpy state arrays."""
    S, Mt = cur.shape
    w, role = tmpl.weights(), tmpl.roles()
    score, reason, raw = np.zeros(S, np.int32), np.zeros(S, np.int8), np.zeros(S, F32)
    for s in range(S):
        u_ = d_ = F32(0)
        viol = False
        for j in range(Mt):
            c, u, l = F32(cur[s, j]), F32(up[s, j]), F32(lo[s, j])
            if not (np.isfinite(c) and np.isfinite(u) and np.isfinite(l)):
                continue
            scale = max(abs(u), F32(1e-12)) if tmpl.is_absolute[j] else max(F32(u - l), F32(1e-12))
            dev = F32((c - u) / scale) if c > u else (F32((c - l) / scale) if c < l else F32(0))
            if not tmpl.is_increase[j]:
                dev = -dev
            if role[j] == 1:
                viol = viol or dev > 0
            elif dev > 0:
                u_ = max(u_, F32(w[j] * dev))
            elif dev < 0:
                d_ = max(d_, F32(-w[j] * dev))
        if not (role == 1).any():
            viol = u_ > 0
        r = 50
        if u_ > 0 and viol:
            r = 50 + int(np.rint(F32(50) * min(F32(1), u_)))
        elif d_ > 0 and u_ == 0 and not viol:
            r = 50 - int(np.rint(F32(50) * min(F32(1), d_)))
        raw[s] = r
        if now - st["flip_t0"][s] > flip_window:
            st["flips"][s], st["flip_t0"][s] = 0, now
        dr = (r > 50) - (r < 50)
        score[s], reason[s] = r, {1: 1, -1: 2, 0: 0}[dr]
        if dr:
            ld = st["last_dir"][s]
            if ld != 0 and now - st["last_time"][s] < (breath_up if dr > 0 else breath_down):
                score[s], reason[s] = 50, 3
            elif ld != 0 and dr != ld and st["flips"][s] >= max_flips:
                score[s], reason[s] = 50, 4
            else:
                if ld != 0 and dr != ld:
                    st["flips"][s] += 1
                st["last_dir"][s], st["last_time"][s] = dr, now
    return score, reason, raw


def _state_np(st):
    return {k: _np(getattr(st, k)).copy() for k in ("last_dir", "last_time", "flips", "flip_t0")}


def _hpa_ref_run(name):
    """The reference over all ticks -> per tick (score, reason, raw, state after)."""
    tmpl, curs, up, lo = hpa_case(name)
    st = MI.HpaState.zeros(curs[0].shape[0])
    out = []
    for now, cur in zip(HPA_TICKS, curs):
        r = MI.hpa_score(*(torch.from_numpy(v) for v in (cur, up, lo)), tmpl, st, now, **HPA_PARAMS)
        out.append(tuple(_np(v).copy() for v in r) + (_state_np(st),))
    reasons = np.concatenate([o[1] for o in out])
    assert set(reasons.tolist()) == {0, 1, 2, 3, 4}, np.bincount(reasons)
    # the window reset meets services that have flipped
    assert ((out[-2][3]["flips"] > 0) & (out[-1][3]["flip_t0"] == HPA_TICKS[-1])).any()
    return out


@pytest.fixture(scope="module", params=list(HPA_TEMPLATES))
def hpa_ref(request):
    return request.param, _hpa_ref_run(request.param)


def test_ref_hpa_score_matches_scalar_spec(hpa_ref):
    name, ref = hpa_ref
    tmpl, curs, up, lo = hpa_case(name)
    st = _state_np(MI.HpaState.zeros(curs[0].shape[0]))
    for now, cur, want in zip(HPA_TICKS, curs, ref):
        sc, rs, raw = spec_hpa_tick(cur, up, lo, tmpl, st, now, **HPA_PARAMS)
        np.testing.assert_array_equal(want[0], sc)
        np.testing.assert_array_equal(want[1], rs)
        np.testing.assert_array_equal(want[2], raw)
        for k, v in st.items():
            np.testing.assert_array_equal(want[3][k], v, err_msg=k)
    assert want[0].dtype == np.int32 and want[1].dtype == np.int8


@pytest.mark.gpu
def test_gpu_hpa_score_sequence(cuda, hpa_ref):
    """Reasons 0-4 over seven ticks, isAbsolute, isIncrease = false, NaN in the
    point and in the bands, a template without an SLA metric, upper == lower."""
    name, ref = hpa_ref
    tmpl, curs, up, lo = hpa_case(name)
    st = MI.HpaState.zeros(curs[0].shape[0], cuda)
    for now, cur, want in zip(HPA_TICKS, curs, ref):
        g = MI.hpa_score(*(torch.from_numpy(v).to(cuda) for v in (cur, up, lo)), tmpl, st, now, **HPA_PARAMS)
        for a, b in zip(g, want[:3]):
            np.testing.assert_array_equal(_np(a), b)
        for k, v in _state_np(st).items():
            np.testing.assert_array_equal(v, want[3][k], err_msg=f"{k} at {now}")


@pytest.mark.gpu
def test_gpu_hpa_score_slots(cuda):
    """fm_hpa_score_slots as the brain's steady cycle calls it: the state of 300
    services lives in a 500-slot table and is updated in place through ``slots``."""
    from foremast_amd.engine.fp_types import _hpa_tables
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    tmpl, curs, up, lo = hpa_case("sla", seed=1)
    S, Mt, N = curs[0].shape[0], curs[0].shape[1], 500
    rng = np.random.default_rng(9)
    slots = rng.permutation(N)[:S].astype(np.int64)
    table = MI.HpaState(torch.from_numpy(rng.integers(-1, 2, N).astype(np.int8)),
                        torch.from_numpy(rng.choice([-1e18, -30.0, -8.0, 0.0], N)),
                        torch.from_numpy(rng.integers(0, 3, N).astype(np.int32)),
                        torch.from_numpy(rng.choice([-200.0, -50.0, 0.0], N)))
    before = _state_np(table)
    sub = MI.HpaState(*(getattr(table, k)[torch.from_numpy(slots)].clone()
                        for k in ("last_dir", "last_time", "flips", "flip_t0")))
    dev = MI.HpaState(*(getattr(table, k).to(cuda) for k in ("last_dir", "last_time", "flips", "flip_t0")))
    sl = torch.from_numpy(slots).to(cuda)
    packed = torch.empty((S,), dtype=torch.int32, device=cuda)
    td = _hpa_tables(tmpl, cuda)
    ud, ldv = torch.from_numpy(up).to(cuda), torch.from_numpy(lo).to(cuda)
    p = HPA_PARAMS
    seen = set()
    for now, cur in zip(HPA_TICKS[:4], curs):
        sc, rs, _ = MI.hpa_score(*(torch.from_numpy(v) for v in (cur, up, lo)), tmpl, sub, now, **p)
        cd = torch.from_numpy(cur).to(cuda)
        LIB.call("fm_hpa_score_slots", ptr(cd), ptr(ud), ptr(ldv), S, Mt, *map(ptr, td), float(now),
                 float(p["breath_up"]), float(p["breath_down"]), int(p["max_flips"]), float(p["flip_window"]),
                 ptr(dev.last_dir), ptr(dev.last_time), ptr(dev.flips), ptr(dev.flip_t0), ptr(sl), ptr(packed),
                 stream_of(cd))
        np.testing.assert_array_equal(_np(packed), _np(sc) | (_np(rs).astype(np.int32) << 16))
        seen |= set(_np(rs).tolist())
        after = _state_np(dev)
        want = _state_np(sub)
        rest = np.setdiff1d(np.arange(N), slots)
        for k in after:
            np.testing.assert_array_equal(after[k][slots], want[k], err_msg=f"{k} at {now}")
            np.testing.assert_array_equal(after[k][rest].view(np.uint8), before[k][rest].view(np.uint8), err_msg=k)
    assert seen == {0, 1, 2, 3, 4}


# ====================================================== K9 and the segment maximum
def impact_case(with_nan, S=200):
    rng = np.random.default_rng(90)
    leaf = rng.choice(np.arange(2, S), 20, replace=False)        # no out-edges
    src = [np.zeros(150, np.int64), np.ones(64, np.int64)]
    dst = [rng.integers(0, S, 150), rng.integers(0, S, 64)]
    rest = np.setdiff1d(np.arange(2, S), leaf)
    s = np.concatenate([rest, rng.choice(rest, 700 - len(rest))])   # every other node calls someone
    src.append(s)
    dst.append(rng.integers(0, S, 700))
    loops = rest[:30]
    src.append(loops)                                            # self-loops
    dst.append(loops)
    src.append(s[:50])                                           # duplicate edges, other weights
    dst.append(dst[2][:50])
    src, dst = np.concatenate(src), np.concatenate(dst)
    w = (1.0 - rng.random(len(src))).astype(F32)                 # (0, 1]
    w[:10] = 1.0
    g = MI.CallGraph.from_edges(S, src, dst, w)
    deg = np.diff(g.rowptr)
    assert deg[0] == 150 and deg[1] == 64 and (deg[leaf] == 0).all() and (deg == 0).sum() == 20
    a = rng.uniform(0, 1, S).astype(F32)
    a[rng.random(S) < 0.3] = 0.0
    if with_nan:
        a[[int(dst[0]), int(loops[0]), int(leaf[0])]] = np.nan
    return g, a


def spec_downstream_impact(g, a, hops):
    """impact_h[u] = max(0, max over the out-edges (u, v, w) of max(a[v], impact_{h-1}[v]) w)
    in fp32, a NaN score counting as no evidence (0)."""
    S = a.size
    a = np.where(np.isnan(a), F32(0), a).astype(F32)
    prev = np.zeros(S, F32)
    for h in range(hops):
        out = np.zeros(S, F32)
        for u in range(S):
            for k in range(int(g.rowptr[u]), int(g.rowptr[u + 1])):
                v = int(g.col[k])
                out[u] = max(out[u], F32(max(a[v], prev[v]) * g.weight[k]))
        prev = out
    return prev


@pytest.mark.parametrize("with_nan", [False, True])
def test_ref_downstream_impact_matches_scalar_spec(with_nan):
    g, a = impact_case(with_nan)
    for hops in (1, 2, 3, 4):
        ref = MI.downstream_impact(g, torch.from_numpy(a), hops).numpy()
        np.testing.assert_array_equal(ref, spec_downstream_impact(g, a, hops))
        assert np.isfinite(ref).all() and (ref[np.diff(g.rowptr) == 0] == 0).all()
    assert (ref > 0).sum() > 100


@pytest.mark.gpu
@pytest.mark.parametrize("with_nan", [False, True])
def test_gpu_downstream_impact_edges(cuda, with_nan):
    """Rows of 150 and 64 edges (the lane-stride loop runs 3 and 1 times), rows
    without edges, self-loops, duplicate edges, zero and NaN scores, 1-4 hops."""
    g, a = impact_case(with_nan)
    for hops in (1, 2, 3, 4):
        ig = MI.downstream_impact(g, torch.from_numpy(a).to(cuda), hops).cpu().numpy()
        ic = MI.downstream_impact(g, torch.from_numpy(a), hops).numpy()
        np.testing.assert_allclose(ig, ic, rtol=1e-6)
        np.testing.assert_array_equal(ig == 0, ic == 0)


def segmax_case(S, K):
    rng = np.random.default_rng(S + K)
    v = rng.normal(0.3, 1, S).astype(F32)
    v[rng.random(S) < 0.1] = 0.0
    v[rng.random(S) < 0.05] = np.nan
    seg = rng.integers(0, K, S).astype(np.int64)
    seg[rng.random(S) < 0.05] = -1
    seg[rng.random(S) < 0.05] = K
    if S > 1:
        v[0], seg[0] = np.inf, 0
        v[1], seg[1] = 1e9, K                                    # a large value that must not land anywhere
        seg[seg == K - 1] = 0                                    # the last segment stays empty
    return v, seg


def spec_segment_max(v, seg, K):
    out = np.zeros(K, F32)
    for x, k in zip(v.tolist(), seg.tolist()):
        if 0 <= k < K and not math.isnan(x) and x > out[k]:
            out[k] = x
    return out


SEGMAX_CASES = [(1, 1), (5000, 300), (5000, 16384)]


@pytest.mark.parametrize("S,K", SEGMAX_CASES)
def test_ref_segment_max_matches_scalar_spec(S, K):
    v, seg = segmax_case(S, K)
    ref = MI.segment_max(torch.from_numpy(v), torch.from_numpy(seg), K).numpy()
    np.testing.assert_array_equal(ref, spec_segment_max(v, seg, K))
    if S > 1:
        assert ref[0] == np.inf and ref[K - 1] == 0 and ref.max() == np.inf and (ref == 0).any()


@pytest.mark.gpu
@pytest.mark.parametrize("S,K", SEGMAX_CASES)
def test_gpu_segment_max_edges(cuda, S, K):
    """K past one trip of the 256-thread loops and at the LDS limit, three blocks
    merging, NaN / negative / zero values, ids -1 and K, empty segments."""
    v, seg = segmax_case(S, K)
    mg = MI.segment_max(torch.from_numpy(v).to(cuda), torch.from_numpy(seg).to(cuda), K).cpu().numpy()
    mc = MI.segment_max(torch.from_numpy(v), torch.from_numpy(seg), K).numpy()
    np.testing.assert_array_equal(mg, mc)


@pytest.mark.gpu
def test_gpu_segment_max_rejects_too_many_segments(cuda):
    v = torch.zeros(8, device=cuda)
    seg = torch.zeros(8, dtype=torch.int64, device=cuda)
    with pytest.raises(RuntimeError):
        MI.segment_max(v, seg, 16385)
    torch.cuda.synchronize()


# ========================================================================== K10
LSQ_H = 10


def lsq_case(T, R):
    """Rows [R, ceil4(T)]; the first rows (as far as R reaches) hold: 5 % NaN, a
    NaN first sample, +inf and -inf samples, no data, NaN on the first 40 columns."""
    rng = np.random.default_rng(T + R)
    t = np.arange(T)
    x = (10 + rng.uniform(0.5, 2, (R, 1)) * np.sin(2 * np.pi * t / 1440 + rng.uniform(0, 6, (R, 1))) + 0.0005 * t
         + rng.normal(0, 0.05, (R, T))).astype(F32)
    special = [lambda r: r.__setitem__(rng.random(T) < 0.05, np.nan),
               lambda r: r.__setitem__(0, np.nan),
               lambda r: (r.__setitem__(T // 3, np.inf), r.__setitem__(T // 2, -np.inf), r.__setitem__(T - 1, np.inf)),
               lambda r: r.__setitem__(slice(None), np.nan),
               lambda r: r.__setitem__(slice(0, 40), np.nan)]
    for i, f in enumerate(special):
        if 1 + i < R:
            f(x[1 + i])
    if R == 1:
        special[0](x[0])
    Y = np.zeros((R, _ceil4(T)), F32)
    Y[:, :T] = x
    return Y


def _lsq_basis(T, dev="cpu"):
    ut = LQ._basis(T, LSQ_H, 60.0)[0]
    return torch.from_numpy(ut).to(dev)


def spec_lsq(Y, T, ut, rows):
    """z = U^T (y - c) over the finite samples, c = the first sample when finite
    else 0; sse = sum over the finite samples of (y - c - U z)^2 with z in fp32."""
    out = {}
    U = ut[:, :T].astype(np.float64)
    for r in rows:
        y = [float(v) for v in Y[r, :T]]
        c = y[0] if math.isfinite(y[0]) else 0.0
        fin = [t for t in range(T) if math.isfinite(y[t])]
        z = [math.fsum((y[t] - c) * U[f, t] for t in fin) for f in range(LQ.F)]
        yy = math.fsum((y[t] - c) ** 2 for t in fin)
        z32 = np.asarray(z, F32).astype(np.float64)
        sse = math.fsum((y[t] - c - float(z32 @ U[:, t])) ** 2 for t in fin)
        out[r] = (np.asarray(z), yy, c, len(fin), sse)
    return out


@pytest.mark.parametrize("T", [84, 2017])
def test_ref_lsq_matches_scalar_spec(T):
    R = 33
    Y = lsq_case(T, R)
    XT = _lsq_basis(T)
    Z, yy, sh, nv = LQ.lsq_project(torch.from_numpy(Y), T, XT)
    sse = LQ.lsq_residual(torch.from_numpy(Y), T, XT, Z, sh)
    assert nv.dtype == torch.int32
    rows = list(range(7))
    for r, (z, y2, c, n, s) in spec_lsq(Y, T, XT.numpy(), rows).items():
        scale = max(1.0, float(np.abs(z).max()))
        np.testing.assert_allclose(Z[r].numpy(), z, rtol=1e-6, atol=1e-6 * scale)
        np.testing.assert_allclose(float(yy[r]), y2, rtol=1e-6)
        assert float(sh[r]) == c and int(nv[r]) == n
        np.testing.assert_allclose(float(sse[r]), s, rtol=1e-6, atol=1e-9)
    assert int(nv[4]) == 0 and float(sh[2]) == 0 and int(nv[3]) == T - 3 and int(nv[5]) == T - 40
    fit = LQ.prophet_fit(torch.from_numpy(Y), T, LSQ_H)
    rank = LQ._basis(T, LSQ_H, 60.0)[3]
    want = np.sqrt(sse.numpy() / np.maximum(nv.numpy() - rank, 1))
    np.testing.assert_allclose(fit.sigma.numpy(), want, rtol=1e-6)


LSQ_CASES = [(T, R) for T in (84, 100, 160, 2017) for R in (1, 33, 133)]


@pytest.mark.gpu
@pytest.mark.parametrize("T,R", LSQ_CASES)
def test_gpu_lsq_edges(cuda, T, R):
    """T % 64 = 20, 36, 32, 33 (a chunk partly past T in either half-wave, T % 4 != 0,
    T % 32 != 0 in the residual pass), R < 32 and R % 32 = 1, NaN / inf samples, a NaN
    first sample, an empty row."""
    Y = lsq_case(T, R)
    Yg = torch.from_numpy(Y).to(cuda)
    XTc, XTg = _lsq_basis(T), _lsq_basis(T, cuda)
    Zc, yyc, shc, nvc = LQ.lsq_project(torch.from_numpy(Y), T, XTc)
    Zg, yyg, shg, nvg = LQ.lsq_project(Yg, T, XTg)
    np.testing.assert_array_equal(nvg.cpu().numpy(), nvc.numpy())
    np.testing.assert_array_equal(shg.cpu().numpy(), shc.numpy())
    np.testing.assert_allclose(Zg.cpu().numpy(), Zc.numpy(), rtol=1e-4, atol=1e-2)
    # the residual pass alone, on the CPU projection
    sc = LQ.lsq_residual(torch.from_numpy(Y), T, XTc, Zc, shc).numpy()
    sg = LQ.lsq_residual(Yg, T, XTg, Zc.to(cuda), shc.to(cuda)).cpu().numpy()
    print("K10 sse gpu/cpu", T, R, (sg / np.where(sc > 0, sc, 1)).tolist()[:8])
    np.testing.assert_allclose(sg, sc, rtol=1e-4)
    g = LQ.prophet_fit(Yg, T, LSQ_H)
    c = LQ.prophet_fit(torch.from_numpy(Y), T, LSQ_H)
    print("K10 forecast err", T, R, float((g.forecast.cpu() - c.forecast).abs().max()),
          "sigma", g.sigma.cpu().numpy()[:8].tolist(), c.sigma.numpy()[:8].tolist())
    np.testing.assert_allclose(g.forecast.cpu().numpy(), c.forecast.numpy(), rtol=1e-3, atol=2e-3)
    np.testing.assert_allclose(g.sigma.cpu().numpy(), c.sigma.numpy(), rtol=1e-3)
