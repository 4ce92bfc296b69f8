"""K5 bivariate normal, K12 multivariate normal, K17 robust multivariate, K13 robust (median / MAD) statistics,
K14 seasonal robust model, K15 level-shift robust model, K16 trend robust model, K22 seasonal scale robust
model, K23 hold-out score, K24 quantile robust statistics (csrc/kernels/quantile_robust.hip), K26 seasonal
quantile robust model (csrc/kernels/seasonal_quantile_robust.hip), K8 HPA score,
K9 downstream impact (csrc/kernels/bivariate.hip, csrc/kernels/mvn.hip,
csrc/kernels/mvn_robust.hip, csrc/kernels/robust_stats.hip, csrc/kernels/seasonal_robust.hip,
csrc/kernels/level_shift.hip, csrc/kernels/trend_robust.hip, csrc/kernels/seasonal_scale_robust.hip,
csrc/kernels/holdout_score.hip, csrc/kernels/hpa_graph.hip) with numpy references."""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from ._lib import LIB, check, ptr, require_native, stream_of


# --------------------------------------------------------------------------- K5
def bivariate(ha: torch.Tensor, hb: torch.Tensor, T: int, ca: torch.Tensor, cb: torch.Tensor, threshold: float):
    """Mahalanobis-distance detector over metric pairs.  Returns
    (params [P,5] = (mean_a, mean_b, cov_aa, cov_ab, cov_bb), dist [P,n],
    flags [P,NW] int64, count [P] int32)."""
    P, n = ca.shape
    NW = max(1, (n + 63) // 64)
    if not ha.is_cuda:
        return tuple(torch.from_numpy(a) for a in ref_bivariate(ha.numpy()[:, :T], hb.numpy()[:, :T], ca.numpy(),
                                                                cb.numpy(), threshold))
    require_native(ha)
    check(ha.stride(0) == hb.stride(0) and ca.stride(0) == cb.stride(0), "pair rows must share strides")
    d = ha.device
    thr = torch.tensor([threshold], dtype=torch.float32, device=d)
    params = torch.empty((P, 5), dtype=torch.float32, device=d)
    dist = torch.empty((P, n), dtype=torch.float32, device=d)
    flags = torch.empty((P, NW), dtype=torch.int64, device=d)
    cnt = torch.empty((P,), dtype=torch.int32, device=d)
    LIB.call("fm_bivariate", ptr(ha), ptr(hb), ha.stride(0), T, ptr(ca), ptr(cb), ca.stride(0), n, P, ptr(thr),
             ptr(params), ptr(dist), ptr(flags), NW, ptr(cnt), stream_of(ha))
    return params, dist, flags, cnt


# Relative ridge on the diagonal of the 2x2 covariance (MVN_RIDGE's role in K12).
BIVARIATE_RIDGE = 1e-6


def ref_bivariate(ha, hb, ca, cb, threshold):
    """fp64 oracle of K5.  A history pair counts when both members are finite;
    mean and covariance C (n - 1 in the denominator) over those n pairs.
    ``S`` = C with each diagonal entry scaled by ``1 + BIVARIATE_RIDGE`` plus
    1e-30, which is positive definite for any C: on the correlation matrix
    that is the ridge K12 adds, so the detector does not depend on the
    members' units, a dependent pair (correlation 1) keeps a direction across
    its line that is 1e-3 sigma wide, and a constant member stays finite.
    ``dist = sqrt(dx' S^-1 dx)``, flagged when ``dist > threshold``; NaN and
    no flag where a current member is not finite or ``n < 2``."""
    ha = np.asarray(ha, np.float64)
    hb = np.asarray(hb, np.float64)
    ok = np.isfinite(ha) & np.isfinite(hb)
    n = ok.sum(1)
    ma = np.where(ok, ha, 0).sum(1) / np.maximum(n, 1)
    mb = np.where(ok, hb, 0).sum(1) / np.maximum(n, 1)
    da = np.where(ok, ha - ma[:, None], 0)
    db = np.where(ok, hb - mb[:, None], 0)
    den = np.maximum(n - 1, 1)
    caa, cbb, cab = (da * da).sum(1) / den, (db * db).sum(1) / den, (da * db).sum(1) / den
    saa, sbb = caa * (1 + BIVARIATE_RIDGE) + 1e-30, cbb * (1 + BIVARIATE_RIDGE) + 1e-30
    det = saa * sbb - cab * cab
    with np.errstate(invalid="ignore", over="ignore"):
        xa = ca - ma[:, None]
        xb = cb - mb[:, None]
        q = (xa * xa * sbb[:, None] - 2 * xa * xb * cab[:, None] + xb * xb * saa[:, None]) / det[:, None]
        dist = np.sqrt(np.maximum(q, 0))
    # fewer than two complete pairs: no covariance, so no distance and no flag
    fin = np.isfinite(ca) & np.isfinite(cb) & (n > 1)[:, None]
    dist = np.where(fin, dist, np.nan)
    flag = fin & (dist > threshold)
    P, m = ca.shape
    NW = max(1, (m + 63) // 64)
    padded = np.zeros((P, NW * 64), bool)
    padded[:, :m] = flag
    words = np.packbits(padded.reshape(P, NW, 64), axis=2, bitorder="little").view(np.uint64).reshape(P, NW)
    params = np.stack([ma, mb, caa, cab, cbb], 1).astype(np.float32)
    return params, dist.astype(np.float32), words.view(np.int64), flag.sum(1).astype(np.int32)


# --------------------------------------------------------------------------- K12
MVN_MAX_K = 8
MVN_RIDGE = 1e-6
# Moment form of the kernel (csrc/kernels/mvn.hip): 0 = mean sweep then centred
# sweep, 1 = shift from the row tails then one centred sweep.  Form 1 measured
# 0.86 ms against 1.12 ms at the fleet shape with equal results (docs/PERF.md).
MVN_FORM = 1


def mvn_cuts(thr: float, factor: float = 1.0) -> np.ndarray:
    """Flag cuts of the joint detector, [2, 9] fp32: row 0 for ``thr``, row 1
    for ``thr * factor`` (groups with a differing canary), column k for k
    live members.  The threshold stays in sigma units: the cut is the
    Mahalanobis distance whose chi-square(k) upper tail equals the two-sided
    normal tail of ``thr``, so ``cut(thr, 1) == thr``; column 0 is 0."""
    from scipy.special import chdtri, erfc
    out = np.zeros((2, MVN_MAX_K + 1), np.float64)
    for r, t in enumerate((float(thr), float(thr) * float(factor))):
        p = erfc(t / np.sqrt(2.0))
        out[r, 1:] = np.sqrt(chdtri(np.arange(1, MVN_MAX_K + 1), p))
        out[r, 1] = t
    return out.astype(np.float32)


def _pack_words(flag: np.ndarray) -> np.ndarray:
    P, m = flag.shape
    NW = max(1, (m + 63) // 64)
    padded = np.zeros((P, NW * 64), bool)
    padded[:, :m] = flag
    return np.packbits(padded.reshape(P, NW, 64), axis=2, bitorder="little").view(np.uint64).reshape(P, NW).view(
        np.int64)


def ref_mvn(hist, cur, rows, K: int, cuts, lowered, min_n: int):
    """fp64 oracle of the joint multivariate-normal detector over groups of
    ``K`` rows (``rows`` [G, 8] row ids into ``hist`` [R, T] / ``cur`` [R, n]).
    Returns (params [G, 2 + K + K(K+1)/2] = (N, k, mean, upper-triangular
    covariance), dist [G, n], flags [G, NW] int64, count [G] int32,
    valid [G] int32: bit 0 enough complete history, bit 1 a current point
    present)."""
    hist = np.asarray(hist, np.float32)
    cur = np.asarray(cur, np.float32)
    rows = np.asarray(rows)
    cuts = np.asarray(cuts, np.float32)
    G, n = rows.shape[0], cur.shape[1]
    iu = np.triu_indices(K)
    params = np.zeros((G, 2 + K + len(iu[0])), np.float32)
    dist = np.full((G, n), np.nan, np.float32)
    flag = np.zeros((G, n), bool)
    valid = np.zeros(G, np.int32)
    used = np.zeros(G, np.float32)
    for g in range(G):
        r = rows[g, :K].astype(np.int64)
        h = hist[r].astype(np.float64)
        x = cur[r].astype(np.float64)
        h = h[:, np.isfinite(h).all(0)]                      # complete columns
        N = h.shape[1]
        mu = h.mean(1) if N else np.zeros(K)
        d = h - mu[:, None]
        C = d @ d.T / max(N - 1, 1)
        live = np.diag(C) > 1e-12 * mu * mu + 1e-30
        k = int(live.sum())
        params[g, 0], params[g, 1], params[g, 2:2 + K], params[g, 2 + K:] = N, k, mu, C[iu]
        used[g] = cuts[1 if lowered[g] else 0, k]
        present = np.isfinite(x).all(0)
        ok = N >= max(int(min_n), K + 2)
        valid[g] = int(ok) | (int(present.any()) << 1)
        if not ok:
            continue
        dg = np.zeros(n)
        if k:
            sd = np.sqrt(np.diag(C)[live])
            Rm = C[np.ix_(live, live)] / np.outer(sd, sd)
            np.fill_diagonal(Rm, 1.0)
            L = np.linalg.cholesky(Rm + MVN_RIDGE * np.eye(k))
            z = np.where(present, (x[live] - mu[live, None]) / sd[:, None], 0.0)
            dg = np.sqrt((np.linalg.solve(L, z) ** 2).sum(0))
        dead = ~live
        if dead.any():
            with np.errstate(invalid="ignore"):
                moved = (np.abs(x[dead] - mu[dead, None]) > 1e-6 * np.abs(mu[dead, None]) + 1e-12).any(0)
            dg = np.where(moved, np.inf, dg)
        dist[g] = np.where(present, dg, np.nan)
        with np.errstate(invalid="ignore"):
            flag[g] = present & (dist[g] > used[g])
    return params, dist, _pack_words(flag), flag.sum(1).astype(np.int32), valid


def _mvn_args(hist, T, cur, rows, K, cuts, lowered) -> np.ndarray:
    """The argument checks of the joint detectors' wrappers (nothing is
    launched when one fails) -> ``cuts`` as fp32 [2, 9]."""
    check(2 <= int(K) <= MVN_MAX_K, f"group size must be in [2, {MVN_MAX_K}]")
    check(rows.dim() == 2 and rows.shape[1] == MVN_MAX_K and rows.dtype == torch.int32, "rows must be int32 [G, 8]")
    check(hist.dtype == torch.float32 and cur.dtype == torch.float32 and hist.shape[0] == cur.shape[0]
          and 0 < T <= hist.shape[1], "hist / cur must be fp32 with the same rows")
    G = rows.shape[0]
    check(lowered.numel() == G and lowered.dtype == torch.uint8, "lowered must be uint8 [G]")
    cuts = np.asarray(cuts, np.float32)
    check(cuts.shape == (2, MVN_MAX_K + 1), "cuts must be [2, 9]")
    if G:
        used = rows[:, :K]
        check(int(used.min().item()) >= 0 and int(used.max().item()) < hist.shape[0], "row ids out of range")
    if hist.is_cuda:
        check(hist.stride(1) == 1 and hist.stride(0) % 4 == 0 and hist.data_ptr() % 16 == 0 and cur.stride(1) == 1,
              "rows must be contiguous, 16-B aligned, with a row stride that is a multiple of 4")
    return cuts


def _mvn_outputs(G: int, n: int, K: int, d):
    NA, NW = K + K * (K + 1) // 2, max(1, (n + 63) // 64)
    return (torch.empty((G, 2 + NA), dtype=torch.float32, device=d), torch.empty((G, n), dtype=torch.float32, device=d),
            torch.zeros((G, NW), dtype=torch.int64, device=d), torch.empty((G,), dtype=torch.int32, device=d),
            torch.empty((G,), dtype=torch.int32, device=d))


def mvn(hist: torch.Tensor, T: int, cur: torch.Tensor, rows: torch.Tensor, K: int, cuts, lowered: torch.Tensor,
        min_n: int):
    """Joint multivariate-normal detector (K12) over groups of ``K`` member
    rows: ``rows`` [G, 8] int32 row ids into ``hist`` [R, ld] (first ``T``
    columns) and ``cur`` [R, n], -1 padded past ``K``; ``cuts`` from
    :func:`mvn_cuts`; ``lowered`` [G] uint8 picks row 1 of ``cuts``.
    Returns what :func:`ref_mvn` returns, which is also the CPU path."""
    cuts = _mvn_args(hist, T, cur, rows, K, cuts, lowered)
    G, n = rows.shape[0], cur.shape[1]
    if not hist.is_cuda:
        return tuple(torch.from_numpy(a) for a in ref_mvn(hist.numpy()[:, :T], cur.numpy(), rows.numpy(), K, cuts,
                                                          lowered.numpy(), min_n))
    require_native(hist)
    d = hist.device
    params, dist, flags, cnt, valid = _mvn_outputs(G, n, K, d)
    if G == 0 or n == 0:
        return params, dist, flags, cnt, valid
    ct = torch.from_numpy(cuts).to(d)
    rows = rows.contiguous()
    LIB.call("fm_mvn", ptr(hist), hist.stride(0), int(T), hist.shape[0], ptr(cur), cur.stride(0), n, ptr(rows), G,
             int(K), ptr(ct), ptr(lowered.contiguous()), int(min_n), MVN_FORM, ptr(params), ptr(dist), ptr(flags),
             flags.shape[1], ptr(cnt), ptr(valid), stream_of(hist))
    return params, dist, flags, cnt, valid


# --------------------------------------------------------------------------- K17
# Incident columns are those with a member further than this many of its own MAD-sigmas from its median.
MVN_REJECT = 3.5


def ref_mvn_robust(hist, cur, rows, K: int, cuts, lowered, min_n: int, reject: float = MVN_REJECT):
    """Oracle of the robust joint detector: :func:`ref_mvn` over the history
    columns that are not incident columns -> its five arrays and ``rejected``
    [G] int32, the columns set aside.

    ``(c_r, s_r, n_r) = ref_robust_stats(hist, T)`` per member row over its
    own finite samples; ``lim_r = fp32(reject) * s_r``, one fp32 product.  A
    complete column ``t`` (every member finite) is an incident column when
    any member has ``fabs(fp32(x_rt - c_r)) > lim_r``, all in fp32; a
    comparison against a NaN limit is false, and a constant row (``s = 0``,
    every deviation 0) rejects nothing.  ``reject <= 0``, NaN or +inf rejects
    nothing.  Breakdown guard: a group with ``2 * rejected > complete``
    rejects nothing (``rejected = 0``): the robust start does not describe
    its bulk.  The incident columns are then masked (NaN) and the group goes
    through :func:`ref_mvn` itself, so N, the ``valid`` gate ``N >=
    max(min_n, K + 2)`` and everything after are taken over the columns kept,
    and with nothing rejected the result is :func:`ref_mvn`'s.  No
    consistency correction is applied for the trimmed tails."""
    hist = np.asarray(hist, np.float32)
    cur = np.asarray(cur, np.float32)
    rows = np.asarray(rows)
    lowered = np.asarray(lowered)
    G, T = rows.shape[0], hist.shape[1]
    rejected = np.zeros(G, np.int32)
    if G == 0:
        return ref_mvn(hist, cur, rows, K, cuts, lowered, min_n) + (rejected,)
    members = np.unique(rows[:, :K].astype(np.int64))
    c = np.full(hist.shape[0], np.nan, np.float32)
    lim = np.full(hist.shape[0], np.inf, np.float32)
    rj = np.float32(reject)
    c[members], s, _ = ref_robust_stats(hist[members], T)
    if rj > 0 and np.isfinite(rj):
        lim[members] = rj * s
    own = np.full((1, MVN_MAX_K), -1, np.int32)
    own[0, :K] = np.arange(K)
    parts = []
    for g in range(G):
        r = rows[g, :K].astype(np.int64)
        h = hist[r]                                           # a copy
        complete = np.isfinite(h).all(0)
        with np.errstate(invalid="ignore", over="ignore"):
            out = complete & (np.abs(h - c[r, None]) > lim[r, None]).any(0)
        if 2 * int(out.sum()) <= int(complete.sum()):
            rejected[g] = out.sum()
            h[:, out] = np.nan
        parts.append(ref_mvn(h, cur[r], own, K, cuts, lowered[g:g + 1], min_n))
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(5)) + (rejected,)


def mvn_robust(hist: torch.Tensor, T: int, cur: torch.Tensor, rows: torch.Tensor, K: int, cuts,
               lowered: torch.Tensor, min_n: int, reject: float = MVN_REJECT):
    """Robust joint detector (K13 + K17): :func:`mvn`'s arguments and
    ``reject``; returns what :func:`ref_mvn_robust` returns, which is also
    the CPU path.  On the GPU the members' median / MAD statistics come from
    ``fm_robust_stats``: one launch over the whole buffer when the groups'
    ``G * K`` member rows are at least half of its rows, else over a gathered
    copy of the member rows (scattered back by row id)."""
    cuts = _mvn_args(hist, T, cur, rows, K, cuts, lowered)
    G, n = rows.shape[0], cur.shape[1]
    if not hist.is_cuda:
        return tuple(torch.from_numpy(a) for a in ref_mvn_robust(hist.numpy()[:, :T], cur.numpy(), rows.numpy(), K,
                                                                 cuts, lowered.numpy(), min_n, reject))
    require_native(hist)
    d = hist.device
    out = _mvn_outputs(G, n, K, d)
    rejected = torch.zeros((G,), dtype=torch.int32, device=d)
    if G == 0 or n == 0:
        return out + (rejected,)
    params, dist, flags, cnt, valid = out
    R = hist.shape[0]
    stats = torch.empty((R, 3), dtype=torch.float32, device=d)
    if 2 * G * int(K) >= R:
        LIB.call("fm_robust_stats", ptr(hist), hist.stride(0), int(T), R, ptr(stats), stream_of(hist))
    else:
        ids = torch.unique(rows[:, :K]).long()
        sub = hist.index_select(0, ids)
        part = torch.empty((ids.numel(), 3), dtype=torch.float32, device=d)
        LIB.call("fm_robust_stats", ptr(sub), sub.stride(0), int(T), ids.numel(), ptr(part), stream_of(hist))
        stats[ids] = part
    ct = torch.from_numpy(cuts).to(d)
    rows = rows.contiguous()
    LIB.call("fm_mvn_robust", ptr(hist), hist.stride(0), int(T), R, ptr(cur), cur.stride(0), n, ptr(rows), G, int(K),
             ptr(ct), ptr(lowered.contiguous()), int(min_n), ptr(stats), float(reject), ptr(params), ptr(dist),
             ptr(flags), flags.shape[1], ptr(cnt), ptr(valid), ptr(rejected), stream_of(hist))
    return params, dist, flags, cnt, valid, rejected


# --------------------------------------------------------------------------- K13
# Longest row the kernel selects in LDS (csrc/kernels/robust_stats.hip
# kRobustLdsKeys); longer rows take its global-memory path.
ROBUST_LDS_KEYS = 13312


def ref_robust_stats(hist, T: int):
    """Median / MAD statistics of the finite samples of ``hist[r, :T]`` ->
    (center [R] f32, sigma [R] f32, n [R] int32), all arithmetic in fp32.
    With ``s`` the sorted finite samples, ``center = 0.5 s[(n-1)//2] +
    0.5 s[n//2]``; ``mad`` is the same middle of the sorted ``|x - center|``;
    ``sigma = 1.4826 mad`` when ``mad > 0``, else ``1.2533 * mean|x - center|``
    (the mean summed and divided in fp64, rounded once to fp32), which is 0
    for a constant row only.  ``n == 0`` gives NaN, NaN.  The selection is
    exact, so the GPU kernel reproduces ``center`` and ``mad`` bit for bit."""
    x = np.asarray(hist, np.float32)[:, :T]
    R = x.shape[0]
    fin = np.isfinite(x)
    n = fin.sum(1).astype(np.int32)
    center = np.full(R, np.nan, np.float32)
    sigma = np.full(R, np.nan, np.float32)
    if x.shape[1] == 0 or not n.any():
        return center, sigma, n
    half = np.float32(0.5)
    lo = (np.maximum(n, 1) - 1) // 2
    up = np.maximum(n, 1) // 2

    def middle(v):                                  # missing samples sort last as +inf
        s = np.sort(np.where(fin, v, np.float32(np.inf)), axis=1)
        return half * np.take_along_axis(s, lo[:, None], 1)[:, 0] + half * np.take_along_axis(s, up[:, None], 1)[:, 0]

    with np.errstate(invalid="ignore", over="ignore"):
        c = middle(x)
        d = np.abs(x - c[:, None])
        mad = middle(d)
        mean_d = (np.where(fin, d, 0).astype(np.float64).sum(1) / np.maximum(n, 1)).astype(np.float32)
        sg = np.where(mad > 0, np.float32(1.4826) * mad, np.float32(1.2533) * mean_d).astype(np.float32)
    ok = n > 0
    center[ok], sigma[ok] = c[ok], sg[ok]
    return center, sigma, n


def robust_stats(hist: torch.Tensor, T: int) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """K13: per-row (center, sigma, n) of :func:`ref_robust_stats` over
    ``hist[:, :T]``, by exact selection on the GPU.  ``hist`` may be any
    column view with unit column stride: rows need 4-byte alignment only."""
    check(hist.dim() == 2 and hist.dtype == torch.float32 and 0 <= T <= hist.shape[1],
          "hist must be fp32 [R, >= T]")
    if not hist.is_cuda:
        c, s, n = ref_robust_stats(hist.numpy(), T)
        return torch.from_numpy(c), torch.from_numpy(s), torch.from_numpy(n)
    require_native(hist)
    check(hist.stride(1) == 1 or hist.shape[1] <= 1, "rows must have unit column stride")
    R = hist.shape[0]
    out = torch.empty((R, 3), dtype=torch.float32, device=hist.device)
    if R:
        LIB.call("fm_robust_stats", ptr(hist), hist.stride(0), int(T), R, ptr(out), stream_of(hist))
    return out[:, 0], out[:, 1], out[:, 2].to(torch.int32)


# --------------------------------------------------------------------------- K18
def robust_stats_cached(hist: torch.Tensor, T: int, rowmap: torch.Tensor | None, cache,
                        expect_miss: bool | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """K18: :func:`robust_stats` of the rows ``hist[rowmap[r], :T]`` (identity
    without a row map) with the three floats of every physical row kept in
    ``cache`` (an ``engine.resident.RowStatsCache`` over the rows of ``hist``,
    or None): a row whose entry carries the tag ``T`` is copied, any other is
    selected and recorded.  ``expect_miss`` only shapes the launch (None: the
    cache's own estimate): True computes every row without looking at the
    cache, False tests every entry.  Whoever writes a row of ``hist`` calls
    ``cache.touch`` on the same stream.  CPU: :func:`ref_robust_stats` over
    the mapped rows; the cache is ignored."""
    check(hist.dim() == 2 and hist.dtype == torch.float32 and 0 <= T <= hist.shape[1],
          "hist must be fp32 [P, >= T]")
    if rowmap is not None:
        check(rowmap.dim() == 1 and rowmap.dtype == torch.int32 and rowmap.device == hist.device,
              "rowmap must be int32 [R] on the device of hist")
        if rowmap.numel():
            check(0 <= int(rowmap.min()) and int(rowmap.max()) < hist.shape[0], "rowmap points outside hist")
    R = hist.shape[0] if rowmap is None else rowmap.numel()
    if not hist.is_cuda:
        x = hist.numpy() if rowmap is None else hist.numpy()[rowmap.numpy().astype(np.int64)]
        c, s, n = ref_robust_stats(x, T)
        return torch.from_numpy(c), torch.from_numpy(s), torch.from_numpy(n)
    require_native(hist)
    check(hist.stride(1) == 1 or hist.shape[1] <= 1, "rows must have unit column stride")
    if cache is not None:
        check(len(cache) >= hist.shape[0] and cache.valid.device == hist.device,
              "the cache must cover every row of hist, on its device")
    out = torch.empty((R, 3), dtype=torch.float32, device=hist.device)
    if R:
        miss = (cache is None or cache.expect_miss(int(T), R)) if expect_miss is None else bool(expect_miss)
        LIB.call("fm_robust_stats_cached", ptr(hist), hist.stride(0), int(T), R, ptr(out), ptr(rowmap),
                 ptr(cache.stats) if cache is not None else None, ptr(cache.valid) if cache is not None else None,
                 int(miss), 0, stream_of(hist))
        if cache is not None:
            cache.ticked(int(T))
    return out[:, 0], out[:, 1], out[:, 2].to(torch.int32)


# --------------------------------------------------------------------------- K14
# Most cycles the seasonal model reads (csrc/kernels/seasonal_robust.hip kMaxCycles).
SEASONAL_MAX_CYCLES = 16


def seasonal_cycles(T: int, m: int) -> int:
    """Whole cycles J of period ``m`` the seasonal robust model reads from a
    history of ``T`` samples: its span is the last ``J * m`` columns.  At most
    16 cycles, and the span plus two ``m``-word profile buffers fit K13's LDS
    budget.  The model is seasonal when ``J >= 2``."""
    T, m = int(T), int(m)
    if m < 1:
        return 0
    return max(0, min(T // m, SEASONAL_MAX_CYCLES, ROBUST_LDS_KEYS // m - 2))


def seasonal_halfwidth(m: int, smooth: int = 5) -> int:
    """Half width k of the smoothing window: ``smooth`` phases each side, but
    the window stays about a twelfth of the period (``m // 24`` each side)."""
    return max(0, min(int(smooth), int(m) // 24))


def _middle(v, ok, cnt, axis: int = 1):
    """K13's median rule along ``axis`` over the entries of ``v`` where ``ok``
    (``cnt`` of them, ``v``'s shape without that axis; a set with none gives a
    value to be masked).  Missing samples sort last as +inf."""
    s = np.sort(np.where(ok, v, np.float32(np.inf)), axis=axis)
    lo = np.expand_dims((np.maximum(cnt, 1) - 1) // 2, axis)
    up = np.expand_dims(np.maximum(cnt, 1) // 2, axis)
    half = np.float32(0.5)
    return (half * np.take_along_axis(s, lo, axis) + half * np.take_along_axis(s, up, axis)).squeeze(axis)


def _smooth_circular(raw, k: int):
    """``raw`` [R, m] f32 -> the mean of the finite ``raw[:, (p + d) % m]``,
    ``d = -k..k``, summed in that order and divided in fp64, rounded once to
    fp32; NaN where none is finite."""
    tot = np.zeros(raw.shape, np.float64)
    cnt = np.zeros(raw.shape, np.int64)
    for d in range(-k, k + 1):
        nb = np.roll(raw, -d, axis=1)               # nb[:, p] = raw[:, (p + d) % m]
        ok = np.isfinite(nb)
        tot += np.where(ok, nb, 0).astype(np.float64)
        cnt += ok
    return np.where(cnt > 0, tot / np.maximum(cnt, 1), np.nan).astype(np.float32)


def ref_seasonal_robust(hist, T: int, m: int, H: int, smooth: int = 5):
    """Per-phase median / MAD model of ``hist[r, :T]`` with period ``m`` ->
    (forecast [R, H] f32, sigma [R] f32, n [R] int32, profile [R, m] f32).

    The span is the last ``J * m`` columns (:func:`seasonal_cycles`); span
    index ``i`` has phase ``i % m``.  ``raw[p]`` is K13's median rule over the
    finite samples of phase ``p`` (NaN when it has none); ``profile[p]`` the
    mean of the finite ``raw[(p + d) % m]``, ``d = -k..k``
    (:func:`seasonal_halfwidth`), summed in that order and divided in fp64,
    rounded once to fp32.  ``mad`` is K13's middle of the sorted residuals
    ``|x - profile[phase]|`` of the ``n`` finite samples, with no re-centring;
    ``sigma = 1.4826 mad`` when ``mad > 0``, else ``1.2533 * mean residual``
    (fp64, rounded once); ``n == 0`` gives NaN.  ``forecast[:, h - 1] =
    profile[(h - 1) % m]``: the phase after the last sample is phase 0."""
    x = np.asarray(hist, np.float32)[:, :T]
    R = x.shape[0]
    m, H = int(m), int(H)
    J = seasonal_cycles(T, m)
    check(J >= 2, f"seasonal_robust needs two whole cycles within its budget (T = {T}, m = {m}: J = {J})")
    k = seasonal_halfwidth(m, smooth)
    span = x[:, T - J * m:T]
    fin = np.isfinite(span)
    n = fin.sum(1).astype(np.int32)

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        fin3 = fin.reshape(R, J, m)
        c = fin3.sum(1)
        raw = np.where(c > 0, _middle(span.reshape(R, J, m), fin3, c, 1), np.float32(np.nan)).astype(np.float32)
        profile = _smooth_circular(raw, k)
        r = np.abs(span - np.tile(profile, (1, J)))
        mad = _middle(r, fin, n)
        mean_r = (np.where(fin, r, 0).astype(np.float64).sum(1) / np.maximum(n, 1)).astype(np.float32)
        sigma = np.where(mad > 0, np.float32(1.4826) * mad, np.float32(1.2533) * mean_r).astype(np.float32)
    sigma[n == 0] = np.nan
    forecast = np.ascontiguousarray(profile[:, np.arange(H) % m])
    return forecast, sigma, n, profile


def seasonal_robust(hist: torch.Tensor, T: int, m: int, H: int, smooth: int = 5, want_profile: bool = False):
    """K14: (forecast [R, H], sigma [R], n [R] int32) of :func:`ref_seasonal_robust`
    over ``hist[:, :T]``, and the profile [R, m] behind them when
    ``want_profile``.  ``hist`` may be any column view with unit column
    stride: rows need 4-byte alignment only."""
    check(hist.dim() == 2 and hist.dtype == torch.float32 and 0 <= T <= hist.shape[1],
          "hist must be fp32 [R, >= T]")
    T, m, H = int(T), int(m), int(H)
    J = seasonal_cycles(T, m)
    check(J >= 2, f"seasonal_robust needs two whole cycles within its budget (T = {T}, m = {m}: J = {J})")
    check(H >= 0, "H must be >= 0")
    if not hist.is_cuda:
        out = tuple(torch.from_numpy(a) for a in ref_seasonal_robust(hist.numpy(), T, m, H, smooth))
        return out if want_profile else out[:3]
    require_native(hist)
    check(hist.stride(1) == 1 or hist.shape[1] <= 1, "rows must have unit column stride")
    R = hist.shape[0]
    fc = torch.empty((R, H), dtype=torch.float32, device=hist.device)
    stats = torch.empty((R, 2), dtype=torch.float32, device=hist.device)
    prof = torch.empty((R, m), dtype=torch.float32, device=hist.device) if want_profile else None
    if R:
        LIB.call("fm_seasonal_robust", ptr(hist), hist.stride(0), T, R, m, J, seasonal_halfwidth(m, smooth), H,
                 ptr(fc), max(H, 1), ptr(stats), ptr(prof), stream_of(hist))
    out = (fc, stats[:, 0], stats[:, 1].to(torch.int32))
    return out + (prof,) if want_profile else out


# --------------------------------------------------------------------------- K15
# Most blocks the level-shift model cuts a history into (csrc/kernels/level_shift.hip kMaxBlocks).
SHIFT_MAX_BLOCKS = 16


def shift_blocks(T: int, L: int) -> int:
    """Whole blocks J of ``L`` samples the level-shift model cuts from a
    history of ``T`` samples: the last ``J * L`` columns, block 0 the oldest,
    at most 16.  A shift can be found when ``J >= 3 + min_blocks``."""
    T, L = int(T), int(L)
    if L < 1:
        return 0
    return max(0, min(T // L, SHIFT_MAX_BLOCKS))


def shift_candidates(hist, T: int, L: int, min_blocks: int = 2):
    """The candidate table behind :func:`ref_shift_robust` -> (valid
    [R, J + 1] bool, score, d, den, edge [R, J + 1] f32, b [R, J] f32):
    column ``j`` is candidate ``j`` (a shift that ends with transition block
    ``j - 1``), ``edge = |b[j - 1] - p1|`` (NaN for an empty transition
    block), ``b`` the block medians.  Columns of invalid candidates hold 0."""
    x = np.asarray(hist, np.float32)[:, :T]
    R = x.shape[0]
    T, L, mb = int(T), int(L), int(min_blocks)
    check(mb >= 1, "min_blocks must be >= 1")
    J = shift_blocks(T, L)
    valid = np.zeros((R, J + 1), bool)
    score, dd, den, edge = (np.zeros((R, J + 1), np.float32) for _ in range(4))
    b = np.full((R, J), np.nan, np.float32)
    if J == 0 or R == 0:
        return valid, score, dd, den, edge, b
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        blk = x[:, T - J * L:T].reshape(R, J, L)
        fin = np.isfinite(blk)
        c = fin.sum(2)
        for j in range(J):
            b[:, j] = np.where(c[:, j] >= max(1, L // 4), _middle(blk[:, j], fin[:, j], c[:, j]), np.float32(np.nan))
        s_all = ref_robust_stats(x, T)[1]
        se = (np.float32(1.2533) * s_all / np.sqrt(np.float32(L))).astype(np.float32)
        bok = np.isfinite(b)
        for j in range(J - mb, 2, -1):
            pre, post = b[:, :j - 1], b[:, j:]
            npre, npost = bok[:, :j - 1].sum(1), bok[:, j:].sum(1)
            ok = (npre >= 2) & (npost >= mb)
            p0, p1 = _middle(pre, bok[:, :j - 1], npre), _middle(post, bok[:, j:], npost)
            d = (p1 - p0).astype(np.float32)
            dev = np.maximum(np.where(bok[:, :j - 1], np.abs(pre - p0[:, None]), 0).max(1),
                             np.where(bok[:, j:], np.abs(post - p1[:, None]), 0).max(1)).astype(np.float32)
            dn = np.where(se > dev, se, dev).astype(np.float32)
            sc = np.where(dn > 0, np.abs(d) / dn, np.where(d != 0, np.float32(np.inf), np.float32(0))).astype(np.float32)
            valid[:, j] = ok
            score[:, j] = np.where(ok, sc, 0)
            dd[:, j] = np.where(ok, d, 0)
            den[:, j] = np.where(ok, dn, 0)
            edge[:, j] = np.where(ok, np.abs(b[:, j - 1] - p1), 0)
    return valid, score, dd, den, edge, b


def ref_shift_robust(hist, T: int, L: int, k: float = 4.0, min_blocks: int = 2):
    """Median / MAD model of ``hist[r, :T]`` that restarts after the latest
    level shift -> (center [R] f32, sigma [R] f32, n [R] int32, start [R]
    int32, delta [R] f32, score [R] f32), all arithmetic in fp32.

    The last ``J * L`` columns (:func:`shift_blocks`) are cut into J blocks of
    L samples, block 0 the oldest.  ``b[j]`` is K13's median rule over the
    finite samples of block ``j``, NaN (empty) when it has fewer than
    ``max(1, L // 4)``.  ``se = 1.2533 s_all / sqrt(L)`` with ``s_all`` the
    sigma of :func:`ref_robust_stats` over the whole row: the standard error
    of a median of L independent samples, which floors the spread.

    Candidate ``j`` (``J - min_blocks`` down to 3): ``pre`` = the non-empty
    ``b[0..j-2]``, ``post`` = the non-empty ``b[j..J-1]``; block ``j - 1`` is
    the transition block and belongs to neither side.  It is valid with at
    least 2 ``pre`` and ``min_blocks`` ``post`` blocks; then ``p0``, ``p1`` =
    the median rule over each side, ``d = p1 - p0``, ``den = max(largest
    |b[i] - own side's median|, se)`` and ``score_j = |d| / den`` (``den ==
    0``: inf when ``d != 0``, else 0).

    The shift is the largest ``j`` with ``score_j > k``; its start block is
    ``j - 1`` when ``b[j-1]`` is finite and ``|b[j-1] - p1| <= den`` (the
    shift fell on a block boundary), else ``j``; ``start = T - (J -
    startblock) L``, ``delta = d``, ``score = score_j``.  Without a shift
    ``start = 0``, ``delta = 0`` and ``score`` is the largest score seen (0
    without a candidate).  ``(center, sigma, n)`` are
    :func:`ref_robust_stats` over columns ``[start, T)``."""
    x = np.asarray(hist, np.float32)[:, :T]
    R = x.shape[0]
    T, L = int(T), int(L)
    J = shift_blocks(T, L)
    valid, sc, dd, den, edge, _ = shift_candidates(x, T, L, min_blocks)
    start = np.zeros(R, np.int32)
    delta = np.zeros(R, np.float32)
    score = np.zeros(R, np.float32)
    found = np.zeros(R, bool)
    kf = np.float32(k)
    with np.errstate(invalid="ignore"):
        for j in range(J - int(min_blocks), 2, -1):
            live = valid[:, j] & ~found
            hit = live & (sc[:, j] > kf)
            sb = np.where(edge[:, j] <= den[:, j], j - 1, j)       # (a NaN edge compares false)
            start[hit] = (T - (J - sb) * L)[hit]
            delta[hit] = dd[hit, j]
            score[hit] = sc[hit, j]
            found |= hit
            seen = live & ~hit & (sc[:, j] > score)
            score[seen] = sc[seen, j]
    center = np.full(R, np.nan, np.float32)
    sigma = np.full(R, np.nan, np.float32)
    n = np.zeros(R, np.int32)
    for s0 in np.unique(start):
        rows = np.nonzero(start == s0)[0]
        center[rows], sigma[rows], n[rows] = ref_robust_stats(x[rows, s0:], T - int(s0))
    return center, sigma, n, start, delta, score


def shift_robust(hist: torch.Tensor, T: int, L: int, k: float = 4.0, min_blocks: int = 2):
    """K15: (center [R], sigma [R], n [R] int32, start [R] int32, delta [R],
    score [R]) of :func:`ref_shift_robust` over ``hist[:, :T]``.  ``hist`` may
    be any column view with unit column stride: rows need 4-byte alignment
    only.  The row lives in LDS, so ``T <= ROBUST_LDS_KEYS``."""
    check(hist.dim() == 2 and hist.dtype == torch.float32 and 0 <= T <= hist.shape[1],
          "hist must be fp32 [R, >= T]")
    T, L, mb = int(T), int(L), int(min_blocks)
    check(T <= ROBUST_LDS_KEYS, f"shift_robust holds the row in LDS: T = {T} > {ROBUST_LDS_KEYS}")
    check(L >= 1 and mb >= 1, "L and min_blocks must be >= 1")
    if not hist.is_cuda:
        c, s, n, st, dl, sc = ref_shift_robust(hist.numpy(), T, L, k, mb)
        return tuple(torch.from_numpy(a) for a in (c, s, n, st, dl, sc))
    require_native(hist)
    check(hist.stride(1) == 1 or hist.shape[1] <= 1, "rows must have unit column stride")
    R = hist.shape[0]
    out = torch.empty((R, 6), dtype=torch.float32, device=hist.device)
    if R:
        LIB.call("fm_shift_robust", ptr(hist), hist.stride(0), T, R, L, shift_blocks(T, L), float(k), mb, ptr(out),
                 stream_of(hist))
    return out[:, 0], out[:, 1], out[:, 2].to(torch.int32), out[:, 3].to(torch.int32), out[:, 4], out[:, 5]


# --------------------------------------------------------------------------- K16
def ref_trend_robust(hist, T: int, L: int, min_blocks: int = 3):
    """Median / MAD model of ``hist[r, :T]`` about a robustly fitted straight
    line -> (center [R] f32, sigma [R] f32, n [R] int32, slope [R] f32,
    nblocks [R] int32), all arithmetic in fp32.

    The last ``J * L`` columns (:func:`shift_blocks`) are cut into J blocks of
    L samples, block 0 the oldest.  ``b[j]`` is K13's median rule over the
    finite samples of block ``j``; a block with fewer than ``max(1, L // 4)``
    is empty, and ``nblocks`` counts the others, at indices ``q_0 < ... <
    q_{B-1}``.  With ``B >= min_blocks`` the slope is Siegel's repeated median
    of the block medians: ``s_i`` = the median rule over ``j != i`` of
    ``(b[q_j] - b[q_i]) / float((q_j - q_i) L)`` (one subtraction, one
    correctly rounded division), ``slope`` = the median rule over the ``s_i``.
    With fewer blocks, or a non-finite result, ``slope = 0``.

    The line is anchored at the last history sample: ``r_i = x_i - (slope *
    float(i - (T - 1)))``, the product rounded to fp32 and then the difference
    (no fused multiply-add).  ``(center, sigma, n)`` are
    :func:`ref_robust_stats` of ``r``, so the centre is the level at the end of
    the history and the forecast at horizon ``h`` (1 = the next sample) is
    ``center + slope * float(h)``.  A row with ``slope == 0`` gets
    :func:`ref_robust_stats` of the row itself."""
    x = np.asarray(hist, np.float32)[:, :T]
    R = x.shape[0]
    T, L, mb = int(T), int(L), int(min_blocks)
    check(mb >= 2, "min_blocks must be >= 2")
    J = shift_blocks(T, L)
    slope = np.zeros(R, np.float32)
    nblocks = np.zeros(R, np.int32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        if J > 0 and R > 0:
            blk = x[:, T - J * L:T].reshape(R, J, L)
            fin = np.isfinite(blk)
            c = fin.sum(2)
            b = np.full((R, J), np.nan, np.float32)
            for j in range(J):
                b[:, j] = _middle(blk[:, j], fin[:, j], c[:, j])
            ok = c >= max(1, L // 4)
            nblocks = ok.sum(1).astype(np.int32)
            # pair[r, i, j] = (b_j - b_i) / ((j - i) L); the diagonal and the empty blocks are masked out
            q = np.arange(J, dtype=np.int64)
            dist = ((q[None, :] - q[:, None]) * L).astype(np.float32)
            pair = ((b[:, None, :] - b[:, :, None]).astype(np.float32) / dist[None]).astype(np.float32)
            pok = ok[:, None, :] & ok[:, :, None] & (q[None, :] != q[:, None])[None]
            si = np.zeros((R, J), np.float32)
            for i in range(J):
                si[:, i] = _middle(pair[:, i], pok[:, i], pok[:, i].sum(1))
            sl = _middle(si, ok, nblocks)
            slope = np.where((nblocks >= mb) & np.isfinite(sl), sl, np.float32(0)).astype(np.float32)
        t = (np.arange(T, dtype=np.int64) - (T - 1)).astype(np.float32)
        r = x - (slope[:, None] * t[None, :]).astype(np.float32)
    center, sigma, n = ref_robust_stats(r, T)
    return center, sigma, n, slope, nblocks


def trend_robust(hist: torch.Tensor, T: int, L: int, min_blocks: int = 3):
    """K16: (center [R], sigma [R], n [R] int32, slope [R]) of
    :func:`ref_trend_robust` over ``hist[:, :T]``.  ``hist`` may be any column
    view with unit column stride: rows need 4-byte alignment only.  The row
    lives in LDS, so ``T <= ROBUST_LDS_KEYS``."""
    check(hist.dim() == 2 and hist.dtype == torch.float32 and 0 <= T <= hist.shape[1],
          "hist must be fp32 [R, >= T]")
    T, L, mb = int(T), int(L), int(min_blocks)
    check(T <= ROBUST_LDS_KEYS, f"trend_robust holds the row in LDS: T = {T} > {ROBUST_LDS_KEYS}")
    check(L >= 1 and mb >= 2, "L must be >= 1 and min_blocks >= 2")
    if not hist.is_cuda:
        return tuple(torch.from_numpy(a) for a in ref_trend_robust(hist.numpy(), T, L, mb)[:4])
    require_native(hist)
    check(hist.stride(1) == 1 or hist.shape[1] <= 1, "rows must have unit column stride")
    R = hist.shape[0]
    out = torch.empty((R, 4), dtype=torch.float32, device=hist.device)
    if R:
        LIB.call("fm_trend_robust", ptr(hist), hist.stride(0), T, R, L, shift_blocks(T, L), mb, ptr(out),
                 stream_of(hist))
    return out[:, 0], out[:, 1], out[:, 2].to(torch.int32), out[:, 3]


# --------------------------------------------------------------------------- K20
def ref_seasonal_trend_robust(hist, T: int, m: int, H: int, smooth: int = 5, min_blocks: int = 3):
    """Robust trend + per-phase profile model of ``hist[r, :T]`` with period
    ``m`` -> (forecast [R, H] f32, sigma [R] f32, n [R] int32, slope [R] f32,
    nblocks [R] int32, profile [R, m] f32): :func:`ref_trend_robust` and
    :func:`ref_seasonal_robust` composed, fp32 unless they say otherwise.

    The span is the last ``N = J * m`` columns (:func:`seasonal_cycles`, ``J
    >= 2``); a leading partial cycle is ignored.  ``slope`` and ``nblocks``
    are those of ``ref_trend_robust(span, N, L=m, min_blocks)``: the blocks
    are the cycles, so a cycle of any shape moves every block median alike.
    The line is anchored at the last sample: ``r_i = x_i - (slope * float(i -
    (N - 1)))``, the product rounded to fp32 and then the difference (no fused
    multiply-add).  ``(_, sigma, n, profile)`` are ``ref_seasonal_robust(r, N,
    m, H, smooth)``: the profile carries the level at the end of the history
    plus the cycle, and ``n`` counts the finite residuals (an overflowed one
    is missing).  ``forecast[:, h - 1] = profile[(h - 1) % m] + (slope *
    float(h))``, the product rounded, then the sum; a NaN profile phase gives
    a NaN forecast.  A row with ``slope == 0`` equals
    :func:`ref_seasonal_robust` of the span as floats."""
    x = np.asarray(hist, np.float32)[:, :T]
    T, m, H = int(T), int(m), int(H)
    J = seasonal_cycles(T, m)
    check(J >= 2, f"seasonal_trend_robust needs two whole cycles within its budget (T = {T}, m = {m}: J = {J})")
    N = J * m
    span = x[:, T - N:T]
    _, _, _, slope, nblocks = ref_trend_robust(span, N, m, min_blocks)
    with np.errstate(invalid="ignore", over="ignore"):
        t = (np.arange(N, dtype=np.int64) - (N - 1)).astype(np.float32)
        r = (span - (slope[:, None] * t[None, :]).astype(np.float32)).astype(np.float32)
        fc0, sigma, n, profile = ref_seasonal_robust(r, N, m, H, smooth)
        h = np.arange(1, H + 1, dtype=np.int64).astype(np.float32)
        forecast = (fc0 + (slope[:, None] * h[None, :]).astype(np.float32)).astype(np.float32)
    return forecast, sigma, n, slope, nblocks, profile


def seasonal_trend_robust(hist: torch.Tensor, T: int, m: int, H: int, smooth: int = 5, min_blocks: int = 3,
                          want_profile: bool = False):
    """K20: (forecast [R, H], sigma [R], n [R] int32, slope [R]) of
    :func:`ref_seasonal_trend_robust` over ``hist[:, :T]``, and the profile
    [R, m] behind them when ``want_profile``.  ``hist`` may be any column view
    with unit column stride: rows need 4-byte alignment only."""
    check(hist.dim() == 2 and hist.dtype == torch.float32 and 0 <= T <= hist.shape[1],
          "hist must be fp32 [R, >= T]")
    T, m, H, mb = int(T), int(m), int(H), int(min_blocks)
    J = seasonal_cycles(T, m)
    check(J >= 2, f"seasonal_trend_robust needs two whole cycles within its budget (T = {T}, m = {m}: J = {J})")
    check(H >= 0, "H must be >= 0")
    check(mb >= 2, "min_blocks must be >= 2")
    if not hist.is_cuda:
        ref = ref_seasonal_trend_robust(hist.numpy(), T, m, H, smooth, mb)
        fc, sg, n, sl, _, pr = (torch.from_numpy(a) for a in ref)
        return (fc, sg, n, sl, pr) if want_profile else (fc, sg, n, sl)
    require_native(hist)
    check(hist.stride(1) == 1 or hist.shape[1] <= 1, "rows must have unit column stride")
    R = hist.shape[0]
    fc = torch.empty((R, H), dtype=torch.float32, device=hist.device)
    stats = torch.empty((R, 4), dtype=torch.float32, device=hist.device)
    prof = torch.empty((R, m), dtype=torch.float32, device=hist.device) if want_profile else None
    if R:
        LIB.call("fm_seasonal_trend_robust", ptr(hist), hist.stride(0), T, R, m, J, seasonal_halfwidth(m, smooth), mb, H,
                 ptr(fc), max(H, 1), ptr(stats), ptr(prof), stream_of(hist))
    out = (fc, stats[:, 0], stats[:, 1].to(torch.int32), stats[:, 2])
    return out + (prof,) if want_profile else out


# --------------------------------------------------------------------------- K22
def scale_halfwidth(m: int, scale_smooth: int = 30) -> int:
    """Half width w of the window that smooths the per-phase scale:
    ``scale_smooth`` phases each side, but the window stays about a quarter of
    the period (``m // 8`` each side), so ``2 w + 1 <= m`` for every ``m``."""
    return max(0, min(int(scale_smooth), int(m) // 8))


def ref_seasonal_scale_robust(hist, T: int, m: int, H: int, smooth: int = 5, scale_smooth: int = 30,
                              floor: float = 0.1):
    """:func:`ref_seasonal_robust` with a sigma per phase -> (forecast [R, H]
    f32, sigma_h [R, H] f32, n [R] int32, sigma0 [R] f32, kappa [R] f32,
    profile [R, m] f32, scale [R, m] f32), fp32 unless it says otherwise.

    ``forecast``, ``sigma0`` (the one sigma of that model), ``n`` and
    ``profile`` are ``ref_seasonal_robust(hist, T, m, H, smooth)``'s, and so
    are the span and the phases.  With ``r_i = |x_i - profile[phase_i]|`` of
    the finite samples, ``raw_s[p]`` is K13's middle rule over the ``r`` of
    phase ``p`` (NaN when it has none) and ``g[p]`` the mean of the finite
    ``raw_s[(p + d) % m]``, ``d = -w..w`` (:func:`scale_halfwidth`), summed in
    that order and divided in fp64, rounded once.  The floor is ``f =
    fp32(floor) * (sigma0 / 1.4826)``, a share of the pooled MAD: ``g'[p] =
    max(g[p], f)``, and ``f`` where ``g[p]`` is NaN.  ``u_i = r_i /
    g'[phase_i]``; ``kappa = 1.4826 * middle(u)`` over the ``n`` finite
    samples, or ``1.2533 * mean(u)`` (fp64, rounded once) when that middle is
    0: the factor that turns the median of the ``J`` half-normal values of a
    phase into a sigma.  ``scale[p] = kappa * g'[p]`` and ``sigma_h[:, h - 1]
    = scale[(h - 1) % m]``, wrapped like the forecast.  A row with ``sigma0 ==
    0`` (a perfectly periodic span) has ``scale == 0`` and ``kappa`` NaN;
    ``n == 0`` gives NaN everywhere."""
    x = np.asarray(hist, np.float32)[:, :T]
    R = x.shape[0]
    T, m, H = int(T), int(m), int(H)
    check(float(floor) > 0, "floor must be > 0")
    forecast, sigma0, n, profile = ref_seasonal_robust(x, T, m, H, smooth)
    J = seasonal_cycles(T, m)
    w = scale_halfwidth(m, scale_smooth)
    span = x[:, T - J * m:T]
    fin = np.isfinite(span)
    nan = np.float32(np.nan)

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        r = np.abs(span - np.tile(profile, (1, J))).astype(np.float32)
        fin3 = fin.reshape(R, J, m)
        c = fin3.sum(1)
        raw = np.where(c > 0, _middle(r.reshape(R, J, m), fin3, c, 1), nan).astype(np.float32)
        g = _smooth_circular(raw, w)
        f = (np.float32(floor) * (sigma0 / np.float32(1.4826)).astype(np.float32)).astype(np.float32)
        gp = np.where(np.isfinite(g), np.maximum(g, f[:, None]), f[:, None]).astype(np.float32)
        u = (r / np.tile(gp, (1, J))).astype(np.float32)
        mid = _middle(u, fin, n)
        mean_u = (np.where(fin, u, 0).astype(np.float64).sum(1) / np.maximum(n, 1)).astype(np.float32)
        kappa = np.where(mid > 0, np.float32(1.4826) * mid, np.float32(1.2533) * mean_u).astype(np.float32)
        scale = (kappa[:, None] * gp).astype(np.float32)
    flat = sigma0 == 0
    kappa[flat | (n == 0)] = nan
    scale[flat] = 0
    scale[n == 0] = nan
    sigma_h = np.ascontiguousarray(scale[:, np.arange(H) % m])
    return forecast, sigma_h, n, sigma0, kappa, profile, scale


def seasonal_scale_robust(hist: torch.Tensor, T: int, m: int, H: int, smooth: int = 5, scale_smooth: int = 30,
                          floor: float = 0.1, want_profile: bool = False):
    """K22: (forecast [R, H], sigma_h [R, H], n [R] int32, sigma0 [R], kappa
    [R]) of :func:`ref_seasonal_scale_robust` over ``hist[:, :T]``, and the
    profile and the scale [R, m] behind them when ``want_profile``.  ``hist``
    may be any column view with unit column stride: rows need 4-byte alignment
    only."""
    check(hist.dim() == 2 and hist.dtype == torch.float32 and 0 <= T <= hist.shape[1],
          "hist must be fp32 [R, >= T]")
    T, m, H = int(T), int(m), int(H)
    J = seasonal_cycles(T, m)
    check(J >= 2, f"seasonal_scale_robust needs two whole cycles within its budget (T = {T}, m = {m}: J = {J})")
    check(H >= 0, "H must be >= 0")
    check(float(floor) > 0, "floor must be > 0")
    if not hist.is_cuda:
        out = tuple(torch.from_numpy(a) for a in ref_seasonal_scale_robust(hist.numpy(), T, m, H, smooth, scale_smooth,
                                                                          floor))
        return out if want_profile else out[:5]
    require_native(hist)
    check(hist.stride(1) == 1 or hist.shape[1] <= 1, "rows must have unit column stride")
    R = hist.shape[0]
    fc = torch.empty((R, H), dtype=torch.float32, device=hist.device)
    sh = torch.empty((R, H), dtype=torch.float32, device=hist.device)
    stats = torch.empty((R, 3), dtype=torch.float32, device=hist.device)
    prof = torch.empty((R, m), dtype=torch.float32, device=hist.device) if want_profile else None
    scale = torch.empty((R, m), dtype=torch.float32, device=hist.device) if want_profile else None
    if R:
        LIB.call("fm_seasonal_scale_robust", ptr(hist), hist.stride(0), T, R, m, J, seasonal_halfwidth(m, smooth),
                 scale_halfwidth(m, scale_smooth), float(floor), H, ptr(fc), ptr(sh), max(H, 1), ptr(stats), ptr(prof),
                 ptr(scale), stream_of(hist))
    out = (fc, sh, stats[:, 1].to(torch.int32), stats[:, 0], stats[:, 2])
    return out + (prof, scale) if want_profile else out


# --------------------------------------------------------------------------- K23
# Most candidates one launch scores (csrc/kernels/holdout_score.hip kHoldoutMaxCands).
HOLDOUT_MAX_CANDIDATES = 8
AUTO_ZCAP = 8.0
AUTO_MARGIN = 0.05


def ref_holdout_score(x, fc, sigma, zcap: float = AUTO_ZCAP):
    """Capped Laplace log score of ``C`` forecasts of the held-out samples
    ``x`` [R, L] -> (score [R, C] f32, n [R, C] int32, nx [R] int32).

    ``fc`` and ``sigma`` are lists of ``C`` arrays, each [R, L] or [R, 1] (one
    value along the row).  A point ``(r, c, t)`` counts when ``x``, ``fc`` and
    ``sigma`` are finite and ``sigma > 0``; it contributes ``l + z`` with ``z =
    min(fl32(|fl32(x - fc)| / sigma), zcap)`` and ``l = fl32(ln sigma)``, each
    operation in fp32 rounded once.  ``score[r, c]`` is the fp64 sum of
    ``(double) l + (double) z`` over the ``n[r, c]`` points that count, divided
    by their number in fp64 and rounded once to fp32; ``+inf`` without one.
    ``nx[r]`` is the number of finite ``x[r, :]``.  A narrow band scores low, a
    band the held-out points fall outside of scores high, and no point adds
    more than ``zcap``, so an incident inside the hold-out cannot decide."""
    x = np.asarray(x, np.float32)
    R, L = x.shape
    C = len(fc)
    check(len(sigma) == C, "one sigma per forecast")
    zc = np.float32(zcap)
    finx = np.isfinite(x)
    nx = finx.sum(1).astype(np.int32)
    score = np.full((R, C), np.inf, np.float32)
    n = np.zeros((R, C), np.int32)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for c in range(C):
            f = np.broadcast_to(np.asarray(fc[c], np.float32), (R, L))
            s = np.broadcast_to(np.asarray(sigma[c], np.float32), (R, L))
            ok = finx & np.isfinite(f) & np.isfinite(s) & (s > 0)
            d = np.abs((x - f).astype(np.float32))
            z = np.minimum((d / s).astype(np.float32), zc)
            l = np.log(np.where(ok, s, 1).astype(np.float64)).astype(np.float32)
            tot = np.where(ok, l.astype(np.float64) + z.astype(np.float64), 0.0).sum(1)
            cnt = ok.sum(1)
            n[:, c] = cnt
            score[:, c] = np.where(cnt > 0, tot / np.maximum(cnt, 1), np.inf).astype(np.float32)
    return score, n, nx


def ref_auto_pick(score, n, nx, margin: float = AUTO_MARGIN):
    """The candidate each row takes -> choice [R] int32.  Candidate ``c`` is
    eligible when it scored at least one point and at least half of the row's
    finite samples (``n >= 1`` and ``2 n >= nx``); ``best`` is the smallest
    eligible score, and the choice the first eligible candidate, in candidate
    order, with ``score <= fl32(best + margin)``: a later candidate must win
    by more than ``margin``.  0 when no candidate is eligible."""
    score = np.asarray(score, np.float32)
    n = np.asarray(n, np.int64)
    nx = np.asarray(nx, np.int64)
    elig = (n >= 1) & (2 * n >= nx[:, None])
    best = np.where(elig, score, np.float32(np.inf)).min(1).astype(np.float32)
    with np.errstate(invalid="ignore"):
        near = elig & (score <= (best + np.float32(margin)).astype(np.float32)[:, None])
    return np.where(near.any(1), near.argmax(1), 0).astype(np.int32)


def _holdout_operand(t: torch.Tensor, x: torch.Tensor, what: str) -> torch.Tensor:
    """A candidate's forecast or sigma as [R, L] or [R, 1] with column stride 0 or 1."""
    R, L = x.shape
    if t.dim() == 1:
        t = t[:, None]
    check(t.dim() == 2 and t.dtype == torch.float32 and t.device == x.device and t.shape[0] == R
          and t.shape[1] in (1, L), f"{what} must be fp32 [R, L], [R, 1] or [R] on the device of x")
    if t.shape[1] > 1 and t.stride(1) not in (0, 1):
        t = t.contiguous()
    return t


def holdout_score(x: torch.Tensor, fc, sigma, zcap: float = AUTO_ZCAP, margin: float = AUTO_MARGIN):
    """K23: (score [R, C], n [R, C] int32, nx [R] int32, choice [R] int32) of
    :func:`ref_holdout_score` and :func:`ref_auto_pick` for the held-out
    samples ``x`` [R, L] and ``C`` candidates.  ``x`` may be any column view
    with unit column stride (rows need 4-byte alignment only); ``fc[c]`` and
    ``sigma[c]`` are [R, L], [R, 1] or [R], at any row stride, and an expanded
    (column stride 0) tensor counts as one value per row."""
    check(x.dim() == 2 and x.dtype == torch.float32, "x must be fp32 [R, L]")
    R, L = x.shape
    C = len(fc)
    check(len(sigma) == C and 1 <= C <= HOLDOUT_MAX_CANDIDATES,
          f"between 1 and {HOLDOUT_MAX_CANDIDATES} candidates, one sigma per forecast")
    check(L <= ROBUST_LDS_KEYS, f"at most {ROBUST_LDS_KEYS} held-out samples")
    check(float(zcap) > 0 and float(margin) >= 0, "zcap must be > 0 and margin >= 0")
    fc = [_holdout_operand(t, x, "fc") for t in fc]
    sigma = [_holdout_operand(t, x, "sigma") for t in sigma]
    if not x.is_cuda:
        score, n, nx = ref_holdout_score(x.numpy(), [t.numpy() for t in fc], [t.numpy() for t in sigma], zcap)
        return (torch.from_numpy(score), torch.from_numpy(n), torch.from_numpy(nx),
                torch.from_numpy(ref_auto_pick(score, n, nx, margin)))
    require_native(x)
    check(x.stride(1) == 1 or L <= 1, "rows must have unit column stride")
    d = x.device
    score = torch.empty((R, C), dtype=torch.float32, device=d)
    n = torch.empty((R, C), dtype=torch.int32, device=d)
    nx = torch.empty((R,), dtype=torch.int32, device=d)
    choice = torch.empty((R,), dtype=torch.int32, device=d)
    if R:
        col = lambda t: int(t.shape[1] > 1 and t.stride(1) == 1)
        cands = np.array([[f.data_ptr(), f.stride(0), col(f), s.data_ptr(), s.stride(0), col(s)]
                          for f, s in zip(fc, sigma)], np.int64)
        LIB.call("fm_holdout_score", ptr(x), x.stride(0), L, R, cands.ctypes.data, C, float(zcap), float(margin),
                 ptr(score), ptr(n), ptr(nx), ptr(choice), stream_of(x))
    return score, n, nx, choice


# --------------------------------------------------------------------------- K24
QUANTILE_TAIL_Z = 2.0
QUANTILE_TAIL_Z_RANGE = (0.5, 3.0)


def quantile_tail_z(z0) -> float:
    """``QUANTILE_TAIL_Z`` within the range the model takes, [0.5, 3.0] (the
    default for a value that is no number)."""
    z = float(z0)
    if not np.isfinite(z):
        return QUANTILE_TAIL_Z
    return min(max(z, QUANTILE_TAIL_Z_RANGE[0]), QUANTILE_TAIL_Z_RANGE[1])


def quantile_tail_params(z0: float) -> tuple[float, np.float32]:
    """What K24 and its contract take of ``z0``: ``p = Phi(z0)`` in fp64 and
    ``float32(1 / z0)``."""
    import math
    z = float(z0)
    check(z > 0 and math.isfinite(z), "z0 must be a positive number")
    return 0.5 * (1.0 + math.erf(z / math.sqrt(2.0))), np.float32(1.0 / z)


def ref_quantile_robust_stats(hist, T: int, z0: float = QUANTILE_TAIL_Z):
    """Median and one sigma per side, from tail order statistics of the finite
    samples of ``hist[r, :T]`` -> (center [R] f32, sigma_lo [R] f32, sigma_up
    [R] f32, n [R] int32).  With ``s`` the sorted finite samples, ``p =
    Phi(z0)`` (fp64) and ``iz = float32(1 / z0)``: ``center = 0.5 s[(n-1)//2]
    + 0.5 s[n//2]`` (:func:`ref_robust_stats`' centre), ``k_up = ceil(p (n -
    1))`` in fp64, ``k_lo = (n - 1) - k_up``, ``d_up = s[k_up] - center``,
    ``d_lo = center - s[k_lo]`` in fp32, and ``sigma = d * iz`` on either side:
    the band at ``thr = z0`` ends on those two samples.  A side with ``d == 0``
    takes ``1.2533`` times the mean of ``x - center`` over the finite ``x >=
    center`` (of ``center - x`` over ``x <= center``), summed and divided in
    fp64 and rounded once, which is 0 only where no sample lies on that side.
    ``n == 0`` gives NaN for all three.  Single order statistics, nothing
    interpolated: the GPU kernel reproduces centre and ``d`` bit for bit."""
    p, iz = quantile_tail_params(z0)
    x = np.asarray(hist, np.float32)[:, :T]
    R = x.shape[0]
    fin = np.isfinite(x)
    n = fin.sum(1).astype(np.int32)
    center = np.full(R, np.nan, np.float32)
    sigma_lo = np.full(R, np.nan, np.float32)
    sigma_up = np.full(R, np.nan, np.float32)
    if x.shape[1] == 0 or not n.any():
        return center, sigma_lo, sigma_up, n
    n1 = (np.maximum(n, 1) - 1).astype(np.int64)
    k_up = np.minimum(np.ceil(p * n1.astype(np.float64)).astype(np.int64), n1)
    k_lo = n1 - k_up
    s = np.sort(np.where(fin, x, np.float32(np.inf)), axis=1)         # missing samples sort last
    at = lambda k: np.take_along_axis(s, k[:, None], 1)[:, 0]
    half, mean_dev = np.float32(0.5), np.float32(1.2533)
    with np.errstate(invalid="ignore", over="ignore"):
        c = half * at(n1 // 2) + half * at((n1 + 1) // 2)
        d_up = (at(k_up) - c).astype(np.float32)
        d_lo = (c - at(k_lo)).astype(np.float32)
        dev = x - c[:, None]                                            # fp32
        above, below = fin & (dev >= 0), fin & (dev <= 0)
        m_up = (np.where(above, dev, 0).astype(np.float64).sum(1) / np.maximum(above.sum(1), 1)).astype(np.float32)
        m_lo = (np.where(below, -dev, 0).astype(np.float64).sum(1) / np.maximum(below.sum(1), 1)).astype(np.float32)
        su = np.where(d_up > 0, d_up * iz, mean_dev * m_up).astype(np.float32)
        sl = np.where(d_lo > 0, d_lo * iz, mean_dev * m_lo).astype(np.float32)
    ok = n > 0
    center[ok], sigma_lo[ok], sigma_up[ok] = c[ok], sl[ok], su[ok]
    return center, sigma_lo, sigma_up, n


def quantile_robust_stats(hist: torch.Tensor, T: int, z0: float = QUANTILE_TAIL_Z):
    """K24: per-row (center, sigma_lo, sigma_up, n) of
    :func:`ref_quantile_robust_stats` over ``hist[:, :T]``, by exact selection
    of three ranks on the GPU.  ``hist`` may be any column view with unit
    column stride: rows need 4-byte alignment only."""
    check(hist.dim() == 2 and hist.dtype == torch.float32 and 0 <= T <= hist.shape[1],
          "hist must be fp32 [R, >= T]")
    p, iz = quantile_tail_params(z0)
    if not hist.is_cuda:
        return tuple(torch.from_numpy(a) for a in ref_quantile_robust_stats(hist.numpy(), T, z0))
    require_native(hist)
    check(hist.stride(1) == 1 or hist.shape[1] <= 1, "rows must have unit column stride")
    R = hist.shape[0]
    out = torch.empty((R, 4), dtype=torch.float32, device=hist.device)
    if R:
        LIB.call("fm_quantile_robust_stats", ptr(hist), hist.stride(0), int(T), R, p, float(iz), ptr(out),
                 stream_of(hist))
    return out[:, 0], out[:, 1], out[:, 2], out[:, 3].to(torch.int32)


# --------------------------------------------------------------------------- K26
def ref_seasonal_quantile_robust(hist, T: int, m: int, H: int, smooth: int = 5, scale_smooth: int = 30,
                                 floor: float = 0.1, z0: float = QUANTILE_TAIL_Z):
    """:func:`ref_seasonal_scale_robust`'s profile and per-phase scale with a
    sigma per side, from tail order statistics -> (forecast [R, H] f32,
    sigma_lo_h [R, H] f32, sigma_up_h [R, H] f32, n [R] int32, sigma0 [R] f32,
    kappa_lo [R] f32, kappa_up [R] f32, profile [R, m] f32, gscale [R, m] f32),
    fp32 unless it says otherwise.

    The span, the phases, ``forecast``, ``profile``, ``n`` and ``sigma0`` are
    ``ref_seasonal_robust(hist, T, m, H, smooth)``'s, and ``gscale`` is the
    floored, smoothed per-phase scale ``g'`` of
    :func:`ref_seasonal_scale_robust`, as itself.  With ``e_i = x_i -
    profile[phase_i]`` of the finite samples, signed, ``v_i = e_i /
    g'[phase_i]`` clamped to +-FLT_MAX (``|v_i|`` is that model's ``u_i``).
    ``p, iz =`` :func:`quantile_tail_params` ``(z0)``; ``k_up = min(ceil(p (n -
    1)), n - 1)`` in fp64, ``k_lo = (n - 1) - k_up``; with ``s`` the sorted
    ``v``, ``d_up = s[k_up]`` and ``d_lo = -s[k_lo]``: single order
    statistics, nothing interpolated and nothing re-centred, the profile is
    the centre.  ``kappa_up = d_up * iz`` where ``d_up > 0``, else ``1.2533``
    times the mean of ``v`` over ``v >= 0``, summed and divided in fp64 and
    rounded once (0 where there is none); ``kappa_lo`` mirrors it over ``v <=
    0``.  ``scale_up[p] = kappa_up * g'[p]``, ``sigma_up_h[:, h - 1] =
    scale_up[(h - 1) % m]``, and likewise below: the band at ``thr = z0`` ends
    on the history's own tail quantiles, phase by phase.  A row with ``sigma0
    == 0`` has both scales (and ``gscale``) 0 and both kappas NaN; ``n == 0``
    gives NaN everywhere.

    ``v`` is a number wherever ``e`` is finite and ``g'`` is not 0: that holds
    for every row whose finite ``|x|`` stay below 2^126 (about 8.5e37: then
    ``|e| < 2^127``) and whose floor ``fp32(floor) * (sigma0 / 1.4826)`` does
    not underflow to 0.  Beyond that ``inf / inf`` or ``0 / 0`` may make a NaN,
    and what the kernel does with it is not part of the contract."""
    p, iz = quantile_tail_params(z0)
    x = np.asarray(hist, np.float32)[:, :T]
    R = x.shape[0]
    T, m, H = int(T), int(m), int(H)
    forecast, _, n, sigma0, _, profile, _ = ref_seasonal_scale_robust(x, T, m, H, smooth, scale_smooth, floor)
    J = seasonal_cycles(T, m)
    w = scale_halfwidth(m, scale_smooth)
    span = x[:, T - J * m:T]
    fin = np.isfinite(span)
    nan, big = np.float32(np.nan), np.finfo(np.float32).max

    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        e = (span - np.tile(profile, (1, J))).astype(np.float32)
        fin3 = fin.reshape(R, J, m)
        c = fin3.sum(1)
        raw = np.where(c > 0, _middle(np.abs(e).reshape(R, J, m), fin3, c, 1), nan).astype(np.float32)
        g = _smooth_circular(raw, w)
        f = (np.float32(floor) * (sigma0 / np.float32(1.4826)).astype(np.float32)).astype(np.float32)
        gp = np.where(np.isfinite(g), np.maximum(g, f[:, None]), f[:, None]).astype(np.float32)
        v = np.clip((e / np.tile(gp, (1, J))).astype(np.float32), -big, big)
        n1 = (np.maximum(n, 1) - 1).astype(np.int64)
        k_up = np.minimum(np.ceil(p * n1.astype(np.float64)).astype(np.int64), n1)
        k_lo = n1 - k_up
        s = np.sort(np.where(fin, v, np.float32(np.inf)), axis=1)      # missing samples sort last
        at = lambda k: np.take_along_axis(s, k[:, None], 1)[:, 0]      # noqa: E731
        d_up, d_lo = at(k_up), -at(k_lo)
        above, below = fin & (v >= 0), fin & (v <= 0)
        m_up = (np.where(above, v, 0).astype(np.float64).sum(1) / np.maximum(above.sum(1), 1)).astype(np.float32)
        m_lo = (np.where(below, -v, 0).astype(np.float64).sum(1) / np.maximum(below.sum(1), 1)).astype(np.float32)
        kappa_up = np.where(d_up > 0, d_up * iz, np.float32(1.2533) * m_up).astype(np.float32)
        kappa_lo = np.where(d_lo > 0, d_lo * iz, np.float32(1.2533) * m_lo).astype(np.float32)
        scale_up = (kappa_up[:, None] * gp).astype(np.float32)
        scale_lo = (kappa_lo[:, None] * gp).astype(np.float32)
    flat, none = sigma0 == 0, n == 0
    kappa_lo[flat | none] = kappa_up[flat | none] = nan
    scale_lo[flat] = scale_up[flat] = gp[flat] = 0
    scale_lo[none] = scale_up[none] = gp[none] = nan
    wrap = np.arange(H) % m
    return (forecast, np.ascontiguousarray(scale_lo[:, wrap]), np.ascontiguousarray(scale_up[:, wrap]), n, sigma0,
            kappa_lo, kappa_up, profile, gp)


def seasonal_quantile_robust(hist: torch.Tensor, T: int, m: int, H: int, smooth: int = 5, scale_smooth: int = 30,
                             floor: float = 0.1, z0: float = QUANTILE_TAIL_Z, want_profile: bool = False):
    """K26: (forecast [R, H], sigma_lo_h [R, H], sigma_up_h [R, H], n [R]
    int32, sigma0 [R], kappa_lo [R], kappa_up [R]) of
    :func:`ref_seasonal_quantile_robust` over ``hist[:, :T]``, and the profile
    and the per-phase scale ``g'`` [R, m] behind them when ``want_profile``.
    ``hist`` may be any column view with unit column stride: rows need 4-byte
    alignment only."""
    check(hist.dim() == 2 and hist.dtype == torch.float32 and 0 <= T <= hist.shape[1],
          "hist must be fp32 [R, >= T]")
    T, m, H = int(T), int(m), int(H)
    J = seasonal_cycles(T, m)
    check(J >= 2, f"seasonal_quantile_robust needs two whole cycles within its budget (T = {T}, m = {m}: J = {J})")
    check(H >= 0, "H must be >= 0")
    check(float(floor) > 0, "floor must be > 0")
    p, iz = quantile_tail_params(z0)
    if not hist.is_cuda:
        out = tuple(torch.from_numpy(a) for a in ref_seasonal_quantile_robust(hist.numpy(), T, m, H, smooth,
                                                                             scale_smooth, floor, z0))
        return out if want_profile else out[:7]
    require_native(hist)
    check(hist.stride(1) == 1 or hist.shape[1] <= 1, "rows must have unit column stride")
    R = hist.shape[0]
    fc = torch.empty((R, H), dtype=torch.float32, device=hist.device)
    slo = torch.empty((R, H), dtype=torch.float32, device=hist.device)
    sup = torch.empty((R, H), dtype=torch.float32, device=hist.device)
    stats = torch.empty((R, 4), dtype=torch.float32, device=hist.device)
    prof = torch.empty((R, m), dtype=torch.float32, device=hist.device) if want_profile else None
    gscale = torch.empty((R, m), dtype=torch.float32, device=hist.device) if want_profile else None
    if R:
        LIB.call("fm_seasonal_quantile_robust", ptr(hist), hist.stride(0), T, R, m, J, seasonal_halfwidth(m, smooth),
                 scale_halfwidth(m, scale_smooth), float(floor), p, float(iz), H, ptr(fc), ptr(slo), ptr(sup),
                 max(H, 1), ptr(stats), ptr(prof), ptr(gscale), stream_of(hist))
    out = (fc, slo, sup, stats[:, 1].to(torch.int32), stats[:, 0], stats[:, 2], stats[:, 3])
    return out + (prof, gscale) if want_profile else out


# --------------------------------------------------------------------------- K25
# The static band models: a band that is constant over the current window, made
# of four numbers per history row (centre, sigma_lo, sigma_up, n), computed from
# the whole history and valid until the row is written again.
BAND_CODES = {"moving_average_all": 0, "robust_moving_average_all": 1, "quantile_robust": 2}
BAND_MAX_METRICS = 16
# longest view whose code-0 rows the register-resident K1 takes (fm_row_stats.h row_stats_dispatch_nv)
BAND_MEAN_MAX_T = 16 * 256 * 4
BAND_TAG_SHIFT = 28


def band_tag(code: int, T: int) -> int:
    """The validity word of a band record: ``((code + 1) << 28) | T``."""
    return ((int(code) + 1) << BAND_TAG_SHIFT) | int(T)


def ref_hist_stats(hist, T: int):
    """K1's contract, the statistics of ``ops.reference.stats_decide``: mean
    and population std of the finite samples of ``hist[r, :T]`` in fp64,
    rounded once -> (mean [R] f32, std [R] f32, n [R] int32); 0, 0 for a row
    without a finite sample, NaN, NaN when ``T == 0``."""
    x = np.asarray(hist, np.float32)[:, :T].astype(np.float64)
    fin = np.isfinite(x)
    n = fin.sum(1)
    if x.shape[1] == 0:
        nan = np.full(x.shape[0], np.nan, np.float32)
        return nan, nan.copy(), n.astype(np.int32)
    h = np.where(fin, x, 0.0)
    mean = np.where(n > 0, h.sum(1) / np.maximum(n, 1), 0.0)
    var = np.where(n > 0, (np.where(fin, x - mean[:, None], 0.0) ** 2).sum(1) / np.maximum(n, 1), 0.0)
    return mean.astype(np.float32), np.sqrt(var).astype(np.float32), n.astype(np.int32)


def _band_codes(codes) -> np.ndarray:
    c = np.asarray(codes.cpu() if isinstance(codes, torch.Tensor) else codes).astype(np.int64).reshape(-1)
    check(1 <= c.size <= BAND_MAX_METRICS, f"between 1 and {BAND_MAX_METRICS} model codes, one per metric")
    check(bool(((c >= 0) & (c <= 2)).all()), "model codes are 0, 1 or 2 (BAND_CODES)")
    return c


def ref_band_stats(hist, T: int, codes, z0: float = QUANTILE_TAIL_Z):
    """Band records of the static band models: row ``r`` of ``hist`` under the
    model ``codes[r % M]`` (``BAND_CODES``) -> (records [R, 4] f32 = centre,
    sigma_lo, sigma_up, n; n [R] int32).  Code 0 is :func:`ref_hist_stats`,
    code 1 :func:`ref_robust_stats` (either with its one sigma on both sides),
    code 2 :func:`ref_quantile_robust_stats` at ``z0``."""
    c = _band_codes(codes)
    x = np.asarray(hist, np.float32)
    R = x.shape[0]
    rec = np.zeros((R, 4), np.float32)
    n = np.zeros(R, np.int32)
    code = c[np.arange(R) % c.size]
    for k in (0, 1, 2):
        rows = np.flatnonzero(code == k)
        if not len(rows):
            continue
        if k == 2:
            ce, sl, su, nn = ref_quantile_robust_stats(x[rows], T, z0)
        else:
            ce, sl, nn = (ref_hist_stats if k == 0 else ref_robust_stats)(x[rows], T)
            su = sl
        rec[rows, 0], rec[rows, 1], rec[rows, 2], rec[rows, 3] = ce, sl, su, nn
        n[rows] = nn
    return rec, n


def band_stats_cached(hist: torch.Tensor, T: int, rowmap: torch.Tensor | None, codes, cache,
                      z0: float = QUANTILE_TAIL_Z, expect_miss: bool | None = None, blocks: int = 0,
                      out: torch.Tensor | None = None, codes_dev: torch.Tensor | None = None) -> torch.Tensor:
    """K25: the band records ``[R, 4]`` (centre, sigma_lo, sigma_up, n) of the
    rows ``hist[rowmap[r], :T]`` (identity without a row map), row ``r`` under
    the model ``codes[r % M]`` (``BAND_CODES``; a sequence or a host tensor),
    bit for bit what K1, K13 and K24 give for the row.  The record of every
    physical row is kept in ``cache`` (an ``engine.resident.RowStatsCache`` of
    width 4 over the rows of ``hist``, or None): an entry whose tag names this
    model and ``T`` is copied, any other is computed and recorded.  Within one
    call a physical row is mapped under one code only.  ``expect_miss`` only
    shapes the launch (None: the cache's own estimate), as ``blocks`` does (0:
    the kernel's own grid).  Whoever writes a row of ``hist`` calls
    ``cache.touch`` on the same stream, and ``cache.rekey(z0)`` precedes a call
    with another ``z0`` (done here).  ``codes_dev``: the codes as int32 on the
    device, when the caller keeps them.  CPU: :func:`ref_band_stats` over the
    mapped rows; the cache is ignored."""
    check(hist.dim() == 2 and hist.dtype == torch.float32 and 0 <= T <= hist.shape[1],
          "hist must be fp32 [P, >= T]")
    c = _band_codes(codes)
    M = int(c.size)
    if rowmap is not None:
        check(rowmap.dim() == 1 and rowmap.dtype == torch.int32 and rowmap.device == hist.device,
              "rowmap must be int32 [R] on the device of hist")
        if rowmap.numel():
            check(0 <= int(rowmap.min()) and int(rowmap.max()) < hist.shape[0], "rowmap points outside hist")
    R = hist.shape[0] if rowmap is None else rowmap.numel()
    z0 = float(z0)
    if not hist.is_cuda:
        x = hist.numpy() if rowmap is None else hist.numpy()[rowmap.numpy().astype(np.int64)]
        return torch.from_numpy(ref_band_stats(x, T, c, z0)[0])
    require_native(hist)
    check(hist.stride(1) == 1 or hist.shape[1] <= 1, "rows must have unit column stride")
    check(T < (1 << BAND_TAG_SHIFT), "view length beyond the tag's 28 bits")
    if cache is not None:
        check(len(cache) >= hist.shape[0] and cache.valid.device == hist.device and cache.stats.shape[1] == 4,
              "the cache must hold 4 floats for every row of hist, on its device")
        cache.rekey(z0)
    if out is None:
        out = torch.empty((R, 4), dtype=torch.float32, device=hist.device)
    if R:
        p, iz = quantile_tail_params(z0)
        if codes_dev is None:
            codes_dev = torch.from_numpy(c.astype(np.int32)).to(hist.device)
        mask = int(np.bitwise_or.reduce(1 << c))
        miss = (cache is None or cache.expect_miss(int(T), R)) if expect_miss is None else bool(expect_miss)
        LIB.call("fm_band_stats_cached", ptr(hist), hist.stride(0), int(T), R, M, ptr(codes_dev), mask, p, float(iz),
                 ptr(out), ptr(rowmap), ptr(cache.stats) if cache is not None else None,
                 ptr(cache.valid) if cache is not None else None, int(miss), int(blocks), stream_of(hist))
        if cache is not None:
            cache.ticked(int(T))
    return out


# --------------------------------------------------------------------------- K8
SLA_HINTS = ("latency", "error", "5xx", "4xx", "sla")
REASONS = {0: "hpa is holding", 1: "hpa is scaling up", 2: "hpa is scaling down",
           3: "hpa is holding (breath duration)", 4: "hpa is holding (flip limit)"}


@dataclass
class HpaTemplate:
    """Template metrics in priority order (DeploymentMetadata.spec.hpaScoreTemplates,
    types.go:63-67; priorities/isIncrease/isAbsolute from models.go:179-183)."""

    aliases: list[str]
    priority: list[int]
    is_increase: list[bool]
    is_absolute: list[bool]

    @classmethod
    def from_aliases(cls, aliases: list[str], hpa_metrics: dict | None = None) -> "HpaTemplate":
        pr, inc, ab = [], [], []
        for i, a in enumerate(aliases):
            cfg = (hpa_metrics or {}).get(a, {})
            pr.append(int(cfg.get("priority", i + 1)))
            inc.append(bool(cfg.get("isIncrease", True)))
            ab.append(bool(cfg.get("isAbsolute", False)))
        return cls(list(aliases), pr, inc, ab)

    def roles(self) -> np.ndarray:
        return np.array([1 if any(h in a.lower() for h in SLA_HINTS) else 0 for a in self.aliases], np.int8)

    def weights(self) -> np.ndarray:
        p = np.asarray(self.priority, np.float32)
        return (p.min() / p).astype(np.float32)


@dataclass
class HpaState:
    last_dir: torch.Tensor    # [S] int8
    last_time: torch.Tensor   # [S] float64
    flips: torch.Tensor       # [S] int32
    flip_t0: torch.Tensor     # [S] float64

    @classmethod
    def zeros(cls, S: int, device="cpu") -> "HpaState":
        return cls(torch.zeros(S, dtype=torch.int8, device=device), torch.full((S,), -1e18, dtype=torch.float64,
                                                                             device=device),
                   torch.zeros(S, dtype=torch.int32, device=device), torch.zeros(S, dtype=torch.float64,
                                                                               device=device))


def hpa_score(cur, upper, lower, tmpl: HpaTemplate, state: HpaState, now: float, breath_up: float = 60.0,
              breath_down: float = 300.0, max_flips: int = 4, flip_window: float = 1800.0):
    """Returns (score [S] int32, reason [S] int8, raw [S] f32); updates ``state`` in place."""
    S, Mt = cur.shape
    check(Mt == len(tmpl.aliases), "template/metric count mismatch")
    w, inc, ab, role = tmpl.weights(), np.asarray(tmpl.is_increase, np.int8), np.asarray(tmpl.is_absolute, np.int8), \
        tmpl.roles()
    if not cur.is_cuda:
        sc, rs, raw = ref_hpa_score(cur.numpy(), upper.numpy(), lower.numpy(), w, inc, ab, role, state, now,
                                    breath_up, breath_down, max_flips, flip_window)
        return torch.from_numpy(sc), torch.from_numpy(rs), torch.from_numpy(raw)
    require_native(cur)
    d = cur.device
    t = lambda a: torch.from_numpy(a).to(d)
    wt, it, at, rt = t(w), t(inc), t(ab), t(role)
    sc = torch.empty((S,), dtype=torch.int32, device=d)
    rs = torch.empty((S,), dtype=torch.int8, device=d)
    raw = torch.empty((S,), dtype=torch.float32, device=d)
    LIB.call("fm_hpa_score", ptr(cur), ptr(upper), ptr(lower), S, Mt, ptr(wt), ptr(it), ptr(at), ptr(rt), float(now),
             float(breath_up), float(breath_down), int(max_flips), float(flip_window), ptr(state.last_dir),
             ptr(state.last_time), ptr(state.flips), ptr(state.flip_t0), ptr(sc), ptr(rs), ptr(raw), stream_of(cur))
    return sc, rs, raw


def ref_hpa_score(cur, upper, lower, w, inc, ab, role, state: HpaState, now, breath_up, breath_down, max_flips,
                  flip_window):
    cur = np.asarray(cur, np.float32)
    ok = np.isfinite(cur) & np.isfinite(upper) & np.isfinite(lower)
    scale = np.where(ab[None, :] != 0, np.maximum(np.abs(upper), np.float32(1e-12)),
                     np.maximum(upper - lower, np.float32(1e-12)))
    dev = np.where(cur > upper, (cur - upper) / scale, np.where(cur < lower, (cur - lower) / scale, 0)).astype(
        np.float32)
    dev = np.where(inc[None, :] != 0, dev, -dev)
    dev = np.where(ok, dev, 0)
    is_sla = (role == 1)[None, :]
    has_sla = np.broadcast_to(is_sla.any(), (cur.shape[0],))
    sla_v = ((dev > 0) & is_sla & ok).any(1)
    up = np.where(~is_sla & (dev > 0), w[None, :] * dev, 0).max(1, initial=0)
    down = np.where(~is_sla & (dev < 0), -w[None, :] * dev, 0).max(1, initial=0)
    sla_v = np.where(has_sla, sla_v, up > 0)
    raw = np.full(cur.shape[0], 50, np.int32)
    upm = (up > 0) & sla_v
    dnm = ~upm & (down > 0) & (up == 0) & ~sla_v
    raw[upm] = 50 + np.rint(50 * np.minimum(1, up[upm])).astype(np.int32)
    raw[dnm] = 50 - np.rint(50 * np.minimum(1, down[dnm])).astype(np.int32)
    ld = state.last_dir.numpy()
    lt = state.last_time.numpy()
    fl = state.flips.numpy()
    f0 = state.flip_t0.numpy()
    reset = now - f0 > flip_window
    fl[reset] = 0
    f0[reset] = now
    score = raw.copy()
    reason = np.where(raw > 50, 1, np.where(raw < 50, 2, 0)).astype(np.int8)
    for s in np.nonzero(raw != 50)[0]:
        dr = 1 if raw[s] > 50 else -1
        wait = breath_up if dr > 0 else breath_down
        if ld[s] != 0 and now - lt[s] < wait:
            score[s] = 50
            reason[s] = 3
        elif ld[s] != 0 and dr != ld[s] and fl[s] >= max_flips:
            score[s] = 50
            reason[s] = 4
        else:
            if ld[s] != 0 and dr != ld[s]:
                fl[s] += 1
            ld[s] = dr
            lt[s] = now
    return score, reason, raw.astype(np.float32)


# --------------------------------------------------------------------------- K9
@dataclass
class CallGraph:
    """caller -> callee CSR adjacency over global service ids."""

    rowptr: np.ndarray   # [S+1] int64
    col: np.ndarray      # [E] int32
    weight: np.ndarray   # [E] float32

    @classmethod
    def from_edges(cls, S: int, src, dst, weight=None) -> "CallGraph":
        src = np.asarray(src, np.int64)
        dst = np.asarray(dst, np.int32)
        w = np.ones(len(src), np.float32) if weight is None else np.asarray(weight, np.float32)
        order = np.argsort(src, kind="stable")
        src, dst, w = src[order], dst[order], w[order]
        rowptr = np.zeros(S + 1, np.int64)
        np.add.at(rowptr, src + 1, 1)
        return cls(np.cumsum(rowptr), dst, w)


def downstream_impact(g: CallGraph, score: torch.Tensor, hops: int = 2) -> torch.Tensor:
    """impact[u] = max over callee paths of length <= hops of (weight product) x score."""
    S = score.numel()
    if not score.is_cuda:
        return torch.from_numpy(ref_downstream_impact(g, score.numpy(), hops))
    require_native(score)
    d = score.device
    # the CSR and the ping-pong buffers are uploaded/allocated once per device
    # (the tick replays with no host->device traffic and can be graph-captured)
    cache = g.__dict__.setdefault("_dev", {})
    if d not in cache:
        cache[d] = (torch.from_numpy(g.rowptr).to(d), torch.from_numpy(g.col).to(d),
                    torch.from_numpy(g.weight).to(d), torch.empty((S,), dtype=torch.float32, device=d),
                    torch.empty((S,), dtype=torch.float32, device=d))
    rp, col, w, b0, b1 = cache[d]
    LIB.call("fm_downstream_impact", ptr(rp), ptr(col), ptr(w), ptr(score), S, hops, ptr(b0), ptr(b1),
             stream_of(score))
    return b0 if (hops - 1) % 2 == 0 else b1


def ref_downstream_impact(g: CallGraph, a: np.ndarray, hops: int) -> np.ndarray:
    S = a.size
    prev = np.zeros(S, np.float32)
    src = np.repeat(np.arange(S), np.diff(g.rowptr))
    for h in range(hops):
        # fmax: a NaN score is no evidence and counts as 0, as in the kernel
        val = np.fmax(a[g.col], prev[g.col] if h > 0 else 0) * g.weight
        out = np.zeros(S, np.float32)
        np.maximum.at(out, src, val.astype(np.float32))
        prev = out
    return prev


def segment_max(v: torch.Tensor, seg: torch.Tensor, K: int) -> torch.Tensor:
    """out[k] = max(0, max of v[i] with seg[i] == k) for non-negative scores
    (per-cluster aggregate of the impact step).  A NaN value is no evidence
    and an id outside [0, K) belongs to no segment: both are ignored."""
    check(v.dtype == torch.float32 and seg.dtype == torch.int64 and v.numel() == seg.numel(), "bad segment_max args")
    if not v.is_cuda:
        out = torch.zeros((K,), dtype=torch.float32)
        ok = (seg >= 0) & (seg < K) & ~torch.isnan(v)
        return out.scatter_reduce(0, seg[ok], v[ok].clamp(min=0), reduce="amax", include_self=True)
    require_native(v)
    out = torch.empty((K,), dtype=torch.float32, device=v.device)
    LIB.call("fm_segment_max", ptr(v.contiguous()), ptr(seg.contiguous()), v.numel(), K, ptr(out), stream_of(v))
    return out


# ---------------------------------------------------------------------------
# K1 rolling bands (csrc/kernels/rolling.hip)
# ---------------------------------------------------------------------------
ROLLING_MAX_WINDOW = 2048


def rolling_stats(x: torch.Tensor, T: int, w: int, min_count: int = 1) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-time-point mean and population std of the finite samples in the
    trailing window [t - w + 1, t] of every row of ``x[:, :T]`` (NaN where
    the window holds fewer than ``min_count`` finite samples).  Returns
    (mean [R, T], std [R, T]) fp32."""
    check(1 <= w <= ROLLING_MAX_WINDOW, f"rolling window must be in [1, {ROLLING_MAX_WINDOW}]")
    check(0 < T <= x.shape[1], "T must be within the row length")
    if not x.is_cuda:
        m, s = ref_rolling_stats(x.numpy()[:, :T], w, min_count)
        return torch.from_numpy(m), torch.from_numpy(s)
    require_native(x)
    check(x.dtype == torch.float32 and x.stride(1) == 1 and x.stride(0) % 4 == 0 and x.data_ptr() % 16 == 0,
          "rows must be fp32, contiguous and 16-B aligned")
    R = x.shape[0]
    mean = torch.empty((R, T), dtype=torch.float32, device=x.device)
    sd = torch.empty((R, T), dtype=torch.float32, device=x.device)
    LIB.call("fm_rolling_stats", ptr(x), x.stride(0), T, R, w, int(min_count), ptr(mean), ptr(sd), T, stream_of(x))
    return mean, sd


def ref_rolling_stats(x: np.ndarray, w: int, min_count: int = 1) -> tuple[np.ndarray, np.ndarray]:
    """fp64 oracle: windowed sums from prefix sums of the finite-sample mask,
    the values and their squares about the row mean."""
    x = np.asarray(x, dtype=np.float64)
    f = np.isfinite(x)
    cnt_all = f.sum(1, keepdims=True)
    c = np.where(cnt_all > 0, np.where(f, x, 0.0).sum(1, keepdims=True) / np.maximum(cnt_all, 1), 0.0)
    d = np.where(f, x - c, 0.0)

    def win(a):
        p = np.cumsum(a, axis=1)
        out = p.copy()
        out[:, w:] -= p[:, :-w]
        return out
    n, s, q = win(f.astype(np.float64)), win(d), win(d * d)
    with np.errstate(invalid="ignore", divide="ignore"):
        m = s / n
        var = np.maximum(q / n - m * m, 0.0)
    ok = (n >= min_count) & (n > 0)
    return (np.where(ok, c + m, np.nan).astype(np.float32), np.where(ok, np.sqrt(var), np.nan).astype(np.float32))


# ---------------------------------------------------------------------------
# resident-history row gather (csrc/kernels/gather.hip)
def gather_cols(src: torch.Tensor, rm: torch.Tensor | None, off: torch.Tensor, lim: torch.Tensor, ncols: int,
                out: torch.Tensor) -> torch.Tensor:
    """``out[r, j] = src[rm[r], off[r] + j]`` when ``0 <= off[r] + j <
    lim[r]``, NaN otherwise, for ``j < ncols`` (``out`` may be a column view
    of a wider buffer).  ``rm``/``off``/``lim`` are int32 [R]."""
    R = off.numel()
    check(src.dim() == 2 and src.stride(1) == 1 and out.stride(1) == 1, "row-major float32 operands")
    check(out.shape[0] >= R and out.shape[1] >= ncols, "output too small")
    if R == 0 or ncols <= 0:
        return out
    if not src.is_cuda:
        return ref_gather_cols(src, rm, off, lim, ncols, out)
    require_native(src)
    check(int(lim.max().item()) <= src.shape[1] if R else True, "limit past the source rows")
    check(rm is None or (int(rm.max().item()) < src.shape[0] and int(rm.min().item()) >= 0), "row map out of range")
    LIB.call("fm_gather_cols", ptr(src), src.stride(0), ptr(rm), ptr(off), ptr(lim), R, int(ncols), ptr(out),
             out.stride(0), stream_of(src))
    return out


def ref_gather_cols(src, rm, off, lim, ncols, out):
    rows = src if rm is None else src.index_select(0, rm.long())
    c = off.long()[:, None] + torch.arange(ncols)[None, :]
    ok = (c >= 0) & (c < lim.long()[:, None])
    vals = torch.gather(rows, 1, c.clamp(0, max(0, src.shape[1] - 1)))
    out[:len(off), :ncols] = torch.where(ok, vals, torch.full_like(vals, float("nan")))
    return out
