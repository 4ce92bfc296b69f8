"""Vectorised numpy reference implementations (CPU path + numerics oracles).

These implement exactly the semantics documented in docs/BRAIN_SPEC.md and
are what the HIP kernels are tested against (together with scipy for the
statistical tests).  Everything is batched over rows: a row is one
(service, metric) series.
"""
from __future__ import annotations

import numpy as np
from scipy import special

# ---------------------------------------------------------------------------
# rank helpers


def avg_ranks(x: np.ndarray):
    """Average 1-based ranks along axis 1 of a 2-D array where missing entries
    are +inf.  Returns (ranks, n_valid, tie_term) with tie_term = sum(t^3 - t)
    over tie runs of valid entries, plus the sort order and end-of-run mask in
    sorted order (used for the KS statistic)."""
    R, n = x.shape
    order = np.argsort(x, axis=1, kind="stable")
    xs = np.take_along_axis(x, order, axis=1)
    nvalid = np.isfinite(x).sum(axis=1)
    idx = np.broadcast_to(np.arange(n), (R, n))
    is_start = np.ones((R, n), dtype=bool)
    if n > 1:
        is_start[:, 1:] = xs[:, 1:] != xs[:, :-1]
    is_end = np.ones((R, n), dtype=bool)
    if n > 1:
        is_end[:, :-1] = is_start[:, 1:]
    valid_pos = idx < nvalid[:, None]
    is_end = is_end & valid_pos
    is_end[np.arange(R), np.maximum(nvalid - 1, 0)] |= nvalid > 0
    start = np.maximum.accumulate(np.where(is_start, idx, 0), axis=1)
    end_src = np.where(is_end | ~valid_pos, idx, n)
    # positions >= nvalid end themselves; reverse min-scan
    end = np.minimum.accumulate(end_src[:, ::-1], axis=1)[:, ::-1]
    rs = 0.5 * (start + end) + 1.0
    ranks = np.empty_like(rs)
    np.put_along_axis(ranks, order, rs, axis=1)
    t = (end - start + 1).astype(np.float64)
    tie = np.where(is_start & valid_pos, t ** 3 - t, 0.0).sum(axis=1)
    return ranks, nvalid, tie, order, is_end


def _norm_sf(z):
    return 0.5 * special.erfc(z / np.sqrt(2.0))


def kolmogorov_sf(lam):
    return special.kolmogorov(lam)


TEST_NAMES = ("MANN_WHITE", "WILCOXON", "KRUSKAL", "KS", "TTEST", "FRIEDMAN")


def special_rank2(cb):
    """Within-block average ranks of a [R, b, 2] array (1/2, or 1.5/1.5 on a tie)."""
    lt = (cb[..., 0] < cb[..., 1]).astype(np.float64)
    eq = (cb[..., 0] == cb[..., 1]).astype(np.float64)
    r0 = np.where(eq > 0, 1.5, np.where(lt > 0, 1.0, 2.0))
    return np.stack([r0, 3.0 - r0], axis=-1)


def pairwise_tests(cur, base, mask, combine_any, p_thr, min_mw, min_wil, min_kru):
    cur = np.asarray(cur, dtype=np.float64)
    base = np.asarray(base, dtype=np.float64)
    R = cur.shape[0]
    c = np.where(np.isfinite(cur), cur, np.inf)
    b = np.where(np.isfinite(base), base, np.inf)
    pooled = np.concatenate([c, b], axis=1)
    tags = np.concatenate([np.zeros_like(c, dtype=np.int8), np.ones_like(b, dtype=np.int8)], axis=1)
    tags = np.where(np.isfinite(pooled), tags, -1)
    n1 = (tags == 0).sum(1).astype(np.float64)
    n2 = (tags == 1).sum(1).astype(np.float64)
    n = n1 + n2
    ranks, _, tie, order, is_end = avg_ranks(pooled)
    r1 = np.where(tags == 0, ranks, 0.0).sum(1)
    P = np.full((R, 6), np.nan)
    S = np.full((R, 6), np.nan)
    with np.errstate(divide="ignore", invalid="ignore"):
        # Mann-Whitney
        u1 = r1 - n1 * (n1 + 1) / 2
        u2 = n1 * n2 - u1
        u = np.maximum(u1, u2)
        var = n1 * n2 / 12.0 * ((n + 1) - tie / (n * (n - 1)))
        z = (u - n1 * n2 / 2 - 0.5) / np.sqrt(var)
        pmw = np.where(var > 0, np.minimum(2 * _norm_sf(z), 1.0), 1.0)
        g = (n1 >= min_mw) & (n2 >= min_mw) & (n1 > 0) & (n2 > 0)
        P[:, 0] = np.where(g, pmw, np.nan)
        S[:, 0] = np.where(g, u1, np.nan)
        # Kruskal (2 groups)
        r2 = n * (n + 1) / 2 - r1
        h = 12.0 / (n * (n + 1)) * (r1 ** 2 / n1 + r2 ** 2 / n2) - 3 * (n + 1)
        corr = 1 - tie / (n ** 3 - n)
        hk = h / corr
        g = (n1 >= min_kru) & (n2 >= min_kru) & (n1 > 0) & (n2 > 0) & (corr > 0)
        P[:, 2] = np.where(g, special.chdtrc(1.0, hk), np.nan)
        S[:, 2] = np.where(g, hk, np.nan)
        # KS on sorted tags
        ts = np.take_along_axis(tags, order, axis=1)
        c1 = np.cumsum(ts == 0, axis=1)
        c2 = np.cumsum(ts == 1, axis=1)
        dd = np.abs(c1 / n1[:, None] - c2 / n2[:, None])
        D = np.where(is_end, dd, 0.0).max(axis=1)
        g = (n1 >= min_mw) & (n2 >= min_mw) & (n1 > 0) & (n2 > 0)
        en = n1 * n2 / (n1 + n2)
        P[:, 3] = np.where(g, kolmogorov_sf(np.sqrt(en) * D), np.nan)
        S[:, 3] = np.where(g, D, np.nan)
        # Welch t
        cm = np.where(np.isfinite(c), c, np.nan)
        bm = np.where(np.isfinite(b), b, np.nan)
        m1 = np.nanmean(cm, axis=1) if cm.shape[1] else np.full(R, np.nan)
        m2 = np.nanmean(bm, axis=1) if bm.shape[1] else np.full(R, np.nan)
        v1 = np.nansum((cm - m1[:, None]) ** 2, axis=1) / (n1 - 1)
        v2 = np.nansum((bm - m2[:, None]) ** 2, axis=1) / (n2 - 1)
        se2 = v1 / n1 + v2 / n2
        t = (m1 - m2) / np.sqrt(se2)
        dof = se2 ** 2 / ((v1 / n1) ** 2 / (n1 - 1) + (v2 / n2) ** 2 / (n2 - 1))
        pt = special.betainc(0.5 * dof, 0.5, dof / (dof + t * t))
        g = (n1 >= 2) & (n2 >= 2) & (n1 >= min_kru) & (n2 >= min_kru) & (se2 > 0)
        P[:, 4] = np.where(g, pt, np.nan)
        S[:, 4] = np.where(g, t, np.nan)
        # Wilcoxon signed rank on paired differences
        npair = min(cur.shape[1], base.shape[1])
        # differences are formed in fp32 exactly as on device (tie structure
        # of |d| depends on that rounding), then ranked in fp64
        d = (cur[:, :npair].astype(np.float32) - base[:, :npair].astype(np.float32)).astype(np.float64)
        okd = np.isfinite(d) & (d != 0)
        ad = np.where(okd, np.abs(d), np.inf)
        if npair > 0:
            rw, nw, tiew, _, _ = avg_ranks(ad)
            rplus = np.where(okd & (d > 0), rw, 0.0).sum(1)
        else:
            nw = np.zeros(R)
            tiew = np.zeros(R)
            rplus = np.zeros(R)
        nw = nw.astype(np.float64)
        tot = nw * (nw + 1) / 2
        T = np.minimum(rplus, tot - rplus)
        mn = nw * (nw + 1) / 4
        se = np.sqrt(nw * (nw + 1) * (2 * nw + 1) / 24 - tiew / 48)
        pw = np.where(se > 0, np.minimum(2 * _norm_sf(np.abs((T - mn) / se)), 1.0), np.nan)
        g = (nw >= min_wil) & (nw > 0)
        P[:, 1] = np.where(g, pw, np.nan)
        S[:, 1] = np.where(g, T, np.nan)
        # Friedman chi-square, k = 2 treatments over the paired blocks, in
        # its general form (per-block ranks, sum of rank sums, tie correction)
        if npair > 0:
            cb = np.stack([cur[:, :npair].astype(np.float32), base[:, :npair].astype(np.float32)], axis=2)
            okb = np.isfinite(cb).all(axis=2)
            rk = special_rank2(cb)
            b = okb.sum(1).astype(np.float64)
            Rj = np.where(okb[:, :, None], rk, 0.0).sum(1)                 # [R, 2]
            k = 2.0
            q = 12.0 / (b * k * (k + 1)) * (Rj ** 2).sum(1) - 3.0 * b * (k + 1)
            ties = np.where(okb & (cb[:, :, 0] == cb[:, :, 1]), 6.0, 0.0).sum(1)
            c = 1.0 - ties / (b * (k ** 3 - k))
            qf = np.where(c > 0, q / c, 0.0)
            pf = np.where(qf > 0, special.chdtrc(1.0, qf), 1.0)
            g = (b >= min_wil) & (b > 0)
            P[:, 5] = np.where(g, pf, np.nan)
            S[:, 5] = np.where(g, qf, np.nan)
    sel = np.array([(mask >> i) & 1 for i in range(6)], dtype=bool)
    app = ~np.isnan(P[:, sel])
    sig = app & (np.nan_to_num(P[:, sel], nan=1.0) < p_thr)
    na = app.sum(1)
    ns = sig.sum(1)
    diff = np.where(na > 0, (ns > 0) if combine_any else (ns == na), False).astype(np.int8)
    return P.astype(np.float32), S.astype(np.float32), diff


SUFF_NAMES = ("n1", "n2", "nw", "r1", "tie", "D", "rplus", "tiew", "m1", "m2", "q1", "q2", "npos", "nzero")


def pairwise_suff(cur, base):
    """The 14 sufficient statistics per row that the GPU rank-test kernels hand
    to the p-value kernel ([R, 14] fp64, SUFF_NAMES order), from the same
    sorts and ranks as ``pairwise_tests``:

    n1, n2 finite samples per side; r1 the rank sum of the current sample and
    tie = sum(t^3 - t) over the pooled tie runs; D = max |a1 n2 - a2 n1| /
    (n1 n2) over tie-run ends (0 when a side is empty); m1, m2 the means and
    q1, q2 the sums of squared deviations (0 for an empty side); over the
    first min(n_cur, n_base) position pairs with both members finite and d =
    cur - base formed in fp32: nzero pairs with d == 0, nw the others, npos of
    them positive, rplus the rank sum of the positive pairs among the |d| and
    tiew their tie term.  A difference that overflows fp32 counts as the
    largest magnitude."""
    c32 = np.asarray(cur, dtype=np.float32)
    b32 = np.asarray(base, dtype=np.float32)
    R = c32.shape[0]
    c = np.where(np.isfinite(c32), c32, np.inf).astype(np.float64)
    b = np.where(np.isfinite(b32), b32, np.inf).astype(np.float64)
    pooled = np.concatenate([c, b], axis=1)
    tags = np.concatenate([np.zeros(c.shape, np.int8), np.ones(b.shape, np.int8)], axis=1)
    tags = np.where(np.isfinite(pooled), tags, -1)
    n1 = (tags == 0).sum(1)
    n2 = (tags == 1).sum(1)
    out = np.zeros((R, 14), np.float64)
    out[:, 0], out[:, 1] = n1, n2
    if pooled.shape[1]:
        ranks, _, tie, order, is_end = avg_ranks(pooled)
        out[:, 3] = np.where(tags == 0, ranks, 0.0).sum(1)
        out[:, 4] = tie
        ts = np.take_along_axis(tags, order, axis=1)
        a1 = np.cumsum(ts == 0, axis=1)
        a2 = np.cumsum(ts == 1, axis=1)
        dnum = np.where(is_end, np.abs(a1 * n2[:, None] - a2 * n1[:, None]), 0).max(axis=1)
        both = (n1 > 0) & (n2 > 0)
        out[:, 5] = np.where(both, dnum / np.maximum(n1 * n2, 1).astype(np.float64), 0.0)
    for col, x, cnt in ((8, c, n1), (9, b, n2)):
        fin = np.isfinite(x)
        m = np.where(fin, x, 0.0).sum(1) / np.maximum(cnt, 1)
        out[:, col] = m
        out[:, col + 2] = np.where(fin, (np.where(fin, x, 0.0) - m[:, None]) ** 2, 0.0).sum(1)
    npair = min(c32.shape[1], b32.shape[1])
    if npair > 0:
        pc, pb = c32[:, :npair], b32[:, :npair]
        ok = np.isfinite(pc) & np.isfinite(pb)
        with np.errstate(over="ignore", invalid="ignore"):
            d = np.where(ok, pc - pb, np.float32(0)).astype(np.float64)
        big = 2.0 * float(np.finfo(np.float32).max)
        d = np.clip(d, -big, big)                       # an overflowed difference: the largest magnitude
        nz = ok & (d != 0)
        rw, _, tiew, _, _ = avg_ranks(np.where(nz, np.abs(d), np.inf))
        out[:, 2] = nz.sum(1)
        out[:, 6] = np.where(nz & (d > 0), rw, 0.0).sum(1)
        out[:, 7] = tiew
        out[:, 12] = (nz & (d > 0)).sum(1)
        out[:, 13] = (ok & ~nz).sum(1)
    return out


# ---------------------------------------------------------------------------
# moving_average_all + decision


def stats_decide(hist, cur, M, thr, bound, minlb, diff, pair_factor, min_hist):
    hist = np.asarray(hist, dtype=np.float64)
    cur = np.asarray(cur, dtype=np.float32)
    R = hist.shape[0]
    h = np.where(np.isfinite(hist), hist, np.nan)
    n = np.isfinite(h).sum(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.where(n > 0, np.nansum(h, 1) / np.maximum(n, 1), 0.0)
        var = np.where(n > 0, np.nansum((h - mean[:, None]) ** 2, 1) / np.maximum(n, 1), 0.0)
    sd = np.sqrt(var)
    m = np.arange(R) % M
    th = np.asarray(thr, dtype=np.float64)[m].copy()
    if diff is not None:
        th = np.where(np.asarray(diff) != 0, th * pair_factor, th)
    bd = np.asarray(bound)[m]
    up = (mean + th * sd).astype(np.float32)
    lo = np.maximum(mean - th * sd, np.asarray(minlb, dtype=np.float64)[m]).astype(np.float32)
    has_hist = (n >= min_hist) & (n > 0)
    fin = np.isfinite(cur)
    hi = ((bd & 1) != 0)[:, None] & (cur > up[:, None]) & fin
    lw = ((bd & 2) != 0)[:, None] & (cur < lo[:, None]) & fin
    flag = (hi | lw) & has_hist[:, None]
    count = flag.sum(1).astype(np.int32)
    sdf = sd.astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.where(hi, cur - up[:, None], np.where(lw, lo[:, None] - cur, 0.0))
        z = np.where(sdf[:, None] > 0, e / np.where(sdf > 0, sdf, 1)[:, None], 1e30)
    score = np.where(flag, z, 0.0).max(1, initial=0.0).astype(np.float32)
    valid = (has_hist.astype(np.int32) | (fin.any(1).astype(np.int32) << 1)).astype(np.int32)
    ncur = cur.shape[1]
    NW = max(1, (ncur + 63) // 64)
    padded = np.zeros((R, NW * 64), dtype=bool)
    padded[:, :ncur] = flag
    words = np.packbits(padded.reshape(R, NW, 64), axis=2, bitorder="little").view(np.uint64).reshape(R, NW)
    stats = np.stack([mean.astype(np.float32), sdf, up, lo], 1)
    return stats, words.view(np.int64), count, score, valid


def service_reduce(count, score, valid, M):
    S = count.size // M
    c = count.reshape(S, M)
    tot = c.sum(1)
    mask = ((c > 0) * (1 << np.arange(M))).sum(1)
    unknown = ((valid.reshape(S, M) & 3) != 3).any(1)
    status = np.where(tot > 0, 1, np.where(unknown, 2, 0))
    best = np.maximum(score.reshape(S, M).max(1), 0)
    return np.stack([status, best, mask, tot], 1).astype(np.float32)


def compact_anomalies(flags, cur, count):
    R = flags.shape[0]
    n = cur.shape[1]
    f = flags.view(np.uint64)
    bits = ((f[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(R, -1)[:, :n]
    rows, pts = np.nonzero(bits)
    idx = np.stack([rows, pts], 1).astype(np.int32)
    return idx, cur[rows, pts].astype(np.float32)


# ---------------------------------------------------------------------------
# synthetic fleet (must mirror synth_kernel in csrc/kernels/synth.hip)

_U = np.uint32


def hash_u32(x):
    x = np.atleast_1d(np.asarray(x, dtype=np.uint32))
    x = x ^ (x >> _U(16))
    x = x * _U(0x7FEB352D)
    x = x ^ (x >> _U(15))
    x = x * _U(0x846CA68B)
    x = x ^ (x >> _U(16))
    return x


def hash3(a, b, c):
    a = np.asarray(a, dtype=np.uint32)
    b = np.asarray(b, dtype=np.uint32)
    c = np.asarray(c, dtype=np.uint32)
    return hash_u32((a * _U(0x9E3779B1)) ^ hash_u32((b * _U(0x85EBCA77)) ^ hash_u32(c + _U(0x165667B1))))


def u01(h):
    return ((np.asarray(h, dtype=np.uint32) >> _U(8)).astype(np.float32) + np.float32(1.0)) * np.float32(1.0 / 16777216.0)


def synth_params(gs, m, seed):
    key = np.asarray(gs, dtype=np.uint32) * _U(64) + np.asarray(m, dtype=np.uint32)
    f = np.float32
    level = f(1.0) + f(99.0) * u01(hash3(key, 0, seed))
    amp_d = f(0.1) + f(0.3) * u01(hash3(key, 1, seed))
    amp_w = f(0.01) + f(0.04) * u01(hash3(key, 2, seed))
    phase = f(6.2831853) * u01(hash3(key, 3, seed))
    noise = f(0.005) + f(0.015) * u01(hash3(key, 4, seed))
    return key, level, amp_d, amp_w, phase, noise


def synth_value(params, t, stream_id, seed):
    key, level, amp_d, amp_w, phase, noise = params
    f = np.float32
    tf = np.asarray(t).astype(np.float32)
    season = f(1.0) + amp_d * np.sin(f(6.2831853) * tf / f(1440.0) + phase) + \
        amp_w * np.sin(f(6.2831853) * tf / f(10080.0) + phase)
    tt = (np.asarray(t, dtype=np.int64) & 0xFFFFFFFF).astype(np.uint32) * _U(2654435761) + \
        np.asarray(stream_id, dtype=np.uint32)
    h1 = hash3(key, tt, _U(seed) ^ _U(0xA5A5A5A5))
    h2 = hash_u32(h1 ^ _U(0x68E31DA4))
    g = np.sqrt(f(-2.0) * np.log(u01(h1))) * np.cos(f(6.2831853) * u01(h2))
    v = level * season * (f(1.0) + noise * g)
    return np.maximum(v, f(0.0)).astype(np.float32)


def synth_fleet(S, M, T, P, W, svc0, seed, fault_rate, fault_mag, ldh):
    gs = (svc0 + np.arange(S))[:, None].astype(np.uint32)
    m = np.arange(M)[None, :].astype(np.uint32)
    gsr = np.repeat(gs, M, axis=1).reshape(-1, 1)
    mr = np.tile(m, (S, 1)).reshape(-1, 1)
    prm = synth_params(gsr, mr, seed)
    hist = np.full((S * M, ldh), np.nan, dtype=np.float32)
    hist[:, :T] = synth_value(prm, np.arange(T)[None, :], 0, seed)
    pod = np.repeat(np.arange(P), W)[None, :]
    w = np.tile(np.arange(W), P)[None, :]
    base = synth_value(prm, T - W + w, 1000 + pod, seed)
    cur = synth_value(prm, T + w, 1000 + pod + 500, seed)
    faulty = (u01(hash3(gsr, 7, seed)) < np.float32(fault_rate)) & ((mr % 4) == 0)
    _, level, amp_d, amp_w, _, _ = prm
    shift = level * np.float32(fault_mag) * (np.float32(1.0) + amp_d + amp_w)
    cur = np.where(faulty, cur + shift, cur).astype(np.float32)
    return hist, base.astype(np.float32), cur


# ---------------------------------------------------------------------------
# effect size of current vs baseline (K19), straight from the definitions in
# docs/BRAIN_SPEC.md: every pair difference materialised in fp32 and sorted


def _mid_sorted(xs, n):
    """Median of the first n entries of every ascending row of xs (fp32):
    the middle one, or 0.5 * lo + 0.5 * up of the two middle ones; NaN if n == 0."""
    f = np.float32
    R = xs.shape[0]
    out = np.full(R, np.nan, dtype=np.float32)
    ok = n > 0
    if xs.shape[1] and ok.any():
        r = np.nonzero(ok)[0]
        lo = xs[r, (n[r] - 1) // 2].astype(np.float32)
        up = xs[r, n[r] // 2].astype(np.float32)
        with np.errstate(invalid="ignore", over="ignore"):
            out[r] = f(0.5) * lo + f(0.5) * up
    return out


def pairwise_effect(cur, base, chunk_elems: int = 1 << 22):
    """(effect [R, 4] fp32 = (Cliff's delta, Hodges-Lehmann shift, baseline
    median, N), counts [R, 2] int32 = (#{d > 0}, #{d < 0})) over the
    N = n1 * n2 differences d = fl32(x_i - y_j) of the finite samples of each
    row.  NaN / +-inf samples are missing; N == 0 gives NaN and zero counts."""
    cur = np.asarray(cur, dtype=np.float32)
    base = np.asarray(base, dtype=np.float32)
    R, nc = cur.shape
    nb = base.shape[1]
    effect = np.full((R, 4), np.nan, dtype=np.float32)
    counts = np.zeros((R, 2), dtype=np.int32)
    effect[:, 3] = 0.0
    if R == 0:
        return effect, counts
    x = np.where(np.isfinite(cur), cur, np.float32(np.nan))
    y = np.where(np.isfinite(base), base, np.float32(np.nan))
    n1 = np.isfinite(cur).sum(1).astype(np.int64)
    n2 = np.isfinite(base).sum(1).astype(np.int64)
    N = n1 * n2
    effect[:, 3] = N.astype(np.float32)
    if nc == 0 or nb == 0:
        return effect, counts
    bmed = _mid_sorted(np.sort(y, axis=1), n2)          # NaN sorts last
    step = max(1, chunk_elems // (nc * nb))
    for r0 in range(0, R, step):
        r1 = min(R, r0 + step)
        with np.errstate(invalid="ignore", over="ignore"):
            d = (x[r0:r1, :, None] - y[r0:r1, None, :]).reshape(r1 - r0, nc * nb)
        counts[r0:r1, 0] = (d > 0).sum(1)
        counts[r0:r1, 1] = (d < 0).sum(1)
        d.sort(axis=1)
        effect[r0:r1, 1] = _mid_sorted(d, N[r0:r1])
    ok = N > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        delta = (counts[:, 0] - counts[:, 1]).astype(np.float32) / N.astype(np.float32)
    effect[:, 0] = np.where(ok, delta, np.float32(np.nan))
    effect[:, 2] = np.where(ok, bmed, np.float32(np.nan))
    return effect, counts


def effect_gate(effect, bound_per_row, min_effect, min_shift, min_shift_abs, directional):
    """passed [R] int8 of the effect-size gate: 0 where the row's difference is
    too small (|delta| < min_effect, or the shift is zero or below
    min_shift * |base_med| + min_shift_abs, all fp32) or, with ``directional``,
    points away from the only bound the metric judges (bound 1: shift <= 0,
    bound 2: shift >= 0).  A row with NaN delta / shift passes: the gate never
    sets a verdict, it only clears one."""
    f = np.float32
    e = np.asarray(effect, dtype=np.float32)
    delta, shift, bmed = e[:, 0], e[:, 1], e[:, 2]
    me, ms, ma = f(min_effect), f(min_shift), f(min_shift_abs)
    fail = np.zeros(e.shape[0], dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        if me > 0:
            fail |= np.abs(delta) < me
        if ms > 0 or ma > 0:
            a = np.abs(shift)
            fail |= ~((a > 0) & (a >= ms * np.abs(bmed) + ma))
        if directional:
            b = np.asarray(bound_per_row)
            fail |= ((b == 1) & (shift <= 0)) | ((b == 2) & (shift >= 0))
    fail &= ~(np.isnan(delta) | np.isnan(shift))
    return (~fail).astype(np.int8)


# ---------------------------------------------------------------------------
# scale test of current vs baseline (K27): Brown-Forsythe, i.e. Levene's test
# on the absolute deviations from each side's median, straight from the
# definitions in docs/BRAIN_SPEC.md section 4.2


def pairwise_scale(cur, base, min_points: int = 20):
    """scale [R, 6] fp32 = (W, p, ratio, med_c, med_b, N) per row.

    Over the finite samples of each side (NaN / +-inf are missing): the
    medians in fp32 (``_mid_sorted``), the deviations u = fl32(|fl32(x -
    med_c)|) and v likewise, and from there everything in fp64: the means
    ubar, vbar, SSW = sum (u - ubar)^2 + sum (v - vbar)^2 (two passes), SSB =
    n1 (ubar - zbar)^2 + n2 (vbar - zbar)^2 about the pooled mean zbar, nu =
    N - 2, W = nu SSB / SSW, p = the two-sided Student t tail of sqrt(W) at nu
    degrees of freedom (F(1, nu)), ratio = ubar / vbar; rounded to fp32 once.
    W, p and ratio are NaN where a side has fewer than max(min_points, 1)
    finite samples, a deviation overflows, or SSW == SSB == 0; SSW == 0 < SSB
    gives W = +inf, p = 0.  The medians are NaN for an empty side only; N =
    n1 + n2 always."""
    f = np.float32
    cur = np.asarray(cur, dtype=np.float32)
    base = np.asarray(base, dtype=np.float32)
    R = cur.shape[0]
    out = np.full((R, 6), np.nan, dtype=np.float32)
    if R == 0:
        return out
    x = np.where(np.isfinite(cur), cur, f(np.nan))
    y = np.where(np.isfinite(base), base, f(np.nan))
    n1 = np.isfinite(cur).sum(1).astype(np.int64)
    n2 = np.isfinite(base).sum(1).astype(np.int64)
    N = n1 + n2
    med_c = _mid_sorted(np.sort(x, axis=1), n1)         # NaN sorts last
    med_b = _mid_sorted(np.sort(y, axis=1), n2)
    out[:, 3], out[:, 4], out[:, 5] = med_c, med_b, N.astype(np.float32)
    need = max(int(min_points), 1)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        u = np.abs((x - med_c[:, None]).astype(np.float32)).astype(np.float64)
        v = np.abs((y - med_b[:, None]).astype(np.float32)).astype(np.float64)
        su = np.nansum(u, axis=1) if u.shape[1] else np.zeros(R)
        sv = np.nansum(v, axis=1) if v.shape[1] else np.zeros(R)
        d1, d2, dn = n1.astype(np.float64), n2.astype(np.float64), N.astype(np.float64)
        ubar, vbar = su / d1, sv / d2
        ssw = np.zeros(R)
        if u.shape[1]:
            ssw = ssw + np.nansum((u - ubar[:, None]) ** 2, axis=1)
        if v.shape[1]:
            ssw = ssw + np.nansum((v - vbar[:, None]) ** 2, axis=1)
        zbar = (su + sv) / dn
        ssb = d1 * (ubar - zbar) ** 2 + d2 * (vbar - zbar) ** 2
        nu = dn - 2.0
        W = nu * ssb / ssw                               # SSW == 0 < SSB: +inf
        t = np.sqrt(W)
        p = special.betainc(0.5 * nu, 0.5, nu / (nu + t * t))
        p = np.where(np.isinf(W), 0.0, p)
        ratio = ubar / vbar                              # vbar == 0 < ubar: +inf
        ok = (n1 >= need) & (n2 >= need) & np.isfinite(su) & np.isfinite(sv) & ~((ssw == 0) & (ssb == 0))
        out[:, 0] = np.where(ok, W, np.nan).astype(np.float32)
        out[:, 1] = np.where(ok, p, np.nan).astype(np.float32)
        out[:, 2] = np.where(ok, ratio, np.nan).astype(np.float32)
    return out


def scale_verdict(scale, p_thr, min_ratio: float = 1.0, both: bool = False):
    """scale_diff [R] int8 of the scale test: 1 where the test applies (p is a
    number), p < fp32(p_thr) (the comparison the decision makes on the six
    tests' p-values) and the current window is the wider one by at least
    min_ratio (ratio >= min_ratio) or, with ``both``, the narrower one by as
    much (ratio <= fl32(1 / min_ratio)); all in fp32."""
    f = np.float32
    s = np.asarray(scale, dtype=np.float32)
    p, ratio = s[:, 1], s[:, 2]
    with np.errstate(invalid="ignore"):
        hit = ratio >= f(min_ratio)
        if both:
            hit = hit | (ratio <= f(1.0) / f(min_ratio))
        return (~np.isnan(p) & (p < f(p_thr)) & hit).astype(np.int8)


# ---------------------------------------------------------------------------
# per-pod test of current vs baseline (K29): Kruskal-Wallis over the baseline
# and the canary's pods as groups, then Dunn's contrast of every pod against
# the baseline, straight from the definitions in docs/BRAIN_SPEC.md section 4.3


def pairwise_pods(cur, seg_end, base, min_points: int = 5):
    """(pods [R, 6] fp32 = (H, p_H, z_worst, p_worst, worst, k), pod_z [R, G]
    fp32, pod_n [R, G] int32, pod_rank2 [R, G] int64, base_rank2 [R] int64,
    tie [R] int64) per row.

    ``cur`` is pod-major and pod g owns the columns [seg_end[g - 1],
    seg_end[g]); NaN / +-inf are missing.  A pod with fewer than
    max(min_points, 1) finite samples is dropped (n = 0, z = NaN, rank2 = 0).
    Over the N pooled values of the baseline (group 0) and the k kept pods:
    average ranks, as exact integers the doubled rank sums and the tie term
    sum(t^3 - t); then in fp64, each line left to right, rounded to fp32 once:
    C = 1 - tie / (N^3 - N), H = (12 / (N (N + 1)) sum_g (rank2_g / 2)^2 / n_g
    - 3 (N + 1)) / C, p_H = the chi-square tail of H at k degrees of freedom,
    sigma2 = N (N + 1) / 12 - tie / (12 (N - 1)), z_g = (rank2_g / (2 n_g) -
    rank2_0 / (2 n_0)) / sqrt(sigma2 (1 / n_g + 1 / n_0)), p_g = min(1, k
    erfc(|z_g| / sqrt 2)); worst = the kept pod with the largest |z_g| (the
    lowest on ties).  Not applicable (H, p_H, z_worst, p_worst and every z_g
    NaN, worst = -1) when k < 2, the baseline has fewer than max(min_points,
    1) finite samples or C <= 0; the integers and k are reported regardless."""
    cur = np.asarray(cur, dtype=np.float32)
    base = np.asarray(base, dtype=np.float32)
    seg = np.asarray(seg_end, dtype=np.int64)
    R, G = seg.shape
    pods = np.full((R, 6), np.nan, dtype=np.float32)
    pods[:, 4], pods[:, 5] = -1.0, 0.0
    pod_z = np.full((R, G), np.nan, dtype=np.float32)
    pod_n = np.zeros((R, G), dtype=np.int32)
    pod_rank2 = np.zeros((R, G), dtype=np.int64)
    base_rank2 = np.zeros(R, dtype=np.int64)
    tie = np.zeros(R, dtype=np.int64)
    need = max(int(min_points), 1)
    for r in range(R):
        groups, kept, lo = [base[r][np.isfinite(base[r])]], [], 0
        for g in range(G):
            x = cur[r, lo:max(lo, seg[r, g])]
            lo = max(lo, int(seg[r, g]))
            x = x[np.isfinite(x)]
            if len(x) >= need:
                kept.append(g)
                groups.append(x)
        k = len(kept)
        pods[r, 5] = k
        pooled = np.concatenate(groups).astype(np.float64)          # (-0.0 == 0.0: one tie run)
        srt = np.sort(pooled)
        lt, le = np.searchsorted(srt, pooled, "left"), np.searchsorted(srt, pooled, "right")
        t = (le - lt).astype(np.int64)
        rank2 = 2 * lt.astype(np.int64) + t + 1
        n = np.array([len(x) for x in groups], dtype=np.int64)
        r2 = np.add.reduceat(rank2, np.concatenate([[0], np.cumsum(n)[:-1]])) * (n > 0) if len(pooled) else 0 * n
        tie[r] = int((t * t - 1).sum())
        base_rank2[r] = r2[0]
        pod_n[r, kept], pod_rank2[r, kept] = n[1:], r2[1:]
        if k < 2 or n[0] < need:
            continue
        dN, dt = float(n.sum()), float(tie[r])
        C = 1.0 - dt / (dN * dN * dN - dN)
        if not C > 0.0:
            continue
        dn, dr = n.astype(np.float64), r2.astype(np.float64)
        s = 0.0
        for g in range(k + 1):
            s += (dr[g] / 2.0) ** 2 / dn[g]
        H = (12.0 / (dN * (dN + 1.0)) * s - 3.0 * (dN + 1.0)) / C
        var = dN * (dN + 1.0) / 12.0 - dt / (12.0 * (dN - 1.0))
        z = (dr[1:] / (2.0 * dn[1:]) - dr[0] / (2.0 * dn[0])) / np.sqrt(var * (1.0 / dn[1:] + 1.0 / dn[0]))
        w = int(np.argmax(np.abs(z)))
        pods[r, :5] = (H, special.chdtrc(k, H) if H > 0 else 1.0, z[w],
                       min(1.0, k * special.erfc(abs(z[w]) / np.sqrt(2.0))), kept[w])
        pod_z[r, kept] = z
    return pods, pod_z, pod_n, pod_rank2, base_rank2, tie


def pods_verdict(pods, p_thr):
    """pod_diff [R] int8 of the per-pod test: 1 where the test applies (p_H is
    a number) and both the omnibus p_H and the worst pod's Bonferroni p-value
    are below fp32(p_thr), compared in fp32 as the decision compares the six
    tests' p-values."""
    p = np.asarray(pods, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return (~np.isnan(p[:, 1]) & (p[:, 1] < np.float32(p_thr)) & (p[:, 3] < np.float32(p_thr))).astype(np.int8)


# ---------------------------------------------------------------------------
# joint multi-metric test of current vs baseline (K30): the Puri-Sen
# multivariate rank-sum statistic over the metrics of a job, straight from the
# definition in docs/BRAIN_SPEC.md section 4.4

JOINT_MAX_K = 8


def pairwise_joint(cur, base, rows, K, min_points: int = 20):
    """(joint [G, 6] fp32 = (L, p, dof, z_worst, worst, N), n12 [G, 2] int32,
    T [G, 8] int64, A [G, 8, 8] int64, member_z [G, 8] fp32) per group.

    Member j of group g is row ``rows[g, j]`` (j < K[g] <= 8) of ``cur`` /
    ``base``; column c of every member is the same sample.  NaN / +-inf are
    missing, and a column counts only where every member is finite (n1 current
    and n2 baseline columns kept, N = n1 + n2).  Per member the midranks over
    its N kept pooled values (-0.0 == 0.0) as exact integers rank2 = 2 lt + t +
    1, centred: a_j = rank2_j - (N + 1).  T_j = sum of a_j over the kept
    current columns, A_jk = sum of a_j a_k over all kept columns (int64).  Then
    in fp64, in member order, each line left to right, over the members kept
    so far: l_jk = (A_jk - sum_{m<k} l_jm l_km d_m) / d_k, d_j = A_jj - sum_k
    l_jk^2 d_k, y_j = T_j - sum_k l_jk y_k; member j is dropped when A_jj == 0
    or d_j <= 1e-9 A_jj (constant, or rank-collinear with those before it);
    dof = the number kept.  L = N (N - 1) / (n1 n2) sum_j y_j^2 / d_j, p = the
    chi-square tail of L at dof degrees of freedom (1 where L <= 0); z_j = T_j
    / sqrt(n1 n2 / (N (N - 1)) A_jj) (NaN where A_jj == 0), worst = the member
    with the largest |z_j| (the lowest on ties).  Not applicable (L, p,
    z_worst and every z_j NaN, worst = -1) when n1 or n2 < max(min_points, 1)
    or dof == 0; the integers are reported regardless.  Everything is rounded
    to fp32 once."""
    cur = np.asarray(cur, dtype=np.float32)
    base = np.asarray(base, dtype=np.float32)
    rows = np.asarray(rows, dtype=np.int64).reshape(-1, JOINT_MAX_K)
    K = np.asarray(K, dtype=np.int64).reshape(-1)
    G = len(K)
    joint = np.full((G, 6), np.nan, dtype=np.float32)
    joint[:, 2], joint[:, 4], joint[:, 5] = 0.0, -1.0, 0.0
    n12 = np.zeros((G, 2), dtype=np.int32)
    T = np.zeros((G, JOINT_MAX_K), dtype=np.int64)
    A = np.zeros((G, JOINT_MAX_K, JOINT_MAX_K), dtype=np.int64)
    member_z = np.full((G, JOINT_MAX_K), np.nan, dtype=np.float32)
    need = max(int(min_points), 1)
    for g in range(G):
        k = int(K[g])
        c, b = cur[rows[g, :k]], base[rows[g, :k]]
        kc, kb = np.isfinite(c).all(0), np.isfinite(b).all(0)
        n1, n2 = int(kc.sum()), int(kb.sum())
        N = n1 + n2
        x = np.concatenate([c[:, kc], b[:, kb]], axis=1).astype(np.float64)
        a = np.zeros((k, N), dtype=np.int64)
        for j in range(k):
            srt = np.sort(x[j])
            a[j] = np.searchsorted(srt, x[j], "left") + np.searchsorted(srt, x[j], "right") - N   # rank2 - (N + 1)
        T[g, :k], A[g, :k, :k] = a[:, :n1].sum(1), a @ a.T
        n12[g], joint[g, 5] = (n1, n2), N
        Tg, Ag = T[g].astype(np.float64), A[g].astype(np.float64)
        kept, d, y, l = [], np.zeros(k), np.zeros(k), np.zeros((k, k))
        q = 0.0
        for j in range(k):
            for kk in kept:
                s = 0.0
                for m in kept:
                    if m < kk:
                        s += l[j, m] * l[kk, m] * d[m]
                l[j, kk] = (Ag[j, kk] - s) / d[kk]
            s, t = 0.0, 0.0
            for kk in kept:
                s += l[j, kk] * l[j, kk] * d[kk]
            for kk in kept:
                t += l[j, kk] * y[kk]
            dj, yj = Ag[j, j] - s, Tg[j] - t
            if Ag[j, j] == 0.0 or dj <= 1e-9 * Ag[j, j]:
                continue
            kept.append(j)
            d[j], y[j] = dj, yj
            q += yj * yj / dj
        dof = len(kept)
        joint[g, 2] = dof
        if n1 < need or n2 < need or dof == 0:
            continue
        dN, d12 = float(N), float(n1) * float(n2)
        L = dN * (dN - 1.0) / d12 * q
        z = np.full(k, np.nan)
        nz = np.diag(Ag)[:k] != 0.0
        z[nz] = Tg[:k][nz] / np.sqrt(d12 / (dN * (dN - 1.0)) * np.diag(Ag)[:k][nz])
        w = int(np.argmax(np.nan_to_num(np.abs(z), nan=-1.0)))
        joint[g, :5] = (L, special.chdtrc(dof, L) if L > 0 else 1.0, dof, z[w], w)
        member_z[g, :k] = z
    return joint, n12, T, A, member_z


def joint_verdict(joint, p_thr):
    """joint_diff [G] int8 of the joint test: 1 where the test applies (p is a
    number) and p is below fp32(p_thr), compared in fp32 as ``pods_verdict``
    compares."""
    p = np.asarray(joint, dtype=np.float32).reshape(-1, 6)[:, 1]
    with np.errstate(invalid="ignore"):
        return (~np.isnan(p) & (p < np.float32(p_thr))).astype(np.int8)


# ---------------------------------------------------------------------------
# drift test of current vs baseline (K31): the Mann-Kendall trend of the
# canary's samples over time, stratified by pod, against the baseline's own,
# straight from the definition in docs/BRAIN_SPEC.md section 4.5


def mann_kendall_counts(x):
    """(S, P, Tx2, V18) of one segment's finite samples ``x`` in time order, as
    exact integers: with g_j / l_j / c_j the earlier samples below / above /
    equal to x_j, S = sum g_j - l_j, P = n (n - 1) / 2, Tx2 = sum 2 c_j and
    V18 = n (n - 1) (2 n + 5) - sum (6 c_j^2 + 12 c_j), 18 times the
    tie-corrected Mann-Kendall variance."""
    x = np.asarray(x, dtype=np.float64)                             # (-0.0 == 0.0: a tie)
    n = len(x)
    S = c1 = c2 = 0
    for a in range(0, n, 512):                                      # (blocks of j, to bound the pair matrix)
        blk = x[a:a + 512, None]
        earlier = np.arange(n)[None, :] < np.arange(a, a + len(blk))[:, None]
        S += int(((x[None, :] < blk) & earlier).sum()) - int(((x[None, :] > blk) & earlier).sum())
        c = ((x[None, :] == blk) & earlier).sum(1).astype(np.int64)
        c1, c2 = c1 + int(c.sum()), c2 + int((c * c).sum())
    return S, n * (n - 1) // 2, 2 * c1, n * (n - 1) * (2 * n + 5) - (6 * c2 + 12 * c1)


def pairwise_drift(cur, seg_end, base, min_points: int = 10):
    """(drift [R, 6] fp32 = (z, p, z_c, tau_c, z_b, tau_b), counts [R, 2, 4]
    int64 = (S, P, Tx2, V18) of the current side and the baseline, pod_S [R, G]
    int32, pod_n [R, G] int32, k [R] int32) per row.

    ``cur`` is pod-major and pod g owns the columns [seg_end[g - 1],
    seg_end[g]); ``base`` is one segment.  NaN / +-inf are missing, the rest
    keep their column order as time.  A pod with fewer than max(min_points, 1)
    finite samples is dropped (n = 0, S = 0).  The current side's integers are
    those of ``mann_kendall_counts`` summed over the k kept pods (pods are never
    compared with each other), the baseline's those of its one segment.  Then
    in fp64, each line left to right, rounded to fp32 once, per side: z_side =
    (S - sgn S) / sqrt(V18 / 18), tau_side = S / sqrt(P (P - Tx2 / 2)), both 0
    for a side with V18 == 0; z = (z_c - z_b) / sqrt(1 + v_b) with v_b = 1 if
    the baseline's V18 > 0 else 0; p = erfc(|z| / sqrt 2).  Not applicable (all
    six NaN) when k == 0, the baseline has fewer than max(min_points, 1) finite
    samples or the current side's V18 == 0; the integers and k are reported
    regardless."""
    cur = np.asarray(cur, dtype=np.float32)
    base = np.asarray(base, dtype=np.float32)
    seg = np.asarray(seg_end, dtype=np.int64)
    R, G = seg.shape
    drift = np.full((R, 6), np.nan, dtype=np.float32)
    counts = np.zeros((R, 2, 4), dtype=np.int64)
    pod_S = np.zeros((R, G), dtype=np.int32)
    pod_n = np.zeros((R, G), dtype=np.int32)
    k = np.zeros(R, dtype=np.int32)
    need = max(int(min_points), 1)

    def side(S, P, T2, V):
        if V == 0:
            return 0.0, 0.0
        return ((S - np.sign(S)) / np.sqrt(float(V) / 18.0),
                float(S) / np.sqrt(float(P) * (float(P) - float(T2) / 2.0)))

    for r in range(R):
        lo = 0
        for g in range(G):
            x = cur[r, lo:max(lo, seg[r, g])]
            lo = max(lo, int(seg[r, g]))
            x = x[np.isfinite(x)]
            if len(x) >= need:
                c = mann_kendall_counts(x)
                counts[r, 0] += c
                pod_S[r, g], pod_n[r, g] = c[0], len(x)
                k[r] += 1
        b = base[r][np.isfinite(base[r])]
        counts[r, 1] = mann_kendall_counts(b)
        if k[r] == 0 or len(b) < need or counts[r, 0, 3] == 0:
            continue
        (zc, tc), (zb, tb) = side(*(int(v) for v in counts[r, 0])), side(*(int(v) for v in counts[r, 1]))
        z = (zc - zb) / np.sqrt(1.0 + (1.0 if counts[r, 1, 3] > 0 else 0.0))
        drift[r] = (z, special.erfc(abs(z) / np.sqrt(2.0)), zc, tc, zb, tb)
    return drift, counts, pod_S, pod_n, k


def drift_verdict(drift, p_thr, min_tau: float = 0.0):
    """drift_diff [R] int8 of the drift test: 1 where the test applies (p is a
    number), p is below fp32(p_thr) and |tau_c| is at least fp32(min_tau),
    compared in fp32 as ``pods_verdict`` compares."""
    d = np.asarray(drift, dtype=np.float32).reshape(-1, 6)
    with np.errstate(invalid="ignore"):
        return (~np.isnan(d[:, 1]) & (d[:, 1] < np.float32(p_thr)) &
                (np.abs(d[:, 3]) >= np.float32(min_tau))).astype(np.int8)


# ---------------------------------------------------------------------------
# tail test of current vs baseline (K32): the share of samples beyond the
# pooled q-quantiles, an exact conditional (Fisher / Mood) test per level,
# straight from the definition in docs/BRAIN_SPEC.md section 4.6

TAIL_SIDES = {"BOUND": 0, "UPPER": 1, "LOWER": 2, "BOTH": 3}
TAIL_TABLE_MAX = 8192
_TAIL_LF = np.zeros(0, dtype=np.float64)


def tail_log_factorials(n: int = TAIL_TABLE_MAX):
    """lf[i] = lgamma(i + 1) for i = 0 .. max(n, 8,192) in fp64 (``math.lgamma``):
    the table the kernel is handed, so device and definition read the same
    numbers."""
    global _TAIL_LF
    n = max(int(n), TAIL_TABLE_MAX)
    if len(_TAIL_LF) < n + 1:
        import math
        _TAIL_LF = np.array([math.lgamma(i + 1.0) for i in range(n + 1)], dtype=np.float64)
    return _TAIL_LF[:n + 1]


def hypergeom_upper_tail(a: int, m: int, n_c: int, n_b: int) -> float:
    """P(X >= a) for X the current side's share of the m pooled samples beyond
    a threshold, n_c of the N = n_c + n_b samples being the current side's:
    the sum over x = max(a, m - n_b) .. min(m, n_c) of C(m, x) C(N - m, n_c -
    x) / C(N, n_c), each term exp of nine table entries added left to right;
    exactly 1 when a <= max(0, m - n_b), capped at 1."""
    N = n_c + n_b
    if a <= max(0, m - n_b):
        return 1.0
    lf = tail_log_factorials(N)
    x = np.arange(max(a, m - n_b), min(m, n_c) + 1)
    s = lf[m] - lf[x] - lf[m - x] + lf[N - m] - lf[n_c - x] - lf[N - m - n_c + x] - lf[N] + lf[n_c] + lf[n_b]
    return min(1.0, float(np.exp(s).sum()))


def pairwise_tail(cur, base, q_i=(9000, 9500, 9900), sides="BOUND", bound_per_row=None, min_points: int = 20,
                  min_tail_points: int = 5):
    """(tail [R, 4] fp32 = (p, p_min, excess, t of the deciding level), which
    [R] int32 = side * L + level of the deciding level or -1, J [R] int32, n
    [R, 2] int32 = finite samples per side, counts [R, 2, L, 3] int32 = (a, b,
    k) per side and level) per row.

    ``q_i`` are the L levels in parts per 10,000.  NaN / +-inf are missing;
    samples compare as fp32 (-0.0 == 0.0).  The row applies when both sides
    have max(min_points, 1) finite samples.  ``sides`` names the sides that
    run; under BOUND the row's code in ``bound_per_row`` decides (1 upper, 2
    lower, anything else both).  Upper side, level l: k = min(N - 1, ceil(q_i
    N / 10,000)), t the k-th smallest pooled value, a / b the current /
    baseline samples above t, m = a + b.  The lower side is the upper side of
    the negated samples: t the k-th largest pooled value (reported in the
    samples' own sign), a / b the samples below it.  A level counts when m >=
    min_tail_points and m differs from the previous counting level's m on its
    side; its p-value is ``hypergeom_upper_tail``.  J = counting levels over
    the sides that run; the deciding level has the smallest p (ties: the upper
    side, then the lower level); p = min(1, J p_min), excess = a / n_c - b /
    n_b in fp64, each rounded to fp32 once.  Rows that do not apply report
    zero counts; tail is NaN and which -1 there and where J == 0."""
    cur = np.asarray(cur, dtype=np.float32)
    base = np.asarray(base, dtype=np.float32)
    R, L = cur.shape[0], len(q_i)
    tail = np.full((R, 4), np.nan, dtype=np.float32)
    which = np.full(R, -1, dtype=np.int32)
    J = np.zeros(R, dtype=np.int32)
    n = np.zeros((R, 2), dtype=np.int32)
    counts = np.zeros((R, 2, L, 3), dtype=np.int32)
    need = max(int(min_points), 1)
    fixed = TAIL_SIDES[str(sides).upper()]
    for r in range(R):
        c, b = cur[r][np.isfinite(cur[r])], base[r][np.isfinite(base[r])]
        n_c, n_b = len(c), len(b)
        n[r] = (n_c, n_b)
        if n_c < need or n_b < need:
            continue
        code = fixed if fixed else int(bound_per_row[r])
        N = n_c + n_b
        pooled = np.sort(np.concatenate([c, b]))
        best = None
        for s in (0, 1):
            if code == (2, 1)[s]:
                continue
            prev = -1
            for l, q in enumerate(q_i):
                k = min(N - 1, -(-int(q) * N // 10000))
                if s == 0:
                    t = pooled[k - 1]
                    a, bb = int((c > t).sum()), int((b > t).sum())
                else:
                    t = pooled[N - k]
                    a, bb = int((c < t).sum()), int((b < t).sum())
                counts[r, s, l] = (a, bb, k)
                m = a + bb
                if m < min_tail_points or m == prev:
                    continue
                prev = m
                J[r] += 1
                p = hypergeom_upper_tail(a, m, n_c, n_b)
                if best is None or p < best[0]:
                    best = (p, s * L + l, a / n_c - bb / n_b, t)
        if best is not None:
            tail[r] = (min(1.0, int(J[r]) * best[0]), best[0], best[2], best[3])
            which[r] = best[1]
    return tail, which, J, n, counts


def tail_verdict(tail, p_thr, min_excess: float = 0.0):
    """tail_diff [R] int8 of the tail test: 1 where the test applies with J >=
    1 (p is a number), p is below fp32(p_thr) and the excess is at least
    fp32(min_excess), compared in fp32 as ``drift_verdict`` compares."""
    d = np.asarray(tail, dtype=np.float32).reshape(-1, 4)
    with np.errstate(invalid="ignore"):
        return (~np.isnan(d[:, 0]) & (d[:, 0] < np.float32(p_thr)) & (d[:, 2] >= np.float32(min_excess))).astype(np.int8)


# ---------------------------------------------------------------------------
# dependence gate of the pairwise verdict (K33): the rank-sum z of current vs
# baseline with each side's sample size deflated by a variance-inflation factor
# from the autocorrelation of the pooled midranks along time, straight from the
# definition in docs/BRAIN_SPEC.md section 4.7

ACF_MAX_LAG = 16


def pairwise_dependence(cur, seg_end, base, max_lag: int = 8, min_points: int = 12):
    """(dep [R, 6] fp32 = (p_adj, z_adj, z, VIF_c, VIF_b, N), rho [R, 2, 16]
    fp32, n [R, 2] int32, TA [R, 2] int64 = (T, A), kept [R, 2] int32, pairs
    [R, 2, 16] int32) per row; entry j of ``rho`` / ``pairs`` is lag j + 1.

    ``cur`` is pod-major and pod g owns the columns [seg_end[g - 1],
    seg_end[g]) in time order; ``base`` is one segment.  NaN / +-inf are
    missing; samples compare as fp32 (-0.0 == 0.0).  n = the finite counts
    (n1, n2), N their sum.  Over the N pooled finite values rank2 = 2 lt + t +
    1 and a = rank2 - (N + 1); T = sum of a over the current side, A = sum of
    a^2 over both, exact.  A lag is a column distance: the pair (i, i + k)
    counts when both columns lie in the same segment and both are finite;
    nothing is compacted.  A segment with n_s finite samples is kept when n_s
    >= max(min_points, 1), with lags up to L_s = min(max_lag, n_s // 4): mean
    = (sum a) / n_s, e = a - mean, c0 = sum e^2, c_k = sum over its pairs of
    e_i e_(i+k), in fp64.  Per side C0 / C_k / pairs sum the kept segments,
    rho_k = C_k / C0 (0 where C0 == 0), VIF = min(max(1, 1 + 2 sum_k (1 - k /
    (L + 1)) rho_k), max(1, n_side / 2)).  z = T / sqrt(n1 n2 / (N (N - 1))
    A), z_adj = z sqrt((1 / n1 + 1 / n2) / (VIF_c / n1 + VIF_b / n2)), p_adj =
    erfc(|z_adj| / sqrt 2), in fp64, rounded to fp32 once; NaN when n1 < 2, n2
    < 2 or A == 0.  The integers, rho and the VIFs are reported regardless."""
    cur = np.asarray(cur, dtype=np.float32)
    base = np.asarray(base, dtype=np.float32)
    seg = np.asarray(seg_end, dtype=np.int64)
    R, G = seg.shape
    L = int(max_lag)
    if not 1 <= L <= ACF_MAX_LAG:
        raise ValueError(f"max_lag must lie in 1..{ACF_MAX_LAG}, got {max_lag!r}")
    need = max(int(min_points), 1)
    n_cur = cur.shape[1]
    dep = np.full((R, 6), np.nan, dtype=np.float32)
    rho = np.zeros((R, 2, ACF_MAX_LAG), dtype=np.float32)
    n = np.zeros((R, 2), dtype=np.int32)
    TA = np.zeros((R, 2), dtype=np.int64)
    kept = np.zeros((R, 2), dtype=np.int32)
    pairs = np.zeros((R, 2, ACF_MAX_LAG), dtype=np.int32)
    w = 1.0 - np.arange(1, L + 1) / (L + 1.0)
    for r in range(R):
        x = np.concatenate([cur[r], base[r]]).astype(np.float64)
        fin = np.isfinite(x)
        n1, n2 = int(fin[:n_cur].sum()), int(fin[n_cur:].sum())
        N = n1 + n2
        v = np.sort(x[fin])
        lt, le = np.searchsorted(v, x[fin], "left"), np.searchsorted(v, x[fin], "right")
        a = np.zeros(len(x), dtype=np.int64)
        a[fin] = 2 * lt + (le - lt) + 1 - (N + 1)
        T, A = int(a[:n_cur][fin[:n_cur]].sum()), int((a * a).sum())
        n[r], TA[r] = (n1, n2), (T, A)
        # the segments: the pods of the current side, then the baseline
        segs, lo = [], 0
        for g in range(G):
            hi = max(lo, min(int(seg[r, g]), n_cur))
            segs.append((0, lo, hi))
            lo = hi
        segs.append((1, n_cur, len(x)))
        C0, Ck = np.zeros(2), np.zeros((2, L))
        for s, lo, hi in segs:
            f, n_s = fin[lo:hi], int(fin[lo:hi].sum())
            if n_s < need:
                continue
            kept[r, s] += 1
            e = np.where(f, a[lo:hi] - float(a[lo:hi][f].sum()) / n_s, 0.0)
            C0[s] += float((e * e).sum())
            for k in range(1, min(L, n_s // 4) + 1):
                both = f[:-k] & f[k:]
                Ck[s, k - 1] += float((e[:-k] * e[k:])[both].sum())
                pairs[r, s, k - 1] += int(both.sum())
        vif = np.ones(2)
        for s, n_s in ((0, n1), (1, n2)):
            rk = Ck[s] / C0[s] if C0[s] > 0 else np.zeros(L)
            rho[r, s, :L] = rk
            vif[s] = min(max(1.0, 1.0 + 2.0 * float((w * rk).sum())), max(1.0, n_s / 2.0))
        dep[r, 3:] = (vif[0], vif[1], N)
        if n1 < 2 or n2 < 2 or A == 0:
            continue
        z = T / np.sqrt(float(n1) * n2 / (float(N) * (N - 1.0)) * A)
        z_adj = z * np.sqrt((1.0 / n1 + 1.0 / n2) / (vif[0] / n1 + vif[1] / n2))
        dep[r, :3] = (special.erfc(abs(z_adj) / np.sqrt(2.0)), z_adj, z)
    return dep, rho, n, TA, kept, pairs


def dependence_verdict(dep, p_thr):
    """dep_keep [R] int8 of the dependence gate: 1 where the gate does not apply
    (p_adj is NaN: the row keeps its verdict) or p_adj is below fp32(p_thr),
    compared in fp32 as ``drift_verdict`` compares."""
    p = np.asarray(dep, dtype=np.float32).reshape(-1, 6)[:, 0]
    with np.errstate(invalid="ignore"):
        return (np.isnan(p) | (p < np.float32(p_thr))).astype(np.int8)
