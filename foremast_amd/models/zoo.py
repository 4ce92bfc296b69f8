"""Model zoo: every ``ML_ALGORITHM`` of the brain as one batched call over a
packed shard ``hist [R, ld]`` (rows = jobs x metrics) that returns per-point
decisions for the current window.

Algorithms (docs/guides/design.md:53-85; default moving_average_all,
deploy/foremast/3_brain/foremast-brain.yaml:24-25):

==============================  ======================================  ==================
name                            model                                   kernels
==============================  ======================================  ==================
moving_average_all              mean/std over the whole history         K1+K7 fused
moving_average                  mean/std over the last ``window`` pts   K1+K7 fused (view)
exponential_smoothing           SES, alpha grid                         K2 + band decide
double_exponential_smoothing    Holt, (alpha, beta) grid                K2 + band decide
holt_winters                    additive HW, period from the FFT        K3 + K2 + band
holt_winters_multiplicative     multiplicative HW (seasonal ratio)      K3 + K2 + band
prophet                         trend+hinges+daily/weekly Fourier LSQ   K10 (f32 MFMA)
lstm                            LSTM forecaster (bf16 MFMA)             K6 + band decide
bivariate_normal                Mahalanobis over metric pairs           K5
multivariate_normal             joint Mahalanobis over all metrics      K12
robust_multivariate             the same, past incident columns aside   K13 + K17
robust_moving_average_all       median / MAD over the whole history     K13 + band decide
robust_moving_average           median / MAD over the last ``window``   K13 (view) + band
seasonal_robust                 per-phase median profile + residual MAD K14 + band decide
shift_robust                    median / MAD behind the last shift      K15 + band decide
trend_robust                    repeated-median line + residual MAD     K16 + band decide
seasonal_trend_robust           repeated-median line + phase profile    K20 + band decide
seasonal_scale_robust           phase profile + a sigma per phase       K22 + band decide (per point)
auto_robust                     per row, the robust model that back-    K13-K22 fits + K23 + band
                                tests best on the end of its history    decide (per point)
quantile_robust                 median + a sigma per side, tail ranks   K24 + band decide (two sigmas)
seasonal_quantile_robust        phase profile + a sigma per phase and   K26 + band decide (per point,
                                per side, tail ranks                    two sigmas)
==============================  ======================================  ==================

The exponential-smoothing family goes through the brain's fitted-model cache
when one is given (``models/cache.py``, ``MAX_CACHE_SIZE``): cached series are
advanced over their new samples instead of re-fitting the grid.

Thresholds are in sigma units per metric (``BrainConfig.rule_for``), lowered
by ``pairwise_threshold_factor`` on rows whose canary distribution differs.
``multivariate_normal`` takes one joint threshold (``mvn_threshold``), turned
into a cut on the Mahalanobis distance per number of live members;
``robust_multivariate`` shares it and sets aside the history columns where a
member lies more than ``mvn_reject`` MAD-sigmas from its median.
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from ..ops import canary as C
from ..ops import fft as FF
from ..ops import lsq as LQ
from ..ops import smoothing as SM

ALGORITHMS = ("moving_average_all", "moving_average", "exponential_smoothing", "double_exponential_smoothing",
              "holt_winters", "holt_winters_multiplicative", "prophet", "lstm", "bivariate_normal", "multivariate_normal",
              "robust_moving_average_all", "robust_moving_average", "seasonal_robust", "shift_robust",
              "trend_robust", "robust_multivariate", "seasonal_trend_robust", "seasonal_scale_robust", "auto_robust",
              "quantile_robust", "seasonal_quantile_robust")

ALIASES = {"moving_average_all": "moving_average_all", "ma_all": "moving_average_all",
           "moving_average": "moving_average", "ma": "moving_average",
           "exponential_smoothing": "exponential_smoothing", "ses": "exponential_smoothing",
           "double_exponential_smoothing": "double_exponential_smoothing", "holt": "double_exponential_smoothing",
           "holt_winters": "holt_winters", "hw": "holt_winters", "triple_exponential_smoothing": "holt_winters",
           "holt_winters_multiplicative": "holt_winters_multiplicative", "hw_mul": "holt_winters_multiplicative",
           "prophet": "prophet", "lstm": "lstm", "bivariate_normal": "bivariate_normal", "bivariate": "bivariate_normal",
           "multivariate_normal": "multivariate_normal", "multivariate": "multivariate_normal",
           "mvn": "multivariate_normal",
           "robust_moving_average_all": "robust_moving_average_all", "median_mad": "robust_moving_average_all",
           "mad": "robust_moving_average_all", "robust": "robust_moving_average_all",
           "robust_moving_average": "robust_moving_average", "robust_ma": "robust_moving_average",
           "seasonal_robust": "seasonal_robust", "seasonal_median": "seasonal_robust",
           "seasonal_mad": "seasonal_robust", "robust_seasonal": "seasonal_robust",
           "shift_robust": "shift_robust", "level_shift": "shift_robust", "robust_shift": "shift_robust",
           "shift_mad": "shift_robust",
           "trend_robust": "trend_robust", "robust_trend": "trend_robust", "trend_median": "trend_robust",
           "repeated_median": "trend_robust",
           "seasonal_trend_robust": "seasonal_trend_robust", "trend_seasonal_robust": "seasonal_trend_robust",
           "robust_seasonal_trend": "seasonal_trend_robust", "robust_stl": "seasonal_trend_robust",
           "seasonal_scale_robust": "seasonal_scale_robust", "seasonal_hetero_robust": "seasonal_scale_robust",
           "robust_seasonal_scale": "seasonal_scale_robust", "seasonal_mad_profile": "seasonal_scale_robust",
           "auto_robust": "auto_robust", "auto": "auto_robust", "robust_auto": "auto_robust",
           "auto_select": "auto_robust",
           "quantile_robust": "quantile_robust", "skew_robust": "quantile_robust",
           "asymmetric_robust": "quantile_robust", "tail_quantile": "quantile_robust",
           "seasonal_quantile_robust": "seasonal_quantile_robust", "seasonal_skew_robust": "seasonal_quantile_robust",
           "seasonal_asymmetric_robust": "seasonal_quantile_robust",
           "robust_seasonal_quantile": "seasonal_quantile_robust",
           "robust_multivariate": "robust_multivariate", "robust_mvn": "robust_multivariate",
           "mvn_robust": "robust_multivariate", "multivariate_robust": "robust_multivariate"}


def canonical(name: str) -> str:
    k = (name or "moving_average_all").strip().lower()
    if k not in ALIASES:
        raise ValueError(f"unknown ML_ALGORITHM {name!r}; supported: {', '.join(ALGORITHMS)}")
    return ALIASES[k]


@dataclass
class RowDecision:
    upper: torch.Tensor      # [R, n] per-point upper bound
    lower: torch.Tensor      # [R, n]
    flags: torch.Tensor      # [R, NW] int64 bit-packed
    count: torch.Tensor      # [R] int32
    score: torch.Tensor      # [R] f32
    valid: torch.Tensor      # [R] int32 bit0 history ok, bit1 current present
    center: torch.Tensor | None = None
    choice: torch.Tensor | None = None   # [R] int32 index into AUTO_CANDIDATES (auto_robust only)


@dataclass
class CacheContext:
    """Which cached model each row maps to (see ``models/cache.py``)."""
    cache: "ModelCache"
    keys: list              # one hashable key per row, e.g. (job id, alias, algorithm)
    t_last: np.ndarray      # [R] timestamp of each row's last history sample
    step: float             # sample spacing, seconds
    now: float              # wall clock (refit age)
    plan: object = None     # this batch's ModelCache.es_lookup, when already made


@dataclass
class Tables:
    thr: torch.Tensor
    bound: torch.Tensor
    minlb: torch.Tensor
    pair_factor: float
    min_hist: int


def _expand_stats(dec: C.DecideResult, n: int) -> RowDecision:
    up = dec.stats[:, 2:3].expand(-1, n)
    lo = dec.stats[:, 3:4].expand(-1, n)
    return RowDecision(up, lo, dec.flags, dec.count, dec.score, dec.valid, dec.stats[:, 0:1].expand(-1, n))


def _valid(hist: torch.Tensor, T: int, cur: torch.Tensor, min_hist: int) -> torch.Tensor:
    if hist.is_cuda and hist.stride(0) % 4 == 0 and hist.data_ptr() % 16 == 0:
        # finite-sample count from the streaming history-stats kernel (one HBM
        # pass) instead of isfinite -> bool [R, T] -> sum
        from ..ops._lib import LIB, ptr, stream_of
        hs = torch.empty((hist.shape[0], 3), dtype=torch.float32, device=hist.device)
        LIB.call("fm_hist_stats", ptr(hist), hist.stride(0), T, hist.shape[0], ptr(hs), stream_of(hist))
        nh = hs[:, 2]
    else:
        nh = torch.isfinite(hist[:, :T]).sum(1)
    has_cur = torch.isfinite(cur).any(1)
    return ((nh >= max(min_hist, 1)).to(torch.int32) | (has_cur.to(torch.int32) << 1))


def decide(algorithm: str, hist: torch.Tensor, T: int, cur: torch.Tensor, horizon: torch.Tensor, M: int,
           tables: Tables, diff: torch.Tensor | None = None, window: int = 60, period: int | None = None,
           lstm_model=None, pairs=None, cache: CacheContext | None = None, H: int | None = None,
           groups=None, mvn_threshold: float | None = None, smooth: int = 5, block: int | None = None,
           shift_threshold: float = 4.0, min_blocks: int = 2, trend_min_blocks: int = 3,
           mvn_reject: float = 3.5, scale_smooth: int = 30, scale_floor: float = 0.1, holdout: int = 0,
           candidates=None, zcap: float = 8.0, margin: float = 0.05, auto: "AutoContext | None" = None,
           trend_block: int | None = None, tail_z: float = 2.0) -> RowDecision:
    """Score current points of every row.

    ``horizon`` [R, n] int64: steps past the end of the history of each current
    point (1 = the next sample), used by forecasting models; ``H`` its
    maximum when the caller knows it (saves a device sync).  ``block``,
    ``shift_threshold`` and ``min_blocks`` are ``shift_robust``'s block length
    in samples (default 1,440: a day at 60 s), score threshold and the blocks
    a new level must have held; ``trend_robust`` cuts its blocks by ``block``
    too and fits a slope from ``trend_min_blocks`` non-empty ones, and
    ``seasonal_trend_robust`` from as many non-empty cycles of ``period``.
    ``mvn_reject`` is ``robust_multivariate``'s rejection limit in MAD-sigmas
    (<= 0: nothing is rejected).  ``scale_smooth`` and ``scale_floor`` are
    ``seasonal_scale_robust``'s: the half width of the window that smooths
    its per-phase scale, and that scale's floor as a share of the pooled MAD.
    ``holdout``, ``candidates``, ``zcap`` and ``margin`` are ``auto_robust``'s
    (:func:`auto_select`), which takes every other model's parameters for its
    candidates (``trend_block``: its ``trend_robust``'s block where that
    differs from ``block``); ``auto`` is its memory of earlier choices, when
    there is one.  ``tail_z`` is ``quantile_robust``'s: the threshold at which
    its band ends on the history's own tail quantiles;
    ``seasonal_quantile_robust`` takes it too, with ``seasonal_scale_robust``'s
    parameters."""
    algo = canonical(algorithm)
    n = cur.shape[1]
    if algo == "moving_average_all":
        dec = C.stats_decide(hist, cur, T, M, tables.thr, tables.bound, tables.minlb, diff, tables.pair_factor,
                             tables.min_hist)
        return _expand_stats(dec, n)
    if algo == "moving_average":
        w = min(T, max(4, (window + 3) // 4 * 4))
        start = (T - w) // 4 * 4        # keep the view 16-B aligned for the vector loads
        view = hist[:, start:T]
        dec = C.stats_decide(view, cur, T - start, M, tables.thr, tables.bound, tables.minlb, diff,
                             tables.pair_factor, tables.min_hist)
        return _expand_stats(dec, n)
    if algo in ROBUST:
        return _robust(hist, T, robust_start(algo, T, window), cur, horizon, M, tables, diff)
    if algo == "quantile_robust":
        return _quantile_robust(hist, T, cur, horizon, M, tables, diff, tail_z)
    if algo == "shift_robust":
        return _shift_robust(hist, T, cur, horizon, M, tables, diff, block or 1440, shift_threshold, min_blocks)
    if algo == "bivariate_normal":
        return _bivariate(hist, T, cur, M, tables, pairs)
    if algo == "multivariate_normal":
        return _multivariate(hist, T, cur, M, tables, diff, groups, mvn_threshold)
    if algo == "robust_multivariate":
        return _multivariate_robust(hist, T, cur, horizon, M, tables, diff, groups, mvn_threshold, mvn_reject)
    if H is None:
        H = int(horizon.max().item()) if horizon.numel() else 1
    H = max(int(H), 1)
    if algo in ES_KINDS and cache is None:
        # the grid fit counts each row's finite samples on its way through the
        # history: no separate history pass for the MIN_HISTORICAL_DATA gate
        kind, m = ES_KINDS[algo], 1
        if kind >= 2:
            m = period or _detect_period(hist, T)
            if 2 * m > T:
                kind, m = 1, 1
        fit = SM.es_fit(hist, T, kind, H, m, prune=SM.HW_SCAN_PRUNE)
        has_cur = torch.isfinite(cur).any(1).to(torch.int32)
        valid = (fit.nfin.to(cur.device) >= max(tables.min_hist, 1)).to(torch.int32) | (has_cur << 1)
        return band(fit.forecast, fit.sigma, horizon, cur, M, tables, diff, valid)
    if algo == "seasonal_robust":
        # the kernel counts the finite samples it models: no separate history pass
        fc, sigma, nfin = _seasonal_robust(hist, T, H, period, smooth)
        has_cur = torch.isfinite(cur).any(1).to(torch.int32)
        valid = (nfin >= max(tables.min_hist, 1)).to(torch.int32) | (has_cur << 1)
        return band(fc, sigma, horizon, cur, M, tables, diff, valid)
    if algo == "trend_robust":
        # gated on the finite count of the residuals the kernel modelled
        fc, sigma, nfin = _trend_robust(hist, T, H, block or 1440, trend_min_blocks)
        has_cur = torch.isfinite(cur).any(1).to(torch.int32)
        valid = (nfin >= max(tables.min_hist, 1)).to(torch.int32) | (has_cur << 1)
        return band(fc, sigma, horizon, cur, M, tables, diff, valid)
    if algo == "seasonal_trend_robust":
        # gated on the finite count of the residuals the kernel modelled
        fc, sigma, nfin = _seasonal_trend_robust(hist, T, H, period, smooth, trend_min_blocks)
        has_cur = torch.isfinite(cur).any(1).to(torch.int32)
        valid = (nfin >= max(tables.min_hist, 1)).to(torch.int32) | (has_cur << 1)
        return band(fc, sigma, horizon, cur, M, tables, diff, valid)
    if algo == "seasonal_scale_robust":
        # gated on the span's finite count, as seasonal_robust; sigma is [R, H] (1-D from the fallback)
        fc, sigma, nfin = _seasonal_scale_robust(hist, T, H, period, smooth, scale_smooth, scale_floor)
        has_cur = torch.isfinite(cur).any(1).to(torch.int32)
        valid = (nfin >= max(tables.min_hist, 1)).to(torch.int32) | (has_cur << 1)
        return band(fc, sigma, horizon, cur, M, tables, diff, valid)
    if algo == "seasonal_quantile_robust":
        # gated on the span's finite count, as seasonal_scale_robust; sigma is a pair, [R, H] each ([R] from the fallback)
        fc, sigma, nfin = _seasonal_quantile_robust(hist, T, H, period, smooth, scale_smooth, scale_floor, tail_z)
        has_cur = torch.isfinite(cur).any(1).to(torch.int32)
        valid = (nfin >= max(tables.min_hist, 1)).to(torch.int32) | (has_cur << 1)
        return band(fc, sigma, horizon, cur, M, tables, diff, valid)
    if algo == "auto_robust":
        # gated, row by row, on the finite count of the model the row chose
        fc, sigma, nfin, choice = _auto_remembered(auto, hist, T, H, period, smooth, block, shift_threshold,
                                                   min_blocks, trend_min_blocks, scale_smooth, scale_floor, holdout,
                                                   candidates, zcap, margin, trend_block=trend_block)
        has_cur = torch.isfinite(cur).any(1).to(torch.int32)
        valid = (nfin >= max(tables.min_hist, 1)).to(torch.int32) | (has_cur << 1)
        dec = band(fc, sigma, horizon, cur, M, tables, diff, valid)
        dec.choice = choice
        return dec
    fc, sigma = forecast(algo, hist, T, H, period=period, lstm_model=lstm_model, cache=cache, smooth=smooth)
    return band(fc, sigma, horizon, cur, M, tables, diff, _valid(hist, T, cur, tables.min_hist))


def band(fc: torch.Tensor, sigma, horizon: torch.Tensor, cur: torch.Tensor, M: int, tables: Tables,
         diff: torch.Tensor | None, valid: torch.Tensor) -> RowDecision:
    """Forecast -> per-point bands and decisions: each current point is
    judged against the forecast at its own horizon, centre +/- thr * sigma.
    ``sigma`` is [R], or [R, H] with a sigma per forecast step, which is
    gathered at the horizon like the centre, or a pair (sigma_lo, sigma_up)
    with a sigma per side of the centre, both [R] or both [R, H] and gathered
    at the horizon.  Rows without enough history (``valid`` bit 0) flag
    nothing."""
    H = fc.shape[1]
    idx = (horizon.clamp(1, H) - 1).to(fc.device)
    center = torch.gather(fc, 1, idx).contiguous()
    if isinstance(sigma, (tuple, list)):
        sigma_lo, sigma_up = sigma
        if sigma_lo.dim() == 2:
            up, lo, flags, cnt, sc = SM.band_decide_pp_2s(cur, center, torch.gather(sigma_lo, 1, idx).contiguous(),
                                                          torch.gather(sigma_up, 1, idx).contiguous(), M, tables.thr,
                                                          tables.bound, tables.minlb, diff, tables.pair_factor)
        else:
            up, lo, flags, cnt, sc = SM.band_decide_2s(cur, center, sigma_lo.contiguous(), sigma_up.contiguous(), M,
                                                       tables.thr, tables.bound, tables.minlb, diff,
                                                       tables.pair_factor)
    elif sigma.dim() == 2:
        up, lo, flags, cnt, sc = SM.band_decide_pp(cur, center, torch.gather(sigma, 1, idx).contiguous(), M,
                                                   tables.thr, tables.bound, tables.minlb, diff, tables.pair_factor)
    else:
        up, lo, flags, cnt, sc = SM.band_decide(cur, center, sigma.contiguous(), M, tables.thr, tables.bound,
                                                tables.minlb, diff, tables.pair_factor)
    has = (valid & 1).bool().to(cnt.device)
    cnt = torch.where(has, cnt, torch.zeros_like(cnt))
    flags = torch.where(has[:, None], flags, torch.zeros_like(flags))
    return RowDecision(up, lo, flags, cnt, sc, valid, center)


ROBUST = ("robust_moving_average_all", "robust_moving_average")


def robust_start(algo: str, T: int, window: int = 60) -> int:
    """First history column the robust model ``algo`` reads: 0, or the start
    of the last ``window`` points (any column: K13 takes unaligned views)."""
    return 0 if algo == "robust_moving_average_all" else T - min(T, max(1, int(window)))


def _robust(hist, T, start, cur, horizon, M, tables, diff) -> RowDecision:
    """Hampel band: centre = median, sigma = 1.4826 MAD (or its mean-deviation
    fallback) of the finite history samples in columns [start, T), K13; the
    existing band decision then applies the per-metric thresholds, bounds and
    canary factor in those sigma units.  The history gate is the kernel's
    finite count, not a second pass over the history."""
    from ..ops import misc as MI
    center, sigma, nfin = MI.robust_stats(hist[:, start:T], T - start)
    has_cur = torch.isfinite(cur).any(1).to(torch.int32)
    valid = (nfin >= max(tables.min_hist, 1)).to(torch.int32) | (has_cur << 1)
    return band(center[:, None], sigma, horizon, cur, M, tables, diff, valid)


def _quantile_robust(hist, T, cur, horizon, M, tables, diff, tail_z=2.0) -> RowDecision:
    """Asymmetric band for skewed metrics: centre = median, and a sigma per
    side such that the band at ``thr = tail_z`` ends on the history's own
    ``Phi(-tail_z)`` and ``Phi(tail_z)`` quantiles (K24; the one-sided mean
    deviation where a side's quantile is the median itself); the band decision
    with two sigmas then applies the per-metric thresholds, bounds and canary
    factor, each side in its own sigma units.  The history gate is the
    kernel's finite count, as ``_robust``'s.  Whole history only: no window,
    no cache; the seasonal form is ``seasonal_quantile_robust``."""
    from ..ops import misc as MI
    center, sigma_lo, sigma_up, nfin = MI.quantile_robust_stats(hist[:, :T], T, MI.quantile_tail_z(tail_z))
    has_cur = torch.isfinite(cur).any(1).to(torch.int32)
    valid = (nfin >= max(tables.min_hist, 1)).to(torch.int32) | (has_cur << 1)
    return band(center[:, None], (sigma_lo, sigma_up), horizon, cur, M, tables, diff, valid)


def shift_start(T: int) -> int:
    """First history column ``shift_robust`` reads: 0, or the start of the
    last ``ROBUST_LDS_KEYS`` columns of a longer history (K15 holds the row in
    LDS and has no global-memory path)."""
    from ..ops import misc as MI
    return max(0, int(T) - MI.ROBUST_LDS_KEYS)


def _shift_robust(hist, T, cur, horizon, M, tables, diff, block, k, min_blocks) -> RowDecision:
    """Hampel band on the history behind the latest persistent level shift
    (K15): the blocks of ``block`` samples are scanned for the most recent
    change of level that has held for ``min_blocks`` blocks, and centre and
    sigma are the median and 1.4826 MAD of the samples from there on; a row
    without a shift gets ``robust_moving_average_all``'s band.  The history
    gate is the finite count of the segment modelled, so a segment shorter
    than MIN_HISTORICAL_DATA is not judged rather than misjudged."""
    from ..ops import misc as MI
    s0 = shift_start(T)
    center, sigma, nseg, _, _, _ = MI.shift_robust(hist[:, s0:T], T - s0, int(block), float(k), int(min_blocks))
    has_cur = torch.isfinite(cur).any(1).to(torch.int32)
    valid = (nseg >= max(tables.min_hist, 1)).to(torch.int32) | (has_cur << 1)
    return band(center[:, None], sigma, horizon, cur, M, tables, diff, valid)


ES_KINDS = {"exponential_smoothing": 0, "double_exponential_smoothing": 1, "holt_winters": 2,
            "holt_winters_multiplicative": 3}
FORECASTERS = tuple(ES_KINDS) + ("prophet", "lstm", "seasonal_robust", "trend_robust", "seasonal_trend_robust",
                                 "seasonal_scale_robust", "auto_robust", "seasonal_quantile_robust")


def seasonal_start(T: int, period: int | None) -> int:
    """First history column ``seasonal_robust`` (and ``seasonal_trend_robust``,
    whose span is the same) reads when ``period`` is given:
    the start of its span of whole cycles, or 0 when it falls back to the
    whole-history median (and when the period is still to be detected)."""
    from ..ops import misc as MI
    J = MI.seasonal_cycles(T, period) if period else 0
    return T - J * int(period) if J >= 2 else 0


def _seasonal_robust(hist, T, H, period, smooth):
    """Per-phase median profile over the last whole cycles of the history and
    the MAD-sigma of the residuals about it, K14 -> (forecast [R, H], sigma
    [R], finite count [R]).  ``period`` None: detected from the history.  A
    history shorter than two periods, or a period too long for the kernel's
    budget, falls back to a constant forecast of the whole-history median with
    K13's sigma (as Holt-Winters falls back to Holt)."""
    from ..ops import misc as MI
    m = int(period or _detect_period(hist, T))
    if MI.seasonal_cycles(T, m) >= 2:
        return MI.seasonal_robust(hist, T, m, H, smooth)
    center, sigma, nfin = MI.robust_stats(hist, T)
    return center[:, None].expand(-1, H), sigma, nfin


def trend_start(T: int) -> int:
    """First history column ``trend_robust`` reads: as :func:`shift_start`,
    the last ``ROBUST_LDS_KEYS`` columns of a longer history (K16 holds the
    row in LDS and has no global-memory path)."""
    return shift_start(T)


def _trend_robust(hist, T, H, block, min_blocks):
    """Straight line through the history by the repeated median of the pair
    slopes of its block medians, and the median / MAD-sigma of the residuals
    about it, K16 -> (forecast [R, H], sigma [R], finite count [R]).  The
    centre is the level at the last history sample, so the forecast at
    horizon ``h`` is ``center + slope * h`` (a product and a sum, each rounded
    to fp32)."""
    from ..ops import misc as MI
    s0 = trend_start(T)
    center, sigma, nfin, slope = MI.trend_robust(hist[:, s0:T], T - s0, int(block), int(min_blocks))
    h = torch.arange(1, int(H) + 1, dtype=torch.float32, device=center.device)
    return center[:, None] + slope[:, None] * h[None, :], sigma, nfin


def _seasonal_trend_robust(hist, T, H, period, smooth, min_blocks):
    """Repeated-median line through the medians of the last whole cycles of
    the history, a per-phase median profile of the residuals about it and
    their MAD-sigma, K20 -> (forecast [R, H], sigma [R], finite count [R]).
    The span is ``seasonal_robust``'s (:func:`seasonal_start`), ``period``
    None is detected from the history, and so is the fallback: a history
    shorter than two periods, or a period too long for the kernel's budget,
    gets a constant forecast of the whole-history median with K13's sigma
    (slope 0)."""
    from ..ops import misc as MI
    m = int(period or _detect_period(hist, T))
    if MI.seasonal_cycles(T, m) >= 2:
        return MI.seasonal_trend_robust(hist, T, m, H, smooth, int(min_blocks))[:3]
    center, sigma, nfin = MI.robust_stats(hist, T)
    return center[:, None].expand(-1, H), sigma, nfin


def _seasonal_scale_robust(hist, T, H, period, smooth, scale_smooth, floor):
    """``seasonal_robust``'s per-phase median profile with a sigma per phase:
    the middle of each phase's residuals, smoothed over neighbouring phases,
    floored at a share of the pooled MAD and calibrated to a sigma, K22 ->
    (forecast [R, H], sigma [R, H], finite count [R]).  The span, ``period``
    None and the fallback are ``seasonal_robust``'s: a history shorter than
    two periods, or a period too long for the kernel's budget, gets the
    whole-history median with K13's one sigma, [R]."""
    from ..ops import misc as MI
    m = int(period or _detect_period(hist, T))
    if MI.seasonal_cycles(T, m) >= 2:
        fc, sigma_h, nfin = MI.seasonal_scale_robust(hist, T, m, H, smooth, int(scale_smooth), float(floor))[:3]
        return fc, sigma_h, nfin
    center, sigma, nfin = MI.robust_stats(hist, T)
    return center[:, None].expand(-1, H), sigma, nfin


def _seasonal_quantile_robust(hist, T, H, period, smooth, scale_smooth, floor, tail_z=2.0):
    """``seasonal_scale_robust``'s profile and per-phase scale with a sigma
    per side: each side's tail order statistic of the signed residuals over
    their phase's scale calibrates it, so that the band at ``thr = tail_z``
    ends on the history's own tail quantiles in every phase, K26 -> (forecast
    [R, H], (sigma_lo [R, H], sigma_up [R, H]), finite count [R]).  The span
    and ``period`` None are ``seasonal_robust``'s.  A history shorter than two
    periods, or a period too long for the kernel's budget, gets
    ``quantile_robust``'s flat band: the whole-history median with K24's pair
    of sigmas, [R] each."""
    from ..ops import misc as MI
    m = int(period or _detect_period(hist, T))
    z0 = MI.quantile_tail_z(tail_z)
    if MI.seasonal_cycles(T, m) >= 2:
        fc, slo, sup, nfin = MI.seasonal_quantile_robust(hist, T, m, H, smooth, int(scale_smooth), float(floor), z0)[:4]
        return fc, (slo, sup), nfin
    center, sigma_lo, sigma_up, nfin = MI.quantile_robust_stats(hist[:, :T], T, z0)
    return center[:, None].expand(-1, H), (sigma_lo, sigma_up), nfin


# auto_robust's candidates in order of parsimony: a later one must back-test
# better than an earlier one by more than the margin to be chosen.
AUTO_CANDIDATES = ("robust_moving_average_all", "shift_robust", "trend_robust", "seasonal_robust",
                   "seasonal_scale_robust", "seasonal_trend_robust")


def auto_candidates(names=None) -> tuple[int, ...]:
    """Indices into ``AUTO_CANDIDATES`` of a candidate list (names or aliases;
    None or empty: all six), in the table's order whatever order they came in."""
    if not names:
        return tuple(range(len(AUTO_CANDIDATES)))
    if isinstance(names, str):
        names = [p for p in names.split(",") if p.strip()]
    picked = set()
    for nm in names:
        k = str(nm).strip().lower()
        if ALIASES.get(k) not in AUTO_CANDIDATES:
            raise ValueError(f"unknown AUTO_CANDIDATES entry {nm!r}; supported: {', '.join(AUTO_CANDIDATES)}")
        picked.add(AUTO_CANDIDATES.index(ALIASES[k]))
    if not picked:
        raise ValueError("AUTO_CANDIDATES names no model")
    return tuple(sorted(picked))


@dataclass
class AutoContext:
    """Which remembered choice each row of an ``auto_robust`` call maps to
    (``models/cache.py`` AutoChoices)."""
    choices: "AutoChoices"
    keys: list              # one hashable key per row, e.g. (series, alias, base metric)
    t_last: np.ndarray      # [R] timestamp of each row's last history sample
    selected: int = 0       # out: rows this call selected anew
    choice: np.ndarray | None = None    # out: [R] the model each row ran under (index into AUTO_CANDIDATES)


def _auto_fit(ci: int, hist, T: int, H: int, m: int, smooth, block, shift_threshold, min_blocks, trend_min_blocks,
              scale_smooth, scale_floor, trend_block=None):
    """Candidate ``ci``'s own batched fit of ``hist[:, :T]``, exactly as its
    single-model branch of :func:`decide` calls it -> (forecast [R, H] or
    [R, 1], sigma [R] or [R, H], finite count [R]).  ``block`` is
    ``shift_robust``'s and, unless ``trend_block`` names another,
    ``trend_robust``'s."""
    from ..ops import misc as MI
    name = AUTO_CANDIDATES[ci]
    if name == "robust_moving_average_all":
        center, sigma, nfin = MI.robust_stats(hist[:, :T], T)
        return center[:, None], sigma, nfin
    if name == "shift_robust":
        s0 = shift_start(T)
        center, sigma, nseg = MI.shift_robust(hist[:, s0:T], T - s0, int(block), float(shift_threshold),
                                              int(min_blocks))[:3]
        return center[:, None], sigma, nseg
    if name == "trend_robust":
        return _trend_robust(hist, T, H, trend_block or block, trend_min_blocks)
    if name == "seasonal_robust":
        return _seasonal_robust(hist, T, H, m, smooth)
    if name == "seasonal_scale_robust":
        return _seasonal_scale_robust(hist, T, H, m, smooth, scale_smooth, scale_floor)
    return _seasonal_trend_robust(hist, T, H, m, smooth, trend_min_blocks)


def auto_select(hist: torch.Tensor, T: int, period: int | None = None, holdout: int = 0, smooth: int = 5,
                block: int | None = None, shift_threshold: float = 4.0, min_blocks: int = 2,
                trend_min_blocks: int = 3, scale_smooth: int = 30, scale_floor: float = 0.1, candidates=None,
                zcap: float = 8.0, margin: float = 0.05, trend_block: int | None = None):
    """Back-test selection of ``auto_robust`` -> (choice [R] int32 into
    ``AUTO_CANDIDATES``, score [R, C] f32, n [R, C] int32; C = the candidates
    in play).  The last ``L = holdout or period`` samples are held out, every
    candidate is fitted on columns ``[0, T - L)`` of the same tensor (no copy)
    with a forecast of ``L`` steps, and K23 scores the forecasts against
    ``hist[:, T - L:T]`` and picks (``ops/misc.py`` ref_holdout_score,
    ref_auto_pick).  A history shorter than ``2 L`` is not back-tested: every
    row gets the first candidate.  A seasonal candidate that falls back
    produces the first candidate's numbers and loses the tie by order."""
    from ..ops import misc as MI
    cand = auto_candidates(candidates)
    R = hist.shape[0]
    m = int(period or _detect_period(hist, T))
    L = min(int(holdout) if holdout and int(holdout) > 0 else m, MI.ROBUST_LDS_KEYS)
    if T < 2 * L or R == 0:
        return (torch.full((R,), cand[0], dtype=torch.int32, device=hist.device),
                torch.full((R, len(cand)), float("inf"), dtype=torch.float32, device=hist.device),
                torch.zeros((R, len(cand)), dtype=torch.int32, device=hist.device))
    fcs, sigmas = [], []
    for ci in cand:
        fc, sigma, _ = _auto_fit(ci, hist, T - L, L, m, smooth, block or 1440, shift_threshold, min_blocks,
                                 trend_min_blocks, scale_smooth, scale_floor, trend_block)
        fcs.append(fc)
        sigmas.append(sigma)
    score, n, _, pick = MI.holdout_score(hist[:, T - L:T], fcs, sigmas, zcap, margin)
    choice = pick if len(cand) == len(AUTO_CANDIDATES) else \
        torch.tensor(cand, dtype=torch.int32, device=pick.device)[pick.long()]
    return choice, score, n


def _auto_robust(hist, T, H, period=None, smooth=5, block=None, shift_threshold=4.0, min_blocks=2,
                 trend_min_blocks=3, scale_smooth=30, scale_floor=0.1, holdout=0, candidates=None, zcap=8.0,
                 margin=0.05, choice=None, trend_block=None):
    """Every row under the robust model that back-tests best on it ->
    (forecast [R, H], sigma [R, H], finite count [R] int32, choice [R] int32).
    ``choice`` brings the caller's memory: entries ``>= 0`` are kept, ``-1``
    (and all rows without it) are selected now (:func:`auto_select`).  Each
    chosen model then runs once over the rows that chose it, on the whole
    history; a sigma per row is broadcast along ``H``."""
    R = hist.shape[0]
    dev = hist.device
    m = int(period or _detect_period(hist, T))
    block = block or 1440
    args = (smooth, block, shift_threshold, min_blocks, trend_min_blocks, scale_smooth, scale_floor)
    trend_block = trend_block or block
    if choice is None:
        choice = torch.full((R,), -1, dtype=torch.int32, device=dev)
    choice = choice.to(device=dev, dtype=torch.int32).clone()
    if choice.numel() != R or bool((choice >= len(AUTO_CANDIDATES)).any()):
        raise ValueError("choice must hold one candidate index (or -1) per row")
    todo = (choice < 0).nonzero().squeeze(1)
    if todo.numel():
        sub = hist if todo.numel() == R else _aligned_rows(hist, todo, T)
        choice[todo] = auto_select(sub, T, m, holdout, *args, candidates=candidates, zcap=zcap, margin=margin,
                                    trend_block=trend_block)[0]
    fc = torch.empty((R, H), dtype=torch.float32, device=dev)
    sigma = torch.empty((R, H), dtype=torch.float32, device=dev)
    nfin = torch.zeros((R,), dtype=torch.int32, device=dev)
    for ci in torch.unique(choice).tolist():
        idx = (choice == ci).nonzero().squeeze(1)
        sub = hist if idx.numel() == R else _aligned_rows(hist, idx, T)
        f, s, n = _auto_fit(int(ci), sub, T, H, m, *args, trend_block)
        s = s[:, None] if s.dim() == 1 else s
        fc[idx], sigma[idx], nfin[idx] = f.expand(-1, H), s.expand(-1, H), n.to(torch.int32)
    return fc, sigma, nfin, choice


def _auto_remembered(auto, hist, T, H, *args, trend_block=None):
    """:func:`_auto_robust` with the choices ``auto`` remembers (an
    :class:`AutoContext`, or None: every row is selected): rows it knows skip
    the selection, and what is selected now is remembered."""
    if auto is None:
        return _auto_robust(hist, T, H, *args, trend_block=trend_block)
    known = torch.from_numpy(auto.choices.lookup(auto.keys, auto.t_last))
    out = _auto_robust(hist, T, H, *args, choice=known, trend_block=trend_block)
    fresh = (known < 0).numpy()
    auto.selected = int(fresh.sum())
    auto.choice = out[3].cpu().numpy()
    if auto.selected:
        auto.choices.remember(auto.keys, auto.t_last, auto.choice, fresh)
    return out


def forecast(algorithm: str, hist: torch.Tensor, T: int, H: int, period: int | None = None,
             lstm_model=None, cache: CacheContext | None = None,
             smooth: int = 5, block: int | None = None,
             trend_min_blocks: int = 3, scale_smooth: int = 30,
             scale_floor: float = 0.1, shift_threshold: float = 4.0, min_blocks: int = 2, holdout: int = 0,
             candidates=None, zcap: float = 8.0, margin: float = 0.05,
             auto: AutoContext | None = None, trend_block: int | None = None,
             tail_z: float = 2.0) -> tuple[torch.Tensor, torch.Tensor]:
    """H-step forecast past the end of the history for every row with a
    forecasting model -> (forecast [R, H], residual sigma [R]; sigma [R, H],
    one per step, from ``seasonal_scale_robust`` unless it fell back; a pair
    (sigma_lo, sigma_up) of those from ``seasonal_quantile_robust``).  Used by the
    band decision and, for HPA jobs, to publish the load forecast a cluster
    autoscaler can act on ahead of time (README.md:58-59 "ClusterAutoScaler
    prediction"; BASELINE config 4)."""
    algo = canonical(algorithm)
    if algo in ES_KINDS:
        kind = ES_KINDS[algo]
        if cache is not None:
            return cache.cache.es_forecast(cache.keys, cache.t_last, cache.step, cache.now, hist, T, kind, H,
                                           lambda sub: period or _detect_period(sub, T), plan=cache.plan)
        m = 1
        if kind >= 2:
            m = period or _detect_period(hist, T)
            if 2 * m > T:
                kind, m = 1, 1
        fit = SM.es_fit(hist, T, kind, H, m, prune=SM.HW_SCAN_PRUNE)
        return fit.forecast, fit.sigma
    if algo == "prophet":
        fit = LQ.prophet_fit(hist, T, H)
        return fit.forecast, fit.sigma
    if algo == "lstm":
        if lstm_model is None:
            from .lstm import LSTMForecaster
            lstm_model = LSTMForecaster.default(device=hist.device)
        return lstm_model.forecast(hist, T, H)
    if algo == "seasonal_robust":
        return _seasonal_robust(hist, T, H, period, smooth)[:2]
    if algo == "trend_robust":
        return _trend_robust(hist, T, H, block or 1440, trend_min_blocks)[:2]
    if algo == "seasonal_trend_robust":
        return _seasonal_trend_robust(hist, T, H, period, smooth, trend_min_blocks)[:2]
    if algo == "seasonal_scale_robust":
        return _seasonal_scale_robust(hist, T, H, period, smooth, scale_smooth, scale_floor)[:2]
    if algo == "seasonal_quantile_robust":
        return _seasonal_quantile_robust(hist, T, H, period, smooth, scale_smooth, scale_floor, tail_z)[:2]
    if algo == "auto_robust":
        return _auto_remembered(auto, hist, T, H, period, smooth, block, shift_threshold, min_blocks,
                                trend_min_blocks, scale_smooth, scale_floor, holdout, candidates, zcap, margin,
                                trend_block=trend_block)[:2]
    raise ValueError(f"{algorithm!r} is not a forecasting model ({', '.join(FORECASTERS)})")


def _detect_period(hist: torch.Tensor, T: int, default: int = 1440) -> int:
    """Fleet period for Holt-Winters: the median of per-row FFT peaks with
    strong seasonality, else ``default`` (daily at 60 s)."""
    nr = T - (T % 2)
    while nr > 64 and not FF.supported_length(nr):
        nr -= 2
    if nr <= 64:
        return min(default, max(2, T // 2))
    off = T - nr
    off -= off % 2
    view = hist[:, off:off + nr] if off % 4 == 0 else hist[:, :nr]
    s = FF.fft_seasonal(view.contiguous() if off % 2 else view, nr, min_period=12, max_period=nr / 2)
    # the period is a launch parameter of the fit: one small copy of the
    # per-row peaks and a host median (no device sort pipeline)
    per, strength = s.period.cpu().numpy(), s.strength.cpu().numpy()
    strong = strength > 0.1
    if not strong.any():
        return min(default, T // 2)
    p = int(np.median(per[strong]))
    return max(2, min(p, T // 2))


def _aligned_rows(hist, idx, T: int) -> torch.Tensor:
    """Rows ``idx`` of ``hist[:, :T]`` in a buffer whose rows stay 16-B
    aligned (ld a multiple of 4 floats) for the vector-load kernels."""
    w = max(4, (T + 3) // 4 * 4)
    out = torch.empty((int(idx.numel()), w), dtype=torch.float32, device=hist.device)
    out[:, :T] = hist[idx, :T]
    return out[:, :T]


def _bivariate(hist, T, cur, M, tables, pairs=None) -> RowDecision:
    """Metric pairs scored jointly; both rows of a pair get the pair's decision
    (bounds reported in Mahalanobis units: upper = threshold, lower = 0).
    ``pairs`` = (ia, ib, singles) row-index tensors; default: (0,1), (2,3), ...
    of each service with M metrics, an odd last metric -> moving_average_all."""
    from ..ops import misc as MI
    R, n = cur.shape
    device = hist.device
    if pairs is None:
        S = R // M
        base = torch.arange(S, device=device) * M
        ia = torch.cat([base + a for a in range(0, M - 1, 2)]) if M > 1 else base[:0]
        ib = ia + 1
        singles = base + (M - 1) if M % 2 == 1 else base[:0]
    else:
        ia, ib, singles = (p.to(device) for p in pairs)
    flags_all = torch.zeros((R, max(1, (n + 63) // 64)), dtype=torch.int64, device=device)
    count_all = torch.zeros((R,), dtype=torch.int32, device=device)
    score_all = torch.zeros((R,), dtype=torch.float32, device=device)
    up_all = torch.full((R, n), float("nan"), device=device)
    lo_all = torch.full((R, n), float("nan"), device=device)
    if ia.numel():
        ha, hb = _aligned_rows(hist, ia, T), _aligned_rows(hist, ib, T)
        ca, cb = cur[ia].contiguous(), cur[ib].contiguous()
        thr = float(tables.thr[0].item()) if tables.thr.numel() == 1 else float(tables.thr.max().item())
        params, dist, flags, cnt = MI.bivariate(ha, hb, T, ca, cb, thr)
        sc = torch.nan_to_num(dist, nan=0.0).amax(1)
        for i in (ia, ib):
            flags_all[i] = flags
            count_all[i] = cnt
            score_all[i] = sc
            up_all[i] = thr
            lo_all[i] = 0.0
    if singles.numel():
        sub = C.stats_decide(_aligned_rows(hist, singles, T), cur[singles].contiguous(), T, 1,
                             tables.thr[:1].contiguous(), tables.bound[:1].contiguous(), tables.minlb[:1].contiguous(),
                             None, tables.pair_factor, tables.min_hist)
        flags_all[singles], count_all[singles], score_all[singles] = sub.flags, sub.count, sub.score
        up_all[singles] = sub.stats[:, 2:3].expand(-1, n)
        lo_all[singles] = sub.stats[:, 3:4].expand(-1, n)
    valid = _valid(hist, T, cur, tables.min_hist)
    return RowDecision(up_all, lo_all, flags_all, count_all, score_all, valid)


MVN_MAX_K = 8


def mvn_groups(jobs) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """Row groups of the joint detector; ``jobs`` holds each job's row indices.
    A job's rows are cut into chunks of 8 in row order; a leftover of one row
    (and a job with one metric) is a single.  Returns (rows [G, 8] int32, -1
    padded; K [G] int64; singles int64)."""
    rows, ks, singles = [], [], []
    for idx in jobs:
        for c0 in range(0, len(idx), MVN_MAX_K):
            part = list(idx[c0:c0 + MVN_MAX_K])
            if len(part) == 1:
                singles.append(part[0])
            else:
                rows.append(part + [-1] * (MVN_MAX_K - len(part)))
                ks.append(len(part))
    return (torch.tensor(rows, dtype=torch.int32).reshape(-1, MVN_MAX_K), torch.tensor(ks, dtype=torch.int64),
            torch.tensor(singles, dtype=torch.int64))


MVN_MODELS = ("multivariate_normal", "robust_multivariate")


def _multivariate_robust(hist, T, cur, horizon, M, tables, diff, groups=None, thr=None, reject=3.5) -> RowDecision:
    """``_multivariate`` with the moments taken past the incident columns of
    the history (K13 + K17, ``ops/misc.py:ref_mvn_robust``): a complete
    column where any member lies more than ``reject`` of its MAD-sigmas from
    its median is set aside, unless that would set aside more than half.
    Singles go through ``robust_moving_average_all``."""
    return _multivariate(hist, T, cur, M, tables, diff, groups, thr, reject=float(reject), horizon=horizon)


def _multivariate(hist, T, cur, M, tables, diff, groups=None, thr=None, reject=None, horizon=None) -> RowDecision:
    """All metrics of a job scored jointly (K12): every member row of a group
    gets the group's decision, bounds in Mahalanobis units (upper = the cut
    the group used, lower = 0).  ``groups`` = (rows [G, 8] int32, K [G],
    singles) as :func:`mvn_groups` makes them; default: each service's M
    consecutive rows.  Singles go through ``moving_average_all``.  ``thr`` is
    the joint threshold in sigma units (default: the largest of the table);
    a group is judged at ``thr * pair_factor`` when any member's canary
    distribution differs.  ``reject`` not None: the robust model (K17) with
    that rejection limit, and singles through ``_robust`` (which needs their
    ``horizon``)."""
    from ..ops import misc as MI
    R, n = cur.shape
    device = hist.device
    if groups is None:
        groups = mvn_groups([range(s * M, (s + 1) * M) for s in range(R // M)])
    grows, gk, singles = (g.to(device) for g in groups)
    NW = max(1, (n + 63) // 64)
    flags_all = torch.zeros((R, NW), dtype=torch.int64, device=device)
    count_all = torch.zeros((R,), dtype=torch.int32, device=device)
    score_all = torch.zeros((R,), dtype=torch.float32, device=device)
    up_all = torch.full((R, n), float("nan"), device=device)
    lo_all = torch.full((R, n), float("nan"), device=device)
    valid = _valid(hist, T, cur, tables.min_hist)
    if hist.is_cuda and (hist.stride(0) % 4 or hist.data_ptr() % 16 or hist.stride(1) != 1):
        hist = _aligned_rows(hist, torch.arange(R, device=device), T)
    cur = cur.contiguous()
    if grows.shape[0]:
        if thr is None:
            thr = float(tables.thr[0].item()) if tables.thr.numel() == 1 else float(tables.thr.max().item())
        cuts = MI.mvn_cuts(thr, tables.pair_factor)
        cuts_d = torch.from_numpy(cuts).to(device)
        member = grows >= 0
        safe = grows.clamp(min=0).long()
        if diff is None:
            lowered = torch.zeros((grows.shape[0],), dtype=torch.uint8, device=device)
        else:
            lowered = ((diff.to(device)[safe] != 0) & member).any(1).to(torch.uint8)
        for K in sorted(set(gk.tolist())):
            sel = (gk == K).nonzero().squeeze(1)
            if reject is None:
                params, dist, flags, cnt, gvalid = MI.mvn(hist, T, cur, grows[sel].contiguous(), K, cuts,
                                                          lowered[sel], tables.min_hist)
            else:
                params, dist, flags, cnt, gvalid, _ = MI.mvn_robust(hist, T, cur, grows[sel].contiguous(), K, cuts,
                                                                    lowered[sel], tables.min_hist, reject)
            sc = torch.nan_to_num(dist, nan=0.0).amax(1)
            used = cuts_d[lowered[sel].long(), params[:, 1].long()]
            hist_ok = (gvalid & 1).to(torch.int32)
            for j in range(K):
                i = safe[sel, j]
                flags_all[i] = flags
                count_all[i] = cnt
                score_all[i] = sc
                up_all[i] = used[:, None].expand(-1, n)
                lo_all[i] = 0.0
                valid[i] = (valid[i] & 2) | hist_ok
    if singles.numel():
        S1 = int(singles.numel())
        pick = lambda t: t[singles % t.numel()].contiguous()
        sdiff = None if diff is None else diff[singles].contiguous()
        if reject is None:
            sub = C.stats_decide(_aligned_rows(hist, singles, T), cur[singles].contiguous(), T, S1, pick(tables.thr),
                                 pick(tables.bound), pick(tables.minlb), sdiff, tables.pair_factor, tables.min_hist)
            up_all[singles] = sub.stats[:, 2:3].expand(-1, n)
            lo_all[singles] = sub.stats[:, 3:4].expand(-1, n)
        else:
            sub = _robust(hist[singles], T, 0, cur[singles].contiguous(), horizon.to(device)[singles], S1,
                          Tables(pick(tables.thr), pick(tables.bound), pick(tables.minlb), tables.pair_factor,
                                 tables.min_hist), sdiff)
            up_all[singles], lo_all[singles], valid[singles] = sub.upper, sub.lower, sub.valid
        flags_all[singles], count_all[singles], score_all[singles] = sub.flags, sub.count, sub.score
    return RowDecision(up_all, lo_all, flags_all, count_all, score_all, valid)


def make_tables(aliases_per_row: list[str], cfg, device) -> Tables:
    """Per-row metric tables when rows of one batch carry different aliases:
    M = 1 logical metric per row (row r -> table entry r)."""
    rules = [cfg.rule_for(a) for a in aliases_per_row]
    return Tables(torch.tensor([r.threshold for r in rules], dtype=torch.float32, device=device),
                  torch.tensor([r.bound for r in rules], dtype=torch.int32, device=device),
                  torch.tensor([r.min_lower_bound for r in rules], dtype=torch.float32, device=device),
                  cfg.pairwise_threshold_factor, cfg.min_historical_points)


def rolling_bands(hist: torch.Tensor, T: int, M: int, tables: Tables, window: int = 60,
                  min_count: int | None = None) -> tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """moving_average bands at every time point of the history (the
    dashboard's metric bands, foremast-dashboard/src/config/metrics.js:21-29):
    center = trailing-window mean, upper = center + thr * std, lower =
    max(center - thr * std, min_lower_bound), with the metric's bound code
    masking the side it does not judge (NaN).  Row r uses table entry r % M.
    Returns (center, upper, lower) [R, T] fp32 (K1 rolling kernel on GPU)."""
    from ..ops import misc as MI
    mc = tables.min_hist if min_count is None else min_count
    w = max(1, min(int(window), MI.ROLLING_MAX_WINDOW, T))
    mean, sd = MI.rolling_stats(hist, T, w, max(1, min(mc, w)))
    R = hist.shape[0]
    idx = torch.arange(R, device=mean.device) % M
    thr = tables.thr.to(mean.device)[idx].unsqueeze(1)
    bd = tables.bound.to(mean.device)[idx].unsqueeze(1)
    mlb = tables.minlb.to(mean.device)[idx].unsqueeze(1)
    nan = torch.full_like(mean, float("nan"))
    up = torch.where((bd & 1) != 0, mean + thr * sd, nan)
    lo = torch.where((bd & 2) != 0, torch.maximum(mean - thr * sd, mlb.expand_as(mean)), nan)
    return mean, up, lo
