"""Canary-scoring ops: pairwise tests (K4), fused moving-average bounds +
anomaly decision (K1+K7), service reduce, anomaly compaction, synthetic fleet
(K11).

GPU tensors run the hand-written CDNA4 kernels in ``csrc/kernels/``
(``pairwise.hip``, ``pairwise_wide.hip``, ``pairwise_effect.hip``, ``pairwise_scale.hip``, ``pairwise_pods.hip``, ``pairwise_joint.hip``, ``pairwise_drift.hip``, ``pairwise_tail.hip``, ``pairwise_dependence.hip``, ``hist_stats.hip``, ``tick_front.hip``, ``canary_rows.hip``,
``decide.hip``, ``decide_2s.hip``, ``synth.hip``);
CPU tensors run the vectorised numpy reference in
:mod:`foremast_amd.ops.reference` (the BASELINE config-1 CPU path and the
numerics oracle for tests).
"""
from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from . import reference as ref
from ._lib import LIB, check, ptr, require_native, stream_of

TEST_NAMES = ("MANN_WHITE", "WILCOXON", "KRUSKAL", "KS", "TTEST", "FRIEDMAN")
N_TESTS = len(TEST_NAMES)
SUFF = 14  # per-row sufficient statistics written by the wave kernel, read by the p-value kernel


@dataclass(frozen=True)
class PairwiseConfig:
    """Pairwise canary test settings (foremast-brain/README.md:32-38,
    deploy/foremast/3_brain/foremast-brain.yaml:74-79)."""

    algorithm: str = "ALL"          # ML_PAIRWISE_ALGORITHM: ALL | ANY | MANN_WHITE | WILCOXON | KRUSKAL | KS | TTEST | FRIEDMAN
    p_threshold: float = 0.05       # ML_PAIRWISE_THRESHOLD
    min_mann_white: int = 20        # MIN_MANN_WHITE_DATA_POINTS
    min_wilcoxon: int = 20          # MIN_WILCOXON_DATA_POINTS
    min_kruskal: int = 5            # MIN_KRUSKAL_DATA_POINTS

    def mask_and_combine(self) -> tuple[int, int]:
        a = self.algorithm.upper()
        if a == "ALL":
            return (1 << N_TESTS) - 1, 0
        if a == "ANY":
            return (1 << N_TESTS) - 1, 1
        alias = {"MANN_WHITNEY": "MANN_WHITE", "MANNWHITNEY": "MANN_WHITE", "T_TEST": "TTEST", "KS_2SAMP": "KS",
                 "FRIEDMANCHISQUARE": "FRIEDMAN", "FRIEDMAN_CHI_SQUARE": "FRIEDMAN"}
        a = alias.get(a, a)
        if a not in TEST_NAMES:
            raise ValueError(f"unknown pairwise algorithm {self.algorithm!r}")
        return 1 << TEST_NAMES.index(a), 0


def _rows(x: torch.Tensor) -> tuple[int, int]:
    check(x.dim() == 2, "expected a 2-D [rows, points] tensor")
    check(x.dtype == torch.float32, "expected float32")
    check(x.stride(1) == 1, "inner dimension must be contiguous")
    return x.shape[0], x.stride(0)


# widest pooled sample (n_cur + n_base) the wave rank-test kernel sorts in
# registers (16 values per lane: a 60-minute canary window of 8 pods per side
# at a 1-minute step); wider rows take the workgroup kernel K21 up to
# PAIRWISE_WIDE_MAX and the fp64 CPU oracle beyond
PAIRWISE_MAX = 1024
# widest pooled sample K21 (csrc/kernels/pairwise_wide.hip, kPairwiseWideMax)
# ranks in LDS, any split between the sides.  Set to PAIRWISE_MAX, the tier is
# off and every row the wave kernel cannot take goes to the oracle.
PAIRWISE_WIDE_MAX = 8192

# rows ``pairwise_tests`` has sent down each route since the last reset:
# "wave" (K4, registers of one wave), "wide" (K21), "oracle" (numpy on the host)
_ROUTE_ROWS = {"wave": 0, "wide": 0, "oracle": 0}


def route_rows() -> dict[str, int]:
    """Rows of GPU batches per pairwise route so far (a copy)."""
    return dict(_ROUTE_ROWS)


def reset_route_rows() -> None:
    for k in _ROUTE_ROWS:
        _ROUTE_ROWS[k] = 0


def pairwise_tests(cur: torch.Tensor, base: torch.Tensor, cfg: PairwiseConfig = PairwiseConfig()):
    """Returns (pvals [R,6] f32, stats [R,6] f32, diff [R] int8) in TEST_NAMES order.

    NaN / inf samples are treated as missing.  A test whose min-points gate is
    not met yields NaN and is excluded from the ALL/ANY combination.
    """
    R, ldc = _rows(cur)
    Rb, ldb = _rows(base)
    check(R == Rb, "current/baseline row mismatch")
    mask, anyc = cfg.mask_and_combine()
    if not cur.is_cuda:
        p, s, d = ref.pairwise_tests(cur.numpy(), base.numpy(), mask, anyc, cfg.p_threshold, cfg.min_mann_white,
                                     cfg.min_wilcoxon, cfg.min_kruskal)
        return torch.from_numpy(p), torch.from_numpy(s), torch.from_numpy(d)
    require_native(cur)
    n_cur, n_base = cur.shape[1], base.shape[1]
    if n_cur + n_base > PAIRWISE_MAX:
        return _pairwise_bucketed(cur, base, cfg)
    _ROUTE_ROWS["wave"] += R
    pv = torch.empty((R, N_TESTS), dtype=torch.float32, device=cur.device)
    st = torch.empty_like(pv)
    df = torch.empty((R,), dtype=torch.int8, device=cur.device)
    suff = torch.empty((R, SUFF), dtype=torch.float64, device=cur.device)
    LIB.call("fm_pairwise_tests", ptr(cur), ldc, n_cur, ptr(base), ldb, n_base, R, mask, anyc,
             float(cfg.p_threshold), cfg.min_mann_white, cfg.min_wilcoxon, cfg.min_kruskal, ptr(pv), ptr(st),
             ptr(df), ptr(suff), stream_of(cur))
    return pv, st, df


def used_width(x: torch.Tensor) -> torch.Tensor:
    """[R, n] -> [R] int64: 1 + column of the last finite sample (0 if none).
    Columns past it are padding, so slicing them off leaves every test exact."""
    idx = torch.arange(1, x.shape[1] + 1, device=x.device, dtype=torch.int64)
    return (torch.isfinite(x).to(torch.int64) * idx).amax(1) if x.shape[1] else \
        torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)


def pairwise_suff_wide(cur: torch.Tensor, base: torch.Tensor) -> torch.Tensor:
    """The 14 sufficient statistics of the pairwise tests per row ([R, 14]
    fp64, ``reference.SUFF_NAMES``) for windows of up to PAIRWISE_WIDE_MAX
    pooled columns: K21 on GPU tensors, ``reference.pairwise_suff`` on CPU
    tensors.  ``fm_pvalues`` turns them into p-values."""
    R, ldc = _rows(cur)
    Rb, ldb = _rows(base)
    check(R == Rb, "current/baseline row mismatch")
    if not cur.is_cuda:
        return torch.from_numpy(ref.pairwise_suff(cur.numpy(), base.numpy()))
    require_native(cur)
    n_cur, n_base = cur.shape[1], base.shape[1]
    check(n_cur + n_base <= PAIRWISE_WIDE_MAX,
          f"n_cur + n_base = {n_cur + n_base} columns, the workgroup rank kernel takes {PAIRWISE_WIDE_MAX}")
    suff = torch.empty((R, SUFF), dtype=torch.float64, device=cur.device)
    LIB.call("fm_pairwise_suff_wide", ptr(cur), ldc, n_cur, ptr(base), ldb, n_base, R, ptr(suff), stream_of(cur))
    return suff


def _pairwise_wide_tests(cur: torch.Tensor, base: torch.Tensor, cfg: PairwiseConfig):
    """K21 + the p-value kernel on the stream of ``cur`` (CPU tensors: the oracle)."""
    if not cur.is_cuda:
        return pairwise_tests(cur, base, cfg)
    R = cur.shape[0]
    _ROUTE_ROWS["wide"] += R
    mask, anyc = cfg.mask_and_combine()
    suff = pairwise_suff_wide(cur, base)
    pv = torch.empty((R, N_TESTS), dtype=torch.float32, device=cur.device)
    st = torch.empty_like(pv)
    df = torch.empty((R,), dtype=torch.int8, device=cur.device)
    LIB.call("fm_pvalues", ptr(suff), R, mask, anyc, float(cfg.p_threshold), cfg.min_mann_white, cfg.min_wilcoxon,
             cfg.min_kruskal, ptr(pv), ptr(st), ptr(df), stream_of(cur))
    return pv, st, df


def _bucket(lc: torch.Tensor, lb: torch.Tensor, among: torch.Tensor, cap: int) -> torch.Tensor:
    """The rows of ``among`` a kernel that takes ``cap`` pooled columns can run
    as ONE narrowed batch: those whose used widths fit the cap, and, if the
    widest current and the widest baseline of them together break it, only
    those within half the cap per side."""
    fit = among & ((lc + lb) <= cap)
    if fit.any() and int(lc[fit].max()) + int(lb[fit].max()) > cap:
        fit &= (lc <= cap // 2) & (lb <= cap // 2)
    return fit


def _pairwise_bucketed(cur: torch.Tensor, base: torch.Tensor, cfg: PairwiseConfig):
    """A batch padded wider than the register sort (n_cur + n_base > PAIRWISE_MAX):
    rows are bucketed by their own used widths into three tiers.  Rows whose
    samples fit the wave kernel (<= PAIRWISE_MAX / 2 per side, or <=
    PAIRWISE_MAX together when the whole bucket does) run it on a narrowed
    copy, exactly as they always have; of the rest, rows that fit
    PAIRWISE_WIDE_MAX by the same rule run K21 + the p-value kernel on a
    narrowed copy; only rows wider than that take the fp64 CPU oracle.  One
    wide job never moves the whole batch off the GPU and never fails it
    (ADVICE r1)."""
    R = cur.shape[0]
    lc, lb = used_width(cur).cpu(), used_width(base).cpu()
    every = torch.ones((R,), dtype=torch.bool)
    fit = _bucket(lc, lb, every, PAIRWISE_MAX)
    wide = _bucket(lc, lb, ~fit, PAIRWISE_WIDE_MAX) if PAIRWISE_WIDE_MAX > PAIRWISE_MAX else ~every
    pv = torch.full((R, N_TESTS), float("nan"), dtype=torch.float32, device=cur.device)
    st = torch.full_like(pv, float("nan"))
    df = torch.zeros((R,), dtype=torch.int8, device=cur.device)
    for rows, run in ((fit, pairwise_tests), (wide, _pairwise_wide_tests)):
        k = torch.nonzero(rows).flatten()
        if len(k):
            a, b = max(1, int(lc[k].max())), max(1, int(lb[k].max()))
            kd = k.to(cur.device)
            p1, s1, d1 = run(cur.index_select(0, kd)[:, :a].contiguous(),
                             base.index_select(0, kd)[:, :b].contiguous(), cfg)
            pv.index_copy_(0, kd, p1)
            st.index_copy_(0, kd, s1)
            df.index_copy_(0, kd, d1)
    w = torch.nonzero(~(fit | wide)).flatten()
    if len(w):
        if cur.is_cuda:
            _ROUTE_ROWS["oracle"] += len(w)
        a, b = max(1, int(lc[w].max())), max(1, int(lb[w].max()))
        wd = w.to(cur.device)
        mask, anyc = cfg.mask_and_combine()
        p2, s2, d2 = ref.pairwise_tests(cur.index_select(0, wd)[:, :a].cpu().numpy(),
                                        base.index_select(0, wd)[:, :b].cpu().numpy(), mask, anyc, cfg.p_threshold,
                                        cfg.min_mann_white, cfg.min_wilcoxon, cfg.min_kruskal)
        pv.index_copy_(0, wd, torch.from_numpy(np.asarray(p2, np.float32)).to(cur.device))
        st.index_copy_(0, wd, torch.from_numpy(np.asarray(s2, np.float32)).to(cur.device))
        df.index_copy_(0, wd, torch.from_numpy(np.asarray(d2).astype(np.int8)).to(cur.device))
    return pv, st, df


@dataclass(frozen=True)
class EffectGate:
    """Effect-size gate of the pairwise verdict (K19, docs/BRAIN_SPEC.md): a row
    whose tests say "different" keeps that verdict only if the difference is
    also large enough.  All zero / false = off."""

    min_effect: float = 0.0         # ML_PAIRWISE_MIN_EFFECT: |Cliff's delta| below this fails
    min_shift: float = 0.0          # ML_PAIRWISE_MIN_SHIFT: |Hodges-Lehmann shift| as a fraction of |baseline median|
    min_shift_abs: float = 0.0      # ML_PAIRWISE_MIN_SHIFT_ABS: the same in metric units (added to the fraction)
    directional: bool = False       # ML_PAIRWISE_DIRECTIONAL: a shift away from a one-sided bound fails

    def __post_init__(self):
        if not 0.0 <= float(self.min_effect) <= 1.0:      # (NaN fails the comparison too)
            raise ValueError(f"min_effect must be within [0, 1], got {self.min_effect!r}")
        for name in ("min_shift", "min_shift_abs"):
            v = float(getattr(self, name))
            if not (v >= 0.0 and v != float("inf")):
                raise ValueError(f"{name} must be finite and >= 0, got {v!r}")

    @property
    def enabled(self) -> bool:
        return bool(self.min_effect or self.min_shift or self.min_shift_abs or self.directional)

    @classmethod
    def from_config(cls, cfg) -> "EffectGate":
        """The gate of a ``BrainConfig`` (its four ``pairwise_*`` effect settings)."""
        return cls(float(cfg.pairwise_min_effect), float(cfg.pairwise_min_shift), float(cfg.pairwise_min_shift_abs),
                   bool(cfg.pairwise_directional))


@dataclass
class EffectResult:
    effect: torch.Tensor                 # [R, 4] fp32: Cliff's delta, Hodges-Lehmann shift, baseline median, N
    counts: torch.Tensor                 # [R, 2] int32: #{d > 0}, #{d < 0}
    passed: torch.Tensor                 # [R] int8
    pvals_gated: torch.Tensor | None     # [R, 6] fp32: pvals where passed, NaN elsewhere (None without pvals)


def alloc_effect(R: int, device, with_pvals: bool = True) -> EffectResult:
    return EffectResult(
        effect=torch.empty((R, 4), dtype=torch.float32, device=device),
        counts=torch.empty((R, 2), dtype=torch.int32, device=device),
        passed=torch.empty((R,), dtype=torch.int8, device=device),
        pvals_gated=torch.empty((R, N_TESTS), dtype=torch.float32, device=device) if with_pvals else None,
    )


# rows ``pairwise_effect`` has sent down each route since the last reset:
# "wave" (K19), "wide" (K28), "oracle" (the numpy definition on the host)
_EFFECT_ROUTE_ROWS = {"wave": 0, "wide": 0, "oracle": 0}


def effect_route_rows() -> dict[str, int]:
    """Rows of GPU batches per effect-gate route so far (a copy)."""
    return dict(_EFFECT_ROUTE_ROWS)


def reset_effect_route_rows() -> None:
    for k in _EFFECT_ROUTE_ROWS:
        _EFFECT_ROUTE_ROWS[k] = 0


def pairwise_effect(cur: torch.Tensor, base: torch.Tensor, gate: EffectGate = EffectGate(),
                    bound: torch.Tensor | None = None, M: int = 1, pvals: torch.Tensor | None = None,
                    out: EffectResult | None = None, tier: str = "auto") -> EffectResult:
    """Effect size of current vs baseline per row and the gate's verdict on it.

    ``bound`` (int32 [M], the bound code of metric r % M; needed when the gate
    is directional) and ``pvals`` ([R, 6] fp32, optional: ``pvals_gated`` is
    its copy with the failing rows set to NaN, which ``fm_decide_services``
    reads as "no test applies").  CPU tensors run the numpy reference, GPU
    tensors K19 up to PAIRWISE_MAX pooled columns and its workgroup tier K28
    up to PAIRWISE_WIDE_MAX (``tier="wide"`` runs K28 for any batch that fits
    it); a batch padded wider than that is bucketed by the rows' own used
    widths like the pairwise tests."""
    R, ldc = _rows(cur)
    Rb, ldb = _rows(base)
    check(R == Rb, "current/baseline row mismatch")
    check(M >= 1, "M must be >= 1")
    check(tier in ("auto", "wide"), "tier is 'auto' or 'wide'")
    check(not gate.directional or (bound is not None and bound.numel() == M),
          "a directional gate needs the per-metric bound codes [M]")
    if pvals is not None:
        check(pvals.shape == (R, N_TESTS) and pvals.dtype == torch.float32 and pvals.is_contiguous()
              and pvals.device == cur.device, "pvals must be a contiguous fp32 [R, 6] tensor on the samples' device")
    if not cur.is_cuda:
        eff, cnt = ref.pairwise_effect(cur.numpy(), base.numpy())
        bpr = None if bound is None else bound.numpy()[np.arange(R) % M]
        ps = ref.effect_gate(eff, bpr, gate.min_effect, gate.min_shift, gate.min_shift_abs, gate.directional)
        pg = None
        if pvals is not None:
            pg = torch.from_numpy(np.where(ps[:, None] != 0, pvals.numpy(), np.float32(np.nan)).astype(np.float32))
        return EffectResult(torch.from_numpy(eff), torch.from_numpy(cnt), torch.from_numpy(ps), pg)
    require_native(cur)
    n_cur, n_base = cur.shape[1], base.shape[1]
    if n_cur + n_base > PAIRWISE_WIDE_MAX:
        return _effect_bucketed(cur, base, gate, bound, M, pvals)
    wide = tier == "wide" or n_cur + n_base > PAIRWISE_MAX
    _EFFECT_ROUTE_ROWS["wide" if wide else "wave"] += R
    o = out if out is not None else alloc_effect(R, cur.device, pvals is not None)
    if bound is not None:
        check(bound.is_cuda and bound.dtype == torch.int32 and bound.is_contiguous(), "bound must be a device int32 [M]")
    check(pvals is None or o.pvals_gated is not None, "out has no pvals_gated buffer")
    LIB.call("fm_pairwise_effect_wide" if wide else "fm_pairwise_effect", ptr(cur), ldc, n_cur, ptr(base), ldb,
             n_base, R, float(gate.min_effect),
             float(gate.min_shift), float(gate.min_shift_abs), int(gate.directional), ptr(bound), M, ptr(pvals),
             ptr(o.effect), ptr(o.counts), ptr(o.passed), ptr(o.pvals_gated) if pvals is not None else None,
             stream_of(cur))
    return o


def gate_diff(diff: torch.Tensor, cur: torch.Tensor, base: torch.Tensor, gate: EffectGate, bound: torch.Tensor,
              M: int) -> torch.Tensor:
    """``diff & passed`` for the op-by-op model paths (``diff`` from
    ``pairwise_tests``; row r is judged by bound code ``bound[r % M]``)."""
    if not gate.enabled:
        return diff
    return diff & pairwise_effect(cur, base, gate, bound.contiguous(), M).passed


def _effect_bucketed(cur, base, gate: EffectGate, bound, M: int, pvals) -> EffectResult:
    """A batch padded wider than PAIRWISE_WIDE_MAX pooled columns: rows
    bucketed by their own used widths exactly as ``_pairwise_bucketed`` does;
    rows that fit run K19 on a narrowed copy, of the rest those that fit
    PAIRWISE_WIDE_MAX run K28 the same way, only really wider rows the numpy
    definition on the host.  The gate is per row, so it is evaluated once over
    the assembled effects (bound codes follow the ORIGINAL row index r % M)."""
    R = cur.shape[0]
    dev = cur.device
    lc, lb = used_width(cur).cpu(), used_width(base).cpu()
    every = torch.ones((R,), dtype=torch.bool)
    fit = _bucket(lc, lb, every, PAIRWISE_MAX)
    wide = _bucket(lc, lb, ~fit, PAIRWISE_WIDE_MAX)
    eff = torch.empty((R, 4), dtype=torch.float32, device=dev)
    cnt = torch.empty((R, 2), dtype=torch.int32, device=dev)
    for rows, tier in ((fit, "auto"), (wide, "wide")):
        k = torch.nonzero(rows).flatten()
        if len(k):
            a, b = max(1, int(lc[k].max())), max(1, int(lb[k].max()))
            kd = k.to(dev)
            r1 = pairwise_effect(cur.index_select(0, kd)[:, :a].contiguous(),
                                 base.index_select(0, kd)[:, :b].contiguous(), tier=tier)
            eff.index_copy_(0, kd, r1.effect)
            cnt.index_copy_(0, kd, r1.counts)
    w = torch.nonzero(~(fit | wide)).flatten()
    if len(w):
        _EFFECT_ROUTE_ROWS["oracle"] += len(w)
        a, b = max(1, int(lc[w].max())), max(1, int(lb[w].max()))
        wd = w.to(dev)
        e2, c2 = ref.pairwise_effect(cur.index_select(0, wd)[:, :a].cpu().numpy(),
                                     base.index_select(0, wd)[:, :b].cpu().numpy())
        eff.index_copy_(0, wd, torch.from_numpy(e2).to(dev))
        cnt.index_copy_(0, wd, torch.from_numpy(c2).to(dev))
    # the gate over the assembled rows, on the host: this path already
    # synchronises for the widths, and the arithmetic is the reference's fp32
    bpr = None if bound is None else bound.cpu().numpy()[np.arange(R) % M]
    ps = ref.effect_gate(eff.cpu().numpy(), bpr, gate.min_effect, gate.min_shift, gate.min_shift_abs,
                         gate.directional)
    passed = torch.from_numpy(ps).to(dev)
    pg = None
    if pvals is not None:
        pg = torch.where(passed[:, None] != 0, pvals, torch.full_like(pvals, float("nan")))
    return EffectResult(eff, cnt, passed, pg)


# widest side (columns) K27's wave tier sorts in registers (csrc/kernels/pairwise_scale.hip kScaleWaveMax); wider
# batches take its workgroup tier up to PAIRWISE_WIDE_MAX pooled columns and the numpy definition beyond
SCALE_WAVE_MAX = 1024
SCALE_TESTS = {"": "", "OFF": "", "BROWN_FORSYTHE": "BROWN_FORSYTHE", "LEVENE": "BROWN_FORSYTHE"}


@dataclass(frozen=True)
class ScaleTest:
    """Pairwise scale test (K27, docs/BRAIN_SPEC.md 4.2): Brown-Forsythe on the
    spread of current vs baseline.  A row it flags counts as "different"
    whatever the location tests (and the effect gate) say.  ``test == ""`` = off."""

    test: str = ""                  # ML_PAIRWISE_SCALE_TEST: "" | OFF | BROWN_FORSYTHE (alias LEVENE)
    p_threshold: float = 0.05       # ML_PAIRWISE_THRESHOLD
    min_points: int = 20            # MIN_SCALE_DATA_POINTS: finite samples needed on each side
    min_ratio: float = 1.0          # ML_PAIRWISE_SCALE_MIN_RATIO: mean deviation of current / baseline, >= 1
    both: bool = False              # ML_PAIRWISE_SCALE_BOTH: a narrower current window (ratio <= 1 / min_ratio) too

    def __post_init__(self):
        name = str(self.test or "").strip().upper()
        if name not in SCALE_TESTS:
            raise ValueError(f"unknown pairwise scale test {self.test!r} (BROWN_FORSYTHE, LEVENE or OFF)")
        object.__setattr__(self, "test", SCALE_TESTS[name])
        r = float(self.min_ratio)
        if not (r >= 1.0 and r != float("inf")):          # (NaN fails the comparison too)
            raise ValueError(f"min_ratio must be finite and >= 1, got {self.min_ratio!r}")
        if int(self.min_points) < 0:
            raise ValueError(f"min_points must be >= 0, got {self.min_points!r}")

    @property
    def enabled(self) -> bool:
        return self.test != ""

    @classmethod
    def from_config(cls, cfg) -> "ScaleTest":
        """The scale test of a ``BrainConfig`` (its ``pairwise_scale_*`` settings and the pairwise threshold)."""
        return cls(cfg.pairwise_scale_test, float(cfg.pairwise_threshold), int(cfg.min_scale_points),
                   float(cfg.pairwise_scale_min_ratio), bool(cfg.pairwise_scale_both))


@dataclass
class ScaleResult:
    scale: torch.Tensor                  # [R, 6] fp32: W, p, ratio, current median, baseline median, N
    scale_diff: torch.Tensor             # [R] int8
    pvals_scaled: torch.Tensor | None    # [R, 6] fp32: pvals, 0 in the six columns of a flagged row (None without pvals)
    moments: torch.Tensor | None = None  # [R, 8] fp64 scratch of the kernel


def alloc_scale(R: int, device, with_pvals: bool = True) -> ScaleResult:
    return ScaleResult(
        scale=torch.empty((R, 6), dtype=torch.float32, device=device),
        scale_diff=torch.empty((R,), dtype=torch.int8, device=device),
        pvals_scaled=torch.empty((R, N_TESTS), dtype=torch.float32, device=device) if with_pvals else None,
        moments=torch.empty((R, 8), dtype=torch.float64, device=device),
    )


def _scale_host(cur, base, test: ScaleTest):
    """The numpy definition: (scale [R, 6] fp32, scale_diff [R] int8)."""
    s = ref.pairwise_scale(cur, base, test.min_points)
    return s, ref.scale_verdict(s, test.p_threshold, test.min_ratio, test.both)


def _force_pvals(pvals: torch.Tensor, flagged: torch.Tensor) -> torch.Tensor:
    return torch.where(flagged[:, None] != 0, torch.zeros_like(pvals), pvals)


def pairwise_scale(cur: torch.Tensor, base: torch.Tensor, test: ScaleTest = ScaleTest("BROWN_FORSYTHE"),
                   pvals: torch.Tensor | None = None, out: ScaleResult | None = None,
                   tier: str = "auto") -> ScaleResult:
    """Brown-Forsythe scale test of current vs baseline per row and its verdict.

    ``pvals`` ([R, 6] fp32, optional: what the decision would read, the effect
    gate's copy where it ran): ``pvals_scaled`` is its copy with 0 in all six
    columns of a flagged row, which every ``ML_PAIRWISE_ALGORITHM`` reads as
    "different".  CPU tensors run the numpy definition, GPU tensors K27: its
    wave tier while each side has at most SCALE_WAVE_MAX columns, its
    workgroup tier up to PAIRWISE_WIDE_MAX pooled columns (``tier="wide"``
    runs it for any batch that fits), and a batch padded wider than that is
    bucketed by the rows' own used widths like the pairwise tests."""
    R, ldc = _rows(cur)
    Rb, ldb = _rows(base)
    check(R == Rb, "current/baseline row mismatch")
    check(tier in ("auto", "wide"), "tier is 'auto' or 'wide'")
    if pvals is not None:
        check(pvals.shape == (R, N_TESTS) and pvals.dtype == torch.float32 and pvals.is_contiguous()
              and pvals.device == cur.device, "pvals must be a contiguous fp32 [R, 6] tensor on the samples' device")
    if not cur.is_cuda:
        s, d = _scale_host(cur.numpy(), base.numpy(), test)
        sd = torch.from_numpy(d)
        return ScaleResult(torch.from_numpy(s), sd, None if pvals is None else _force_pvals(pvals, sd))
    require_native(cur)
    n_cur, n_base = cur.shape[1], base.shape[1]
    wave = tier == "auto" and max(n_cur, n_base) <= SCALE_WAVE_MAX
    if not wave and n_cur + n_base > PAIRWISE_WIDE_MAX:
        return _scale_bucketed(cur, base, test, pvals)
    o = out if out is not None else alloc_scale(R, cur.device, pvals is not None)
    check(pvals is None or o.pvals_scaled is not None, "out has no pvals_scaled buffer")
    if o.moments is None:
        o.moments = torch.empty((R, 8), dtype=torch.float64, device=cur.device)
    f = np.float32
    LIB.call("fm_pairwise_scale", ptr(cur), ldc, n_cur, ptr(base), ldb, n_base, R, int(test.min_points),
             float(test.p_threshold), float(test.min_ratio), float(f(1.0) / f(test.min_ratio)), int(test.both),
             0 if tier == "auto" else 2, ptr(pvals), ptr(o.moments), ptr(o.scale), ptr(o.scale_diff),
             ptr(o.pvals_scaled) if pvals is not None else None, stream_of(cur))
    return o


def scale_diff(diff: torch.Tensor, cur: torch.Tensor, base: torch.Tensor, test: ScaleTest) -> torch.Tensor:
    """``diff | flagged`` for the op-by-op model paths (``diff`` from
    ``pairwise_tests``, after ``gate_diff`` where the effect gate is on: the
    gate never clears a scale verdict)."""
    if not test.enabled:
        return diff
    return diff | pairwise_scale(cur, base, test).scale_diff.to(diff.dtype)


def _scale_bucketed(cur, base, test: ScaleTest, pvals) -> ScaleResult:
    """A batch padded wider than K27 takes: rows bucketed by their own used
    widths exactly as ``_pairwise_bucketed`` does (the wave tier, then the
    workgroup tier, each on a narrowed copy); only rows really wider than
    PAIRWISE_WIDE_MAX run the numpy definition on the host."""
    R = cur.shape[0]
    dev = cur.device
    lc, lb = used_width(cur).cpu(), used_width(base).cpu()
    every = torch.ones((R,), dtype=torch.bool)
    fit = _bucket(lc, lb, every, PAIRWISE_MAX)
    wide = _bucket(lc, lb, ~fit, PAIRWISE_WIDE_MAX)
    sc = torch.empty((R, 6), dtype=torch.float32, device=dev)
    sd = torch.empty((R,), dtype=torch.int8, device=dev)
    for rows in (fit, wide):
        k = torch.nonzero(rows).flatten()
        if len(k):
            a, b = max(1, int(lc[k].max())), max(1, int(lb[k].max()))
            kd = k.to(dev)
            r1 = pairwise_scale(cur.index_select(0, kd)[:, :a].contiguous(),
                                base.index_select(0, kd)[:, :b].contiguous(), test)
            sc.index_copy_(0, kd, r1.scale)
            sd.index_copy_(0, kd, r1.scale_diff)
    w = torch.nonzero(~(fit | wide)).flatten()
    if len(w):
        a, b = max(1, int(lc[w].max())), max(1, int(lb[w].max()))
        wd = w.to(dev)
        s2, d2 = _scale_host(cur.index_select(0, wd)[:, :a].cpu().numpy(),
                             base.index_select(0, wd)[:, :b].cpu().numpy(), test)
        sc.index_copy_(0, wd, torch.from_numpy(s2).to(dev))
        sd.index_copy_(0, wd, torch.from_numpy(d2).to(dev))
    return ScaleResult(sc, sd, None if pvals is None else _force_pvals(pvals, sd))


# most pods per row K29 takes (csrc/kernels/pairwise_pods.hip kPodMax: one lane per pod in its finishing pass)
POD_MAX = 64
POD_TESTS = {"": "", "OFF": "", "KRUSKAL_DUNN": "KRUSKAL_DUNN"}


@dataclass(frozen=True)
class PodTest:
    """Per-pod canary test (K29, docs/BRAIN_SPEC.md 4.3): Kruskal-Wallis over the
    baseline and the canary's pods, then Dunn's contrast of every pod against
    the baseline.  A row it flags counts as "different" whatever the pooled
    tests say; it never clears a verdict.  ``test == ""`` = off."""

    test: str = ""                  # ML_PAIRWISE_POD_TEST: "" | OFF | KRUSKAL_DUNN
    p_threshold: float = 0.05       # ML_PAIRWISE_THRESHOLD (the omnibus and the worst pod's p-value)
    min_points: int = 5             # MIN_POD_DATA_POINTS: finite samples a pod, and the baseline, need

    def __post_init__(self):
        name = str(self.test or "").strip().upper()
        if name not in POD_TESTS:
            raise ValueError(f"unknown pairwise pod test {self.test!r} (KRUSKAL_DUNN or OFF)")
        object.__setattr__(self, "test", POD_TESTS[name])
        if int(self.min_points) < 1:
            raise ValueError(f"min_points must be >= 1, got {self.min_points!r}")

    @property
    def enabled(self) -> bool:
        return self.test != ""

    @classmethod
    def from_config(cls, cfg) -> "PodTest":
        """The pod test of a ``BrainConfig`` (``pairwise_pod_test``, ``min_pod_points`` and the pairwise threshold)."""
        return cls(cfg.pairwise_pod_test, float(cfg.pairwise_threshold), int(cfg.min_pod_points))


@dataclass
class PodResult:
    pods: torch.Tensor                   # [R, 6] fp32: H, p_H, z_worst, p_worst, worst, k
    pod_z: torch.Tensor                  # [R, G] fp32: Dunn's z of every kept pod against the baseline
    pod_n: torch.Tensor                  # [R, G] int32: finite samples of every kept pod
    pod_rank2: torch.Tensor              # [R, G] int64: doubled rank sums
    base_rank2: torch.Tensor             # [R] int64
    tie: torch.Tensor                    # [R] int64: sum of t^3 - t over tie runs
    pod_diff: torch.Tensor               # [R] int8

    def tensors(self) -> tuple:
        return (self.pods, self.pod_z, self.pod_n, self.pod_rank2, self.base_rank2, self.tie, self.pod_diff)


def alloc_pods(R: int, G: int, device, fill: bool = False) -> PodResult:
    """Output buffers of K29, which writes all of them for every row; ``fill``:
    holding what a row without pods gets (NaN, worst = -1, zeros)."""
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)  # noqa: E731
    o = PodResult(new((R, 6), torch.float32), new((R, G), torch.float32), new((R, G), torch.int32),
                  new((R, G), torch.int64), new((R,), torch.int64), new((R,), torch.int64), new((R,), torch.int8))
    if fill:
        for t in o.tensors():
            t.fill_(float("nan") if t.dtype == torch.float32 else 0)
        o.pods[:, 4], o.pods[:, 5] = -1.0, 0.0
    return o


# rows ``pairwise_pods`` has sent down each route since the last reset:
# "wave" / "wide" (K29's tiers), "host" (the numpy definition)
_POD_ROUTE_ROWS = {"wave": 0, "wide": 0, "host": 0}


def pod_route_rows() -> dict[str, int]:
    """Rows of GPU batches per pod-test route so far (a copy)."""
    return dict(_POD_ROUTE_ROWS)


def reset_pod_route_rows() -> None:
    for k in _POD_ROUTE_ROWS:
        _POD_ROUTE_ROWS[k] = 0


def _pods_host(cur, seg_end, base, test: PodTest) -> PodResult:
    """The numpy definition on host arrays, as CPU tensors."""
    o = ref.pairwise_pods(cur, seg_end, base, test.min_points)
    return PodResult(*(torch.from_numpy(a) for a in o), torch.from_numpy(ref.pods_verdict(o[0], test.p_threshold)))


def pairwise_pods(cur: torch.Tensor, seg_end: torch.Tensor, base: torch.Tensor,
                  test: PodTest = PodTest("KRUSKAL_DUNN"), tier: str = "auto",
                  out: PodResult | None = None) -> PodResult:
    """Per-pod test of current vs baseline per row and its verdict.

    ``cur`` [R, n_cur] is pod-major; ``seg_end`` [R, G] int32 holds the column
    at which pod g's segment ends (cumulative; an empty pod repeats the
    previous end).  CPU tensors run the numpy definition, GPU tensors K29: its
    wave tier up to PAIRWISE_MAX pooled columns, its workgroup tier up to
    PAIRWISE_WIDE_MAX (``tier="wide"`` runs it for any batch that fits); a
    batch padded wider than that, or with more than POD_MAX pod columns, is
    bucketed by the rows' own used widths like the pairwise tests, and only
    rows really wider, or with more than POD_MAX pods, run the definition on
    the host."""
    R, ldc = _rows(cur)
    Rb, ldb = _rows(base)
    check(R == Rb, "current/baseline row mismatch")
    check(tier in ("auto", "wide"), "tier is 'auto' or 'wide'")
    check(seg_end.dim() == 2 and seg_end.shape[0] == R and seg_end.dtype == torch.int32 and seg_end.is_contiguous()
          and seg_end.device == cur.device, "seg_end must be a contiguous int32 [R, G] tensor on the samples' device")
    if not cur.is_cuda:
        return _pods_host(cur.numpy(), seg_end.numpy(), base.numpy(), test)
    require_native(cur)
    n_cur, n_base, G = cur.shape[1], base.shape[1], seg_end.shape[1]
    if n_cur + n_base > PAIRWISE_WIDE_MAX or G > POD_MAX:
        return _pods_bucketed(cur, seg_end, base, test)
    wide = tier == "wide" or n_cur + n_base > PAIRWISE_MAX
    _POD_ROUTE_ROWS["wide" if wide else "wave"] += R
    o = out if out is not None else alloc_pods(R, G, cur.device)
    LIB.call("fm_pairwise_pods", ptr(cur), ldc, n_cur, ptr(seg_end) if G else None, G, ptr(base), ldb, n_base, R,
             int(test.min_points), float(test.p_threshold), 2 if wide else 0, ptr(o.pods), ptr(o.pod_z), ptr(o.pod_n),
             ptr(o.pod_rank2), ptr(o.base_rank2), ptr(o.tie), ptr(o.pod_diff), stream_of(cur))
    return o


def pods_diff(diff: torch.Tensor, cur: torch.Tensor, seg_end: torch.Tensor, base: torch.Tensor,
              test: PodTest) -> torch.Tensor:
    """``diff | pod_diff`` for the op-by-op model paths (``diff`` from
    ``pairwise_tests``, after ``gate_diff`` and ``scale_diff``: the pod test
    only ever sets a verdict)."""
    if not test.enabled:
        return diff
    return diff | pairwise_pods(cur, seg_end, base, test).pod_diff.to(diff.dtype)


def _pods_bucketed(cur, seg_end, base, test: PodTest) -> PodResult:
    """A batch padded wider than K29 takes, or with more than POD_MAX pod
    columns: rows bucketed by their own used widths exactly as
    ``_pairwise_bucketed`` does (the wave tier, then the workgroup tier, each
    on a narrowed copy whose segment ends are cut at the copy's width: the
    columns cut off hold no finite sample).  A row whose pods past POD_MAX are
    all empty loses only those columns; rows with more pods, and rows really
    wider than PAIRWISE_WIDE_MAX, run the numpy definition on the host."""
    R, G = seg_end.shape
    dev = cur.device
    Gk = min(G, POD_MAX)
    lc, lb = used_width(cur).cpu(), used_width(base).cpu()
    many = (seg_end[:, POD_MAX - 1] != seg_end[:, -1]).cpu() if G > POD_MAX else torch.zeros((R,), dtype=torch.bool)
    fit = _bucket(lc, lb, ~many, PAIRWISE_MAX)
    wide = _bucket(lc, lb, ~many & ~fit, PAIRWISE_WIDE_MAX)
    o = alloc_pods(R, G, dev, fill=True)

    def put(k, r):
        for dst, src in zip(o.tensors(), r.tensors()):
            if dst.dim() == 2 and dst.shape[1] == G:
                dst[k, :src.shape[1]] = src.to(dev)
            else:
                dst[k] = src.to(dev)

    for rows in (fit, wide):
        k = torch.nonzero(rows).flatten()
        if len(k):
            a, b = max(1, int(lc[k].max())), max(1, int(lb[k].max()))
            kd = k.to(dev)
            put(kd, pairwise_pods(cur.index_select(0, kd)[:, :a].contiguous(),
                                  seg_end.index_select(0, kd)[:, :Gk].clamp(max=a).contiguous(),
                                  base.index_select(0, kd)[:, :b].contiguous(), test))
    w = torch.nonzero(~(fit | wide)).flatten()
    if len(w):
        _POD_ROUTE_ROWS["host"] += len(w)
        a, b = max(1, int(lc[w].max())), max(1, int(lb[w].max()))
        wd = w.to(dev)
        put(wd, _pods_host(cur.index_select(0, wd)[:, :a].cpu().numpy(),
                           seg_end.index_select(0, wd).clamp(max=a).cpu().numpy(),
                           base.index_select(0, wd)[:, :b].cpu().numpy(), test))
    return o


# most members per group K30 takes (csrc/kernels/pairwise_joint.hip kJointMembers: one wave per member)
JOINT_MAX_K = ref.JOINT_MAX_K
JOINT_TESTS = {"": "", "OFF": "", "RANK_SUM": "RANK_SUM"}


@dataclass(frozen=True)
class JointTest:
    """Joint multi-metric canary test (K30, docs/BRAIN_SPEC.md 4.4): the
    Puri-Sen multivariate rank-sum statistic over the metrics of a job.  A
    group it flags counts as "different" on every member row whatever the
    per-row tests say; it never clears a verdict.  ``test == ""`` = off."""

    test: str = ""                  # ML_PAIRWISE_JOINT_TEST: "" | OFF | RANK_SUM
    p_threshold: float = 0.05       # ML_PAIRWISE_THRESHOLD
    min_points: int = 20            # MIN_JOINT_DATA_POINTS: kept columns each side needs

    def __post_init__(self):
        name = str(self.test or "").strip().upper()
        if name not in JOINT_TESTS:
            raise ValueError(f"unknown pairwise joint test {self.test!r} (RANK_SUM or OFF)")
        object.__setattr__(self, "test", JOINT_TESTS[name])
        if int(self.min_points) < 1:
            raise ValueError(f"min_points must be >= 1, got {self.min_points!r}")

    @property
    def enabled(self) -> bool:
        return self.test != ""

    @classmethod
    def from_config(cls, cfg) -> "JointTest":
        """The joint test of a ``BrainConfig`` (``pairwise_joint_test``, ``min_joint_points`` and the pairwise
        threshold)."""
        return cls(cfg.pairwise_joint_test, float(cfg.pairwise_threshold), int(cfg.min_joint_points))


@dataclass
class JointResult:
    joint: torch.Tensor                  # [G, 6] fp32: L, p, dof, z_worst, worst, N
    n12: torch.Tensor                    # [G, 2] int32: kept current / baseline columns
    T: torch.Tensor                      # [G, 8] int64: centred doubled rank sums of the current side
    A: torch.Tensor                      # [G, 8, 8] int64: Gram matrix of the centred doubled ranks
    member_z: torch.Tensor               # [G, 8] fp32: every member's marginal z
    joint_diff: torch.Tensor             # [G] int8

    def tensors(self) -> tuple:
        return (self.joint, self.n12, self.T, self.A, self.member_z, self.joint_diff)


def alloc_joint(G: int, device) -> JointResult:
    """Output buffers of K30, which writes all of them for every group."""
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)  # noqa: E731
    return JointResult(new((G, 6), torch.float32), new((G, 2), torch.int32), new((G, JOINT_MAX_K), torch.int64),
                       new((G, JOINT_MAX_K, JOINT_MAX_K), torch.int64), new((G, JOINT_MAX_K), torch.float32),
                       new((G,), torch.int8))


# groups ``pairwise_joint`` has sent down each route since the last reset:
# "wave" (K30), "host" (the numpy definition)
_JOINT_ROUTE_ROWS = {"wave": 0, "host": 0}


def joint_route_rows() -> dict[str, int]:
    """Groups of GPU batches per joint-test route so far (a copy)."""
    return dict(_JOINT_ROUTE_ROWS)


def reset_joint_route_rows() -> None:
    for k in _JOINT_ROUTE_ROWS:
        _JOINT_ROUTE_ROWS[k] = 0


def _joint_host(cur, base, rows, K, test: JointTest) -> JointResult:
    """The numpy definition on host arrays, as CPU tensors."""
    o = ref.pairwise_joint(cur, base, rows, K, test.min_points)
    return JointResult(*(torch.from_numpy(a) for a in o), torch.from_numpy(ref.joint_verdict(o[0], test.p_threshold)))


def pairwise_joint(cur: torch.Tensor, base: torch.Tensor, rows: torch.Tensor, K: torch.Tensor,
                   test: JointTest = JointTest("RANK_SUM"), out: JointResult | None = None) -> JointResult:
    """Joint rank-sum test of current vs baseline per group and its verdict.

    ``rows`` [G, 8] int32 (-1 padded) names the member rows of every group,
    ``K`` [G] their number (1..8), as ``zoo.mvn_groups`` makes them; column c
    of every member of a group is the same sample.  CPU tensors run the numpy
    definition, GPU tensors K30 for up to PAIRWISE_MAX pooled columns.  A batch
    padded wider than that is narrowed by the used widths of the groups' rows
    (the columns cut off are missing in every member), and only groups really
    wider run the definition on the host."""
    R, ldc = _rows(cur)
    Rb, ldb = _rows(base)
    check(R == Rb, "current/baseline row mismatch")
    check(rows.dim() == 2 and rows.shape[1] == JOINT_MAX_K and rows.dtype == torch.int32 and rows.is_contiguous()
          and rows.device == cur.device, "rows must be a contiguous int32 [G, 8] tensor on the samples' device")
    G = rows.shape[0]
    check(K.dim() == 1 and K.shape[0] == G and not K.is_floating_point(), "K must be an integer [G] tensor")
    K = K.to(device=cur.device, dtype=torch.int32).contiguous()
    if not cur.is_cuda:
        check(G == 0 or (int(K.min()) >= 1 and int(K.max()) <= JOINT_MAX_K), "K must lie in 1..8")
        return _joint_host(cur.numpy(), base.numpy(), rows.numpy(), K.numpy(), test)
    require_native(cur)
    n_cur, n_base = cur.shape[1], base.shape[1]
    if n_cur + n_base > PAIRWISE_MAX:
        return _joint_bucketed(cur, base, rows, K, test)
    _JOINT_ROUTE_ROWS["wave"] += G
    o = out if out is not None else alloc_joint(G, cur.device)
    LIB.call("fm_pairwise_joint", ptr(cur), ldc, n_cur, ptr(base), ldb, n_base, R, ptr(rows), ptr(K), G,
             int(test.min_points), float(test.p_threshold), ptr(o.joint), ptr(o.n12), ptr(o.T), ptr(o.A),
             ptr(o.member_z), ptr(o.joint_diff), stream_of(cur))
    return o


def joint_diff(diff: torch.Tensor, cur: torch.Tensor, base: torch.Tensor, rows: torch.Tensor, K: torch.Tensor,
               test: JointTest) -> torch.Tensor:
    """``diff`` with the verdict of every group ORed into all of its member
    rows, for the op-by-op model paths (``diff`` from ``pairwise_tests``, after
    ``gate_diff``, ``scale_diff`` and ``pods_diff``: the joint test only ever
    sets a verdict).  ``diff`` itself when the test is off or there is no group."""
    if not test.enabled or rows.shape[0] == 0:
        return diff
    hit = pairwise_joint(cur, base, rows, K, test).joint_diff.to(device=diff.device, dtype=diff.dtype)
    member = (torch.arange(JOINT_MAX_K, device=diff.device)[None, :] < K.to(diff.device)[:, None]) & (rows >= 0)
    flagged = torch.zeros_like(diff).index_put_((rows[member].long(),), hit[:, None].expand(-1, JOINT_MAX_K)[member],
                                                accumulate=True)
    return diff | (flagged > 0).to(diff.dtype)


def _joint_bucketed(cur, base, rows, K, test: JointTest) -> JointResult:
    """A batch padded wider than K30 takes: a group is as wide as the widest
    used width among its member rows, per side.  The groups that fit
    PAIRWISE_MAX by ``_bucket``'s rule run K30 on the batch cut to their
    widths (a view: a column cut off is missing in every member of such a
    group); groups really
    wider run the numpy definition on the host, on their own rows."""
    G = rows.shape[0]
    dev = cur.device
    member = (torch.arange(JOINT_MAX_K, device=dev)[None, :] < K[:, None]) & (rows >= 0)
    at = rows.clamp(min=0).long()
    width = lambda x: (used_width(x)[at] * member).amax(1).cpu()  # noqa: E731
    lc, lb = width(cur), width(base)
    o = alloc_joint(G, dev)
    left = (lc + lb) <= PAIRWISE_MAX
    host = ~left
    while left.any():
        # (groups that fit alone but not next to each other, a wide current beside a wide baseline, take turns)
        fit = _bucket(lc, lb, left, PAIRWISE_MAX)
        if not fit.any():
            fit = left & (torch.cumsum(left.to(torch.int64), 0) == 1)
        left = left & ~fit
        k = torch.nonzero(fit).flatten()
        a, b = max(1, int(lc[k].max())), max(1, int(lb[k].max()))
        kd = k.to(dev)
        r = pairwise_joint(cur[:, :a], base[:, :b], rows.index_select(0, kd).contiguous(), K.index_select(0, kd), test)
        for dst, src in zip(o.tensors(), r.tensors()):
            dst[kd] = src
    w = torch.nonzero(host).flatten()
    if len(w):
        _JOINT_ROUTE_ROWS["host"] += len(w)
        wd = w.to(dev)
        # the host gets the member rows alone, renumbered in group order
        sel = member.index_select(0, wd)
        idx = at.index_select(0, wd)[sel]
        sub = torch.full((len(w), JOINT_MAX_K), -1, dtype=torch.int32)
        sub[sel.cpu()] = torch.arange(len(idx), dtype=torch.int32)
        a, b = max(1, int(lc[w].max())), max(1, int(lb[w].max()))
        r = _joint_host(cur.index_select(0, idx)[:, :a].cpu().numpy(), base.index_select(0, idx)[:, :b].cpu().numpy(),
                        sub.numpy(), K.index_select(0, wd).cpu().numpy(), test)
        for dst, src in zip(o.tensors(), r.tensors()):
            dst[wd] = src.to(dev)
    return o


DRIFT_TESTS = {"": "", "OFF": "", "MANN_KENDALL": "MANN_KENDALL"}


@dataclass(frozen=True)
class DriftTest:
    """Drift canary test (K31, docs/BRAIN_SPEC.md 4.5): the Mann-Kendall trend of
    the canary's samples over time, stratified by pod, against the baseline's
    own trend.  A row it flags counts as "different" whatever the other tests
    say; it never clears a verdict.  ``test == ""`` = off."""

    test: str = ""                  # ML_PAIRWISE_DRIFT_TEST: "" | OFF | MANN_KENDALL
    p_threshold: float = 0.05       # ML_PAIRWISE_THRESHOLD
    min_points: int = 10            # MIN_DRIFT_DATA_POINTS: finite samples a pod, and the baseline, need
    min_tau: float = 0.0            # ML_PAIRWISE_DRIFT_MIN_TAU: floor on |tau| of the current side

    def __post_init__(self):
        name = str(self.test or "").strip().upper()
        if name not in DRIFT_TESTS:
            raise ValueError(f"unknown pairwise drift test {self.test!r} (MANN_KENDALL or OFF)")
        object.__setattr__(self, "test", DRIFT_TESTS[name])
        if int(self.min_points) < 3:
            raise ValueError(f"min_points must be >= 3, got {self.min_points!r}")
        if not 0.0 <= float(self.min_tau) <= 1.0:
            raise ValueError(f"min_tau must lie in [0, 1], got {self.min_tau!r}")

    @property
    def enabled(self) -> bool:
        return self.test != ""

    @classmethod
    def from_config(cls, cfg) -> "DriftTest":
        """The drift test of a ``BrainConfig`` (``pairwise_drift_test``, ``min_drift_points``, ``drift_min_tau`` and
        the pairwise threshold)."""
        return cls(cfg.pairwise_drift_test, float(cfg.pairwise_threshold), int(cfg.min_drift_points),
                   float(cfg.drift_min_tau))


@dataclass
class DriftResult:
    drift: torch.Tensor                  # [R, 6] fp32: z, p, z_c, tau_c, z_b, tau_b
    counts: torch.Tensor                 # [R, 2, 4] int64: S, P, Tx2, V18 of the current side and the baseline
    pod_S: torch.Tensor                  # [R, G] int32: S of every kept pod
    pod_n: torch.Tensor                  # [R, G] int32: finite samples of every kept pod
    k: torch.Tensor                      # [R] int32: kept pods
    drift_diff: torch.Tensor             # [R] int8

    def tensors(self) -> tuple:
        return (self.drift, self.counts, self.pod_S, self.pod_n, self.k, self.drift_diff)


def alloc_drift(R: int, G: int, device, fill: bool = False) -> DriftResult:
    """Output buffers of K31, which writes all of them for every row; ``fill``:
    holding what a row without samples gets (NaN, zeros)."""
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)  # noqa: E731
    o = DriftResult(new((R, 6), torch.float32), new((R, 2, 4), torch.int64), new((R, G), torch.int32),
                    new((R, G), torch.int32), new((R,), torch.int32), new((R,), torch.int8))
    if fill:
        for t in o.tensors():
            t.fill_(float("nan") if t.dtype == torch.float32 else 0)
    return o


# rows ``pairwise_drift`` has sent down each route since the last reset:
# "wave" / "wide" (K31's tiers), "host" (the numpy definition)
_DRIFT_ROUTE_ROWS = {"wave": 0, "wide": 0, "host": 0}


def drift_route_rows() -> dict[str, int]:
    """Rows of GPU batches per drift-test route so far (a copy)."""
    return dict(_DRIFT_ROUTE_ROWS)


def reset_drift_route_rows() -> None:
    for k in _DRIFT_ROUTE_ROWS:
        _DRIFT_ROUTE_ROWS[k] = 0


def _drift_host(cur, seg_end, base, test: DriftTest) -> DriftResult:
    """The numpy definition on host arrays, as CPU tensors."""
    o = ref.pairwise_drift(cur, seg_end, base, test.min_points)
    return DriftResult(*(torch.from_numpy(a) for a in o),
                       torch.from_numpy(ref.drift_verdict(o[0], test.p_threshold, test.min_tau)))


def pairwise_drift(cur: torch.Tensor, seg_end: torch.Tensor, base: torch.Tensor,
                   test: DriftTest = DriftTest("MANN_KENDALL"), tier: str = "auto",
                   out: DriftResult | None = None) -> DriftResult:
    """Drift test of current vs baseline per row and its verdict.

    ``cur`` [R, n_cur] is pod-major, the samples of a pod in time order;
    ``seg_end`` [R, G] int32 holds the column at which pod g's segment ends
    (cumulative; an empty pod repeats the previous end); ``base`` is one
    segment in column order.  CPU tensors run the numpy definition, GPU
    tensors K31: its wave tier up to PAIRWISE_MAX pooled columns, its
    workgroup tier up to PAIRWISE_WIDE_MAX (``tier="wide"`` runs it for any
    batch that fits); a batch padded wider than that, or with more than
    POD_MAX pod columns, is bucketed by the rows' own used widths, and only
    rows really wider, or with more than POD_MAX non-empty pods, run the
    definition on the host."""
    R, ldc = _rows(cur)
    Rb, ldb = _rows(base)
    check(R == Rb, "current/baseline row mismatch")
    check(tier in ("auto", "wide"), "tier is 'auto' or 'wide'")
    check(seg_end.dim() == 2 and seg_end.shape[0] == R and seg_end.dtype == torch.int32 and seg_end.is_contiguous()
          and seg_end.device == cur.device, "seg_end must be a contiguous int32 [R, G] tensor on the samples' device")
    if not cur.is_cuda:
        return _drift_host(cur.numpy(), seg_end.numpy(), base.numpy(), test)
    require_native(cur)
    n_cur, n_base, G = cur.shape[1], base.shape[1], seg_end.shape[1]
    if n_cur + n_base > PAIRWISE_WIDE_MAX or G > POD_MAX:
        return _drift_bucketed(cur, seg_end, base, test)
    wide = tier == "wide" or n_cur + n_base > PAIRWISE_MAX
    _DRIFT_ROUTE_ROWS["wide" if wide else "wave"] += R
    o = out if out is not None else alloc_drift(R, G, cur.device)
    LIB.call("fm_pairwise_drift", ptr(cur), ldc, n_cur, ptr(seg_end) if G else None, G, ptr(base), ldb, n_base, R,
             int(test.min_points), float(test.p_threshold), float(test.min_tau), 2 if wide else 0, ptr(o.drift),
             ptr(o.counts), ptr(o.pod_S), ptr(o.pod_n), ptr(o.k), ptr(o.drift_diff), stream_of(cur))
    return o


def drift_diff(diff: torch.Tensor, cur: torch.Tensor, seg_end: torch.Tensor, base: torch.Tensor,
               test: DriftTest) -> torch.Tensor:
    """``diff | drift_diff`` for the op-by-op model paths (``diff`` from
    ``pairwise_tests``, after the gate and the other optional tests: the drift
    test only ever sets a verdict)."""
    if not test.enabled:
        return diff
    return diff | pairwise_drift(cur, seg_end, base, test).drift_diff.to(diff.dtype)


def _drift_bucketed(cur, seg_end, base, test: DriftTest) -> DriftResult:
    """A batch padded wider than K31 takes, or with more than POD_MAX pod
    columns: rows bucketed by their own used widths exactly as
    ``_pods_bucketed`` does (the wave tier, then the workgroup tier, each on a
    narrowed copy whose segment ends are cut at the copy's width: the columns
    cut off hold no finite sample, and dropping trailing missing samples
    changes no pair).  A row whose pods past POD_MAX are all empty loses only
    those columns; rows with more pods, and rows really wider than
    PAIRWISE_WIDE_MAX, run the numpy definition on the host."""
    R, G = seg_end.shape
    dev = cur.device
    Gk = min(G, POD_MAX)
    lc, lb = used_width(cur).cpu(), used_width(base).cpu()
    many = (seg_end[:, POD_MAX - 1] != seg_end[:, -1]).cpu() if G > POD_MAX else torch.zeros((R,), dtype=torch.bool)
    fit = _bucket(lc, lb, ~many, PAIRWISE_MAX)
    wide = _bucket(lc, lb, ~many & ~fit, PAIRWISE_WIDE_MAX)
    o = alloc_drift(R, G, dev, fill=True)

    def put(k, r):
        for dst, src in zip(o.tensors(), r.tensors()):
            if dst.dim() == 2 and dst.shape[1] == G and src.shape[1] != G:
                dst[k, :src.shape[1]] = src.to(dev)
            else:
                dst[k] = src.to(dev)

    for rows in (fit, wide):
        k = torch.nonzero(rows).flatten()
        if len(k):
            a, b = max(1, int(lc[k].max())), max(1, int(lb[k].max()))
            kd = k.to(dev)
            put(kd, pairwise_drift(cur.index_select(0, kd)[:, :a].contiguous(),
                                   seg_end.index_select(0, kd)[:, :Gk].clamp(max=a).contiguous(),
                                   base.index_select(0, kd)[:, :b].contiguous(), test))
    w = torch.nonzero(~(fit | wide)).flatten()
    if len(w):
        _DRIFT_ROUTE_ROWS["host"] += len(w)
        a, b = max(1, int(lc[w].max())), max(1, int(lb[w].max()))
        wd = w.to(dev)
        put(wd, _drift_host(cur.index_select(0, wd)[:, :a].cpu().numpy(),
                            seg_end.index_select(0, wd).clamp(max=a).cpu().numpy(),
                            base.index_select(0, wd)[:, :b].cpu().numpy(), test))
    return o


TAIL_TESTS = {"": "", "OFF": "", "EXCEEDANCE": "EXCEEDANCE"}
TAIL_MAX_LEVELS = 4


@dataclass(frozen=True)
class TailTest:
    """Tail canary test (K32, docs/BRAIN_SPEC.md 4.6): the share of each side's
    samples beyond the pooled q-quantiles, an exact conditional test per level,
    Bonferroni over the levels that count.  A row it flags counts as
    "different" whatever the other tests say; it never clears a verdict.
    ``test == ""`` = off."""

    test: str = ""                  # ML_PAIRWISE_TAIL_TEST: "" | OFF | EXCEEDANCE
    p_threshold: float = 0.05       # ML_PAIRWISE_THRESHOLD
    quantiles: tuple = (0.9, 0.95, 0.99)   # ML_PAIRWISE_TAIL_QUANTILES (a comma list as a string is parsed)
    sides: str = "BOUND"            # ML_PAIRWISE_TAIL_SIDES: BOUND | UPPER | LOWER | BOTH
    min_points: int = 20            # MIN_TAIL_DATA_POINTS: finite samples each side needs
    min_tail_points: int = 5        # MIN_TAIL_POINTS: pooled samples beyond a level's threshold
    min_excess: float = 0.0         # ML_PAIRWISE_TAIL_MIN_EXCESS: floor on the exceedance-share difference

    def __post_init__(self):
        name = str(self.test or "").strip().upper()
        if name not in TAIL_TESTS:
            raise ValueError(f"unknown pairwise tail test {self.test!r} (EXCEEDANCE or OFF)")
        object.__setattr__(self, "test", TAIL_TESTS[name])
        qs = self.quantiles
        try:
            qs = tuple(float(v) for v in (qs.split(",") if isinstance(qs, str) else qs))
        except (TypeError, ValueError):
            raise ValueError(f"tail quantiles must be numbers, got {self.quantiles!r}") from None
        q_i = tuple(int(round(q * 10000)) for q in qs if q == q)
        if not (1 <= len(qs) <= TAIL_MAX_LEVELS and len(q_i) == len(qs) and all(5000 <= q <= 9999 for q in q_i)
                and all(a < b for a, b in zip(q_i, q_i[1:]))):
            raise ValueError(f"tail quantiles must be 1 to {TAIL_MAX_LEVELS} strictly increasing levels in "
                             f"[0.5, 0.9999], got {self.quantiles!r}")
        object.__setattr__(self, "quantiles", qs)
        side = str(self.sides or "").strip().upper()
        if side not in ref.TAIL_SIDES:
            raise ValueError(f"unknown tail sides {self.sides!r} (BOUND, UPPER, LOWER or BOTH)")
        object.__setattr__(self, "sides", side)
        if int(self.min_points) < 2:
            raise ValueError(f"min_points must be >= 2, got {self.min_points!r}")
        if int(self.min_tail_points) < 1:
            raise ValueError(f"min_tail_points must be >= 1, got {self.min_tail_points!r}")
        if not 0.0 <= float(self.min_excess) < 1.0:
            raise ValueError(f"min_excess must lie in [0, 1), got {self.min_excess!r}")

    @property
    def enabled(self) -> bool:
        return self.test != ""

    @property
    def q_i(self) -> tuple:
        """The levels in parts per 10,000, rounded once; every rank is integer arithmetic on these."""
        return tuple(int(round(q * 10000)) for q in self.quantiles)

    @classmethod
    def from_config(cls, cfg) -> "TailTest":
        """The tail test of a ``BrainConfig`` (``pairwise_tail_test``, ``pairwise_tail_quantiles``,
        ``pairwise_tail_sides``, ``min_tail_data_points``, ``min_tail_points``, ``tail_min_excess`` and the pairwise
        threshold)."""
        return cls(cfg.pairwise_tail_test, float(cfg.pairwise_threshold), cfg.pairwise_tail_quantiles,
                   cfg.pairwise_tail_sides, int(cfg.min_tail_data_points), int(cfg.min_tail_points),
                   float(cfg.tail_min_excess))


@dataclass
class TailResult:
    tail: torch.Tensor                   # [R, 4] fp32: p, p_min, excess, t of the deciding level
    which: torch.Tensor                  # [R] int32: side * L + level of the deciding level, or -1
    J: torch.Tensor                      # [R] int32: counting levels
    n: torch.Tensor                      # [R, 2] int32: finite samples per side
    counts: torch.Tensor                 # [R, 2, L, 3] int32: (a, b, k) per side and level
    tail_diff: torch.Tensor              # [R] int8

    def tensors(self) -> tuple:
        return (self.tail, self.which, self.J, self.n, self.counts, self.tail_diff)


def alloc_tail(R: int, L: int, device) -> TailResult:
    """Output buffers of K32, which writes all of them for every row."""
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)  # noqa: E731
    return TailResult(new((R, 4), torch.float32), new((R,), torch.int32), new((R,), torch.int32),
                      new((R, 2), torch.int32), new((R, 2, L, 3), torch.int32), new((R,), torch.int8))


# rows ``pairwise_tail`` has sent down each route since the last reset:
# "wave" / "wide" (K32's tiers), "host" (the numpy definition)
_TAIL_ROUTE_ROWS = {"wave": 0, "wide": 0, "host": 0}
_TAIL_TABLES: dict = {}


def tail_route_rows() -> dict[str, int]:
    """Rows of GPU batches per tail-test route so far (a copy)."""
    return dict(_TAIL_ROUTE_ROWS)


def reset_tail_route_rows() -> None:
    for k in _TAIL_ROUTE_ROWS:
        _TAIL_ROUTE_ROWS[k] = 0


def _tail_table(device) -> torch.Tensor:
    """lf[n] = lgamma(n + 1), n = 0 .. 8,192, fp64 on ``device``: the reference's own table, built once per device."""
    t = _TAIL_TABLES.get(device)
    if t is None:
        t = _TAIL_TABLES[device] = torch.from_numpy(ref.tail_log_factorials().copy()).to(device)
    return t


def _tail_host(cur, base, test: TailTest, bound_per_row) -> TailResult:
    """The numpy definition on host arrays, as CPU tensors."""
    o = ref.pairwise_tail(cur, base, test.q_i, test.sides, bound_per_row, test.min_points, test.min_tail_points)
    return TailResult(*(torch.from_numpy(a) for a in o),
                      torch.from_numpy(ref.tail_verdict(o[0], test.p_threshold, test.min_excess)))


def pairwise_tail(cur: torch.Tensor, base: torch.Tensor, test: TailTest = TailTest("EXCEEDANCE"),
                  bound: torch.Tensor | None = None, M: int = 1, out: TailResult | None = None,
                  tier: str = "auto") -> TailResult:
    """Tail test of current vs baseline per row and its verdict.

    ``bound`` (int32 [M], the bound code of metric r % M) is needed when
    ``test.sides`` is BOUND: code 1 runs the upper side alone, 2 the lower side
    alone, anything else both.  CPU tensors run the numpy definition, GPU
    tensors K32: its wave tier up to PAIRWISE_MAX pooled columns, its workgroup
    tier up to PAIRWISE_WIDE_MAX (``tier="wide"`` runs it for any batch that
    fits); a batch padded wider than that is bucketed by the rows' own used
    widths, and only rows really wider run the definition on the host."""
    R, ldc = _rows(cur)
    Rb, ldb = _rows(base)
    check(R == Rb, "current/baseline row mismatch")
    check(M >= 1, "M must be >= 1")
    check(tier in ("auto", "wide"), "tier is 'auto' or 'wide'")
    by_bound = test.sides == "BOUND"
    check(not by_bound or (bound is not None and bound.numel() == M and bound.dtype == torch.int32
                           and bound.device == cur.device),
          "sides BOUND needs the per-metric bound codes, int32 [M] on the samples' device")
    if not cur.is_cuda:
        return _tail_host(cur.numpy(), base.numpy(), test, bound.numpy()[np.arange(R) % M] if by_bound else None)
    require_native(cur)
    n_cur, n_base = cur.shape[1], base.shape[1]
    if n_cur + n_base > PAIRWISE_WIDE_MAX:
        return _tail_bucketed(cur, base, test, bound, M)
    wide = tier == "wide" or n_cur + n_base > PAIRWISE_MAX
    _TAIL_ROUTE_ROWS["wide" if wide else "wave"] += R
    q = test.q_i
    o = out if out is not None else alloc_tail(R, len(q), cur.device)
    check(o.counts.shape == (R, 2, len(q), 3), "out was allocated for another batch or number of levels")
    q4 = q + (9999,) * (TAIL_MAX_LEVELS - len(q))
    LIB.call("fm_pairwise_tail", ptr(cur), ldc, n_cur, ptr(base), ldb, n_base, R, len(q), *q4,
             ref.TAIL_SIDES[test.sides], ptr(bound.contiguous()) if by_bound else None, M, int(test.min_points),
             int(test.min_tail_points), float(test.p_threshold), float(test.min_excess), ptr(_tail_table(cur.device)),
             2 if wide else 0, ptr(o.tail), ptr(o.which), ptr(o.J), ptr(o.n), ptr(o.counts), ptr(o.tail_diff),
             stream_of(cur))
    return o


def tail_diff(diff: torch.Tensor, cur: torch.Tensor, base: torch.Tensor, test: TailTest, bound: torch.Tensor,
              M: int) -> torch.Tensor:
    """``diff | tail_diff`` for the op-by-op model paths (``diff`` from
    ``pairwise_tests``, after the gate and the other optional tests: the tail
    test only ever sets a verdict; row r is judged by bound code ``bound[r % M]``)."""
    if not test.enabled:
        return diff
    return diff | pairwise_tail(cur, base, test, bound, M).tail_diff.to(diff.dtype)


def _tail_bucketed(cur, base, test: TailTest, bound, M: int) -> TailResult:
    """A batch padded wider than K32 takes: rows bucketed by their own used
    widths exactly as ``_drift_bucketed`` does (the wave tier, then the
    workgroup tier, each on a narrowed copy: the columns cut off hold no finite
    sample); rows really wider than PAIRWISE_WIDE_MAX run the numpy definition
    on the host.  Every row brings its own bound code (the ORIGINAL row index r
    % M), so the narrowed batches run with M = their row count."""
    R = cur.shape[0]
    dev = cur.device
    lc, lb = used_width(cur).cpu(), used_width(base).cpu()
    fit = _bucket(lc, lb, torch.ones((R,), dtype=torch.bool), PAIRWISE_MAX)
    wide = _bucket(lc, lb, ~fit, PAIRWISE_WIDE_MAX)
    o = alloc_tail(R, len(test.q_i), dev)
    per_row = bound[torch.arange(R, device=bound.device) % M] if test.sides == "BOUND" else None
    for rows in (fit, wide):
        k = torch.nonzero(rows).flatten()
        if len(k):
            a, b = max(1, int(lc[k].max())), max(1, int(lb[k].max()))
            kd = k.to(dev)
            r = pairwise_tail(cur.index_select(0, kd)[:, :a].contiguous(), base.index_select(0, kd)[:, :b].contiguous(),
                              test, None if per_row is None else per_row.index_select(0, kd).contiguous(), len(k))
            for dst, src in zip(o.tensors(), r.tensors()):
                dst[kd] = src
    w = torch.nonzero(~(fit | wide)).flatten()
    if len(w):
        _TAIL_ROUTE_ROWS["host"] += len(w)
        a, b = max(1, int(lc[w].max())), max(1, int(lb[w].max()))
        wd = w.to(dev)
        r = _tail_host(cur.index_select(0, wd)[:, :a].cpu().numpy(), base.index_select(0, wd)[:, :b].cpu().numpy(), test,
                       None if per_row is None else per_row.index_select(0, wd).cpu().numpy())
        for dst, src in zip(o.tensors(), r.tensors()):
            dst[wd] = src.to(dev)
    return o


DEPENDENCE_GATES = {"": "", "OFF": "", "RANK_ACF": "RANK_ACF"}
ACF_MAX_LAG = ref.ACF_MAX_LAG


@dataclass(frozen=True)
class DependenceGate:
    """Dependence gate of the pairwise verdict (K33, docs/BRAIN_SPEC.md 4.7): the
    rank-sum z of current vs baseline with each side's sample size deflated by
    a variance-inflation factor from the autocorrelation of the pooled midranks
    along time inside each pod.  A row keeps its "different" verdict only while
    the adjusted p-value is still below the threshold; the gate never sets a
    verdict.  ``gate == ""`` = off."""

    gate: str = ""                  # ML_PAIRWISE_DEPENDENCE: "" | OFF | RANK_ACF
    p_threshold: float = 0.05       # ML_PAIRWISE_THRESHOLD
    max_lag: int = 8                # ML_PAIRWISE_ACF_MAX_LAG: L, 1..16
    min_points: int = 12            # MIN_ACF_DATA_POINTS: finite samples a segment needs to contribute

    def __post_init__(self):
        name = str(self.gate or "").strip().upper()
        if name not in DEPENDENCE_GATES:
            raise ValueError(f"unknown pairwise dependence gate {self.gate!r} (RANK_ACF or OFF)")
        object.__setattr__(self, "gate", DEPENDENCE_GATES[name])
        if not 1 <= int(self.max_lag) <= ACF_MAX_LAG:
            raise ValueError(f"max_lag must lie in 1..{ACF_MAX_LAG}, got {self.max_lag!r}")
        if int(self.min_points) < 4:
            raise ValueError(f"min_points must be >= 4, got {self.min_points!r}")

    @property
    def enabled(self) -> bool:
        return self.gate != ""

    @classmethod
    def from_config(cls, cfg) -> "DependenceGate":
        """The dependence gate of a ``BrainConfig`` (``pairwise_dependence``, ``pairwise_acf_max_lag``,
        ``min_acf_points`` and the pairwise threshold)."""
        return cls(cfg.pairwise_dependence, float(cfg.pairwise_threshold), int(cfg.pairwise_acf_max_lag),
                   int(cfg.min_acf_points))


@dataclass
class DependenceResult:
    dep: torch.Tensor                    # [R, 6] fp32: p_adj, z_adj, z, VIF_c, VIF_b, N
    rho: torch.Tensor                    # [R, 2, 16] fp32: entry j = lag j + 1 of the current side / the baseline
    n: torch.Tensor                      # [R, 2] int32: finite samples per side
    TA: torch.Tensor                     # [R, 2] int64: T, A
    kept: torch.Tensor                   # [R, 2] int32: kept segments per side
    pairs: torch.Tensor                  # [R, 2, 16] int32: pairs per lag over the kept segments
    dep_keep: torch.Tensor               # [R] int8

    def tensors(self) -> tuple:
        return (self.dep, self.rho, self.n, self.TA, self.kept, self.pairs, self.dep_keep)


def alloc_dependence(R: int, device) -> DependenceResult:
    """Output buffers of K33, which writes all of them for every row."""
    new = lambda shape, dt: torch.empty(shape, dtype=dt, device=device)  # noqa: E731
    return DependenceResult(new((R, 6), torch.float32), new((R, 2, ACF_MAX_LAG), torch.float32),
                            new((R, 2), torch.int32), new((R, 2), torch.int64), new((R, 2), torch.int32),
                            new((R, 2, ACF_MAX_LAG), torch.int32), new((R,), torch.int8))


# rows ``pairwise_dependence`` has sent down each route since the last reset:
# "wave" / "wide" (K33's tiers), "host" (the numpy definition)
_DEPENDENCE_ROUTE_ROWS = {"wave": 0, "wide": 0, "host": 0}


def dependence_route_rows() -> dict[str, int]:
    """Rows of GPU batches per dependence-gate route so far (a copy)."""
    return dict(_DEPENDENCE_ROUTE_ROWS)


def reset_dependence_route_rows() -> None:
    for k in _DEPENDENCE_ROUTE_ROWS:
        _DEPENDENCE_ROUTE_ROWS[k] = 0


def _dependence_host(cur, seg_end, base, gate: DependenceGate) -> DependenceResult:
    """The numpy definition on host arrays, as CPU tensors."""
    o = ref.pairwise_dependence(cur, seg_end, base, gate.max_lag, gate.min_points)
    return DependenceResult(*(torch.from_numpy(a) for a in o),
                            torch.from_numpy(ref.dependence_verdict(o[0], gate.p_threshold)))


def pairwise_dependence(cur: torch.Tensor, seg_end: torch.Tensor, base: torch.Tensor,
                        gate: DependenceGate = DependenceGate("RANK_ACF"), tier: str = "auto",
                        out: DependenceResult | None = None) -> DependenceResult:
    """Dependence-adjusted rank-sum test of current vs baseline per row and
    which rows keep a "different" verdict.

    ``cur`` [R, n_cur] is pod-major, the samples of a pod in time order, one
    column per time step; ``seg_end`` [R, G] int32 holds the column at which
    pod g's segment ends (cumulative); ``base`` is one segment in column
    order.  CPU tensors run the numpy definition, GPU tensors K33: its wave
    tier up to PAIRWISE_MAX pooled columns, its workgroup tier up to
    PAIRWISE_WIDE_MAX (``tier="wide"`` runs it for any batch that fits); a
    batch padded wider than that, or with more than POD_MAX pod columns, is
    bucketed by the rows' own used widths, and only rows really wider, or
    with more than POD_MAX non-empty pods, run the definition on the host.
    ``out``: buffers from ``alloc_dependence`` that take the result on every
    route (the kernel writes them directly; the host and the bucketed routes
    copy theirs in)."""
    R, ldc = _rows(cur)
    Rb, ldb = _rows(base)
    check(R == Rb, "current/baseline row mismatch")
    check(tier in ("auto", "wide"), "tier is 'auto' or 'wide'")
    check(seg_end.dim() == 2 and seg_end.shape[0] == R and seg_end.dtype == torch.int32 and seg_end.is_contiguous()
          and seg_end.device == cur.device, "seg_end must be a contiguous int32 [R, G] tensor on the samples' device")
    def into_out(r: DependenceResult) -> DependenceResult:
        if out is None:
            return r
        for dst, src in zip(out.tensors(), r.tensors()):
            dst.copy_(src)
        return out

    if not cur.is_cuda:
        return into_out(_dependence_host(cur.numpy(), seg_end.numpy(), base.numpy(), gate))
    require_native(cur)
    n_cur, n_base, G = cur.shape[1], base.shape[1], seg_end.shape[1]
    if n_cur + n_base > PAIRWISE_WIDE_MAX or G > POD_MAX:
        return into_out(_dependence_bucketed(cur, seg_end, base, gate))
    wide = tier == "wide" or n_cur + n_base > PAIRWISE_MAX
    _DEPENDENCE_ROUTE_ROWS["wide" if wide else "wave"] += R
    o = out if out is not None else alloc_dependence(R, cur.device)
    LIB.call("fm_pairwise_dependence", ptr(cur), ldc, n_cur, ptr(seg_end) if G else None, G, ptr(base), ldb, n_base,
             R, int(gate.max_lag), int(gate.min_points), float(gate.p_threshold), 2 if wide else 0, ptr(o.dep),
             ptr(o.rho), ptr(o.n), ptr(o.TA), ptr(o.kept), ptr(o.pairs), ptr(o.dep_keep), stream_of(cur))
    return o


def dependence_diff(diff: torch.Tensor, cur: torch.Tensor, seg_end: torch.Tensor, base: torch.Tensor,
                    gate: DependenceGate) -> torch.Tensor:
    """``diff & dep_keep`` for the op-by-op model paths (``diff`` from
    ``pairwise_tests``, after the effect-size gate and before the optional
    tests, whose own verdicts the gate does not touch: it only ever clears a
    verdict).  ``diff`` itself when the gate is off."""
    if not gate.enabled:
        return diff
    return diff & pairwise_dependence(cur, seg_end, base, gate).dep_keep.to(diff.dtype)


def _dependence_bucketed(cur, seg_end, base, gate: DependenceGate) -> DependenceResult:
    """A batch padded wider than K33 takes, or with more than POD_MAX pod
    columns: rows bucketed by their own used widths exactly as
    ``_drift_bucketed`` does (the wave tier, then the workgroup tier, each on a
    narrowed copy whose segment ends are cut at the copy's width: the columns
    cut off hold no finite sample, and dropping trailing missing samples
    changes no rank and no pair).  A row whose pods past POD_MAX are all empty
    loses only those columns; rows with more pods, and rows really wider than
    PAIRWISE_WIDE_MAX, run the numpy definition on the host."""
    R, G = seg_end.shape
    dev = cur.device
    Gk = min(G, POD_MAX)
    lc, lb = used_width(cur).cpu(), used_width(base).cpu()
    many = (seg_end[:, POD_MAX - 1] != seg_end[:, -1]).cpu() if G > POD_MAX else torch.zeros((R,), dtype=torch.bool)
    fit = _bucket(lc, lb, ~many, PAIRWISE_MAX)
    wide = _bucket(lc, lb, ~many & ~fit, PAIRWISE_WIDE_MAX)
    o = alloc_dependence(R, dev)

    def put(k, r):
        for dst, src in zip(o.tensors(), r.tensors()):
            dst[k] = src.to(dev)

    for rows in (fit, wide):
        k = torch.nonzero(rows).flatten()
        if len(k):
            a, b = max(1, int(lc[k].max())), max(1, int(lb[k].max()))
            kd = k.to(dev)
            put(kd, pairwise_dependence(cur.index_select(0, kd)[:, :a].contiguous(),
                                        seg_end.index_select(0, kd)[:, :Gk].clamp(max=a).contiguous(),
                                        base.index_select(0, kd)[:, :b].contiguous(), gate))
    w = torch.nonzero(~(fit | wide)).flatten()
    if len(w):
        _DEPENDENCE_ROUTE_ROWS["host"] += len(w)
        a, b = max(1, int(lc[w].max())), max(1, int(lb[w].max()))
        wd = w.to(dev)
        put(wd, _dependence_host(cur.index_select(0, wd)[:, :a].cpu().numpy(),
                                 seg_end.index_select(0, wd).clamp(max=a).cpu().numpy(),
                                 base.index_select(0, wd)[:, :b].cpu().numpy(), gate))
    return o


@dataclass
class DecideResult:
    stats: torch.Tensor     # [R, 4] mean, std, upper, lower
    flags: torch.Tensor     # [R, NW] int64 bit-packed anomaly flags (bit i of word w = point 64w+i)
    count: torch.Tensor     # [R] int32 anomalous points
    score: torch.Tensor     # [R] f32 max exceedance in std units
    valid: torch.Tensor     # [R] int32: bit0 enough history, bit1 has current data


def alloc_decide(R: int, n_cur: int, device) -> DecideResult:
    NW = max(1, (n_cur + 63) // 64)
    return DecideResult(
        stats=torch.empty((R, 4), dtype=torch.float32, device=device),
        flags=torch.empty((R, NW), dtype=torch.int64, device=device),
        count=torch.empty((R,), dtype=torch.int32, device=device),
        score=torch.empty((R,), dtype=torch.float32, device=device),
        valid=torch.empty((R,), dtype=torch.int32, device=device),
    )


def stats_decide(hist: torch.Tensor, cur: torch.Tensor, n_hist: int | None, M: int, thr: torch.Tensor,
                 bound: torch.Tensor, minlb: torch.Tensor, diff: torch.Tensor | None = None,
                 pair_factor: float = 0.8, min_hist: int = 1, out: DecideResult | None = None) -> DecideResult:
    """moving_average_all bounds (mean +/- thr*std over the whole history, lower
    clamped at min_lower_bound) fused with the current-window decision.

    ``hist`` is [R, ld] with ld % 4 == 0 (trailing pad = NaN); ``n_hist`` is the
    logical history length (defaults to ld).  Row r belongs to metric r % M.
    """
    R, ldh = _rows(hist)
    Rc, ldc = _rows(cur)
    check(R == Rc, "history/current row mismatch")
    check(R % M == 0, "rows must be services x metrics")
    T = hist.shape[1] if n_hist is None else int(n_hist)
    n_cur = cur.shape[1]
    if not hist.is_cuda:
        o = ref.stats_decide(hist.numpy()[:, :T], cur.numpy(), M, thr.numpy(), bound.numpy(), minlb.numpy(),
                             None if diff is None else diff.numpy(), pair_factor, min_hist)
        return DecideResult(*(torch.from_numpy(a) for a in o))
    require_native(hist)
    check(ldh % 4 == 0 and hist.data_ptr() % 16 == 0, "history rows must be 16-B aligned (ld % 4 == 0)")
    check(T <= 16 * 256 * 4, "history length > 16384 not supported by the register-resident kernel")
    for t, dt in ((thr, torch.float32), (bound, torch.int32), (minlb, torch.float32)):
        check(t.is_cuda and t.dtype == dt and t.numel() == M, "per-metric tables must be device tensors of length M")
    if diff is not None:
        check(diff.dtype == torch.int8 and diff.numel() == R, "diff must be int8 [R]")
    o = out if out is not None else alloc_decide(R, n_cur, hist.device)
    NW = o.flags.shape[1]
    LIB.call("fm_stats_decide", ptr(hist), ldh, T, ptr(cur), ldc, n_cur, R, M, ptr(thr), ptr(bound), ptr(minlb),
             float(pair_factor), ptr(diff), int(min_hist), ptr(o.stats), ptr(o.flags), NW, ptr(o.count),
             ptr(o.score), ptr(o.valid), stream_of(hist))
    return o


def service_reduce(count: torch.Tensor, score: torch.Tensor, valid: torch.Tensor, M: int,
                   out: torch.Tensor | None = None) -> torch.Tensor:
    """Per-service packed verdict [S, 4] = (status, score, anomalous-metric mask, count).
    status: 0 no anomaly, 1 anomaly, 2 unknown (missing data)."""
    R = count.numel()
    S = R // M
    if not count.is_cuda:
        return torch.from_numpy(ref.service_reduce(count.numpy(), score.numpy(), valid.numpy(), M))
    require_native(count)
    check(M <= 24, "at most 24 metrics per service")
    packed = out if out is not None else torch.empty((S, 4), dtype=torch.float32, device=count.device)
    LIB.call("fm_service_reduce", ptr(count), ptr(score), ptr(valid), S, M, ptr(packed), stream_of(count))
    return packed


def combine_pvalues(pvals, test_mask: int, combine_any: int, p_thr: float) -> np.ndarray:
    """"Distribution differs" per row as the decision kernels combine the
    p-values they are given (fp32 [R, N_TESTS], NaN = test not applicable):
    among the tests of ``test_mask`` that apply, any (``combine_any``) or all
    below ``float32(p_thr)``; no applicable test: 0.  -> int8 [R]."""
    P = np.asarray(pvals, np.float32)
    sel = np.array([(int(test_mask) >> i) & 1 for i in range(N_TESTS)], dtype=bool)
    app = ~np.isnan(P[:, sel])
    sig = app & (np.nan_to_num(P[:, sel].astype(np.float64), nan=1.0) < float(np.float32(p_thr)))
    na, ns = app.sum(1), sig.sum(1)
    return np.where(na > 0, (ns > 0) if combine_any else (ns == na), False).astype(np.int8)


def ref_decide_services_2s(bs, cur, M: int, thr, bound, minlb, pair_factor: float = 0.8, min_hist: int = 1,
                           pvals=None, test_mask: int = (1 << N_TESTS) - 1, combine_any: int = 0,
                           p_thr: float = 0.05, diff=None):
    """The contract of :func:`decide_services_2s` on numpy arrays, composed of
    the references that exist: :func:`combine_pvalues`, the two-sigma band
    decision ``ops.smoothing.ref_band_decide_2s`` on the band records ``bs
    [R, 4]`` (centre, sigma_lo, sigma_up, n), the history gate ``n >= min_hist
    and n > 0`` (a row without enough history flags and scores nothing) and
    the service reduce.  ``diff`` (int8 [R]) stands in for the combined
    p-values when the caller has it.  -> (DecideResult with stats = centre,
    sigma_up, upper, lower; packed [S, 4]; diff int8 [R] or None)."""
    from .smoothing import ref_band_decide_2s
    bs = np.asarray(bs, np.float32)
    x = np.asarray(cur, np.float32)
    if diff is not None:
        diff = np.asarray(diff, np.int8)
    elif pvals is not None:
        diff = combine_pvalues(pvals, test_mask, combine_any, p_thr)
    c, slo, sup = bs[:, 0], bs[:, 1], bs[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        up, lo, flags, cnt, sc = ref_band_decide_2s(x, c[:, None], slo, sup, M, np.asarray(thr, np.float32),
                                                    np.asarray(bound), np.asarray(minlb, np.float32), diff,
                                                    pair_factor)
        n = bs[:, 3].astype(np.int64)
    has = torch.from_numpy((n >= min_hist) & (n > 0))
    cnt = torch.where(has, cnt, torch.zeros_like(cnt))
    sc = torch.where(has, sc, torch.zeros_like(sc))
    flags = torch.where(has[:, None], flags, torch.zeros_like(flags))
    valid = has.to(torch.int32) | (torch.from_numpy(np.isfinite(x).any(1)).to(torch.int32) << 1)
    stats = torch.stack([torch.from_numpy(c.copy()), torch.from_numpy(sup.copy()), up[:, 0], lo[:, 0]], 1)
    dec = DecideResult(stats, flags, cnt, sc, valid)
    return dec, service_reduce(cnt, sc, valid, M), (None if diff is None else torch.from_numpy(diff))


def decide_services_2s(bs: torch.Tensor, cur: torch.Tensor, M: int, thr: torch.Tensor, bound: torch.Tensor,
                       minlb: torch.Tensor, pair_factor: float = 0.8, min_hist: int = 1,
                       pvals: torch.Tensor | None = None, test_mask: int = (1 << N_TESTS) - 1, combine_any: int = 0,
                       p_thr: float = 0.05, out: DecideResult | None = None, packed: torch.Tensor | None = None,
                       diff: torch.Tensor | None = None):
    """The service decision over band records ``bs [R, 4]`` = (centre,
    sigma_lo, sigma_up, n) (K25, ``ops.misc.band_stats_cached``), one launch:
    the p-values (fp32 [R, N_TESTS] or None) combine into "distribution
    differs", which lowers the row's threshold by ``pair_factor``; the current
    window is judged against [centre - thr sigma_lo (clamped at
    min_lower_bound), centre + thr sigma_up], each side scoring in its own
    sigma; rows with fewer than ``min_hist`` history samples flag nothing; the
    service verdict is reduced.  Rows are services x M, ``M <= 16``.  With
    ``sigma_lo == sigma_up`` the outputs are fm_decide_services' bit for bit.
    -> (DecideResult with stats = centre, sigma_up, upper, lower; packed
    [S, 4]; diff int8 [R], or None without p-values)."""
    R, n_cur = cur.shape
    check(bs.dim() == 2 and tuple(bs.shape) == (R, 4) and bs.dtype == torch.float32, "bs must be fp32 [R, 4]")
    check(1 <= M <= 16 and R % M == 0, "rows must be services x M, M <= 16")
    check(n_cur >= 1, "the current window is empty")
    if not cur.is_cuda:
        return ref_decide_services_2s(bs.numpy(), cur.numpy(), M, thr.numpy(), bound.numpy(), minlb.numpy(),
                                      pair_factor, min_hist, None if pvals is None else pvals.numpy(), test_mask,
                                      combine_any, p_thr)
    require_native(cur)
    check(bs.is_contiguous() and cur.stride(1) == 1 or n_cur == 1, "bs contiguous, cur with unit column stride")
    for t, dt in ((thr, torch.float32), (bound, torch.int32), (minlb, torch.float32)):
        check(t.is_cuda and t.dtype == dt and t.numel() == M, "per-metric tables must be device tensors of length M")
    if pvals is not None:
        check(pvals.dtype == torch.float32 and tuple(pvals.shape) == (R, N_TESTS) and pvals.is_contiguous(),
              "pvals must be contiguous fp32 [R, N_TESTS]")
    o = out if out is not None else alloc_decide(R, n_cur, cur.device)
    if packed is None:
        packed = torch.empty((R // M, 4), dtype=torch.float32, device=cur.device)
    if diff is None and pvals is not None:
        diff = torch.empty((R,), dtype=torch.int8, device=cur.device)
    LIB.call("fm_decide_services_2s", ptr(bs), ptr(cur), cur.stride(0), n_cur, R // M, M, ptr(thr), ptr(bound),
             ptr(minlb), float(pair_factor), ptr(pvals), int(test_mask), int(combine_any), float(p_thr), int(min_hist),
             ptr(o.stats), ptr(o.flags), o.flags.shape[1], ptr(o.count), ptr(o.score), ptr(o.valid),
             ptr(diff) if pvals is not None else None, ptr(packed), stream_of(cur))
    return o, packed, (diff if pvals is not None else None)


def compact_anomalies(res: DecideResult, cur: torch.Tensor, cap: int | None = None):
    """Stream-compact anomalous points -> (idx [K,2] int32 (row, point), values [K] f32).
    Order of rows is arbitrary on GPU; callers sort by row."""
    R, ldc = _rows(cur)
    n_cur = cur.shape[1]
    if not cur.is_cuda:
        idx, val = ref.compact_anomalies(res.flags.numpy(), cur.numpy(), res.count.numpy())
        return torch.from_numpy(idx), torch.from_numpy(val)
    total = int(res.count.sum().item())
    cap = total if cap is None else min(cap, total)
    if cap == 0:
        return (torch.empty((0, 2), dtype=torch.int32, device=cur.device),
                torch.empty((0,), dtype=torch.float32, device=cur.device))
    counter = torch.zeros((1,), dtype=torch.int32, device=cur.device)
    idx = torch.empty((cap, 2), dtype=torch.int32, device=cur.device)
    val = torch.empty((cap,), dtype=torch.float32, device=cur.device)
    LIB.call("fm_compact_anomalies", ptr(res.flags), res.flags.shape[1], ptr(cur), ldc, n_cur, ptr(res.count), R,
             cap, ptr(counter), ptr(idx), ptr(val), stream_of(cur))
    order = torch.argsort(idx[:, 0].to(torch.int64) * (n_cur + 1) + idx[:, 1].to(torch.int64))
    return idx[order], val[order]


def synth_fleet(S: int, M: int, T: int, P: int, W: int, svc0: int = 0, *, device="cpu", seed: int = 1234,
                fault_rate: float = 0.02, fault_mag: float = 1.0, ld_pad: int = 4):
    """Synthetic Prometheus-shaped fleet for services [svc0, svc0+S).

    Returns (hist [S*M, ldh] with NaN pad, base [S*M, P*W], cur [S*M, P*W]).
    Deterministic in the global service id (identical for any sharding)."""
    ldh = ((T + ld_pad - 1) // ld_pad) * ld_pad
    dev = torch.device(device)
    if dev.type != "cuda":
        h, b, c = ref.synth_fleet(S, M, T, P, W, svc0, seed, fault_rate, fault_mag, ldh)
        return torch.from_numpy(h), torch.from_numpy(b), torch.from_numpy(c)
    R = S * M
    hist = torch.empty((R, ldh), dtype=torch.float32, device=dev)
    base = torch.empty((R, P * W), dtype=torch.float32, device=dev)
    cur = torch.empty((R, P * W), dtype=torch.float32, device=dev)
    require_native(hist)
    s = stream_of(hist)
    LIB.call("fm_synth_fleet", ptr(hist), ldh, T, S, M, svc0, T, P, W, 0, float(fault_rate), float(fault_mag),
             seed, s)
    LIB.call("fm_synth_fleet", ptr(base), P * W, P * W, S, M, svc0, T, P, W, 1, float(fault_rate), float(fault_mag),
             seed, s)
    LIB.call("fm_synth_fleet", ptr(cur), P * W, P * W, S, M, svc0, T, P, W, 2, float(fault_rate), float(fault_mag),
             seed, s)
    return hist, base, cur


def unpack_flags(flags: torch.Tensor, n: int) -> np.ndarray:
    """[R, NW] int64 words -> bool [R, n]."""
    f = flags.cpu().numpy().view(np.uint64)
    bits = ((f[:, :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    return bits.reshape(f.shape[0], -1)[:, :n]
