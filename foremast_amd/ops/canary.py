"""Canary-scoring ops: pairwise tests (K4), fused moving-average bounds +
anomaly decision (K1+K7), service reduce, anomaly compaction, synthetic fleet
(K11).

GPU tensors run the hand-written CDNA4 kernels in ``csrc/kernels/``
(``pairwise.hip``, ``pairwise_wide.hip``, ``pairwise_effect.hip``, ``pairwise_scale.hip``, ``hist_stats.hip``, ``tick_front.hip``, ``canary_rows.hip``,
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


def pairwise_effect(cur: torch.Tensor, base: torch.Tensor, gate: EffectGate = EffectGate(),
                    bound: torch.Tensor | None = None, M: int = 1, pvals: torch.Tensor | None = None,
                    out: EffectResult | None = None) -> EffectResult:
    """Effect size of current vs baseline per row and the gate's verdict on it.

    ``bound`` (int32 [M], the bound code of metric r % M; needed when the gate
    is directional) and ``pvals`` ([R, 6] fp32, optional: ``pvals_gated`` is
    its copy with the failing rows set to NaN, which ``fm_decide_services``
    reads as "no test applies").  CPU tensors run the numpy reference, GPU
    tensors K19 (wider than PAIRWISE_MAX pooled: bucketed by used width like
    the pairwise tests)."""
    R, ldc = _rows(cur)
    Rb, ldb = _rows(base)
    check(R == Rb, "current/baseline row mismatch")
    check(M >= 1, "M must be >= 1")
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
    if n_cur + n_base > PAIRWISE_MAX:
        return _effect_bucketed(cur, base, gate, bound, M, pvals)
    o = out if out is not None else alloc_effect(R, cur.device, pvals is not None)
    if bound is not None:
        check(bound.is_cuda and bound.dtype == torch.int32 and bound.is_contiguous(), "bound must be a device int32 [M]")
    check(pvals is None or o.pvals_gated is not None, "out has no pvals_gated buffer")
    LIB.call("fm_pairwise_effect", ptr(cur), ldc, n_cur, ptr(base), ldb, n_base, R, float(gate.min_effect),
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
    """A batch padded wider than PAIRWISE_MAX pooled columns: rows bucketed by
    their own used widths exactly as ``_pairwise_bucketed`` does; rows that
    fit run K19 on a narrowed copy, only really wider rows the CPU oracle.
    The gate is per row, so it is evaluated once over the assembled effects
    (bound codes follow the ORIGINAL row index r % M)."""
    R = cur.shape[0]
    dev = cur.device
    lc, lb = used_width(cur).cpu(), used_width(base).cpu()
    fit = (lc + lb) <= PAIRWISE_MAX
    if fit.any() and int(lc[fit].max()) + int(lb[fit].max()) > PAIRWISE_MAX:
        fit &= (lc <= PAIRWISE_MAX // 2) & (lb <= PAIRWISE_MAX // 2)
    eff = torch.empty((R, 4), dtype=torch.float32, device=dev)
    cnt = torch.empty((R, 2), dtype=torch.int32, device=dev)
    k = torch.nonzero(fit).flatten()
    if len(k):
        a, b = max(1, int(lc[k].max())), max(1, int(lb[k].max()))
        kd = k.to(dev)
        r1 = pairwise_effect(cur.index_select(0, kd)[:, :a].contiguous(), base.index_select(0, kd)[:, :b].contiguous())
        eff.index_copy_(0, kd, r1.effect)
        cnt.index_copy_(0, kd, r1.counts)
    w = torch.nonzero(~fit).flatten()
    if len(w):
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
