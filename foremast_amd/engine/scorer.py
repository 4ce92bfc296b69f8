"""Batched canary scorer: the brain's per-cycle judgement for a whole shard of
services in three kernel launches.

Pipeline per tick (docs/BRAIN_SPEC.md §4-5; reference intent
docs/guides/design.md:31-43, sequence diagram
.gitbook/assets/foremastjudgementsequencediagram.png):

1. K4 pairwise tests current-vs-baseline -> ``diff`` (distribution changed)
2. K1+K7 moving_average_all bounds over the 7-day history fused with the
   decision on the current window; rows whose distribution changed get the
   lowered threshold (``threshold * pairwise_threshold_factor``)
3. service reduce -> packed [S, 4] verdict (status, score, metric mask, count)

All buffers are pre-allocated per shape so the chain can be captured into a
HIP graph (``capture``) and replayed with zero host work per tick.
"""
from __future__ import annotations

import dataclasses
import os
import weakref
from dataclasses import dataclass

import torch

from ..config import BrainConfig
from ..ops import canary as C


@dataclass
class CanaryOutputs:
    pvals: torch.Tensor
    pstats: torch.Tensor
    diff: torch.Tensor
    suff: torch.Tensor
    decide: C.DecideResult
    packed: torch.Tensor        # [S, 4]
    hs: torch.Tensor | None = None   # [R, 3] history mean, std, count (two-stream path)
    # effect-size gate (K19), None when it is off or the tick has no baseline
    effect: torch.Tensor | None = None          # [R, 4] Cliff's delta, Hodges-Lehmann shift, baseline median, N
    effect_counts: torch.Tensor | None = None   # [R, 2] int32 #{d > 0}, #{d < 0}
    effect_passed: torch.Tensor | None = None   # [R] int8
    pvals_gated: torch.Tensor | None = None     # [R, 6] what the decision reads: pvals, NaN where the gate failed
    bs: torch.Tensor | None = None              # [R, 4] band records (centre, sigma_lo, sigma_up, n): model="band_mix"
    # scale test (K27), None when it is off or the tick has no baseline
    scale: torch.Tensor | None = None           # [R, 6] W, p, ratio, current median, baseline median, N
    scale_diff: torch.Tensor | None = None      # [R] int8: the spread differs
    pvals_scaled: torch.Tensor | None = None    # [R, 6] what the decision reads: 0 in a flagged row, else pvals / gated
    scale_moments: torch.Tensor | None = None   # [R, 8] fp64 scratch of K27


MODES = ("front", "fused", "overlap", "serial")
MODELS = ("moving_average_all", "robust_moving_average_all", "band_mix")


class _BoundHist:
    """A history tensor bound to a launcher for the launcher's life: the strong
    reference (its address cannot be handed to another tensor while statistics
    of its rows are cached), the row-statistics cache, and the tensor version
    the cache was filled under."""

    def __init__(self, hist: torch.Tensor):
        from .resident import RowStatsCache
        self.hist = hist
        self.cache = RowStatsCache(hist.shape[0], hist.device)
        self.version = hist._version

    def expect_miss(self, T: int, rows: int, stream: int | None) -> bool:
        """Called before every launch (``stream``: where it goes; None = the
        current torch stream): a write torch knows of invalidates everything."""
        v = self.hist._version
        if v != self.version:
            self.version = v
            if rows == len(self.cache):
                # the streaming launch this forces looks at no word and
                # rewrites every one of them: nothing to clear ahead of it
                self.cache.dirty = rows
            else:
                self.cache.invalidate(stream)
        return self.cache.expect_miss(T, rows)


class _BaseCache:
    """Baseline cache of one baseline tensor (fm_tick_front_bc, fm_pairwise.h
    PwBaseCache): per row the baseline as last seen (``raw``), its half of the
    pooled sort as it enters the final merge (``sorted``) and (n2, m2, q2,
    n_base) (``stats``; n_base 0 = empty).  The kernel tests and fills it row
    by row; the host only owns the memory.  ~528 bytes per row."""

    def __init__(self, rows: int, device):
        self.raw = torch.zeros((rows, 64), dtype=torch.int32, device=device)
        self.sorted = torch.zeros((rows, 64), dtype=torch.int32, device=device)
        self.stats = torch.zeros((rows, 4), dtype=torch.int32, device=device)

    def __len__(self) -> int:
        return self.raw.shape[0]


class CanaryScorer:
    """``mode`` (GPU only):

    * ``front`` (default) — ONE role-split launch (fm_tick_front): pairwise workgroups
      (sorted-rank statistics, then the p-values of their own rows) and
      history-stats workgroups share the CUs without a second stream, then
      the decide kernel.  No fork/join in the graph;
    * ``overlap`` — pairwise on a side stream || history stats on
      the main stream, joined before the decision (fork/join captured in the
      graph);
    * ``fused`` — one wave per row streams the 7-day history and runs the
      pairwise rank tests while it is in flight (fm_canary_rows).  Measured
      slower on MI355X (profiles/tick_breakdown_1gpu.json: the 160-VGPR row
      image leaves 2 waves/SIMD, too few to keep HBM busy), kept for A/B;
    * ``serial`` — pairwise, then the fused stats+decide kernel.

    Effect gate (``cfg.pairwise_min_effect`` / ``_min_shift`` / ``_min_shift_abs``
    / ``_directional``, all off by default): when any is set and the tick has a
    baseline, K19 (``fm_pairwise_effect``) runs on the tick's stream between
    the p-values and the decision, and the decision combines the gated copy of
    the p-values; ``CanaryOutputs.effect`` / ``effect_counts`` /
    ``effect_passed`` report it.  A gated scorer ticks through ``score`` and
    ``score_resident`` only.

    Scale test (``cfg.pairwise_scale_test``, off by default): when it is set
    and the tick has a baseline, K27 (``fm_pairwise_scale``) runs on the tick's
    stream after the p-values (and K19) and before the decision; it takes the
    p-values the decision would read and hands on a copy with 0 in all six
    columns of a row whose spread differs, so that row is "different" under
    every ``ML_PAIRWISE_ALGORITHM`` and the gate never clears it;
    ``CanaryOutputs.scale`` / ``scale_diff`` report it, ``pvals`` stay what
    the tests computed.  Refused where the gate is.

    Baseline cache (``base_cache``, env ``FM_BASE_CACHE``; front mode, the
    usual window shape only: both windows <= 64 points, more than 64
    together).  A canary job's baseline window is a fixed past interval, so a
    row's baseline is the same numbers tick after tick while its current
    window moves.  The front kernel keeps, per row, the baseline it last saw
    and what the rank tests derive from the baseline alone -- its sorted half
    of the pooled sort and its moments -- and a row whose baseline still
    compares equal, bit for bit, skips that work.  The comparison is made on
    the device for every row of every tick: nothing is expected by the host, a
    rewritten baseline row simply recomputes and refreshes its entry, and the
    results are the same bits with and without the cache.  One cache per
    baseline tensor: ``split_launchers`` / ``capture_front`` hold theirs for
    the launcher's life, ``score_resident`` keeps it while the tensor lives
    (a replaced baseline tensor frees its cache); ``score`` and
    ``front_only`` take whatever tensor the caller brings and use none.
    A row's entry is read and written by the wave that ranks the row with no
    ordering beyond the stream's, so launches that share a cache run one at a
    time -- the rule the pairwise row queue (``_pqueue``) already sets for
    every front launch of one scorer.
    """

    def __init__(self, aliases: list[str], cfg: BrainConfig | None = None, device="cpu", overlap: bool = True,
                 mode: str | None = None, hist_blocks: int = 0, pw_blocks: int = 0, pw_cap_rows: int = 32,
                 front_wgs: tuple[float, float] | None = None, front_queue: bool = True,
                 xcd_balance: bool | None = None, hist_cache: bool = True,
                 front_hot_wgs: tuple[float, float] | None = None, model: str = "moving_average_all",
                 codes=None, tail_z: float = 2.0, base_cache: bool = True):
        """``model``: what the history statistics ``hs [R, 3]`` are --
        ``moving_average_all`` (mean, std, n) or ``robust_moving_average_all``
        (median, 1.4826 MAD or its mean-deviation fallback, n: K13 / K18).  The
        band centre +/- thr * sigma, the thresholds, bounds, pairwise factor,
        history gate and service reduce are the same code for both.  The
        robust model ticks through ``score`` and ``score_resident`` only (no
        graph capture, split launchers or ``mode="fused"``).

        ``band_mix`` is a per-metric mix of the static band models: ``codes``
        names each metric's model (``ops.misc.BAND_CODES``: 0 mean / std, 1
        median / MAD, 2 ``quantile_robust`` with the tail parameter
        ``tail_z``), the statistics are band records ``bs [R, 4]`` = (centre,
        sigma_lo, sigma_up, n) from K25 (``fm_band_stats_cached``, a resident
        store's ``bcache``) and the decision takes a sigma per side
        (``fm_decide_services_2s``).  At most 16 metrics; it ticks through
        ``score`` and ``score_resident`` only, as the robust model.

        ``hist_cache`` (and env ``FM_HIST_CACHE``, ``0`` = off): keep each
        history row's (mean, std, n) across ticks where the history has an
        owner that reports its writes -- a static ``ResidentHistory``
        (``score_resident``) or the tensor bound by ``split_launchers`` /
        ``capture_front``.  A tick then reads only the rows written since the
        previous one; results are the same floats.  See
        :meth:`invalidate_history` for writers the owner cannot see.

        ``base_cache`` (and env ``FM_BASE_CACHE``, ``0`` = off): the baseline
        cache of the class docstring; off, every front launch passes null
        cache pointers and runs the kernels without it."""
        self.mode = mode or ("front" if overlap else "serial")
        if self.mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}")
        if model not in MODELS:
            raise ValueError(f"model must be one of {MODELS}")
        self.model = model
        self.robust = model == "robust_moving_average_all"
        self.band = model == "band_mix"
        if (self.robust or self.band) and self.mode == "fused":
            raise ValueError(f"mode='fused' reads mean/std off the row image: not available for model={model!r}")
        if self.band:
            from ..ops import misc as MI
            if codes is None or len(codes) != len(aliases) or any(int(c) not in (0, 1, 2) for c in codes):
                raise ValueError("model='band_mix' takes codes, one of 0, 1, 2 (ops.misc.BAND_CODES) per metric")
            if len(aliases) > MI.BAND_MAX_METRICS:
                raise ValueError(f"model='band_mix' supports up to {MI.BAND_MAX_METRICS} metrics per service")
            self.codes = tuple(int(c) for c in codes)
            self.tail_z = MI.quantile_tail_z(tail_z)
            self.code_mask = 0
            for c in self.codes:
                self.code_mask |= 1 << c
            self._codes_d = torch.tensor(self.codes, dtype=torch.int32, device=torch.device(device))
        elif codes is not None:
            raise ValueError("codes belong to model='band_mix'")
        self.gate = C.EffectGate.from_config(cfg or BrainConfig())
        if self.gate.enabled and self.mode == "fused":
            raise ValueError("mode='fused' is not available with the pairwise effect gate (ML_PAIRWISE_MIN_EFFECT / "
                             "_MIN_SHIFT / _MIN_SHIFT_ABS / _DIRECTIONAL) enabled")
        self.scale = C.ScaleTest.from_config(cfg or BrainConfig())
        if self.scale.enabled and self.mode == "fused":
            raise ValueError("mode='fused' is not available with the pairwise scale test (ML_PAIRWISE_SCALE_TEST) "
                             "enabled")
        self.overlap = self.mode == "overlap"
        # workgroup caps of the two concurrent kernels of the overlap tick
        # (0 = one workgroup per row / per 4 rows); see tools/tick_breakdown.py
        self.hist_blocks, self.pw_blocks = hist_blocks, pw_blocks
        # cap the pairwise grid only when each capped workgroup still loops
        # over more than this many rows (per workgroup of 4 waves)
        self.pw_cap_rows = pw_cap_rows
        self._side = None
        self.cfg = cfg or BrainConfig()
        self.aliases = list(aliases)
        self.M = len(aliases)
        self.device = torch.device(device)
        if self.mode == "overlap" and self.device.type == "cuda":
            # Concurrent kernels of the tick, capped in workgroups per CU
            # (tools/tick_breakdown.py sweeps, 80k rows): pairwise at 1 WG/CU
            # (one wave per SIMD) and the persistent history stream at 8 WG/CU
            # give 597-613 us vs 668-700 us uncapped; fewer pairwise workgroups
            # make the side stream the critical path (0.5 WG/CU: ~800 us).
            cus = torch.cuda.get_device_properties(self.device).multi_processor_count
            if pw_blocks == 0:
                self.pw_blocks = cus
            if hist_blocks == 0:
                self.hist_blocks = 8 * cus
        # front mode: (pairwise, history) workgroups per CU, 0 = one per 4 rows /
        # one per row (tools/tick_breakdown.py SWEEP_FRONT)
        # (front_wgs shapes the ticks that stream history; a tick whose rows
        # are all expected in the row-statistics cache has no history stream
        # to make room for: front_hot_wgs, workgroups per CU again)
        self.front_wgs = front_wgs or (1.0, 4.0)
        # dynamic row queue of the pairwise role (tick_front.hip, fm_tick_front's
        # pqueue / q_ranges; FM_FRONT_DYN_Q=0 keeps static rows): ranges
        self._q_ranges = int(os.environ.get("FM_FRONT_DYN_Q", "64")) if self.device.type == "cuda" else 0
        if front_hot_wgs is None:
            # with the queue (and its rotating wave priority) four pairwise
            # workgroups per CU measure faster than five (docs/PERF.md,
            # "Dynamic pairwise rows"); static rows keep five
            front_hot_wgs = tuple(float(x) for x in os.environ.get(
                "FM_FRONT_HOT_WGS", "4:0.25" if self._q_ranges > 0 else "5:0.25").split(":"))
        self.front_hot_wgs = front_hot_wgs
        self.hist_cache = hist_cache and os.environ.get("FM_HIST_CACHE", "1") != "0"
        self._bound: dict[int, _BoundHist] = {}            # id(history tensor) -> its cache
        self._store_caches = weakref.WeakSet()             # caches of resident stores this scorer has ticked
        self.base_cache = base_cache and os.environ.get("FM_BASE_CACHE", "1") != "0"
        # id(baseline tensor) -> (weak reference to it, its _BaseCache); the entry goes when the tensor dies
        self._base_caches: dict[int, tuple] = {}
        # dynamic history-row queue (8 per-XCD counters, kept zero between
        # launches by the kernel itself) + the XCD-balance control block
        self._queue = (torch.zeros(8 * 32 + 64, dtype=torch.int32, device=self.device)
                       if front_queue and self.device.type == "cuda" else None)
        # (None = env FM_XCD_BALANCE, default on: one fleet per scorer, every
        # tick the same rows -- bench.py, 0.542 vs 0.554 ms)
        if xcd_balance is None:
            xcd_balance = os.environ.get("FM_XCD_BALANCE", "1") != "0"
        if self._queue is not None and xcd_balance:
            self._queue[8 * 32 + 31] = 1      # control block: XCD-balanced history ranges (tick_front.hip kXcdCtl)
        # the pairwise row queue: one counter line per range, kept zero between
        # launches by the kernel itself.  One front launch of this scorer at a
        # time -- which also serialises the launches that share a baseline
        # cache (_base_caches): its entries are read and rewritten in place
        self._pqueue = (torch.zeros(self._q_ranges * 32, dtype=torch.int32, device=self.device)
                        if self._q_ranges > 0 else None)
        self._cus = (torch.cuda.get_device_properties(self.device).multi_processor_count
                     if self.device.type == "cuda" else 0)
        rules = [self.cfg.rule_for(a) for a in aliases]
        self.thr = torch.tensor([r.threshold for r in rules], dtype=torch.float32, device=self.device)
        self.bound = torch.tensor([r.bound for r in rules], dtype=torch.int32, device=self.device)
        self.minlb = torch.tensor([r.min_lower_bound for r in rules], dtype=torch.float32, device=self.device)
        self.pcfg = C.PairwiseConfig(self.cfg.pairwise_algorithm, self.cfg.pairwise_threshold,
                                     self.cfg.min_mann_white, self.cfg.min_wilcoxon, self.cfg.min_kruskal)
        self._out: dict[tuple, CanaryOutputs] = {}
        self._graph = None
        self._graph_key = None

    def _alloc(self, R: int, n_cur: int, slot: int = 0) -> CanaryOutputs:
        key = (R, n_cur, slot)
        if key not in self._out:
            d = self.device
            self._out[key] = CanaryOutputs(
                pvals=torch.empty((R, C.N_TESTS), dtype=torch.float32, device=d),
                pstats=torch.empty((R, C.N_TESTS), dtype=torch.float32, device=d),
                diff=torch.empty((R,), dtype=torch.int8, device=d),
                suff=torch.empty((R, C.SUFF), dtype=torch.float64, device=d),
                hs=torch.empty((R, 3), dtype=torch.float32, device=d),
                decide=C.alloc_decide(R, n_cur, d),
                packed=torch.empty((R // self.M, 4), dtype=torch.float32, device=d),
            )
            if self.gate.enabled:
                e = C.alloc_effect(R, d)
                o = self._out[key]
                o.effect, o.effect_counts, o.effect_passed, o.pvals_gated = e.effect, e.counts, e.passed, e.pvals_gated
            if self.scale.enabled:
                s = C.alloc_scale(R, d)
                o = self._out[key]
                o.scale, o.scale_diff, o.pvals_scaled, o.scale_moments = s.scale, s.scale_diff, s.pvals_scaled, s.moments
            if self.band:
                self._out[key].bs = torch.empty((R, 4), dtype=torch.float32, device=d)
        return self._out[key]

    # -- effect-size gate (K19) ----------------------------------------------
    def _no_gate(self, what: str) -> None:
        if self.gate.enabled:
            raise ValueError(f"{what} is not available with the pairwise effect gate enabled "
                             "(it ticks through score / score_resident only)")
        if self.scale.enabled:
            raise ValueError(f"{what} is not available with the pairwise scale test enabled "
                             "(it ticks through score / score_resident only)")

    def _gate_into(self, cur, base, o: CanaryOutputs) -> CanaryOutputs:
        """K19 on the current stream, after the p-values of ``o`` exist and
        before the decision reads them: fills the gate buffers of ``o``
        (``pvals_gated`` is what ``_decide_call_args`` then hands on).
        Returns ``o``, or its copy without gate outputs when the tick has no
        gate or no baseline.  The scale test (K27), where it is on, runs right
        behind it on what the gate hands on and fills ``scale`` /
        ``scale_diff`` / ``pvals_scaled`` the same way."""
        if not (self.gate.enabled or self.scale.enabled):
            return o
        if base is None or base.shape[1] == 0:
            return dataclasses.replace(o, effect=None, effect_counts=None, effect_passed=None, pvals_gated=None,
                                       scale=None, scale_diff=None, pvals_scaled=None)
        if self.gate.enabled:
            buf = C.EffectResult(o.effect, o.effect_counts, o.effect_passed, o.pvals_gated)
            r = C.pairwise_effect(cur, base, self.gate, self.bound, self.M, o.pvals, out=buf)
            if r is not buf:                      # padded wider than C.PAIRWISE_MAX: bucketed, its own tensors
                o.effect.copy_(r.effect)
                o.effect_counts.copy_(r.counts)
                o.effect_passed.copy_(r.passed)
                o.pvals_gated.copy_(r.pvals_gated)
        if self.scale.enabled:
            buf = C.ScaleResult(o.scale, o.scale_diff, o.pvals_scaled, o.scale_moments)
            r = C.pairwise_scale(cur, base, self.scale, o.pvals_gated if self.gate.enabled else o.pvals, out=buf)
            if r is not buf:                      # padded wider than K27 takes: bucketed, its own tensors
                o.scale.copy_(r.scale)
                o.scale_diff.copy_(r.scale_diff)
                o.pvals_scaled.copy_(r.pvals_scaled)
        return o

    def _gate_cpu(self, cur, base, pv, df):
        """CPU branches: ((diff & passed) | scale_diff, (EffectResult or None,
        ScaleResult or None))."""
        if base is None or base.shape[1] == 0:
            return df, (None, None)
        eff = sc = None
        if self.gate.enabled:
            eff = C.pairwise_effect(cur, base, self.gate, self.bound, self.M, pv.contiguous())
            df = df & eff.passed
        if self.scale.enabled:
            sc = C.pairwise_scale(cur, base, self.scale, pv.contiguous() if eff is None else eff.pvals_gated)
            df = df | sc.scale_diff
        return df, (eff, sc)

    @staticmethod
    def _with_effect(o: CanaryOutputs, got) -> CanaryOutputs:
        r, s = got
        if r is not None:
            o.effect, o.effect_counts, o.effect_passed, o.pvals_gated = r.effect, r.counts, r.passed, r.pvals_gated
        if s is not None:
            o.scale, o.scale_diff, o.pvals_scaled = s.scale, s.scale_diff, s.pvals_scaled
        return o

    def score(self, hist: torch.Tensor, base: torch.Tensor | None, cur: torch.Tensor,
              n_hist: int | None = None, packed_out: torch.Tensor | None = None) -> CanaryOutputs:
        """``packed_out`` ([S, 4] fp32, optional): where the service verdicts
        go instead of the scorer's own buffer (one per in-flight tick when
        the consumer of tick k overlaps tick k+1)."""
        R = cur.shape[0]
        if self.robust:
            return self._score_robust(hist, base, cur, n_hist, packed_out)
        if self.band:
            return self._score_band(hist, base, cur, n_hist, packed_out)
        if not cur.is_cuda:
            if base is not None and base.shape[1] > 0:
                pv, ps, df = C.pairwise_tests(cur, base, self.pcfg)
            else:
                pv = torch.full((R, C.N_TESTS), float("nan"))
                ps = pv.clone()
                df = torch.zeros((R,), dtype=torch.int8)
            df, eff = self._gate_cpu(cur, base, pv, df)
            dec = C.stats_decide(hist, cur, n_hist, self.M, self.thr, self.bound, self.minlb, df,
                                 self.cfg.pairwise_threshold_factor, self.cfg.min_historical_points)
            packed = C.service_reduce(dec.count, dec.score, dec.valid, self.M)
            return self._with_effect(CanaryOutputs(pv, ps, df, None, dec, packed), eff)
        o = self._alloc(R, cur.shape[1])
        if packed_out is not None:
            C.check(packed_out.shape == o.packed.shape and packed_out.is_contiguous()
                    and packed_out.dtype == torch.float32, "packed_out must be a contiguous fp32 [S, 4] tensor")
            o = dataclasses.replace(o, packed=packed_out)
        has_base = base is not None and base.shape[1] > 0
        if not has_base:
            o = self._gate_into(cur, None, o)
        if self.mode == "front" and has_base and cur.shape[1] + base.shape[1] <= 256:
            self._front(hist, base, cur, n_hist, o)
            return o
        if self.mode == "fused":
            self._fused(hist, base if has_base else None, cur, n_hist, o)
            return o
        elif self.mode == "serial":
            if has_base:
                self._pairwise_into(cur, base, o)
                if self.gate.enabled or self.scale.enabled:
                    # this mode's decision kernel reads `diff`, not the p-values
                    self._gate_into(cur, base, o)
                    if self.gate.enabled:
                        o.diff.mul_(o.effect_passed)
                    if self.scale.enabled:
                        o.diff.bitwise_or_(o.scale_diff)
            C.stats_decide(hist, cur, n_hist, self.M, self.thr, self.bound, self.minlb,
                           o.diff if has_base else None, self.cfg.pairwise_threshold_factor,
                           self.cfg.min_historical_points, out=o.decide)
        else:
            # fork: pairwise (compute-bound) on a side stream || history stats
            # (HBM-bound) on the main stream; join; tiny threshold/decide pass
            from ..ops._lib import LIB, ptr, stream_of
            dev = cur.device
            main = torch.cuda.current_stream(dev)
            T = hist.shape[1] if n_hist is None else int(n_hist)
            C.check(hist.stride(0) % 4 == 0 and hist.data_ptr() % 16 == 0, "history rows must be 16-B aligned")
            if has_base:
                # the capped pairwise grid is issued first so its workgroups
                # are resident before the persistent history grid fills the
                # CUs (history first serialises the two: 0.60 -> 0.87 ms)
                side = self._side_stream(dev)
                side.wait_stream(main)
                # the cap only pays when each capped wave still loops over many
                # rows; a small shard (per-GPU slice of a multi-GPU fleet) runs
                # one row per wave
                cap = self.pw_blocks if R > self.pw_cap_rows * self.pw_blocks else 0
                with torch.cuda.stream(side):
                    self._pairwise_into(cur, base, o, cap, combine=False)
            LIB.call("fm_hist_stats_capped", ptr(hist), hist.stride(0), T, R, ptr(o.hs), self.hist_blocks,
                     stream_of(hist))
            if has_base:
                main.wait_stream(side)
                self._gate_into(cur, base, o)
            self._decide_services(cur, o, has_base)
            return o
        C.service_reduce(o.decide.count, o.decide.score, o.decide.valid, self.M, out=o.packed)
        return o

    # -- resident history (the brain's production path) ----------------------
    def score_resident(self, hview, rowmap: torch.Tensor, cur: torch.Tensor, base: torch.Tensor | None,
                       slot: int = 0) -> CanaryOutputs:
        """The tick over rows of the device-resident history store
        (engine/resident.py): logical row r reads history row ``rowmap[r]`` of
        ``hview.hist`` in place.  GPU: one role-split front launch when the
        pairwise windows fit a wave-sorted 256 (n_cur + n_base <= 256),
        otherwise history stats || pairwise (the wave kernel up to
        C.PAIRWISE_MAX, the workgroup kernel K21 up to C.PAIRWISE_WIDE_MAX, the CPU
        oracle beyond) — then the decision kernel.  Rows are services x M.
        A view that carries a row-statistics cache (a static store's) has only
        the rows written since their last tick reduced again; a hand-made
        ``HistView`` without one streams every row, as does ``hist_cache=False``."""
        R = cur.shape[0]
        has_base = base is not None and base.shape[1] > 0
        if not cur.is_cuda:
            if self.robust and self.hist_cache and getattr(hview, "rcache", None) is not None:
                self._store_caches.add(hview.rcache)       # (invalidate_history reaches it on either device)
            if self.band and self.hist_cache and getattr(hview, "bcache", None) is not None:
                self._store_caches.add(hview.bcache)
            hist = hview.hist.index_select(0, rowmap.to(torch.int64))
            return self.score(hist, base if has_base else None, cur, hview.T)
        from ..ops._lib import LIB, ptr, stream_of
        C.check(rowmap.dtype == torch.int32 and rowmap.numel() == R and rowmap.is_cuda, "rowmap must be int32 [R]")
        C.check(hview.ld % 4 == 0 and hview.hist.data_ptr() % 16 == 0, "history rows must be 16-B aligned")
        C.check(self.M <= 16, "resident tick supports up to 16 metrics per service")
        o = self._gate_into(cur, None, self._alloc(R, cur.shape[1], slot)) if not has_base \
            else self._alloc(R, cur.shape[1], slot)
        st = stream_of(cur)
        n = cur.shape[1] + (base.shape[1] if has_base else 0)
        if self.robust:
            return self._resident_robust(hview, rowmap, cur, base if has_base else None, o, st)
        if self.band:
            return self._resident_band(hview, rowmap, cur, base if has_base else None, o, st)
        # a static store's rows keep their statistics between its writes
        cache = getattr(hview, "cache", None) if self.hist_cache else None
        miss = True
        if cache is not None:
            self._store_caches.add(cache)
            miss = cache.expect_miss(hview.T, R)
        if has_base and n <= 256:
            # (the baseline cache lives as long as the caller's baseline tensor does)
            LIB.call("fm_tick_front_bc",
                     *self._front_args(ptr(hview.hist), hview.ld, hview.T, base, cur, o, rowmap, cache, miss,
                                       self._base_cache_of(base, cur)), st)
        else:
            c_stats, c_valid = (ptr(cache.stats), ptr(cache.valid)) if cache is not None else (None, None)
            LIB.call("fm_hist_stats_cached", ptr(hview.hist), hview.ld, hview.T, R, ptr(o.hs), 0, ptr(rowmap),
                     c_stats, c_valid, int(miss), st)
            if has_base and n <= C.PAIRWISE_MAX:
                self._pairwise_into(cur, base, o, combine=False)
            elif has_base:
                # padded wider than the register sort: rows bucketed by their
                # own widths, rows of more than C.PAIRWISE_MAX pooled points
                # on K21, only those beyond C.PAIRWISE_WIDE_MAX on the fp64
                # CPU oracle
                p, s_, _ = C.pairwise_tests(cur, base, self.pcfg)
                o.pvals.copy_(p)
                o.pstats.copy_(s_)
        if cache is not None:
            cache.ticked(hview.T)
        if has_base:
            self._gate_into(cur, base, o)
        self._decide_services(cur, o, has_base)
        return o

    # -- robust_moving_average_all ------------------------------------------
    def _score_robust(self, hist, base, cur, n_hist, packed_out) -> CanaryOutputs:
        """``score`` of the robust model: K13 into ``hs``, the pairwise tests,
        the decision kernel.  No cache: the tensor has no owner."""
        R = cur.shape[0]
        T = hist.shape[1] if n_hist is None else int(n_hist)
        has_base = base is not None and base.shape[1] > 0
        if not cur.is_cuda:
            import numpy as np
            from ..ops.misc import ref_robust_stats
            from ..ops.smoothing import ref_band_decide
            if has_base:
                pv, ps, df = C.pairwise_tests(cur, base, self.pcfg)
            else:
                pv = torch.full((R, C.N_TESTS), float("nan"))
                ps = pv.clone()
                df = torch.zeros((R,), dtype=torch.int8)
            df, eff = self._gate_cpu(cur, base if has_base else None, pv, df)
            c, s, n = ref_robust_stats(hist.numpy(), T)
            x = cur.numpy()
            with np.errstate(invalid="ignore", over="ignore"):
                up, lo, flags, cnt, sc = ref_band_decide(x, c[:, None], s, self.M, self.thr.numpy(), self.bound.numpy(),
                                                         self.minlb.numpy(), df.numpy(),
                                                         self.cfg.pairwise_threshold_factor)
            # the history gate of the decision kernel: a row without enough
            # history flags nothing and scores nothing
            has = torch.from_numpy((n >= self.cfg.min_historical_points) & (n > 0))
            cnt = torch.where(has, cnt, torch.zeros_like(cnt))
            sc = torch.where(has, sc, torch.zeros_like(sc))
            flags = torch.where(has[:, None], flags, torch.zeros_like(flags))
            valid = has.to(torch.int32) | (torch.from_numpy(np.isfinite(x).any(1)).to(torch.int32) << 1)
            stats = torch.stack([torch.from_numpy(c), torch.from_numpy(s), up[:, 0], lo[:, 0]], 1)
            dec = C.DecideResult(stats, flags, cnt, sc, valid)
            return self._with_effect(CanaryOutputs(pv, ps, df, None, dec, C.service_reduce(cnt, sc, valid, self.M)),
                                     eff)
        from ..ops._lib import LIB, ptr, stream_of
        C.check(hist.dim() == 2 and hist.dtype == torch.float32 and (hist.stride(1) == 1 or hist.shape[1] <= 1)
                and hist.shape[0] == R and 0 <= T <= hist.shape[1],
                "history must be fp32 [R, >= T] with unit column stride")
        o = self._alloc(R, cur.shape[1])
        if packed_out is not None:
            C.check(packed_out.shape == o.packed.shape and packed_out.is_contiguous()
                    and packed_out.dtype == torch.float32, "packed_out must be a contiguous fp32 [S, 4] tensor")
            o = dataclasses.replace(o, packed=packed_out)
        LIB.call("fm_robust_stats", ptr(hist), hist.stride(0), T, R, ptr(o.hs), stream_of(cur))
        if has_base:
            self._pairwise_wide(cur, base, o)
        o = self._gate_into(cur, base if has_base else None, o)
        self._decide_services(cur, o, has_base)
        return o

    def _pairwise_wide(self, cur, base, o: CanaryOutputs) -> None:
        """p-values of windows of any width: the wave kernels up to
        C.PAIRWISE_MAX pooled points; above, rows bucketed by their used widths
        (C.pairwise_tests): K21 up to C.PAIRWISE_WIDE_MAX, the fp64 CPU oracle beyond."""
        if cur.shape[1] + base.shape[1] <= C.PAIRWISE_MAX:
            self._pairwise_into(cur, base, o, combine=False)
        else:
            p, s_, _ = C.pairwise_tests(cur, base, self.pcfg)
            o.pvals.copy_(p)
            o.pstats.copy_(s_)

    def _resident_robust(self, hview, rowmap, cur, base, o: CanaryOutputs, st: int) -> CanaryOutputs:
        """``score_resident`` of the robust model on the GPU: K18 fills ``hs``
        from the store's robust row-statistics cache (selecting only the rows
        written since their last robust tick), then the pairwise kernels, then
        the decision kernel, all on the stream of ``cur``."""
        from ..ops._lib import LIB, ptr
        R = cur.shape[0]
        T = hview.T
        cache = getattr(hview, "rcache", None) if self.hist_cache else None
        miss = True
        if cache is not None:
            self._store_caches.add(cache)
            miss = cache.expect_miss(T, R)
        c_stats, c_valid = (ptr(cache.stats), ptr(cache.valid)) if cache is not None else (None, None)
        # streaming: a workgroup per row; scan: two workgroups per CU (what the
        # LDS of a 7-day row lets a CU hold), so a batch of arrivals spreads out
        LIB.call("fm_robust_stats_cached", ptr(hview.hist), hview.ld, T, R, ptr(o.hs), ptr(rowmap), c_stats, c_valid,
                 int(miss), 0 if miss else 2 * self._cus, st)
        # (the pairwise tests as their own launches: the role-split front launch
        # in its all-hit shape over the robust cache measured 4 % slower here,
        # docs/PERF.md K18, and would have to be kept from ever meeting an
        # invalid tag, whose row it would fill with mean / std)
        if base is not None:
            self._pairwise_wide(cur, base, o)
        o = self._gate_into(cur, base, o)
        self._decide_services(cur, o, base is not None)
        if cache is not None:
            cache.ticked(T)
        return o

    # -- band_mix: a per-metric mix of the static band models ------------------
    def _score_band(self, hist, base, cur, n_hist, packed_out) -> CanaryOutputs:
        """``score`` of the mix: K25 without a cache (the tensor has no owner)
        into ``bs``, the pairwise tests, the gate, the two-sigma decision."""
        from ..ops import misc as MI
        R = cur.shape[0]
        T = hist.shape[1] if n_hist is None else int(n_hist)
        has_base = base is not None and base.shape[1] > 0
        if not cur.is_cuda:
            if has_base:
                pv, ps, df = C.pairwise_tests(cur, base, self.pcfg)
            else:
                pv = torch.full((R, C.N_TESTS), float("nan"))
                ps = pv.clone()
                df = torch.zeros((R,), dtype=torch.int8)
            df, eff = self._gate_cpu(cur, base if has_base else None, pv, df)
            rec, _ = MI.ref_band_stats(hist.numpy(), T, self.codes, self.tail_z)
            dec, packed, _ = C.ref_decide_services_2s(rec, cur.numpy(), self.M, self.thr.numpy(), self.bound.numpy(),
                                                      self.minlb.numpy(), self.cfg.pairwise_threshold_factor,
                                                      self.cfg.min_historical_points, diff=df.numpy())
            return self._with_effect(CanaryOutputs(pv, ps, df, None, dec, packed, bs=torch.from_numpy(rec)), eff)
        C.check(hist.dim() == 2 and hist.dtype == torch.float32 and (hist.stride(1) == 1 or hist.shape[1] <= 1)
                and hist.shape[0] == R and 0 <= T <= hist.shape[1],
                "history must be fp32 [R, >= T] with unit column stride")
        o = self._alloc(R, cur.shape[1])
        if packed_out is not None:
            C.check(packed_out.shape == o.packed.shape and packed_out.is_contiguous()
                    and packed_out.dtype == torch.float32, "packed_out must be a contiguous fp32 [S, 4] tensor")
            o = dataclasses.replace(o, packed=packed_out)
        MI.band_stats_cached(hist, T, None, self.codes, None, self.tail_z, out=o.bs, codes_dev=self._codes_d)
        if has_base:
            self._pairwise_wide(cur, base, o)
        o = self._gate_into(cur, base if has_base else None, o)
        self._decide_services(cur, o, has_base)
        return o

    def _resident_band(self, hview, rowmap, cur, base, o: CanaryOutputs, st: int) -> CanaryOutputs:
        """``score_resident`` of the mix on the GPU: K25 fills ``bs`` from the
        store's band-record cache (computing only the rows written since their
        last tick under this model and view length), then the pairwise kernels,
        the gate and the two-sigma decision, all on the stream of ``cur``."""
        from ..ops import misc as MI
        from ..ops._lib import LIB, ptr
        R = cur.shape[0]
        T = hview.T
        C.check(T < (1 << MI.BAND_TAG_SHIFT) and (not (self.code_mask & 1) or T <= MI.BAND_MEAN_MAX_T),
                "the view is longer than the band-record kernel takes")
        cache = getattr(hview, "bcache", None) if self.hist_cache else None
        miss = True
        if cache is not None:
            self._store_caches.add(cache)
            cache.rekey(self.tail_z)
            miss = cache.expect_miss(T, R)
        c_stats, c_valid = (ptr(cache.stats), ptr(cache.valid)) if cache is not None else (None, None)
        p, iz = MI.quantile_tail_params(self.tail_z)
        # streaming: a workgroup per row; hits: two workgroups per CU, as K18
        LIB.call("fm_band_stats_cached", ptr(hview.hist), hview.ld, T, R, self.M, ptr(self._codes_d), self.code_mask,
                 p, float(iz), ptr(o.bs), ptr(rowmap), c_stats, c_valid, int(miss), 0 if miss else 2 * self._cus, st)
        if base is not None:
            self._pairwise_wide(cur, base, o)
        o = self._gate_into(cur, base, o)
        self._decide_services(cur, o, base is not None)
        if cache is not None:
            cache.ticked(T)
        return o

    def _no_robust(self, what: str) -> None:
        """The forms that bind mean / std history (graph capture, the front
        launch alone, the split launchers) take ``moving_average_all`` only."""
        if self.robust or self.band:
            raise ValueError(f"{what} is not available for model={self.model!r}")

    def _front_grid(self, miss: bool) -> tuple[int, int]:
        """(pairwise, history) workgroups of a front launch: ``front_wgs`` per
        CU when the tick streams history rows, ``front_hot_wgs`` when every row
        is expected in the row-statistics cache."""
        fp, fh = self.front_wgs if miss else self.front_hot_wgs
        n_p = int(fp * self._cus) if fp > 0 else 0
        n_h = int(fh * self._cus) if fh > 0 else 0
        return n_p, (n_h if miss or fh <= 0 else max(1, n_h))

    def _base_cache_of(self, base: torch.Tensor, cur: torch.Tensor) -> _BaseCache | None:
        """The baseline cache of ``base`` for ticks against ``cur`` (one per
        baseline tensor, sized to its rows, shared by the launchers of every
        slot), or None: switched off, or a window shape the kernel has no
        cache for.  Held through a weak reference to the tensor: when ``base``
        dies its cache goes with it (a launcher that needs it longer keeps
        both).  Keyed by the tensor object, like ``_bound``: a caller that
        builds a new view of its baseline for every tick gets a new, empty
        cache every tick and pays the miss path each time -- pass the same
        tensor, as the fast path's groups do with ``base_d``."""
        n_cur, n_base = cur.shape[1], base.shape[1]
        if (not self.base_cache or n_cur > 64 or n_base > 64 or n_cur + n_base <= 64
                or base.shape[0] < cur.shape[0]):
            return None
        key = id(base)
        ent = self._base_caches.get(key)
        if ent is not None and ent[0]() is base and len(ent[1]) == base.shape[0]:
            return ent[1]
        caches = self._base_caches

        def drop(ref, key=key):
            if key in caches and caches[key][0] is ref:
                del caches[key]
        bc = _BaseCache(base.shape[0], base.device)
        caches[key] = (weakref.ref(base, drop), bc)
        return bc

    def _front_args(self, hist_ptr, ld: int, T: int, base, cur, o: CanaryOutputs, rowmap, cache, miss: bool,
                    bcache: _BaseCache | None = None) -> tuple:
        """Arguments of fm_tick_front_bc, all but the stream: the history
        (pointer, leading dimension, view length), ``rowmap`` (int32 [R]) or
        None, its row-statistics cache or None, and whether the tick is
        expected to miss (the launch streams the rows) or to hit; then the
        pairwise row queue unless it is switched off, and the three arrays of
        the baseline cache ``bcache`` or nulls."""
        from ..ops._lib import ptr
        n_p, n_h = self._front_grid(miss)
        c_stats, c_valid = (ptr(cache.stats), ptr(cache.valid)) if cache is not None else (None, None)
        dyn = (ptr(self._pqueue), self._q_ranges) if self._pqueue is not None else (None, 0)
        bc = (ptr(bcache.raw), ptr(bcache.sorted), ptr(bcache.stats)) if bcache is not None else (None, None, None)
        return (hist_ptr, ld, T, cur.shape[0], ptr(o.hs), ptr(cur), cur.stride(0), cur.shape[1], ptr(base),
                base.stride(0), base.shape[1], ptr(o.suff), n_p, n_h, self.pcfg.min_mann_white, self.pcfg.min_wilcoxon,
                self.pcfg.min_kruskal, ptr(o.pvals), ptr(o.pstats), ptr(self._queue), ptr(rowmap), c_stats, c_valid,
                int(miss), *dyn, *bc)

    def _bind(self, hist: torch.Tensor) -> _BoundHist | None:
        """The row-statistics cache of a history tensor bound to a launcher
        (one per tensor, shared by the launchers of every slot)."""
        if not self.hist_cache:
            return None
        bh = self._bound.get(id(hist))
        if bh is None or bh.hist is not hist:
            bh = self._bound[id(hist)] = _BoundHist(hist)
        return bh

    def invalidate_history(self) -> None:
        """Drop every cached row statistic this scorer can reach: the caches of
        the tensors bound by ``split_launchers`` / ``capture_front`` and of the
        resident stores it has ticked (a robust scorer: the stores' robust
        caches; a ``band_mix`` scorer: their band-record caches).  The next
        tick of each recomputes all rows.

        The caches see a write in two ways only: a ``ResidentHistory`` clears
        the rows it writes itself, and a bound tensor is watched through
        torch's version counter.  A write that passes neither -- a raw kernel
        or a copy through the tensor's pointer, another process through IPC,
        ``tensor.data`` tricks that do not bump the version -- is a blind
        spot: whoever does that calls this afterwards, on the stream of the
        write or after synchronising with it.

        The baseline caches need none of this and are not touched here: every
        row compares the baseline it loads with its entry on the device, so
        it sees every write, however it was made."""
        for bh in self._bound.values():
            bh.version = -1                        # invalidated by the next launch, on its own stream
        for cache in self._store_caches:
            cache.invalidate()

    # -- split tick: front kernel and decision on different streams ----------
    def front_only(self, hist, base, cur, n_hist=None, packed_out=None, slot: int = 0) -> CanaryOutputs:
        """First half of a front-mode tick (pairwise tests, p-values, history
        stats: one launch) into the buffers of ``slot``.  ``decide_only`` on
        the returned outputs finishes the tick; with one buffer set per
        in-flight step, the decision of tick k can run on another stream
        while tick k+1's front kernel runs."""
        self._no_robust("front_only")
        self._no_gate("front_only")
        C.check(cur.is_cuda and self.mode == "front" and base is not None and base.shape[1] > 0
                and cur.shape[1] + base.shape[1] <= 256, "front_only needs a GPU front-mode tick with a baseline")
        o = self._alloc(cur.shape[0], cur.shape[1], slot)
        if packed_out is not None:
            C.check(packed_out.shape == o.packed.shape and packed_out.is_contiguous()
                    and packed_out.dtype == torch.float32, "packed_out must be a contiguous fp32 [S, 4] tensor")
            o = dataclasses.replace(o, packed=packed_out)
        self._front(hist, base, cur, n_hist, o, decide=False)
        return o

    def decide_only(self, cur, o: CanaryOutputs) -> CanaryOutputs:
        """Second half of a split tick (p-value combine, window decision,
        service reduce: one launch) on the current stream."""
        self._decide_services(cur, o, True)
        return o

    def capture_front(self, hist, base, cur, n_hist=None, packed_out=None, slot: int = 0):
        """Graph of ``front_only`` for one buffer slot; returns (replay, outputs).

        ``hist`` is bound for the life of the replay callable (it holds a
        reference) and its row statistics are cached: two graphs are captured,
        one that streams every history row and records it, one that expects
        every row cached; ``replay`` picks per call.  A change of
        ``hist._version`` (any torch write) makes the next replay invalidate
        the cache, with a launch of its own ahead of the graph, and stream the
        rows again; for writes torch does not see, :meth:`invalidate_history`."""
        self._no_robust("capture_front")
        self._no_gate("capture_front")
        o = self.front_only(hist, base, cur, n_hist, packed_out, slot)   # warm / allocate
        torch.cuda.synchronize(cur.device)
        bh = self._bind(hist)
        T = hist.shape[1] if n_hist is None else int(n_hist)
        R = cur.shape[0]

        def capture(body):
            g = torch.cuda.CUDAGraph()
            s = torch.cuda.Stream(cur.device)
            s.wait_stream(torch.cuda.current_stream(cur.device))
            with torch.cuda.stream(s):
                with torch.cuda.graph(g, stream=s):
                    body()
            torch.cuda.current_stream(cur.device).wait_stream(s)
            return g
        if bh is None:
            return capture(lambda: self.front_only(hist, base, cur, n_hist, packed_out, slot)).replay, o
        from ..ops._lib import LIB, ptr, stream_of
        bc = self._base_cache_of(base, cur)
        graphs = {miss: capture(lambda miss=miss: LIB.call(
            "fm_tick_front_bc", *self._front_args(ptr(hist), hist.stride(0), T, base, cur, o, None, bh.cache, miss, bc),
            stream_of(cur))) for miss in (True, False)}
        keep = (base, bc)                        # the graphs hold the baseline cache's addresses

        def replay() -> None:
            graphs[bh.expect_miss(T, R, None)].replay()
            bh.cache.ticked(T)
        replay.keep = keep
        return replay, o

    def _decide_services(self, cur, o: CanaryOutputs, has_base: bool) -> None:
        """p-value combine + window decision + service reduce, one launch
        (a workgroup per service, a wave per metric row)."""
        from ..ops._lib import LIB, ptr, stream_of
        C.check(self.M <= 16, "overlap/fused ticks support up to 16 metrics per service (use mode='serial')")
        LIB.call("fm_decide_services_2s" if self.band else "fm_decide_services",
                 *self._decide_call_args(cur, o, has_base), stream_of(cur))

    def _decide_call_args(self, cur, o: CanaryOutputs, has_base: bool) -> tuple:
        from ..ops._lib import ptr
        mask, anyc = self.pcfg.mask_and_combine()
        d = o.decide
        # with the effect gate on, the decision combines the gated copy (NaN rows: "no test applies")
        # with the scale test on, its copy of that (0 in a flagged row: "different" under every algorithm)
        pv = o.pvals if o.pvals_gated is None else o.pvals_gated
        if o.pvals_scaled is not None:
            pv = o.pvals_scaled
        return (ptr(o.bs if self.band else o.hs), ptr(cur), cur.stride(0), cur.shape[1], cur.shape[0] // self.M,
                self.M, ptr(self.thr), ptr(self.bound), ptr(self.minlb), float(self.cfg.pairwise_threshold_factor),
                ptr(pv) if has_base else None, mask, anyc, float(self.pcfg.p_threshold),
                int(self.cfg.min_historical_points), ptr(d.stats), ptr(d.flags), d.flags.shape[1], ptr(d.count),
                ptr(d.score), ptr(d.valid), ptr(o.diff) if has_base else None, ptr(o.packed))

    def _front(self, hist, base, cur, n_hist, o: CanaryOutputs, decide: bool = True) -> None:
        from ..ops._lib import LIB, ptr, stream_of
        T = hist.shape[1] if n_hist is None else int(n_hist)
        C.check(hist.stride(0) % 4 == 0 and hist.data_ptr() % 16 == 0, "history rows must be 16-B aligned")
        # (tensors nobody has bound: no cache of either kind, every row streams)
        LIB.call("fm_tick_front_bc", *self._front_args(ptr(hist), hist.stride(0), T, base, cur, o, None, None, True),
                 stream_of(cur))
        if decide:
            self._gate_into(cur, base, o)
            self._decide_services(cur, o, True)

    def split_launchers(self, hist, base, cur, n_hist=None, packed_out=None, slot: int = 0,
                        front_stream=None, decide_stream=None):
        """Pre-bound launchers of a split tick for one buffer slot: returns
        (front, decide, outputs).  Each launcher is one foreign call with
        every argument resolved up front (no tensor inspection per tick), on
        the stream given here (default: the current stream at creation).  A
        single-kernel HIP graph buys nothing here: at the 1,250-service shard
        the graph launch cost 6 % of the step.

        ``hist`` is bound for the life of the launcher (it holds a reference)
        and its row statistics are cached: the first launch streams and
        records every row, later ones read the 12 bytes per row.  A change of
        ``hist._version`` (any torch write) makes the next launch invalidate
        the cache on the front stream and stream the rows again; for writes
        torch does not see, :meth:`invalidate_history`."""
        from ..ops._lib import LIB, ptr
        self._no_robust("split_launchers")
        self._no_gate("split_launchers")
        o = self.front_only(hist, base, cur, n_hist, packed_out, slot)    # validate / allocate / warm
        torch.cuda.synchronize(cur.device)
        T = hist.shape[1] if n_hist is None else int(n_hist)
        dev = cur.device
        fs = (front_stream or torch.cuda.current_stream(dev)).cuda_stream
        ds = (decide_stream or torch.cuda.current_stream(dev)).cuda_stream
        lib = LIB.load()
        f_fn, d_fn, R = lib.fm_tick_front_bc, lib.fm_decide_services, cur.shape[0]
        d_args = self._decide_call_args(cur, o, True) + (ds,)
        # without a cache (hist_cache off) every tick streams: one argument set
        bh = self._bind(hist)
        # the baseline cache, held (with its tensor) for the launcher's life
        bc = self._base_cache_of(base, cur)
        keep = (base, bc)
        f_args = {miss: self._front_args(ptr(hist), hist.stride(0), T, base, cur, o, None,
                                         bh.cache if bh is not None else None, miss, bc) + (fs,)
                  for miss in ((True, False) if bh is not None else (True,))}
        expect = bh.expect_miss if bh is not None else (lambda T, R, fs: True)
        ticked = bh.cache.ticked if bh is not None else (lambda T: None)

        def front() -> None:
            rc = f_fn(*f_args[expect(T, R, fs)])
            if rc:
                raise RuntimeError(f"fm_tick_front_bc failed with hipError {rc}")
            ticked(T)
        front.keep = keep

        def decide() -> None:
            rc = d_fn(*d_args)
            if rc:
                raise RuntimeError(f"fm_decide_services failed with hipError {rc}")
        return front, decide, o

    def _fused(self, hist, base, cur, n_hist, o: CanaryOutputs) -> None:
        from ..ops._lib import LIB, ptr, stream_of
        R = cur.shape[0]
        T = hist.shape[1] if n_hist is None else int(n_hist)
        C.check(hist.stride(0) % 4 == 0 and hist.data_ptr() % 16 == 0, "history rows must be 16-B aligned")
        st = stream_of(cur)
        has_base = base is not None
        LIB.call("fm_canary_rows", ptr(hist), hist.stride(0), T, ptr(cur), cur.stride(0), cur.shape[1],
                 ptr(base) if has_base else None, base.stride(0) if has_base else 0,
                 base.shape[1] if has_base else 0, R, ptr(o.hs), ptr(o.suff), st)
        if has_base:
            LIB.call("fm_pvalues_only", ptr(o.suff), R, self.pcfg.min_mann_white, self.pcfg.min_wilcoxon,
                     self.pcfg.min_kruskal, ptr(o.pvals), ptr(o.pstats), st)
        self._decide_services(cur, o, has_base)

    def _side_stream(self, dev):
        if self._side is None:
            self._side = torch.cuda.Stream(dev)
        return self._side

    def _pairwise_into(self, cur, base, o: CanaryOutputs, max_blocks: int = 0, combine: bool = True) -> None:
        from ..ops._lib import LIB, ptr, stream_of
        R = cur.shape[0]
        st = stream_of(cur)
        LIB.call("fm_pairwise_suff", ptr(cur), cur.stride(0), cur.shape[1], ptr(base), base.stride(0),
                 base.shape[1], R, ptr(o.suff), int(max_blocks), st)
        if combine:
            mask, anyc = self.pcfg.mask_and_combine()
            LIB.call("fm_pvalues", ptr(o.suff), R, mask, anyc, float(self.pcfg.p_threshold),
                     self.pcfg.min_mann_white, self.pcfg.min_wilcoxon, self.pcfg.min_kruskal, ptr(o.pvals),
                     ptr(o.pstats), ptr(o.diff), st)
        else:
            LIB.call("fm_pvalues_only", ptr(o.suff), R, self.pcfg.min_mann_white, self.pcfg.min_wilcoxon,
                     self.pcfg.min_kruskal, ptr(o.pvals), ptr(o.pstats), st)

    # -- HIP graph capture of the whole tick ---------------------------------
    def capture(self, hist, base, cur, n_hist=None, epilogue=None, packed_out=None):
        """Capture the tick into a graph over static buffers; returns a replay
        callable producing outputs in ``self._out``.  ``epilogue(outputs)`` is
        captured after the tick (e.g. the verdict all-gather and the host
        copy), so a whole brain step is a single graph launch."""
        self._no_robust("capture")
        self._no_gate("capture")
        assert cur.is_cuda
        o = self.score(hist, base, cur, n_hist, packed_out)  # warm / allocate
        if epilogue is not None:
            epilogue(o)                           # warm the collective outside the capture
        torch.cuda.synchronize(cur.device)
        g = torch.cuda.CUDAGraph()
        s = torch.cuda.Stream(cur.device)
        s.wait_stream(torch.cuda.current_stream(cur.device))
        with torch.cuda.stream(s):
            with torch.cuda.graph(g, stream=s):
                self.score(hist, base, cur, n_hist, packed_out)
                if epilogue is not None:
                    epilogue(o)
        torch.cuda.current_stream(cur.device).wait_stream(s)
        self._graph = g

        def replay() -> CanaryOutputs:
            g.replay()
            return o
        return replay
