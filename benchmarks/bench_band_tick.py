#!/usr/bin/env python3
"""The resident tick of the static band models (CanaryScorer(model="band_mix"),
K25) against the robust and mean/std ticks and against the op-by-op route it
replaces in the brain, one GPU, one process.

10,000 services x 8 metrics, T = 10,080, bench.py's headline window shapes,
rows in a static ``ResidentHistory``.  Two fleets of model codes per metric:
``mix`` (two quantile_robust, two robust_moving_average_all, four
moving_average_all) and ``all_quantile``.  Variants per fleet, ms per tick:

* ``band_hot``    every row's band record in the band-record cache
* ``band_cold``   ``invalidate_history()`` before every tick: every row computed
* ``band_mixed``  ``--dirty-frac`` of the rows touched before every tick
* ``op_by_op``    what the brain's model path does for this job class: pairwise
  tests, then per algorithm present ``LazyHist.materialize(0)`` (the gather)
  and the model call with its band decision, the scatter into the group's
  arrays, ``service_reduce``

and the yardsticks ``robust_hot`` / ``robust_cold`` / ``robust_mixed`` (the
robust_moving_average_all tick, K18), ``mean_hot`` (the moving_average_all
tick) and ``empty_launch`` (one launch of a one-workgroup kernel).

The anomaly compaction and the device->host copy that follow every route in
the brain are in none of them.  All variants alternate round by round; a round
times ``--inner`` back-to-back ticks of one variant between two device events
(the slow variants: ``--inner-slow``).  One JSON line with the median of the
rounds and their min / max per variant is printed and appended to ``--out``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from bench_robust_tick import ALIASES, ROBUST, measure, setup  # noqa: E402
from foremast_amd.engine.fp_types import LazyHist  # noqa: E402
from foremast_amd.engine.resident import HistView, RowStatsCache  # noqa: E402
from foremast_amd.engine.scorer import CanaryScorer  # noqa: E402
from foremast_amd.models import zoo  # noqa: E402
from foremast_amd.ops import canary as C  # noqa: E402
from foremast_amd.ops import misc as MI  # noqa: E402

FLEETS = {"mix": (2, 2, 1, 1, 0, 0, 0, 0), "all_quantile": (2,) * 8}
NAMES = {v: k for k, v in MI.BAND_CODES.items()}


def fleet_variants(a, dev, st, rm, cur, base, cfg, name: str, codes: tuple, cache: RowStatsCache) -> dict:
    R, M = cur.shape[0], len(ALIASES)
    S = R // M
    sc = CanaryScorer(ALIASES, cfg, device=dev, model="band_mix", codes=codes, tail_z=MI.QUANTILE_TAIL_Z,
                      xcd_balance=False)
    T = st.view().T
    # each fleet keeps its records in a cache of its own: the same physical
    # rows stand under other models in the other fleet
    view = HistView(st.buf, st.width, T, None, None, cache)
    dirty = torch.randperm(R, device=dev)[:max(1, int(R * a.dirty_frac))].sort().values
    NW = max(1, (cur.shape[1] + 63) // 64)
    subs = []
    for code in sorted(set(codes)):
        ms = [m for m in range(M) if codes[m] == code]
        idx = (torch.arange(S, device=dev)[:, None] * M + torch.tensor(ms, device=dev)[None, :]).reshape(-1)
        n = idx.numel()
        subs.append((NAMES[code], None if len(ms) == M else idx, rm.index_select(0, idx).contiguous(), len(ms),
                     zoo.make_tables([ALIASES[m] for m in ms], cfg, dev),
                     torch.ones((n, cur.shape[1]), dtype=torch.int64, device=dev),
                     torch.zeros((n,), dtype=torch.int32, device=dev),
                     torch.full((n,), T, dtype=torch.int32, device=dev)))

    def band_hot():
        sc.score_resident(view, rm, cur, base)

    def band_cold():
        sc.invalidate_history()
        sc.score_resident(view, rm, cur, base)

    def band_mixed():
        cache.touch(dirty)
        sc.score_resident(view, rm, cur, base)

    def op_by_op():
        _, _, diff = C.pairwise_tests(cur, base, sc.pcfg)
        single = len(subs) == 1
        if not single:
            up = torch.full(cur.shape, float("nan"), device=dev)
            lo = torch.full(cur.shape, float("nan"), device=dev)
            flags = torch.zeros((R, NW), dtype=torch.int64, device=dev)
            count = torch.zeros((R,), dtype=torch.int32, device=dev)
            score = torch.zeros((R,), dtype=torch.float32, device=dev)
            valid = torch.zeros((R,), dtype=torch.int32, device=dev)
        for algo, idx, srm, sm, tables, hor, shift, lim in subs:
            c = cur if idx is None else cur.index_select(0, idx)
            d = diff if idx is None else diff.index_select(0, idx)
            dense = LazyHist(st.buf, srm, shift, lim, T).materialize(0)
            dec = zoo.decide(algo, dense, T, c, hor, sm, tables, d, tail_z=MI.QUANTILE_TAIL_Z)
            if single:
                count, score, valid = dec.count, dec.score, dec.valid
            else:
                up[idx], lo[idx], flags[idx] = dec.upper, dec.lower, dec.flags
                count[idx], score[idx], valid[idx] = dec.count, dec.score, dec.valid.to(torch.int32)
        C.service_reduce(count.contiguous(), score.contiguous(), valid.to(torch.int32).contiguous(), M)

    return {f"{name}.band_hot": (band_hot, False), f"{name}.band_cold": (band_cold, True),
            f"{name}.band_mixed": (band_mixed, False), f"{name}.op_by_op": (op_by_op, True)}


def yardsticks(a, dev, st, rm, cur, base, cfg) -> dict:
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    R = cur.shape[0]
    sc_r = CanaryScorer(ALIASES, cfg, device=dev, model=ROBUST, xcd_balance=False)
    sc_m = CanaryScorer(ALIASES, cfg, device=dev, xcd_balance=False)
    dirty = torch.randperm(R, device=dev)[:max(1, int(R * a.dirty_frac))].sort().values
    one_i = torch.zeros((8,), dtype=torch.int32, device=dev)
    one_f = torch.zeros((8,), dtype=torch.float32, device=dev)

    def robust_hot():
        sc_r.score_resident(st.view(), rm, cur, base)

    def robust_cold():
        sc_r.invalidate_history()
        sc_r.score_resident(st.view(), rm, cur, base)

    def robust_mixed():
        st.rcache.touch(dirty)
        sc_r.score_resident(st.view(), rm, cur, base)

    def mean_hot():
        sc_m.score_resident(st.view(), rm, cur, base)

    def empty_launch():
        LIB.call("fm_service_reduce", ptr(one_i), ptr(one_f), ptr(one_i), 1, 1, ptr(one_f), stream_of(one_f))

    return {"robust_hot": (robust_hot, False), "robust_cold": (robust_cold, True),
            "robust_mixed": (robust_mixed, False), "mean_hot": (mean_hot, False), "empty_launch": (empty_launch, False)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--services", type=int, default=10000)
    ap.add_argument("--hist", type=int, default=10080)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--inner-slow", type=int, default=4)
    ap.add_argument("--dirty-frac", type=float, default=0.005)
    ap.add_argument("--out", default=os.path.join("profiles", "band_tick_bench.jsonl"))
    ap.add_argument("--label", default="")
    ap.add_argument("--only", default="", help="comma-separated variant names: time these alone (a kernel-trace run)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    st, rm, cur, base, cfg = setup(a, dev)
    var = yardsticks(a, dev, st, rm, cur, base, cfg)
    for name, codes in FLEETS.items():
        cache = st.bcache if name == "mix" else RowStatsCache(len(st.bcache), dev, width=4)
        var.update(fleet_variants(a, dev, st, rm, cur, base, cfg, name, codes, cache))
    if a.only:
        var = {k: var[k] for k in a.only.split(",")}
    res = measure(a, dev, var)
    line = json.dumps({"bench": "band_tick", "label": a.label, "services": a.services, "metrics": len(ALIASES),
                       "hist": a.hist, "n_cur": cur.shape[1], "n_base": base.shape[1], "rounds": a.rounds,
                       "inner": a.inner, "inner_slow": a.inner_slow, "dirty_frac": a.dirty_frac,
                       "tail_z": MI.QUANTILE_TAIL_Z, "fleets": {k: list(v) for k, v in FLEETS.items()},
                       "device": torch.cuda.get_device_name(dev), "ms_per_tick": res})
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
