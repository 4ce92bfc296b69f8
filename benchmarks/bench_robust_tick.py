#!/usr/bin/env python3
"""The resident robust_moving_average_all tick against the mean/std tick and
against the op-by-op route it replaces in the brain, one GPU, one process.

10,000 services x 8 metrics, T = 10,080, bench.py's headline window shapes,
rows in a static ``ResidentHistory``.  Variants, ms per tick:

* ``robust_hot``    every row's (median, sigma, n) in the store's robust cache
* ``robust_cold``   ``invalidate_history()`` before every tick: every row selected
* ``robust_mixed``  ``--dirty-frac`` of the rows touched before every tick
* ``mean_hot`` / ``mean_cold``   the moving_average_all tick, the yardstick
* ``op_by_op``      what the brain's model path does for this job class:
  pairwise tests, ``LazyHist.materialize(0)`` (the gather), K13, ``band_decide``,
  ``service_reduce`` as separate ops

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
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from foremast_amd.config import BrainConfig  # noqa: E402
from foremast_amd.engine.fp_types import LazyHist  # noqa: E402
from foremast_amd.engine.resident import ResidentHistory  # noqa: E402
from foremast_amd.engine.scorer import CanaryScorer  # noqa: E402
from foremast_amd.models import zoo  # noqa: E402
from foremast_amd.ops import canary as C  # noqa: E402

ALIASES = ["error5xx", "latency", "traffic", "error4xx", "cpu", "memory", "tomcat_threads", "jvm_heap"]
ROBUST = "robust_moving_average_all"


def setup(a, dev):
    """The fleet in a static store -> (store, row map, cur, base, config)."""
    M = len(ALIASES)
    hist, base, cur = C.synth_fleet(a.services, M, a.hist, 5, 10, 0, device=dev)
    R = cur.shape[0]
    st = ResidentHistory(a.hist, dev, capacity=R)
    rows, _ = st.rows_for([("r", i) for i in range(R)])
    idx = torch.from_numpy(rows.astype(np.int64)).to(dev)
    # the rows are synthesised on the device: written in place, with the
    # bookkeeping write_static keeps (length, newest sample, invalid cache words)
    st.buf.index_copy_(0, idx, hist[:, :st.width].contiguous())
    st.touch(idx)
    st.nlen[rows] = a.hist
    st.nfin[rows] = a.hist
    st.last_t[rows] = 0.0
    st.max_len = a.hist
    del hist
    cfg = BrainConfig()
    cfg.min_historical_points = 10
    return st, torch.from_numpy(rows.astype(np.int32)).to(dev), cur, base, cfg


def variants(a, dev, st, rm, cur, base, cfg) -> dict:
    """name -> (tick callable, slow?)"""
    R, M = cur.shape[0], len(ALIASES)
    sc_r = CanaryScorer(ALIASES, cfg, device=dev, model=ROBUST, xcd_balance=False)
    sc_m = CanaryScorer(ALIASES, cfg, device=dev, xcd_balance=False)
    dirty = torch.randperm(R, device=dev)[:max(1, int(R * a.dirty_frac))].sort().values
    tables = zoo.make_tables(ALIASES, cfg, dev)
    hor = torch.ones(cur.shape, dtype=torch.int64, device=dev)
    T = st.view().T
    shift = torch.zeros((R,), dtype=torch.int32, device=dev)
    lim = torch.full((R,), T, dtype=torch.int32, device=dev)

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

    def mean_cold():
        sc_m.invalidate_history()
        sc_m.score_resident(st.view(), rm, cur, base)

    def op_by_op():
        _, _, diff = C.pairwise_tests(cur, base, sc_r.pcfg)
        dense = LazyHist(st.buf, rm, shift, lim, T).materialize(0)
        dec = zoo.decide(ROBUST, dense, T, cur, hor, M, tables, diff)
        C.service_reduce(dec.count.contiguous(), dec.score.contiguous(), dec.valid.to(torch.int32).contiguous(), M)

    return {"robust_hot": (robust_hot, False), "robust_cold": (robust_cold, True),
            "robust_mixed": (robust_mixed, False), "mean_hot": (mean_hot, False), "mean_cold": (mean_cold, True),
            "op_by_op": (op_by_op, True)}


def measure(a, dev, var: dict) -> dict:
    ms: dict[str, list[float]] = {k: [] for k in var}
    for rnd in range(a.warmup + a.rounds):
        for name, (fn, slow) in var.items():
            n = a.inner_slow if slow else a.inner
            fn()                                              # the variant's own steady state (cache, allocator)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                fn()
            e1.record()
            e1.synchronize()
            if rnd >= a.warmup:
                ms[name].append(e0.elapsed_time(e1) / n)
    return {k: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
            for k, v in ms.items()}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--services", type=int, default=10000)
    ap.add_argument("--hist", type=int, default=10080)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--inner-slow", type=int, default=4)
    ap.add_argument("--dirty-frac", type=float, default=0.005)
    ap.add_argument("--out", default=os.path.join("profiles", "robust_tick_bench.jsonl"))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    st, rm, cur, base, cfg = setup(a, dev)
    res = measure(a, dev, variants(a, dev, st, rm, cur, base, cfg))
    line = json.dumps({"bench": "robust_tick", "label": a.label, "services": a.services, "metrics": len(ALIASES),
                       "hist": a.hist, "n_cur": cur.shape[1], "n_base": base.shape[1], "rounds": a.rounds,
                       "inner": a.inner, "inner_slow": a.inner_slow, "dirty_frac": a.dirty_frac,
                       "device": torch.cuda.get_device_name(dev), "ms_per_tick": res})
    print(line, flush=True)
    if a.out:
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
