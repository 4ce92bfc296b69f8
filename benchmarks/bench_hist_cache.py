#!/usr/bin/env python3
"""Tick time with the row-statistics cache hot and cold, one GPU.

``cold`` calls ``CanaryScorer.invalidate_history()`` before every tick: the
all-miss path (dynamic queue, XCD-balanced ranges, every row streamed and its
cache entry written) -- what the first tick after a history write costs.
``hot`` is the steady state (every row's statistics read from the cache),
``mixed`` a tick after ``--dirty-frac`` of the rows were rewritten (those rows
are invalidated before every tick; the others hit).
``basecold`` is ``hot`` with the baseline cache emptied before every tick (its
tags zeroed, one small fill launch on the stream): every pairwise row misses
and rewrites its entry -- what the first tick against a new baseline tensor
costs.  On a scorer without that cache it is ``hot``.
On a scorer without the cache (``FM_HIST_CACHE=0``, or a build that has none)
both are the plain tick, which is what ``cold`` is compared with.

One tick = front launch + decision launch on one stream (bench.py's pre-bound
launchers, no publish).  Prints one JSON line per (mode, repeat):
``python benchmarks/bench_hist_cache.py --services 10000 --modes cold,hot``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from foremast_amd.config import BrainConfig  # noqa: E402
from foremast_amd.engine.scorer import CanaryScorer  # noqa: E402
from foremast_amd.ops import canary as C  # noqa: E402

ALIASES = ["error5xx", "latency", "traffic", "error4xx", "cpu", "memory", "tomcat_threads", "jvm_heap"]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--services", type=int, default=10000)
    ap.add_argument("--hist", type=int, default=10080)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--modes", default="cold,hot")
    ap.add_argument("--hot-wgs", default="", help="front_hot_wgs of the scorer, pairwise:history workgroups per CU")
    ap.add_argument("--dirty-frac", type=float, default=0.005, help="mixed: share of rows invalidated per tick")
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    hist, base, cur = C.synth_fleet(a.services, 8, a.hist, 5, 10, 0, device=dev)
    cfg = BrainConfig()
    cfg.min_historical_points = 10
    kw = {"front_hot_wgs": tuple(float(x) for x in a.hot_wgs.split(":"))} if a.hot_wgs else {}
    sc = CanaryScorer(ALIASES, cfg, device=dev, **kw)
    front, decide, _ = sc.split_launchers(hist, base, cur, a.hist)
    inv = getattr(sc, "invalidate_history", None)
    cached = bool(getattr(sc, "hist_cache", False))

    bound = getattr(sc, "_bound", {}).get(id(hist))
    bcache = sc._base_cache_of(base, cur) if hasattr(sc, "_base_cache_of") else None
    R = cur.shape[0]
    dirty = torch.randperm(R, device=dev)[:max(1, int(R * a.dirty_frac))].sort().values

    def run(n: int, mode: str) -> float:
        cold = mode == "cold"
        touch = bound.cache.touch if mode == "mixed" and bound is not None else None
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for _ in range(n):
            if cold and inv is not None:
                inv()
            if touch is not None:
                touch(dirty)
            if mode == "basecold" and bcache is not None:
                bcache.stats.zero_()
            front()
            decide()
        torch.cuda.synchronize(dev)
        return (time.perf_counter() - t0) / n * 1e3

    for mode in a.modes.split(","):
        run(a.warmup, mode)
        for r in range(a.repeats):
            print(json.dumps({"bench": "hist_cache", "label": a.label, "mode": mode, "cached": cached,
                              "base_cached": bcache is not None, "services": a.services, "hist": a.hist,
                              "steps": a.steps, "repeat": r,
                              "hot_wgs": a.hot_wgs or None, "dirty_frac": a.dirty_frac if mode == "mixed" else None,
                              "ms_per_tick": round(run(a.steps, mode), 5)}), flush=True)


if __name__ == "__main__":
    main()
