#!/usr/bin/env python3
"""The pairwise tests of windows wider than the wave kernel's 1,024 pooled
points: K21 (``fm_pairwise_suff_wide``) against the host-oracle route it
replaces, one GPU, one process.

``ops`` -- ``C.pairwise_tests`` on 8, 800 and 8,000 rows at 770 + 770 points
(70 pods x 11 points per side) and at 4096 + 4096 (the cap).  Variant ``k21``
is this tree's routing; variant ``oracle`` lowers ``C.PAIRWISE_WIDE_MAX`` to
``C.PAIRWISE_MAX`` so that the rows take the route they took before K21 (used
widths and rows to the host, numpy, results back).  Per call: device events
around it and the host wall time up to a synchronize after it; medians of the
rounds after the warm-ups.

``kernel`` (not in the default modes) -- K21 alone on the same shapes, 10
launches between two device events.

``tick`` -- ``score_resident`` over a static store, 10,000 services x 8
metrics, every history row cached, in which ONE service (8 rows) has a 770 +
770 window and the rest 50 + 50 (the batch is padded to the widest).  On a
tree with K21 both routings run, alternating; on a tree without it (the
parent commit) the one there is.  ``--modes tick`` touches nothing K21 added.

One JSON line per measurement is printed and appended to ``--out``."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from foremast_amd.config import BrainConfig  # noqa: E402
from foremast_amd.engine.resident import ResidentHistory  # noqa: E402
from foremast_amd.engine.scorer import CanaryScorer  # noqa: E402
from foremast_amd.ops import canary as C  # noqa: E402

ALIASES = ["error5xx", "latency", "traffic", "error4xx", "cpu", "memory", "tomcat_threads", "jvm_heap"]
HAS_K21 = hasattr(C, "PAIRWISE_WIDE_MAX")


class Routing:
    """``with Routing("oracle")``: the wide tier off for the block."""

    def __init__(self, name: str):
        self.off = name == "oracle" and HAS_K21

    def __enter__(self):
        if self.off:
            self.keep = C.PAIRWISE_WIDE_MAX
            C.PAIRWISE_WIDE_MAX = C.PAIRWISE_MAX

    def __exit__(self, *a):
        if self.off:
            C.PAIRWISE_WIDE_MAX = self.keep


def timed(var: dict, rounds: int, warmup: int, inner: int = 1) -> dict:
    """name -> fn: per round and variant ``inner`` calls between two device
    events, and the wall time from before the first to a synchronize after
    the last."""
    dev_ms: dict[str, list[float]] = {k: [] for k in var}
    wall_ms: dict[str, list[float]] = {k: [] for k in var}
    for rnd in range(warmup + rounds):
        for name, fn in var.items():
            with Routing(name):
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0 = time.perf_counter()
                e0.record()
                for _ in range(inner):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
            if rnd >= warmup:
                dev_ms[name].append(e0.elapsed_time(e1) / inner)
                wall_ms[name].append((t1 - t0) * 1e3 / inner)

    def summary(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}

    return {k: {"device_ms": summary(dev_ms[k]), "wall_ms": summary(wall_ms[k])} for k in var}


def samples(rows: int, n: int, dev, seed: int):
    g = torch.Generator(device="cpu").manual_seed(seed)
    cur = torch.round(torch.randn((rows, n), generator=g) * 10) / 10
    base = torch.round((0.3 + 1.2 * torch.randn((rows, n), generator=g)) * 10) / 10
    return cur.to(dev), base.to(dev)


def bench_ops(a, dev, common) -> list[dict]:
    lines = []
    for n in (770, 4096):
        for rows in (8, 800, 8000):
            cur, base = samples(rows, n, dev, rows + n)
            var = {"k21": lambda: C.pairwise_tests(cur, base)}
            if not a.no_oracle:
                var["oracle"] = var["k21"]
            if HAS_K21:
                C.reset_route_rows()
            res = timed(var, a.rounds, a.warmup)
            routes = C.route_rows() if HAS_K21 else None
            lines.append({"bench": "pairwise_wide_ops", "rows": rows, "n_cur": n, "n_base": n, **common,
                          "ms_per_call": res, "route_rows_total": routes})
            print(json.dumps(lines[-1]), flush=True)
            del cur, base
            torch.cuda.empty_cache()
    return lines


def bench_kernel(a, dev, common) -> list[dict]:
    """K21 alone (``C.pairwise_suff_wide``: one launch, no bucketing, no p-values)."""
    lines = []
    for n in (770, 4096):
        for rows in (8, 800, 8000):
            cur, base = samples(rows, n, dev, rows + n)
            res = timed({"k21_alone": lambda: C.pairwise_suff_wide(cur, base)}, a.rounds, a.warmup, 10)
            lines.append({"bench": "pairwise_wide_kernel", "rows": rows, "n_cur": n, "n_base": n, **common,
                          "inner": 10, "ms_per_launch": res})
            print(json.dumps(lines[-1]), flush=True)
    return lines


def bench_tick(a, dev, common) -> list[dict]:
    M = len(ALIASES)
    S, T, n_small, n_wide = a.services, a.hist, 50, 770
    hist, base50, cur50 = C.synth_fleet(S, M, T, 5, 10, 0, device=dev)
    R = cur50.shape[0]
    st = ResidentHistory(T, dev, capacity=R)
    rows, _ = st.rows_for([("r", i) for i in range(R)])
    idx = torch.from_numpy(rows.astype(np.int64)).to(dev)
    st.buf.index_copy_(0, idx, hist[:, :st.width].contiguous())
    st.touch(idx)
    st.nlen[rows] = T
    st.nfin[rows] = T
    st.last_t[rows] = 0.0
    st.max_len = T
    del hist
    rm = torch.from_numpy(rows.astype(np.int32)).to(dev)
    cur = torch.full((R, n_wide), float("nan"), device=dev)
    base = torch.full((R, n_wide), float("nan"), device=dev)
    cur[:, :n_small] = cur50
    base[:, :n_small] = base50
    # the one wide service: its 50-point windows repeated out to 770 points
    w = slice(M * (S // 2), M * (S // 2) + M)
    reps = -(-n_wide // n_small)
    cur[w] = cur50[w].repeat(1, reps)[:, :n_wide]
    base[w] = base50[w].repeat(1, reps)[:, :n_wide]
    cfg = BrainConfig()
    cfg.min_historical_points = 10
    sc = CanaryScorer(ALIASES, cfg, device=dev, xcd_balance=False)
    fn = lambda: sc.score_resident(st.view(), rm, cur, base)
    fn()                                                       # fills the row-statistics cache
    var = {"k21": fn, "oracle": fn} if HAS_K21 else {"parent": fn}
    if HAS_K21:
        C.reset_route_rows()
    res = timed(var, a.rounds, a.warmup, a.inner)
    # the same fleet with every window 50 + 50: what the one wide job adds
    fn50 = lambda: sc.score_resident(st.view(), rm, cur50, base50)
    fn50()
    res.update(timed({"all_50x50": fn50}, a.rounds, a.warmup, a.inner))
    line = {"bench": "pairwise_wide_tick", "services": S, "metrics": M, "wide_rows": M, "n_wide": n_wide,
            "n_small": n_small, **common, "inner": a.inner, "ms_per_tick": res,
            "route_rows_total": C.route_rows() if HAS_K21 else None}
    print(json.dumps(line), flush=True)
    return [line]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="ops,tick")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5, help="ticks per round (tick mode)")
    ap.add_argument("--services", type=int, default=10000)
    ap.add_argument("--hist", type=int, default=10080)
    ap.add_argument("--no-oracle", action="store_true", help="ops mode: K21 only")
    ap.add_argument("--out", default=os.path.join("profiles", "pairwise_wide_bench.jsonl"))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pairwise_wide.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    common = {"label": a.label, "rounds": a.rounds, "warmup": a.warmup, "k21": HAS_K21,
              "device": torch.cuda.get_device_name(dev)}
    modes = [m for m in a.modes.split(",") if m]
    lines = []
    if "ops" in modes:
        if not HAS_K21:
            raise SystemExit("ops mode needs a tree with K21")
        lines += bench_ops(a, dev, common)
    if "kernel" in modes:
        if not HAS_K21:
            raise SystemExit("kernel mode needs a tree with K21")
        lines += bench_kernel(a, dev, common)
    if "tick" in modes:
        lines += bench_tick(a, dev, common)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
