#!/usr/bin/env python3
"""The steady resident tick with and without the pairwise effect gate (K19),
and K19 alone, one GPU, one process.

``score_resident`` over a static ``ResidentHistory`` (T = 10,080, 8 metrics),
every row's history statistics in the cache (the all-hit steady tick), at

* 10,000 services, 5 pods x 10 points per side (bench.py's headline shape),
* 10,000 services, 10 pods x 10 points per side,
* the 1,250-service shard, 5 x 10.

Variants alternate round by round: ``gate_off`` (the default configuration),
``gate_on`` (``ML_PAIRWISE_MIN_SHIFT=0.02`` + ``ML_PAIRWISE_DIRECTIONAL=1``; K19's
cost does not depend on which settings are on) and ``front_alone`` (the
role-split front launch of the same tick by itself: the pairwise tests and
their p-values, what bounds the steady tick).  A round times ``--inner``
back-to-back ticks between two device events.  Then K19 alone over 10,000
rows at 64 x 64 and 512 x 512 samples per side.

One JSON line per shape (median of the rounds, their min / max) is printed and
appended to ``--out``.  ``--modes off`` runs on a tree without the gate too
(the parent commit, for the default-path comparison): it touches nothing the
gate added."""
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
from foremast_amd.engine.resident import ResidentHistory  # noqa: E402
from foremast_amd.engine.scorer import CanaryScorer  # noqa: E402
from foremast_amd.ops import canary as C  # noqa: E402
from foremast_amd.ops._lib import LIB, ptr, stream_of  # noqa: E402

ALIASES = ["error5xx", "latency", "traffic", "error4xx", "cpu", "memory", "tomcat_threads", "jvm_heap"]
SHAPES = {"headline": (10000, 5, 10), "10x10": (10000, 10, 10), "shard": (1250, 5, 10)}


def setup(services: int, pods: int, window: int, T: int, dev):
    """The fleet in a static store -> (store, row map, cur, base)."""
    M = len(ALIASES)
    hist, base, cur = C.synth_fleet(services, M, T, pods, window, 0, device=dev)
    R = cur.shape[0]
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
    return st, torch.from_numpy(rows.astype(np.int32)).to(dev), cur, base


def timed(var: dict, rounds: int, warmup: int, inner: int) -> dict:
    ms: dict[str, list[float]] = {k: [] for k in var}
    for rnd in range(warmup + rounds):
        for name, fn in var.items():
            fn()                                              # the variant's own steady state
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                fn()
            e1.record()
            e1.synchronize()
            if rnd >= warmup:
                ms[name].append(e0.elapsed_time(e1) / inner)
    return {k: {"median": round(statistics.median(v), 5), "min": round(min(v), 5), "max": round(max(v), 5)}
            for k, v in ms.items()}


def tick_variants(modes, dev, st, rm, cur, base) -> dict:
    var = {}
    cfg = BrainConfig()
    cfg.min_historical_points = 10
    sc_off = CanaryScorer(ALIASES, cfg, device=dev, xcd_balance=False)
    if "off" in modes:
        var["gate_off"] = lambda: sc_off.score_resident(st.view(), rm, cur, base)
    if "on" in modes:
        cfg_on = BrainConfig(pairwise_min_shift=0.02, pairwise_directional=True)
        cfg_on.min_historical_points = 10
        sc_on = CanaryScorer(ALIASES, cfg_on, device=dev, xcd_balance=False)
        var["gate_on"] = lambda: sc_on.score_resident(st.view(), rm, cur, base)
    if "front" in modes:
        sc_f = CanaryScorer(ALIASES, cfg, device=dev, xcd_balance=False)
        o = sc_f.score_resident(st.view(), rm, cur, base)     # fills this scorer's view of the cache
        v = st.view()
        args = sc_f._front_args(ptr(v.hist), v.ld, v.T, base, cur, o, rm, v.cache, False,
                                sc_f._base_cache_of(base, cur))
        var["front_alone"] = lambda: LIB.call("fm_tick_front_bc", *args, stream_of(cur))
    return var


def k19_alone(dev, rows: int, rounds: int, warmup: int, inner: int) -> dict:
    out = {}
    g = torch.Generator(device="cpu").manual_seed(19)
    bound = torch.ones((len(ALIASES),), dtype=torch.int32, device=dev)
    gate = C.EffectGate(min_shift=0.02, directional=True)
    for n in (64, 512):
        cur = (100 + torch.randn((rows, n), generator=g)).to(dev)
        base = (101 + torch.randn((rows, n), generator=g)).to(dev)
        pv = torch.rand((rows, C.N_TESTS), generator=g).to(dev)
        buf = C.alloc_effect(rows, dev)
        fn = lambda: C.pairwise_effect(cur, base, gate, bound, len(ALIASES), pv, out=buf)
        out[f"{n}x{n}"] = timed({"k19": fn}, rounds, warmup, inner if n <= 64 else max(1, inner // 10))["k19"]
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="headline,10x10,shard")
    ap.add_argument("--modes", default="off,on,front", help="comma list of off, on, front, k19")
    ap.add_argument("--hist", type=int, default=10080)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--k19-rows", type=int, default=10000)
    ap.add_argument("--out", default=os.path.join("profiles", "effect_gate_bench.jsonl"))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_effect_gate.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    modes = [m for m in a.modes.split(",") if m]
    lines = []
    common = {"label": a.label, "hist": a.hist, "rounds": a.rounds, "inner": a.inner,
              "device": torch.cuda.get_device_name(dev)}
    if set(modes) & {"off", "on", "front"}:
        for name in [s for s in a.shapes.split(",") if s]:
            services, pods, window = SHAPES[name]
            st, rm, cur, base = setup(services, pods, window, a.hist, dev)
            res = timed(tick_variants(modes, dev, st, rm, cur, base), a.rounds, a.warmup, a.inner)
            lines.append({"bench": "effect_gate_tick", "shape": name, "services": services, "metrics": len(ALIASES),
                          "n_cur": cur.shape[1], "n_base": base.shape[1], **common, "ms_per_tick": res})
            del st, rm, cur, base
            torch.cuda.empty_cache()
    if "k19" in modes:
        lines.append({"bench": "effect_gate_k19_alone", "rows": a.k19_rows, **common,
                      "ms_per_launch": k19_alone(dev, a.k19_rows, a.rounds, a.warmup, a.inner)})
    for ln in lines:
        s = json.dumps(ln)
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "a") as f:
                f.write(s + "\n")


if __name__ == "__main__":
    main()
