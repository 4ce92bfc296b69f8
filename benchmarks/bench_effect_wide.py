#!/usr/bin/env python3
"""The effect-size gate of windows wider than K19's 1,024 pooled points: K28
(``fm_pairwise_effect_wide``) alone, one GPU, one process.

Per shape (600 + 600, 2,048 + 2,048, 4,096 + 4,096; ``--rows`` rows each), in
rounds that alternate the variants after warm-up rounds of every shape:

``k28``   -- ``C.pairwise_effect(..., tier="wide")``: one launch, no bucketing;
``k21``   -- ``C.pairwise_suff_wide`` on the same rows, for scale (the rank
             tests' kernel for these rows: the same sort, searches instead of
             the bisection);
``host``  -- the route K28 replaces: the rows to the host,
             ``reference.pairwise_effect``, the results back; on
             ``--host-rows`` rows, which the host finishes in reasonable time,
             and reported per row.

Per call: ``--inner`` launches between two device events, and the host wall
time up to a synchronize after them; medians of the rounds after the warm-ups.
The outputs of ``k28`` on the host rows are compared with the host route's
before anything is timed.  One JSON line per shape is printed and appended to
``--out``."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from benchmarks.bench_pairwise_wide import samples, timed  # noqa: E402
from foremast_amd.ops import canary as C  # noqa: E402
from foremast_amd.ops import reference as ref  # noqa: E402

SHAPES = (600, 2048, 4096)


def host_route(cur: torch.Tensor, base: torch.Tensor):
    e, c = ref.pairwise_effect(cur.cpu().numpy(), base.cpu().numpy())
    return torch.from_numpy(e).to(cur.device), torch.from_numpy(c).to(cur.device)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1000)
    ap.add_argument("--host-rows", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=5, help="launches per round")
    ap.add_argument("--out", default=os.path.join("profiles", "effect_wide_bench.jsonl"))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_effect_wide.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    lines = []
    for n in SHAPES:
        cur, base = samples(a.rows, n, dev, a.rows + n)
        hc, hb = cur[:a.host_rows].contiguous(), base[:a.host_rows].contiguous()
        out = C.alloc_effect(a.rows, dev, with_pvals=False)
        k28 = lambda: C.pairwise_effect(cur, base, out=out, tier="wide")
        he, hcnt = host_route(hc, hb)
        r = k28()
        torch.cuda.synchronize()
        same = bool(torch.equal(r.effect[:a.host_rows], he) and torch.equal(r.counts[:a.host_rows], hcnt))
        gpu = timed({"k28": k28, "k21": lambda: C.pairwise_suff_wide(cur, base)}, a.rounds, a.warmup, a.inner)
        host = timed({"host": lambda: host_route(hc, hb)}, max(1, a.rounds // 2), 1)["host"]
        per_row = {k: round(v["median"] / a.host_rows, 4) for k, v in host.items()}
        lines.append({"bench": "effect_wide", "rows": a.rows, "n_cur": n, "n_base": n, "label": a.label,
                      "rounds": a.rounds, "warmup": a.warmup, "inner": a.inner,
                      "device": torch.cuda.get_device_name(dev), "ms_per_launch": gpu,
                      "k28_us_per_row": round(gpu["k28"]["device_ms"]["median"] * 1e3 / a.rows, 3),
                      "k21_us_per_row": round(gpu["k21"]["device_ms"]["median"] * 1e3 / a.rows, 3),
                      "host_rows": a.host_rows, "host_ms_per_call": host, "host_ms_per_row": per_row,
                      "k28_equals_host_route": same})
        print(json.dumps(lines[-1]), flush=True)
        del cur, base
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "a") as f:
            for ln in lines:
                f.write(json.dumps(ln) + "\n")
    if not all(ln["k28_equals_host_route"] for ln in lines):
        raise SystemExit("K28 and the host route disagree")


if __name__ == "__main__":
    main()
