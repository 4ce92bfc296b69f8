#!/usr/bin/env python3
"""The tail canary test (K32): the kernel alone, one GPU, one process.

Wave tier: ``--rows`` rows of 64 + 64 points, K32 (``fm_pairwise_tail``) beside
K4 (``fm_pairwise_tests``: the rank kernel and its p-values) on the same rows,
as context.  Workgroup tier: ``--wide-rows`` rows at 2,048 + 2,048 and at
4,096 + 4,096.  Both sides run on every row (``BOTH``).  Beside the default
three levels the same launch is timed with one level and with four (how the
time moves with L), with a ``MIN_TAIL_POINTS`` no level reaches (no level
counts: the finish sums no term) and with a ``MIN_TAIL_DATA_POINTS`` no row
reaches (no row applies: the load and the stores alone).  Variants alternate
round by round; a round times ``--inner`` back-to-back launches between two
device events.  The numpy definition is timed per row at the same shapes on
the host (``--host-rows`` rows).

One JSON line per shape (median of the rounds, their min / max) is printed and
appended to ``--out``."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from benchmarks.bench_effect_gate import timed  # noqa: E402
from foremast_amd.ops import canary as C  # noqa: E402
from foremast_amd.ops import reference as ref  # noqa: E402

# (current points, baseline points)
WAVE = ((64, 64),)
WIDE = ((2048, 2048), (4096, 4096))


def _windows(rows: int, nc: int, nb: int, dev, seed: int):
    """Both sides lognormal(4, 0.3); every other row's current upper fifth is stretched by 1.2."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    cur = torch.exp(4 + 0.3 * torch.randn((rows, nc), generator=g))
    base = torch.exp(4 + 0.3 * torch.randn((rows, nb), generator=g))
    odd = cur[1::2]
    cur[1::2] = torch.where(odd > odd.quantile(0.8, dim=1, keepdim=True), odd * 1.2, odd)
    return cur.to(dev), base.to(dev)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--wide-rows", type=int, default=1000)
    ap.add_argument("--host-rows", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "tail_test_bench.jsonl"))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tail_test.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    on = dict(test="EXCEEDANCE", sides="BOTH")
    tests = {"k32": C.TailTest(**on), "k32_L1": C.TailTest(quantiles=(0.95,), **on),
             "k32_L4": C.TailTest(quantiles=(0.9, 0.95, 0.99, 0.999), **on),
             "k32_no_terms": C.TailTest(min_tail_points=1 << 20, **on),
             "k32_no_rows": C.TailTest(min_points=1 << 20, **on)}
    cfg = C.PairwiseConfig()
    for shapes, R, tier in ((WAVE, a.rows, "wave"), (WIDE, a.wide_rows, "wide")):
        for nc, nb in shapes:
            cur, base = _windows(R, nc, nb, dev, 32)
            bufs = {k: C.alloc_tail(R, len(t.q_i), dev) for k, t in tests.items()}
            var = {k: (lambda k=k: C.pairwise_tail(cur, base, tests[k], out=bufs[k])) for k in tests}
            if tier == "wave":
                var["k4"] = lambda: C.pairwise_tests(cur, base, cfg)
            res = timed(var, a.rounds, a.warmup, a.inner)
            torch.cuda.synchronize()
            flagged = float(bufs["k32"].tail_diff.float().mean())
            hc, hb = (t[:a.host_rows].cpu().numpy() for t in (cur, base))
            t0 = time.perf_counter()
            ref.pairwise_tail(hc, hb, tests["k32"].q_i, "BOTH")
            host_ms = (time.perf_counter() - t0) * 1e3 / max(1, len(hc))
            ln = {"bench": "tail_test_k32_alone", "tier": tier, "rows": R, "n_cur": nc, "n_base": nb,
                  "flagged": round(flagged, 4), "inner": a.inner, "ms_per_launch": res,
                  "host_ms_per_row": round(host_ms, 4), "label": a.label, "rounds": a.rounds,
                  "device": torch.cuda.get_device_name(dev)}
            s = json.dumps(ln)
            print(s, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(s + "\n")
            del cur, base, bufs
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
