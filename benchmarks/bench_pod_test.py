#!/usr/bin/env python3
"""The per-pod canary test (K29): the kernel alone next to the pooled rank
tests on the same rows, one GPU, one process.

Wave tier: ``--rows`` rows of 8 pods x 8 + 64 baseline points, K29
(``fm_pairwise_pods``) beside K4 (``fm_pairwise_tests``: the rank kernel and
its p-values).  Workgroup tier: ``--wide-rows`` rows at 8 x 256 + 2,048 and at
64 x 64 + 4,096, K29 beside K21 (``fm_pairwise_suff_wide``).  Variants
alternate round by round; a round times ``--inner`` back-to-back launches
between two device events.  The numpy definition is timed per row at the same
shapes on the host (``--host-rows`` rows).

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

# (pods, points per pod, baseline points)
WAVE = ((8, 8, 64),)
WIDE = ((8, 256, 2048), (64, 64, 4096))


def _windows(rows: int, P: int, W: int, n_base: int, dev, seed: int):
    """Baseline and pods N(100, 5); every other row has its last pod 3 sigma up."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    cur = 100 + 5 * torch.randn((rows, P * W), generator=g)
    cur[1::2, (P - 1) * W:] += 15.0
    base = 100 + 5 * torch.randn((rows, n_base), generator=g)
    seg = (torch.arange(1, P + 1, dtype=torch.int32) * W).repeat(rows, 1)
    return cur.to(dev), seg.to(dev), base.to(dev)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--wide-rows", type=int, default=1000)
    ap.add_argument("--host-rows", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "pod_test_bench.jsonl"))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pod_test.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    test, cfg = C.PodTest("KRUSKAL_DUNN"), C.PairwiseConfig()
    for shapes, R, tier in ((WAVE, a.rows, "wave"), (WIDE, a.wide_rows, "wide")):
        for P, W, nb in shapes:
            cur, seg, base = _windows(R, P, W, nb, dev, 29)
            buf = C.alloc_pods(R, P, dev)
            var = {"k29": lambda: C.pairwise_pods(cur, seg, base, test, out=buf)}
            if tier == "wave":
                var["k4"] = lambda: C.pairwise_tests(cur, base, cfg)
            else:
                var["k21"] = lambda: C.pairwise_suff_wide(cur, base)
            res = timed(var, a.rounds, a.warmup, a.inner)
            torch.cuda.synchronize()
            flagged = float(buf.pod_diff.float().mean())
            hc, hs, hb = (t[:a.host_rows].cpu().numpy() for t in (cur, seg, base))
            t0 = time.perf_counter()
            ref.pairwise_pods(hc, hs, hb, test.min_points)
            host_ms = (time.perf_counter() - t0) * 1e3 / max(1, len(hc))
            ln = {"bench": "pod_test_k29_alone", "tier": tier, "rows": R, "pods": P, "per_pod": W, "n_base": nb,
                  "flagged": round(flagged, 4), "inner": a.inner, "ms_per_launch": res,
                  "host_ms_per_row": round(host_ms, 4), "label": a.label, "rounds": a.rounds,
                  "device": torch.cuda.get_device_name(dev)}
            s = json.dumps(ln)
            print(s, flush=True)
            if a.out:
                os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
                with open(a.out, "a") as f:
                    f.write(s + "\n")
            del cur, seg, base, buf
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
