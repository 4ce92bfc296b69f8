#!/usr/bin/env python3
"""The drift canary test (K31): the kernel alone, one GPU, one process.

Wave tier: ``--rows`` rows of 8 pods x 8 + 64 baseline points, K31
(``fm_pairwise_drift``) beside K4 (``fm_pairwise_tests``: the rank kernel and
its p-values) on the same rows, as context.  Workgroup tier: ``--wide-rows``
rows at 8 x 256 + 2,048 and at one pod of 4,096 + 4,096.  Variants alternate
round by round; a round times ``--inner`` back-to-back launches between two
device events.  ``gpairs_per_s`` is the kernel's pair rate: the column pairs
inside the segments of all rows over K31's median time.  The numpy definition
is timed per row at the same shapes on the host (``--host-rows`` rows).

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
WIDE = ((8, 256, 2048), (1, 4096, 4096))


def _windows(rows: int, P: int, W: int, n_base: int, dev, seed: int):
    """Baseline and pods N(100, 5); every other row's pods creep upward by 2 sigma over the window."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    cur = 100 + 5 * torch.randn((rows, P * W), generator=g)
    cur[1::2] += torch.linspace(0, 10, W).repeat(P)
    base = 100 + 5 * torch.randn((rows, n_base), generator=g)
    seg = (torch.arange(1, P + 1, dtype=torch.int32) * W).repeat(rows, 1)
    return cur.to(dev), seg.to(dev), base.to(dev)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--wide-rows", type=int, default=1000)
    ap.add_argument("--host-rows", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "drift_test_bench.jsonl"))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_drift_test.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    # (5 points a pod: at the default 10 the 8-point pods of the wave shape would all be dropped)
    test, cfg = C.DriftTest("MANN_KENDALL", min_points=5), C.PairwiseConfig()
    for shapes, R, tier in ((WAVE, a.rows, "wave"), (WIDE, a.wide_rows, "wide")):
        for P, W, nb in shapes:
            cur, seg, base = _windows(R, P, W, nb, dev, 31)
            buf = C.alloc_drift(R, P, dev)
            var = {"k31": lambda: C.pairwise_drift(cur, seg, base, test, out=buf)}
            if tier == "wave":
                var["k4"] = lambda: C.pairwise_tests(cur, base, cfg)
            res = timed(var, a.rounds, a.warmup, a.inner)
            torch.cuda.synchronize()
            flagged = float(buf.drift_diff.float().mean())
            pairs = R * (P * W * (W - 1) // 2 + nb * (nb - 1) // 2)
            hc, hs, hb = (t[:a.host_rows].cpu().numpy() for t in (cur, seg, base))
            t0 = time.perf_counter()
            ref.pairwise_drift(hc, hs, hb, test.min_points)
            host_ms = (time.perf_counter() - t0) * 1e3 / max(1, len(hc))
            ln = {"bench": "drift_test_k31_alone", "tier": tier, "rows": R, "pods": P, "per_pod": W, "n_base": nb,
                  "flagged": round(flagged, 4), "inner": a.inner, "ms_per_launch": res, "pairs": pairs,
                  "gpairs_per_s": round(pairs / (res["k31"]["median"] * 1e-3) / 1e9, 2),
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
