#!/usr/bin/env python3
"""The dependence gate (K33): the kernel alone, one GPU, one process.

Wave tier: ``--rows`` rows of 8 pods x 8 + 64 baseline points, K33
(``fm_pairwise_dependence``) beside K4 (``fm_pairwise_tests``: the rank kernel
and its p-values) on the same rows, as context.  Workgroup tier: ``--wide-rows``
rows at 8 x 256 + 2,048 and at one pod of 4,096 + 4,096.  Variants alternate
round by round; a round times ``--inner`` back-to-back launches between two
device events.  ``k33_lag1`` is the same kernel asked for one lag instead of
eight: the difference to ``k33`` is seven of the nine sweeps of the lag pass
(lags 0 .. 8), from which ``lag_pass_share`` extrapolates the pass's share of
the kernel; the rest is the load, the sort, the ranks and the finish.  The numpy
definition is timed per row at the same shapes on the host (``--host-rows``).

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
    """Both sides AR(1) noise (rho = 0.7) around 100, pod by pod; every other row's canary sits half a sigma up."""
    g = torch.Generator(device="cpu").manual_seed(seed)

    def ar1(n_seg, n):
        e = torch.randn((rows, n_seg, n), generator=g)
        for i in range(1, n):
            e[:, :, i] += 0.7 * e[:, :, i - 1]
        return (100 + 5 * e).reshape(rows, n_seg * n)

    cur, base = ar1(P, W), ar1(1, n_base)
    cur[1::2] += 3.5
    seg = (torch.arange(1, P + 1, dtype=torch.int32) * W).repeat(rows, 1)
    return cur.to(dev), seg.to(dev), base.to(dev)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--wide-rows", type=int, default=1000)
    ap.add_argument("--host-rows", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--out", default=os.path.join("profiles", "dependence_gate_bench.jsonl"))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_dependence_gate.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    # (8 points a segment: at the default 12 the 8-point pods of the wave shape would all be dropped)
    gate, one, cfg = C.DependenceGate("RANK_ACF", min_points=8), C.DependenceGate("RANK_ACF", max_lag=1,
                                                                               min_points=8), C.PairwiseConfig()
    for shapes, R, tier in ((WAVE, a.rows, "wave"), (WIDE, a.wide_rows, "wide")):
        for P, W, nb in shapes:
            cur, seg, base = _windows(R, P, W, nb, dev, 33)
            buf = C.alloc_dependence(R, dev)
            var = {"k33": lambda: C.pairwise_dependence(cur, seg, base, gate, out=buf),
                   "k33_lag1": lambda: C.pairwise_dependence(cur, seg, base, one, out=buf)}
            if tier == "wave":
                var["k4"] = lambda: C.pairwise_tests(cur, base, cfg)
            res = timed(var, a.rounds, a.warmup, a.inner)
            C.pairwise_dependence(cur, seg, base, gate, out=buf)
            torch.cuda.synchronize()
            kept = float(buf.dep_keep.float().mean())
            # lags 0 .. L are L + 1 sweeps; one lag is two of them
            lag_share = (gate.max_lag + 1) * (res["k33"]["median"] - res["k33_lag1"]["median"]) / (gate.max_lag - 1) \
                / res["k33"]["median"]
            hc, hs, hb = (t[:a.host_rows].cpu().numpy() for t in (cur, seg, base))
            t0 = time.perf_counter()
            ref.pairwise_dependence(hc, hs, hb, gate.max_lag, gate.min_points)
            host_ms = (time.perf_counter() - t0) * 1e3 / max(1, len(hc))
            ln = {"bench": "dependence_gate_k33_alone", "tier": tier, "rows": R, "pods": P, "per_pod": W, "n_base": nb,
                  "kept": round(kept, 4), "inner": a.inner, "ms_per_launch": res,
                  "lag_pass_share": round(lag_share, 3), "host_ms_per_row": round(host_ms, 4), "label": a.label,
                  "rounds": a.rounds, "device": torch.cuda.get_device_name(dev)}
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
