#!/usr/bin/env python3
"""The joint multi-metric canary test (K30): the kernel alone next to the
per-row rank tests on the same rows, one GPU, one process.

``--groups`` groups of 8 members at ``bench.py``'s window shape (50 + 50) and
``--wide-groups`` groups of 8 at 256 + 768: K30 (``fm_pairwise_joint``) beside
K4 (``fm_pairwise_tests``: the rank kernel and its p-values) on the 8 x groups
rows.  Variants alternate round by round; a round times ``--inner``
back-to-back launches between two device events.  The numpy definition is
timed per group at the same shapes on the host (``--host-groups`` groups).

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

M = 8


def _windows(groups: int, n_cur: int, n_base: int, dev, seed: int):
    """8 members per group sharing a common factor, N(100, 5); every other group has member 0 a quarter sigma up."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    n = n_cur + n_base
    x = 100 + 5 * (0.7 * torch.randn((groups, 1, n), generator=g) + torch.randn((groups, M, n), generator=g))
    x[1::2, 0, :n_cur] += 1.25
    x = x.reshape(groups * M, n)
    rows = torch.arange(groups * M, dtype=torch.int32).reshape(groups, M)
    return (x[:, :n_cur].contiguous().to(dev), x[:, n_cur:].contiguous().to(dev), rows.to(dev),
            torch.full((groups,), M, dtype=torch.int32, device=dev))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=10000)
    ap.add_argument("--wide-groups", type=int, default=1000)
    ap.add_argument("--host-groups", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "joint_test_bench.jsonl"))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_joint_test.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    test, cfg = C.JointTest("RANK_SUM"), C.PairwiseConfig()
    for G, n_cur, n_base in ((a.groups, 50, 50), (a.wide_groups, 256, 768)):
        cur, base, rows, K = _windows(G, n_cur, n_base, dev, 30)
        buf = C.alloc_joint(G, dev)
        var = {"k30": lambda: C.pairwise_joint(cur, base, rows, K, test, out=buf),
               "k4": lambda: C.pairwise_tests(cur, base, cfg)}
        res = timed(var, a.rounds, a.warmup, a.inner)
        torch.cuda.synchronize()
        flagged = float(buf.joint_diff.float().mean())
        k4_any = float(C.pairwise_tests(cur, base, cfg)[2].reshape(G, M).amax(1).float().mean())
        h = a.host_groups
        hc, hb = cur[:h * M].cpu().numpy(), base[:h * M].cpu().numpy()
        t0 = time.perf_counter()
        ref.pairwise_joint(hc, hb, rows[:h].cpu().numpy(), K[:h].cpu().numpy(), test.min_points)
        host_ms = (time.perf_counter() - t0) * 1e3 / max(1, h)
        ln = {"bench": "joint_test_k30_alone", "groups": G, "members": M, "n_cur": n_cur, "n_base": n_base,
              "flagged": round(flagged, 4), "k4_any_row_flagged": round(k4_any, 4), "inner": a.inner,
              "ms_per_launch": res, "host_ms_per_group": round(host_ms, 4), "label": a.label, "rounds": a.rounds,
              "device": torch.cuda.get_device_name(dev)}
        s = json.dumps(ln)
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "a") as f:
                f.write(s + "\n")
        del cur, base, rows, K, buf
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
