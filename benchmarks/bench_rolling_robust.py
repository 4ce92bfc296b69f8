"""Stand-alone timing of the rolling robust bands (K34, fm_rolling_robust_stats)
against the rolling mean / std bands (K1, fm_rolling_stats) and the numpy
definition.

Shapes: the headline history, 80,000 rows x T = 10,080 at w = 60, and 1,000
rows at w = 60, 256 and 1,024 (the K = 1, 4 and 16 register windows).  Per
shape, in one process, alternating round by round, device events around
``--iters`` back-to-back launches on the same buffer:

  robust   fm_rolling_robust_stats: median, MAD sigma and finite count of the
           trailing window at every point, a sorted window sliding in registers
  rolling  fm_rolling_stats: mean and std of the same windows, the yardstick
  numpy    ref_rolling_robust_stats on the first ``--host-rows`` rows, one
           call, scaled to the shape's rows by rows / host-rows

Rows are service metrics of different scales with 1 % missing samples and 5 %
earlier incidents; every fourth row is an error count that is mostly 0 (heavy
ties, the MAD = 0 fallback).  The numpy result doubles as the check: center
and n of those rows must be equal, sigma within 1 ulp.

One JSON line per shape is printed and appended to ``--out`` (default
profiles/rolling_robust_bench.jsonl).  Needs a GPU: there is no CPU fallback.

    python -m benchmarks.bench_rolling_robust [--rows 80000] [--T 10080] [--rounds 5] [--iters 3]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def _timed(fn, iters: int) -> float:
    """ms per call: device events around ``iters`` launches."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _history(R: int, ld: int, dev) -> torch.Tensor:
    gen = torch.Generator(device=dev).manual_seed(0)
    hist = torch.empty((R, ld), dtype=torch.float32, device=dev)
    scale = torch.tensor([1.0, 100.0, 0.1, 30.0], device=dev).repeat((R + 3) // 4)[:R, None]
    counts = (torch.arange(R, device=dev) % 4 == 0)[:, None]
    for r0 in range(0, R, 8000):
        sl = slice(r0, min(r0 + 8000, R))
        z = torch.randn((sl.stop - r0, ld), generator=gen, device=dev)
        blk = z * scale[sl] + 5 * scale[sl]
        blk = torch.where(torch.rand(blk.shape, generator=gen, device=dev) < 0.05, blk * 10, blk)   # earlier incidents
        blk = torch.where(counts[sl], torch.floor(torch.relu(z - 0.8) * 3), blk)                    # ~79 % zeros
        blk[torch.rand(blk.shape, generator=gen, device=dev) < 0.01] = float("nan")
        hist[sl] = blk
    return hist


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--small-rows", type=int, default=1000)
    ap.add_argument("--T", type=int, default=10080)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--host-rows", type=int, default=8)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rolling_robust_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rolling_robust needs a GPU")
    from foremast_amd.ops import misc as MI
    from foremast_amd.ops._lib import LIB, ptr, stream_of

    dev = torch.device("cuda", 0)
    T = a.T
    ld = (T + 3) // 4 * 4
    hist = _history(max(a.rows, a.small_rows), ld, dev)
    outs = [torch.empty((hist.shape[0], T), dtype=torch.float32, device=dev) for _ in range(4)]
    cnt = torch.empty((hist.shape[0], T), dtype=torch.int32, device=dev)
    s = stream_of(hist)
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    for R, w in [(a.rows, 60), (a.small_rows, 60), (a.small_rows, 256), (a.small_rows, 1024)]:
        def run_robust():
            LIB.call("fm_rolling_robust_stats", ptr(hist), ld, T, R, w, 1, ptr(outs[0]), ptr(outs[1]), ptr(cnt), T, s)

        def run_rolling():
            LIB.call("fm_rolling_stats", ptr(hist), ld, T, R, w, 1, ptr(outs[2]), ptr(outs[3]), T, s)

        run_robust()
        run_rolling()                                          # warm both at this shape
        torch.cuda.synchronize()
        k = min(a.host_rows, R)
        x = hist[:k, :T].cpu().numpy()
        t0 = time.perf_counter()
        rc, rs, rn = MI.ref_rolling_robust_stats(x, w)
        host_ms = (time.perf_counter() - t0) * 1e3 * R / k
        c, sg, n = outs[0][:k].cpu().numpy(), outs[1][:k].cpu().numpy(), cnt[:k].cpu().numpy()
        ok = ~np.isnan(rs)
        ulps = np.abs(sg[ok].view(np.int32).astype(np.int64) - rs[ok].view(np.int32))
        equal = bool(np.array_equal(c, rc, equal_nan=True) and np.array_equal(n, rn)
                     and np.array_equal(np.isnan(sg), ~ok))
        times: dict[str, list[float]] = {"robust": [], "rolling": []}
        for _ in range(a.rounds):
            times["robust"].append(_timed(run_robust, a.iters))
            times["rolling"].append(_timed(run_rolling, a.iters))
        med = {k_: statistics.median(v) for k_, v in times.items()}
        rec = {"bench": "rolling_robust", "device": torch.cuda.get_device_name(dev), "rows": R, "T": T, "w": w,
               "rounds": a.rounds, "iters": a.iters, "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
               "ms": {k_: round(v, 4) for k_, v in med.items()},
               "ms_min_max": {k_: [round(min(v), 4), round(max(v), 4)] for k_, v in times.items()},
               "robust_over_rolling": round(med["robust"] / med["rolling"], 2),
               "numpy_ms_scaled": round(host_ms, 1), "numpy_rows": k,
               "numpy_over_robust": round(host_ms / med["robust"], 1),
               "ns_per_point": round(med["robust"] * 1e6 / (R * T), 4),
               "oracle_center_n_equal": equal, "oracle_sigma_max_ulp": int(ulps.max(initial=0))}
        line = json.dumps(rec)
        print(line, flush=True)
        with outp.open("a") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
