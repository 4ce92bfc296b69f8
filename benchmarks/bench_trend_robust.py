"""Stand-alone timing of the trend robust kernel (K16, fm_trend_robust) at the
headline history: 80,000 rows x T = 10,080 fp32 samples (3.2 GB), blocks of
1,440 (seven days at 60 s).

Timed in one process, alternating round by round, device events around
``--iters`` back-to-back launches, all on the same buffer:

  trend       fm_trend_robust: the medians of the J blocks selected together,
              the repeated-median slope, the row detrended in place, median
              and MAD-sigma of the residuals (one HBM read of the history)
  shift       fm_shift_robust on the same rows, none of which carries a level
              shift: whole-row median and MAD-sigma, the J block medians one
              selection after another, the candidate scan
  robust      fm_robust_stats: median and MAD-sigma per row (two selections)
  hist_stats  fm_hist_stats: mean, std and finite count, one streaming read of
              the history, the yardstick

Rows are service metrics of different scales that drift by a fifth of their
level over the week (up and down), with 1 % missing samples and 5 % earlier
incidents.  The first ``--check-rows`` rows are compared with the numpy oracle
before timing.

One JSON line is printed and appended to ``--out`` (default
profiles/trend_robust_bench.jsonl): the median per-call milliseconds of each
with their min-max, and the ratios.  Needs a GPU: there is no CPU fallback.

    python -m benchmarks.bench_trend_robust [--rows 80000] [--T 10080] [--block 1440] [--rounds 5] [--iters 10]
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--T", type=int, default=10080)
    ap.add_argument("--block", type=int, default=1440)
    ap.add_argument("--min-blocks", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--check-rows", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "trend_robust_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_trend_robust needs a GPU")
    from foremast_amd.ops import misc as MI
    from foremast_amd.ops._lib import LIB, ptr, stream_of

    dev = torch.device("cuda", 0)
    R, T, L, mb = a.rows, a.T, a.block, a.min_blocks
    J = MI.shift_blocks(T, L)
    if T > MI.ROBUST_LDS_KEYS or J < mb:
        raise SystemExit(f"T = {T}, block = {L}: the row must fit the LDS and hold {mb} blocks")
    ld = (T + 3) // 4 * 4
    gen = torch.Generator(device=dev).manual_seed(0)
    hist = torch.empty((R, ld), dtype=torch.float32, device=dev)
    chunk = 8000
    scale = torch.tensor([1.0, 100.0, 0.1, 30.0], device=dev).repeat((R + 3) // 4)[:R, None]
    drift = torch.tensor([1.0, -1.0], device=dev).repeat((R + 1) // 2)[:R, None]
    ramp = torch.arange(ld, device=dev, dtype=torch.float32)[None, :] / max(T - 1, 1)
    for r0 in range(0, R, chunk):
        sl = slice(r0, min(r0 + chunk, R))
        blk = (torch.randn((sl.stop - r0, ld), generator=gen, device=dev) * 0.2 + 5 + drift[sl] * ramp) * scale[sl]
        u = torch.rand(blk.shape, generator=gen, device=dev)
        blk = torch.where(u < 0.05, blk * 4, blk)                                                   # earlier incidents
        blk[u > 0.99] = float("nan")
        hist[sl] = blk
        del blk, u
    out4 = torch.empty((R, 4), dtype=torch.float32, device=dev)
    out6 = torch.empty((R, 6), dtype=torch.float32, device=dev)
    out3 = torch.empty((R, 3), dtype=torch.float32, device=dev)
    hs = torch.empty((R, 3), dtype=torch.float32, device=dev)

    def run_trend():
        LIB.call("fm_trend_robust", ptr(hist), hist.stride(0), T, R, L, J, mb, ptr(out4), stream_of(hist))

    def run_shift():                                           # no score exceeds an infinite threshold: unshifted rows
        LIB.call("fm_shift_robust", ptr(hist), hist.stride(0), T, R, L, J, float("inf"), 2, ptr(out6), stream_of(hist))

    def run_robust():
        LIB.call("fm_robust_stats", ptr(hist), hist.stride(0), T, R, ptr(out3), stream_of(hist))

    def run_hist_stats():
        LIB.call("fm_hist_stats", ptr(hist), hist.stride(0), T, R, ptr(hs), stream_of(hist))

    variants = {"trend": run_trend, "shift": run_shift, "robust": run_robust, "hist_stats": run_hist_stats}
    for f in variants.values():                                # warm every shape the timed window uses
        f()
    torch.cuda.synchronize()
    k = min(a.check_rows, R)
    ref = MI.ref_trend_robust(hist[:k, :T].cpu().numpy(), T, L, mb)
    got = out4[:k].cpu().numpy()
    exact = all(np.array_equal(got[:, i], ref[i].astype(np.float32), equal_nan=True) for i in (0, 2, 3))
    sigma_rel = float(np.nanmax(np.abs(got[:, 1] - ref[1]) / np.maximum(np.abs(ref[1]), 1e-30)))
    times: dict[str, list[float]] = {k_: [] for k_ in variants}
    for _ in range(a.rounds):
        for k_, f in variants.items():
            times[k_].append(_timed(f, a.iters))
    med = {k_: statistics.median(v) for k_, v in times.items()}
    rec = {"bench": "trend_robust", "device": torch.cuda.get_device_name(dev), "rows": R, "T": T, "block": L,
           "blocks": J, "min_blocks": mb, "rounds": a.rounds, "iters": a.iters,
           "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "history_GB": round(R * T * 4 / 1e9, 3),
           "rows_shifted": int((out6[:, 3] > 0).sum().item()),
           "ms": {k_: round(v, 4) for k_, v in med.items()},
           "ms_min_max": {k_: [round(min(v), 4), round(max(v), 4)] for k_, v in times.items()},
           "trend_over_shift": round(med["trend"] / med["shift"], 3),
           "trend_over_robust": round(med["trend"] / med["robust"], 3),
           "trend_over_hist_stats": round(med["trend"] / med["hist_stats"], 3),
           "history_GBps": {k_: round(R * T * 4 / (v * 1e-3) / 1e9, 1) for k_, v in med.items()},
           "oracle_rows": k, "oracle_center_n_slope_equal": bool(exact), "oracle_sigma_max_rel": sigma_rel}
    line = json.dumps(rec)
    print(line)
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    with outp.open("a") as fh:
        fh.write(line + "\n")
    if not exact:
        raise SystemExit("bench_trend_robust: the kernel differs from the oracle")


if __name__ == "__main__":
    main()
