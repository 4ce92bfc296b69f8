"""Stand-alone timing of the seasonal trend robust kernel (K20,
fm_seasonal_trend_robust) at the headline history: 80,000 rows x T = 10,080
fp32 samples (3.2 GB), period 1,440 (seven days at 60 s).

Timed in one process, alternating round by round, device events around
``--iters`` back-to-back launches, all on the same buffer:

  seasonal_trend  fm_seasonal_trend_robust: the medians of the J cycles
                  selected together, the repeated-median slope, the span
                  detrended in place, the per-phase profile of the residuals,
                  its smoothing, the forecast and the MAD-sigma (one HBM read
                  of the history)
  seasonal        fm_seasonal_robust (K14) on the same rows: profile,
                  smoothing, forecast, MAD-sigma
  trend           fm_trend_robust (K16) on the same rows, blocks of one
                  period: block medians, slope, median and MAD-sigma of the
                  residuals
  hist_stats      fm_hist_stats: mean, std and finite count, one streaming
                  read of the history

The yardstick is ``seasonal`` + ``trend``, the two kernels run back to back:
K20 does the selections of both on one read of the history.

Rows are service metrics of different scales that drift by a fifth of their
level over the week (up and down) under a daily cycle of a tenth of it, with
1 % missing samples and 5 % earlier incidents.  The first ``--check-rows``
rows are compared with the numpy oracle before timing.

One JSON line is printed and appended to ``--out`` (default
profiles/seasonal_trend_robust_bench.jsonl): the median per-call milliseconds
of each with their min-max, and the ratios.  Needs a GPU: there is no CPU
fallback.

    python -m benchmarks.bench_seasonal_trend_robust [--rows 80000] [--T 10080] [--period 1440] [--rounds 5] [--iters 10]
"""
from __future__ import annotations

import argparse
import json
import math
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
    ap.add_argument("--period", type=int, default=1440)
    ap.add_argument("--smooth", type=int, default=5)
    ap.add_argument("--min-blocks", type=int, default=3)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--check-rows", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "seasonal_trend_robust_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seasonal_trend_robust needs a GPU")
    from foremast_amd.ops import misc as MI
    from foremast_amd.ops._lib import LIB, ptr, stream_of

    dev = torch.device("cuda", 0)
    R, T, m, mb, H = a.rows, a.T, a.period, a.min_blocks, a.horizon
    J = MI.seasonal_cycles(T, m)
    if T > MI.ROBUST_LDS_KEYS or J < max(mb, 2):
        raise SystemExit(f"T = {T}, period = {m}: the row must fit the LDS and hold {max(mb, 2)} cycles")
    k = MI.seasonal_halfwidth(m, a.smooth)
    ld = (T + 3) // 4 * 4
    gen = torch.Generator(device=dev).manual_seed(0)
    hist = torch.empty((R, ld), dtype=torch.float32, device=dev)
    chunk = 8000
    scale = torch.tensor([1.0, 100.0, 0.1, 30.0], device=dev).repeat((R + 3) // 4)[:R, None]
    drift = torch.tensor([1.0, -1.0], device=dev).repeat((R + 1) // 2)[:R, None]
    col = torch.arange(ld, device=dev, dtype=torch.float32)[None, :]
    ramp = col / max(T - 1, 1)
    wave = 0.5 * torch.sin(col * (2 * math.pi / m))
    for r0 in range(0, R, chunk):
        sl = slice(r0, min(r0 + chunk, R))
        blk = (torch.randn((sl.stop - r0, ld), generator=gen, device=dev) * 0.2 + 5 + drift[sl] * ramp + wave) * scale[sl]
        u = torch.rand(blk.shape, generator=gen, device=dev)
        blk = torch.where(u < 0.05, blk * 4, blk)                                                   # earlier incidents
        blk[u > 0.99] = float("nan")
        hist[sl] = blk
        del blk, u
    fc20 = torch.empty((R, max(H, 1)), dtype=torch.float32, device=dev)
    st20 = torch.empty((R, 4), dtype=torch.float32, device=dev)
    fc14 = torch.empty((R, max(H, 1)), dtype=torch.float32, device=dev)
    st14 = torch.empty((R, 2), dtype=torch.float32, device=dev)
    out16 = torch.empty((R, 4), dtype=torch.float32, device=dev)
    hs = torch.empty((R, 3), dtype=torch.float32, device=dev)
    J16 = MI.shift_blocks(T, m)

    def run_seasonal_trend():
        LIB.call("fm_seasonal_trend_robust", ptr(hist), hist.stride(0), T, R, m, J, k, mb, H, ptr(fc20), max(H, 1),
                 ptr(st20), None, stream_of(hist))

    def run_seasonal():
        LIB.call("fm_seasonal_robust", ptr(hist), hist.stride(0), T, R, m, J, k, H, ptr(fc14), max(H, 1), ptr(st14),
                 None, stream_of(hist))

    def run_trend():
        LIB.call("fm_trend_robust", ptr(hist), hist.stride(0), T, R, m, J16, max(mb, 2), ptr(out16), stream_of(hist))

    def run_hist_stats():
        LIB.call("fm_hist_stats", ptr(hist), hist.stride(0), T, R, ptr(hs), stream_of(hist))

    variants = {"seasonal_trend": run_seasonal_trend, "seasonal": run_seasonal, "trend": run_trend,
                "hist_stats": run_hist_stats}
    for f in variants.values():                                # warm every shape the timed window uses
        f()
    torch.cuda.synchronize()
    c = min(a.check_rows, R)
    ref = MI.ref_seasonal_trend_robust(hist[:c, :T].cpu().numpy(), T, m, H, a.smooth, mb)
    got = st20[:c].cpu().numpy()
    exact = all(np.array_equal(got[:, i], ref[j].astype(np.float32), equal_nan=True) for i, j in ((1, 2), (2, 3), (3, 4)))
    sigma_rel = float(np.nanmax(np.abs(got[:, 0] - ref[1]) / np.maximum(np.abs(ref[1]), 1e-30)))
    fc_rel = float(np.nanmax(np.abs(fc20[:c, :H].cpu().numpy() - ref[0]) / np.maximum(np.abs(ref[0]), 1e-30))) if H else 0.0
    times: dict[str, list[float]] = {k_: [] for k_ in variants}
    for _ in range(a.rounds):
        for k_, f in variants.items():
            times[k_].append(_timed(f, a.iters))
    med = {k_: statistics.median(v) for k_, v in times.items()}
    both = med["seasonal"] + med["trend"]
    rec = {"bench": "seasonal_trend_robust", "device": torch.cuda.get_device_name(dev), "rows": R, "T": T, "period": m,
           "cycles": J, "halfwidth": k, "min_blocks": mb, "horizon": H, "rounds": a.rounds, "iters": a.iters,
           "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "history_GB": round(R * T * 4 / 1e9, 3),
           "ms": {k_: round(v, 4) for k_, v in med.items()},
           "ms_min_max": {k_: [round(min(v), 4), round(max(v), 4)] for k_, v in times.items()},
           "seasonal_plus_trend_ms": round(both, 4),
           "seasonal_trend_over_seasonal_plus_trend": round(med["seasonal_trend"] / both, 3),
           "seasonal_trend_over_seasonal": round(med["seasonal_trend"] / med["seasonal"], 3),
           "seasonal_trend_over_trend": round(med["seasonal_trend"] / med["trend"], 3),
           "seasonal_trend_over_hist_stats": round(med["seasonal_trend"] / med["hist_stats"], 3),
           "history_GBps": {k_: round(R * T * 4 / (v * 1e-3) / 1e9, 1) for k_, v in med.items()},
           "oracle_rows": c, "oracle_n_slope_nblocks_equal": bool(exact), "oracle_sigma_max_rel": sigma_rel,
           "oracle_forecast_max_rel": fc_rel}
    line = json.dumps(rec)
    print(line)
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    with outp.open("a") as fh:
        fh.write(line + "\n")
    if not exact:
        raise SystemExit("bench_seasonal_trend_robust: the kernel differs from the oracle")


if __name__ == "__main__":
    main()
