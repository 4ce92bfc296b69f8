"""Stand-alone timing of the seasonal robust kernel (K14, fm_seasonal_robust)
at the headline history: 80,000 rows x T = 10,080 fp32 samples (3.2 GB),
period 1,440 (seven daily cycles at 60 s).

Timed in one process, alternating round by round, device events around
``--iters`` back-to-back launches, all on the same buffer:

  seasonal    fm_seasonal_robust: per-phase median profile smoothed over
              +- ``--smooth`` phases, the MAD-sigma of the residuals (one radix
              selection) and an H-step forecast (one HBM read of the history)
  robust      fm_robust_stats: median and MAD-sigma per row (two selections)
  hist_stats  fm_hist_stats: mean, std and finite count, one streaming read of
              the history, the yardstick

Rows are service metrics of different scales with a daily cycle, 1 % missing
samples and two 90-sample earlier incidents; every fourth row is an error
count that is mostly 0 (heavy ties, the MAD = 0 fallback).  The first
``--check-rows`` rows are compared with the numpy oracle before timing.

One JSON line is printed and appended to ``--out`` (default
profiles/seasonal_robust_bench.jsonl): the median per-call milliseconds of
each, the ratios, and the achieved read rate of the history bytes.  Needs a
GPU: there is no CPU fallback.

    python -m benchmarks.bench_seasonal_robust [--rows 80000] [--T 10080] [--period 1440] [--rounds 5] [--iters 10]
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
    ap.add_argument("--H", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--check-rows", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "seasonal_robust_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seasonal_robust needs a GPU")
    from foremast_amd.ops import misc as MI
    from foremast_amd.ops._lib import LIB, ptr, stream_of

    dev = torch.device("cuda", 0)
    R, T, m, H = a.rows, a.T, a.period, a.H
    J = MI.seasonal_cycles(T, m)
    if J < 2:
        raise SystemExit(f"T = {T}, period = {m}: fewer than two whole cycles within the kernel's budget")
    kw = MI.seasonal_halfwidth(m, a.smooth)
    ld = (T + 3) // 4 * 4
    gen = torch.Generator(device=dev).manual_seed(0)
    hist = torch.empty((R, ld), dtype=torch.float32, device=dev)
    chunk = 8000
    scale = torch.tensor([1.0, 100.0, 0.1, 30.0], device=dev).repeat((R + 3) // 4)[:R, None]
    counts = (torch.arange(R, device=dev) % 4 == 0)[:, None]
    wave = torch.sin(torch.arange(ld, device=dev) * (2 * math.pi / m))[None, :]
    for r0 in range(0, R, chunk):
        sl = slice(r0, min(r0 + chunk, R))
        z = torch.randn((sl.stop - r0, ld), generator=gen, device=dev)
        blk = (z * 0.2 + 5 + 2 * wave) * scale[sl]
        for s in (2 * m + m // 3, 4 * m + m // 2):                                                  # earlier incidents
            blk[:, s:s + 90] += 3 * scale[sl]
        blk = torch.where(counts[sl], torch.floor(torch.relu(z - 0.8) * 3), blk)                    # ~79 % zeros
        blk[torch.rand(blk.shape, generator=gen, device=dev) < 0.01] = float("nan")
        hist[sl] = blk
        del z, blk
    fc = torch.empty((R, H), dtype=torch.float32, device=dev)
    st = torch.empty((R, 2), dtype=torch.float32, device=dev)
    out = torch.empty((R, 3), dtype=torch.float32, device=dev)
    hs = torch.empty((R, 3), dtype=torch.float32, device=dev)

    def run_seasonal():
        LIB.call("fm_seasonal_robust", ptr(hist), hist.stride(0), T, R, m, J, kw, H, ptr(fc), H, ptr(st), None,
                 stream_of(hist))

    def run_robust():
        LIB.call("fm_robust_stats", ptr(hist), hist.stride(0), T, R, ptr(out), stream_of(hist))

    def run_hist_stats():
        LIB.call("fm_hist_stats", ptr(hist), hist.stride(0), T, R, ptr(hs), stream_of(hist))

    run_seasonal()
    torch.cuda.synchronize()
    k = min(a.check_rows, R)
    rf, rs, rn, _ = MI.ref_seasonal_robust(hist[:k, :T].cpu().numpy(), T, m, H, a.smooth)
    gf, gs = fc[:k].cpu().numpy(), st[:k].cpu().numpy()
    n_equal = bool(np.array_equal(gs[:, 1], rn.astype(np.float32)))
    fc_rel = float(np.nanmax(np.abs(gf - rf) / np.maximum(np.abs(rf), 1e-30)))
    sigma_rel = float(np.nanmax(np.abs(gs[:, 0] - rs) / np.maximum(np.abs(rs), 1e-30)))

    variants = {"seasonal": (run_seasonal, a.iters), "robust": (run_robust, a.iters),
                "hist_stats": (run_hist_stats, a.iters)}
    for f, _ in variants.values():                             # warm every shape the timed window uses
        f()
    torch.cuda.synchronize()
    times: dict[str, list[float]] = {k_: [] for k_ in variants}
    for _ in range(a.rounds):
        for k_, (f, it) in variants.items():
            times[k_].append(_timed(f, it))
    med = {k_: statistics.median(v) for k_, v in times.items()}
    span_bytes = R * J * m * 4
    rec = {"bench": "seasonal_robust", "device": torch.cuda.get_device_name(dev), "rows": R, "T": T, "period": m,
           "cycles": J, "smooth_halfwidth": kw, "H": H, "rounds": a.rounds, "iters": a.iters,
           "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
           "ms": {k_: round(v, 4) for k_, v in med.items()},
           "ms_min_max": {k_: [round(min(v), 4), round(max(v), 4)] for k_, v in times.items()},
           "seasonal_over_hist_stats": round(med["seasonal"] / med["hist_stats"], 3),
           "seasonal_over_robust": round(med["seasonal"] / med["robust"], 3),
           "history_GB": round(R * T * 4 / 1e9, 3), "span_GB": round(span_bytes / 1e9, 3),
           "span_GBps": {"seasonal": round(span_bytes / (med["seasonal"] * 1e-3) / 1e9, 1)},
           "history_GBps": {k_: round(R * T * 4 / (med[k_] * 1e-3) / 1e9, 1) for k_ in ("robust", "hist_stats")},
           "oracle_rows": k, "oracle_n_equal": n_equal, "oracle_forecast_max_rel": fc_rel,
           "oracle_sigma_max_rel": sigma_rel}
    line = json.dumps(rec)
    print(line)
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    with outp.open("a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
