"""Stand-alone timing of the robust-statistics kernel (K13, fm_robust_stats)
at the headline history: 80,000 rows x T = 10,080 fp32 samples (3.2 GB).

Timed in one process, alternating round by round, device events around
``--iters`` back-to-back launches, all on the same buffer:

  robust      fm_robust_stats: median, MAD-sigma and finite count per row by
              exact radix selection in LDS (one HBM read of the history)
  hist_stats  fm_hist_stats: mean, std and finite count, one streaming read of
              the history, the yardstick
  torch       the same three outputs from torch: nanmedian, subtract, abs,
              nanmedian, isfinite-sum (``--torch-iters`` calls per round)

Rows are service metrics of different scales with 1 % missing samples and
5 % earlier incidents; every fourth row is an error count that is mostly 0
(heavy ties, the MAD = 0 fallback).  The first ``--check-rows`` rows are
compared with the numpy oracle before timing.

One JSON line is printed and appended to ``--out`` (default
profiles/robust_bench.jsonl): the median per-call milliseconds of each, both
ratios, and the achieved read rate of the history bytes.  Needs a GPU: there
is no CPU fallback.

    python -m benchmarks.bench_robust [--rows 80000] [--T 10080] [--rounds 5] [--iters 10]
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=1)
    ap.add_argument("--check-rows", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "robust_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_robust needs a GPU")
    from foremast_amd.ops import misc as MI
    from foremast_amd.ops._lib import LIB, ptr, stream_of

    dev = torch.device("cuda", 0)
    R, T = a.rows, a.T
    ld = (T + 3) // 4 * 4
    gen = torch.Generator(device=dev).manual_seed(0)
    hist = torch.empty((R, ld), dtype=torch.float32, device=dev)
    chunk = 8000
    scale = torch.tensor([1.0, 100.0, 0.1, 30.0], device=dev).repeat((R + 3) // 4)[:R, None]
    counts = (torch.arange(R, device=dev) % 4 == 0)[:, None]
    for r0 in range(0, R, chunk):
        sl = slice(r0, min(r0 + chunk, R))
        z = torch.randn((sl.stop - r0, ld), generator=gen, device=dev)
        blk = z * scale[sl] + 5 * scale[sl]
        blk = torch.where(torch.rand(blk.shape, generator=gen, device=dev) < 0.05, blk * 10, blk)   # earlier incidents
        blk = torch.where(counts[sl], torch.floor(torch.relu(z - 0.8) * 3), blk)                    # ~79 % zeros
        blk[torch.rand(blk.shape, generator=gen, device=dev) < 0.01] = float("nan")
        hist[sl] = blk
        del z, blk
    out = torch.empty((R, 3), dtype=torch.float32, device=dev)
    hs = torch.empty((R, 3), dtype=torch.float32, device=dev)

    def run_robust():
        LIB.call("fm_robust_stats", ptr(hist), hist.stride(0), T, R, ptr(out), stream_of(hist))

    def run_hist_stats():
        LIB.call("fm_hist_stats", ptr(hist), hist.stride(0), T, R, ptr(hs), stream_of(hist))

    def run_torch():
        x = hist[:, :T]
        med = torch.nanmedian(x, dim=1).values
        mad = torch.nanmedian((x - med[:, None]).abs(), dim=1).values
        return med, 1.4826 * mad, torch.isfinite(x).sum(1)

    run_robust()
    torch.cuda.synchronize()
    k = min(a.check_rows, R)
    rc, rs, rn = MI.ref_robust_stats(hist[:k, :T].cpu().numpy(), T)
    got = out[:k].cpu().numpy()
    exact = bool(np.array_equal(got[:, 0], rc, equal_nan=True) and np.array_equal(got[:, 2], rn.astype(np.float32)))
    sigma_rel = float(np.nanmax(np.abs(got[:, 1] - rs) / np.maximum(np.abs(rs), 1e-30)))

    variants = {"robust": (run_robust, a.iters), "hist_stats": (run_hist_stats, a.iters),
                "torch": (run_torch, a.torch_iters)}
    for f, _ in variants.values():                             # warm every shape the timed window uses
        f()
    torch.cuda.synchronize()
    times: dict[str, list[float]] = {k_: [] for k_ in variants}
    for _ in range(a.rounds):
        for k_, (f, it) in variants.items():
            times[k_].append(_timed(f, it))
    med = {k_: statistics.median(v) for k_, v in times.items()}
    hist_bytes = R * T * 4
    rec = {"bench": "robust", "device": torch.cuda.get_device_name(dev), "rows": R, "T": T, "rounds": a.rounds,
           "iters": a.iters, "torch_iters": a.torch_iters,
           "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
           "ms": {k_: round(v, 4) for k_, v in med.items()},
           "ms_min_max": {k_: [round(min(v), 4), round(max(v), 4)] for k_, v in times.items()},
           "robust_over_hist_stats": round(med["robust"] / med["hist_stats"], 3),
           "robust_over_torch": round(med["robust"] / med["torch"], 4),
           "history_GB": round(hist_bytes / 1e9, 3),
           "history_GBps": {k_: round(hist_bytes / (med[k_] * 1e-3) / 1e9, 1) for k_ in variants},
           "lds_keys": MI.ROBUST_LDS_KEYS, "oracle_rows": k, "oracle_center_n_equal": exact,
           "oracle_sigma_max_rel": sigma_rel}
    line = json.dumps(rec)
    print(line)
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    with outp.open("a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
