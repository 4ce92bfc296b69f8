"""Stand-alone timing of the level-shift robust kernel (K15, fm_shift_robust)
at the headline history: 80,000 rows x T = 10,080 fp32 samples (3.2 GB),
blocks of 1,440 (seven days at 60 s).

Timed in one process, alternating round by round, device events around
``--iters`` back-to-back launches, all on the same buffer:

  shift       fm_shift_robust: whole-row median and MAD-sigma, the medians of
              the J blocks, the candidate scan, and for a row with a shift the
              median and MAD-sigma of its segment (one HBM read of the history)
  robust      fm_robust_stats: median and MAD-sigma per row (two selections)
  hist_stats  fm_hist_stats: mean, std and finite count, one streaming read of
              the history, the yardstick

Rows are service metrics of different scales with 1 % missing samples and 5 %
earlier incidents.  The three are timed three times over: with no row, 10 %
of the rows and every row carrying a level shift two and a half days before
the end (the buffer is stepped in place between the stages, so the other
samples stay the same).  The first ``--check-rows`` rows of every stage are
compared with the numpy oracle before timing.

One JSON line is printed and appended to ``--out`` (default
profiles/shift_robust_bench.jsonl): per stage the median per-call milliseconds
of each and the ratios.  Needs a GPU: there is no CPU fallback.

    python -m benchmarks.bench_shift_robust [--rows 80000] [--T 10080] [--block 1440] [--rounds 5] [--iters 10]
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
    ap.add_argument("--k", type=float, default=4.0)
    ap.add_argument("--min-blocks", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--check-rows", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "shift_robust_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_shift_robust needs a GPU")
    from foremast_amd.ops import misc as MI
    from foremast_amd.ops._lib import LIB, ptr, stream_of

    dev = torch.device("cuda", 0)
    R, T, L, mb = a.rows, a.T, a.block, a.min_blocks
    J = MI.shift_blocks(T, L)
    if T > MI.ROBUST_LDS_KEYS or J < 3 + mb:
        raise SystemExit(f"T = {T}, block = {L}: the row must fit the LDS and hold {3 + mb} blocks")
    ld = (T + 3) // 4 * 4
    gen = torch.Generator(device=dev).manual_seed(0)
    hist = torch.empty((R, ld), dtype=torch.float32, device=dev)
    chunk = 8000
    scale = torch.tensor([1.0, 100.0, 0.1, 30.0], device=dev).repeat((R + 3) // 4)[:R, None]
    for r0 in range(0, R, chunk):
        sl = slice(r0, min(r0 + chunk, R))
        blk = (torch.randn((sl.stop - r0, ld), generator=gen, device=dev) * 0.2 + 5) * scale[sl]
        u = torch.rand(blk.shape, generator=gen, device=dev)
        blk = torch.where(u < 0.05, blk * 4, blk)                                                   # earlier incidents
        blk[u > 0.99] = float("nan")
        hist[sl] = blk
        del blk, u
    at = T - 2 * L - L // 2                                    # the step: two and a half blocks before the end
    out6 = torch.empty((R, 6), dtype=torch.float32, device=dev)
    out3 = torch.empty((R, 3), dtype=torch.float32, device=dev)
    hs = torch.empty((R, 3), dtype=torch.float32, device=dev)

    def run_shift():
        LIB.call("fm_shift_robust", ptr(hist), hist.stride(0), T, R, L, J, a.k, mb, ptr(out6), stream_of(hist))

    def run_robust():
        LIB.call("fm_robust_stats", ptr(hist), hist.stride(0), T, R, ptr(out3), stream_of(hist))

    def run_hist_stats():
        LIB.call("fm_hist_stats", ptr(hist), hist.stride(0), T, R, ptr(hs), stream_of(hist))

    variants = {"shift": run_shift, "robust": run_robust, "hist_stats": run_hist_stats}
    stages, done = {}, 0
    for name, frac in (("0", 0.0), ("10", 0.1), ("100", 1.0)):
        upto = int(round(frac * R))
        if upto > done:                                        # step rows [done, upto) up by 30 sigma, in place
            hist[done:upto, at:] += 6.0 * scale[done:upto]
            done = upto
        for f in variants.values():                            # warm every shape the timed window uses
            f()
        torch.cuda.synchronize()
        k = min(a.check_rows, R)
        ref = MI.ref_shift_robust(hist[:k, :T].cpu().numpy(), T, L, a.k, mb)
        got = out6[:k].cpu().numpy()
        exact = all(np.array_equal(got[:, i], ref[i].astype(np.float32), equal_nan=True) for i in (0, 2, 3, 4))
        sigma_rel = float(np.nanmax(np.abs(got[:, 1] - ref[1]) / np.maximum(np.abs(ref[1]), 1e-30)))
        times: dict[str, list[float]] = {k_: [] for k_ in variants}
        for _ in range(a.rounds):
            for k_, f in variants.items():
                times[k_].append(_timed(f, a.iters))
        med = {k_: statistics.median(v) for k_, v in times.items()}
        stages[name] = {"rows_shifted": int((out6[:, 3] > 0).sum().item()),
                        "ms": {k_: round(v, 4) for k_, v in med.items()},
                        "ms_min_max": {k_: [round(min(v), 4), round(max(v), 4)] for k_, v in times.items()},
                        "shift_over_robust": round(med["shift"] / med["robust"], 3),
                        "shift_over_hist_stats": round(med["shift"] / med["hist_stats"], 3),
                        "history_GBps": {k_: round(R * T * 4 / (v * 1e-3) / 1e9, 1) for k_, v in med.items()},
                        "oracle_rows": k, "oracle_center_n_start_delta_equal": bool(exact),
                        "oracle_sigma_max_rel": sigma_rel}
    rec = {"bench": "shift_robust", "device": torch.cuda.get_device_name(dev), "rows": R, "T": T, "block": L,
           "blocks": J, "k": a.k, "min_blocks": mb, "rounds": a.rounds, "iters": a.iters,
           "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "history_GB": round(R * T * 4 / 1e9, 3),
           "percent_shifted": stages}
    line = json.dumps(rec)
    print(line)
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    with outp.open("a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
