"""Stand-alone timing of the quantile robust statistics kernel (K24,
fm_quantile_robust_stats) and of the band decision with two sigmas
(fm_band_decide_2s) at the headline shapes: 80,000 rows x T = 10,080 fp32
samples (3.2 GB) of right-skewed metrics, 30 current points a row.

Timed in one process, alternating round by round, device events around
``--iters`` back-to-back launches, all on the same buffers:

  quantile    fm_quantile_robust_stats: median and a sigma per side from three
              ranks of the row, selected in LDS (one HBM read of the history)
  robust      fm_robust_stats (K13) on the same rows: median and MAD, two
              selections with the keys rewritten in between
  hist_stats  fm_hist_stats: mean, std and finite count, one streaming read of
              the history, the yardstick
  band_2s     fm_band_decide_2s, sigma_lo [R] and sigma_up [R]
  band        fm_band_decide on the same points, one sigma [R]

Rows are 100 exp(s N) with s cycling through 0.5, 0.8 and 0.3 and an
exponential(100) row as every fourth, 1 % of the samples a 5 x incident and
1 % missing.  The first ``--check-rows`` rows are compared with the numpy
oracle before timing.

One JSON line is printed and appended to ``--out`` (default
profiles/quantile_robust_bench.jsonl): the median per-call milliseconds of
each, the ratios, and the achieved read rate of the history bytes.  Needs a
GPU: there is no CPU fallback.

    python -m benchmarks.bench_quantile_robust [--rows 80000] [--T 10080] [--z0 2.0] [--rounds 5] [--iters 10]
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
    ap.add_argument("--z0", type=float, default=2.0)
    ap.add_argument("--points", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--check-rows", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "quantile_robust_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_quantile_robust needs a GPU")
    from foremast_amd.ops import misc as MI
    from foremast_amd.ops import smoothing as SM
    from foremast_amd.ops._lib import LIB, ptr, stream_of

    dev = torch.device("cuda", 0)
    R, T, n = a.rows, a.T, a.points
    p, iz = MI.quantile_tail_params(a.z0)
    ld = (T + 3) // 4 * 4
    gen = torch.Generator(device=dev).manual_seed(0)
    hist = torch.empty((R, ld), dtype=torch.float32, device=dev)
    chunk = 8000
    shape = torch.tensor([0.5, 0.8, 0.3, 0.0], device=dev).repeat((R + 3) // 4)[:R, None]
    for r0 in range(0, R, chunk):
        sl = slice(r0, min(r0 + chunk, R))
        z = torch.randn((sl.stop - r0, ld), generator=gen, device=dev)
        u = torch.rand(z.shape, generator=gen, device=dev)
        blk = torch.where(shape[sl] > 0, 100 * torch.exp(shape[sl] * z), -100 * torch.log1p(-u))
        blk = torch.where(torch.rand(blk.shape, generator=gen, device=dev) < 0.01, blk * 5, blk)    # earlier incidents
        blk[torch.rand(blk.shape, generator=gen, device=dev) < 0.01] = float("nan")
        hist[sl] = blk
        del z, u, blk
    out4 = torch.empty((R, 4), dtype=torch.float32, device=dev)
    out3 = torch.empty((R, 3), dtype=torch.float32, device=dev)
    hs = torch.empty((R, 3), dtype=torch.float32, device=dev)

    def run_quantile():
        LIB.call("fm_quantile_robust_stats", ptr(hist), hist.stride(0), T, R, p, float(iz), ptr(out4),
                 stream_of(hist))

    def run_robust():
        LIB.call("fm_robust_stats", ptr(hist), hist.stride(0), T, R, ptr(out3), stream_of(hist))

    def run_hist_stats():
        LIB.call("fm_hist_stats", ptr(hist), hist.stride(0), T, R, ptr(hs), stream_of(hist))

    run_quantile()
    run_robust()
    torch.cuda.synchronize()
    k = min(a.check_rows, R)
    rc, rsl, rsu, rn = MI.ref_quantile_robust_stats(hist[:k, :T].cpu().numpy(), T, a.z0)
    got = out4[:k].cpu().numpy()
    exact = bool(np.array_equal(got[:, 0], rc, equal_nan=True) and np.array_equal(got[:, 3], rn.astype(np.float32))
                 and np.array_equal(got[:, 0], out3[:k, 0].cpu().numpy(), equal_nan=True))
    rel = lambda g, w: float(np.nanmax(np.abs(g - w) / np.maximum(np.abs(w), 1e-30)))
    sig_rel = max(rel(got[:, 1], rsl), rel(got[:, 2], rsu))

    # the band decision on 30 points a row: K24's two sigmas against one of them on both sides
    M = 4
    ctr = out4[:, 0:1].expand(-1, n).contiguous()
    sig_lo, sig_up = out4[:, 1].contiguous(), out4[:, 2].contiguous()
    cur = (ctr + (torch.randn((R, n), generator=gen, device=dev) * 2) * sig_up[:, None]).contiguous()
    thr = torch.tensor([2.0, 3.0, 2.5, 4.0], device=dev)
    bound = torch.tensor([3, 1, 3, 2], dtype=torch.int32, device=dev)
    minlb = torch.zeros(M, device=dev)

    def run_band_2s():
        SM.band_decide_2s(cur, ctr, sig_lo, sig_up, M, thr, bound, minlb)

    def run_band():
        SM.band_decide(cur, ctr, sig_up, M, thr, bound, minlb)

    variants = {"quantile": run_quantile, "robust": run_robust, "hist_stats": run_hist_stats, "band_2s": run_band_2s,
                "band": run_band}
    for f in variants.values():                                # warm every shape the timed window uses
        f()
    torch.cuda.synchronize()
    times: dict[str, list[float]] = {k_: [] for k_ in variants}
    for _ in range(a.rounds):
        for k_, f in variants.items():
            times[k_].append(_timed(f, a.iters))
    med = {k_: statistics.median(v) for k_, v in times.items()}
    hist_bytes = R * T * 4
    rec = {"bench": "quantile_robust", "device": torch.cuda.get_device_name(dev), "rows": R, "T": T, "z0": a.z0,
           "points": n, "rounds": a.rounds, "iters": a.iters,
           "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
           "history_GB": round(hist_bytes / 1e9, 3),
           "ms": {k_: round(v, 4) for k_, v in med.items()},
           "ms_min_max": {k_: [round(min(v), 4), round(max(v), 4)] for k_, v in times.items()},
           "quantile_over_robust": round(med["quantile"] / med["robust"], 3),
           "quantile_over_hist_stats": round(med["quantile"] / med["hist_stats"], 3),
           "band_2s_over_band": round(med["band_2s"] / med["band"], 3),
           "history_GBps": {k_: round(hist_bytes / (med[k_] * 1e-3) / 1e9, 1)
                            for k_ in ("quantile", "robust", "hist_stats")},
           "oracle_rows": k, "oracle_center_n_equal_and_centre_equals_robust": exact,
           "oracle_sigma_max_rel": sig_rel}
    line = json.dumps(rec)
    print(line)
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    with outp.open("a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
