"""Stand-alone timing of the seasonal scale robust kernel (K22,
fm_seasonal_scale_robust) and of the band decision with a sigma per point
(fm_band_decide_pp) at the headline shapes: 80,000 rows x T = 10,080 fp32
samples (3.2 GB), period 1,440 (seven days at 60 s), and 80,000 rows x 30
current points.

Timed in one process, alternating round by round, device events around
``--iters`` back-to-back launches, all on the same buffers:

  seasonal_scale  fm_seasonal_scale_robust: K14's profile, smoothing, forecast
                  and MAD-sigma, then the per-phase middle of the residuals by
                  a second sorting pass, its smoothing and floor, the residuals
                  over that scale and a second selection for kappa (one HBM
                  read of the history)
  seasonal        fm_seasonal_robust (K14) on the same rows
  hist_stats      fm_hist_stats: mean, std and finite count, one streaming
                  read of the history
  band_pp         fm_band_decide_pp, sigma [R, n]
  band            fm_band_decide on the same points, sigma [R]

Rows are service metrics of different scales under a daily cycle of 80 % of
their level, with noise of 5 % of the current level, 1 % missing samples and
5 % earlier incidents.  The first ``--check-rows`` rows are compared with the
numpy oracle before timing.

The line also carries the LDS bytes of a workgroup of each seasonal kernel
and how many of them the 160 KiB of a CU hold by bytes: LDS is what bounds
their occupancy (a 512-thread workgroup is two waves a SIMD, and both kernels
stay under the 85 VGPRs that six waves a SIMD leave each).  No occupancy
counter is read; docs/PERF.md compares two spans on either side of the edge.

One JSON line is printed and appended to ``--out`` (default
profiles/seasonal_scale_robust_bench.jsonl): the median per-call milliseconds
of each with their min-max, and the ratios.  Needs a GPU: there is no CPU
fallback.

    python -m benchmarks.bench_seasonal_scale_robust [--rows 80000] [--T 10080] [--period 1440] [--rounds 5] [--iters 10]
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

SCRATCH_BYTES = 8336           # SelectScratch<512>: bins, selection state, reduction scratch
LDS_PER_CU = 160 * 1024        # CDNA4


def _timed(fn, iters: int) -> float:
    """ms per call: device events around ``iters`` launches."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _lds(J: int, m: int, buffers_behind: int) -> int:
    """LDS bytes of a workgroup: the keys of the span, the m-word buffers
    behind them, and the static scratch."""
    return (J * m + 6) // 4 * 16 + buffers_behind * m * 4 + SCRATCH_BYTES


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--T", type=int, default=10080)
    ap.add_argument("--period", type=int, default=1440)
    ap.add_argument("--smooth", type=int, default=5)
    ap.add_argument("--scale-smooth", type=int, default=30)
    ap.add_argument("--floor", type=float, default=0.1)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--points", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--check-rows", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "seasonal_scale_robust_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seasonal_scale_robust needs a GPU")
    from foremast_amd.ops import misc as MI
    from foremast_amd.ops import smoothing as SM
    from foremast_amd.ops._lib import LIB, ptr, stream_of

    dev = torch.device("cuda", 0)
    R, T, m, H, n = a.rows, a.T, a.period, a.horizon, a.points
    J = MI.seasonal_cycles(T, m)
    if J < 2:
        raise SystemExit(f"T = {T}, period = {m}: the history must hold two cycles within the LDS budget")
    k = MI.seasonal_halfwidth(m, a.smooth)
    w = MI.scale_halfwidth(m, a.scale_smooth)
    ld = (T + 3) // 4 * 4
    gen = torch.Generator(device=dev).manual_seed(0)
    hist = torch.empty((R, ld), dtype=torch.float32, device=dev)
    chunk = 8000
    scale = torch.tensor([1.0, 100.0, 0.1, 30.0], device=dev).repeat((R + 3) // 4)[:R, None]
    col = torch.arange(ld, device=dev, dtype=torch.float32)[None, :]
    level = 1 + 0.8 * torch.sin(col * (2 * math.pi / m))
    for r0 in range(0, R, chunk):
        sl = slice(r0, min(r0 + chunk, R))
        blk = (1 + 0.05 * torch.randn((sl.stop - r0, ld), generator=gen, device=dev)) * level * scale[sl]
        u = torch.rand(blk.shape, generator=gen, device=dev)
        blk = torch.where(u < 0.05, blk * 3, blk)                                                   # earlier incidents
        blk[u > 0.99] = float("nan")
        hist[sl] = blk
        del blk, u
    Hn = max(H, 1)
    fc22 = torch.empty((R, Hn), dtype=torch.float32, device=dev)
    sh22 = torch.empty((R, Hn), dtype=torch.float32, device=dev)
    st22 = torch.empty((R, 3), dtype=torch.float32, device=dev)
    fc14 = torch.empty((R, Hn), dtype=torch.float32, device=dev)
    st14 = torch.empty((R, 2), dtype=torch.float32, device=dev)
    hs = torch.empty((R, 3), dtype=torch.float32, device=dev)

    def run_seasonal_scale():
        LIB.call("fm_seasonal_scale_robust", ptr(hist), hist.stride(0), T, R, m, J, k, w, float(a.floor), H, ptr(fc22),
                 ptr(sh22), Hn, ptr(st22), None, None, stream_of(hist))

    def run_seasonal():
        LIB.call("fm_seasonal_robust", ptr(hist), hist.stride(0), T, R, m, J, k, H, ptr(fc14), Hn, ptr(st14), None,
                 stream_of(hist))

    def run_hist_stats():
        LIB.call("fm_hist_stats", ptr(hist), hist.stride(0), T, R, ptr(hs), stream_of(hist))

    # the band decisions: n current points a row, centre and sigma of the magnitude of the rows
    M = 4
    cur = (torch.randn((R, n), generator=gen, device=dev) * 0.2 + 1) * scale
    ctr = torch.ones((R, n), device=dev) * scale
    sig_pp = (0.05 + 0.02 * torch.rand((R, n), generator=gen, device=dev)) * scale
    sig = sig_pp[:, 0].contiguous()
    thr = torch.full((M,), 3.0, device=dev)
    bound = torch.full((M,), 3, dtype=torch.int32, device=dev)
    minlb = torch.zeros((M,), device=dev)

    def run_band_pp():
        SM.band_decide_pp(cur, ctr, sig_pp, M, thr, bound, minlb)

    def run_band():
        SM.band_decide(cur, ctr, sig, M, thr, bound, minlb)

    variants = {"seasonal_scale": run_seasonal_scale, "seasonal": run_seasonal, "hist_stats": run_hist_stats,
                "band_pp": run_band_pp, "band": run_band}
    for f in variants.values():                                # warm every shape the timed window uses
        f()
    torch.cuda.synchronize()
    c = min(a.check_rows, R)
    ref = MI.ref_seasonal_scale_robust(hist[:c, :T].cpu().numpy(), T, m, H, a.smooth, a.scale_smooth, a.floor)
    got = st22[:c].cpu().numpy()
    exact = bool(np.array_equal(got[:, 1], ref[2].astype(np.float32))
                 and np.array_equal(fc22[:c, :H].cpu().numpy(), fc14[:c, :H].cpu().numpy(), equal_nan=True)
                 and np.array_equal(got[:, 0], st14[:c, 0].cpu().numpy(), equal_nan=True))
    rel = lambda x, y: float(np.nanmax(np.abs(x - y) / np.maximum(np.abs(y), 1e-30))) if x.size else 0.0  # noqa: E731
    times: dict[str, list[float]] = {k_: [] for k_ in variants}
    for _ in range(a.rounds):
        for k_, f in variants.items():
            times[k_].append(_timed(f, a.iters))
    med = {k_: statistics.median(v) for k_, v in times.items()}
    lds22, lds14 = _lds(J, m, 2 if m > 2048 else 1), _lds(J, m, 1 if m > 2048 else 0)
    rec = {"bench": "seasonal_scale_robust", "device": torch.cuda.get_device_name(dev), "rows": R, "T": T, "period": m,
           "cycles": J, "halfwidth": k, "scale_halfwidth": w, "floor": a.floor, "horizon": H, "points": n,
           "rounds": a.rounds, "iters": a.iters, "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
           "history_GB": round(R * T * 4 / 1e9, 3),
           "ms": {k_: round(v, 4) for k_, v in med.items()},
           "ms_min_max": {k_: [round(min(v), 4), round(max(v), 4)] for k_, v in times.items()},
           "seasonal_scale_over_seasonal": round(med["seasonal_scale"] / med["seasonal"], 3),
           "seasonal_scale_over_hist_stats": round(med["seasonal_scale"] / med["hist_stats"], 3),
           "band_pp_over_band": round(med["band_pp"] / med["band"], 3),
           "history_GBps": {k_: round(R * T * 4 / (med[k_] * 1e-3) / 1e9, 1)
                            for k_ in ("seasonal_scale", "seasonal", "hist_stats")},
           "lds_bytes_per_workgroup": {"seasonal_scale": lds22, "seasonal": lds14},
           "workgroups_per_cu_by_lds": {"seasonal_scale": LDS_PER_CU // lds22, "seasonal": LDS_PER_CU // lds14},
           "oracle_rows": c, "oracle_n_equal_and_centre_equals_seasonal": exact,
           "oracle_sigma_h_max_rel": rel(sh22[:c, :H].cpu().numpy(), ref[1]),
           "oracle_kappa_max_rel": rel(got[:, 2], ref[4])}
    line = json.dumps(rec)
    print(line)
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    with outp.open("a") as fh:
        fh.write(line + "\n")
    if not exact:
        raise SystemExit("bench_seasonal_scale_robust: the kernel differs from the oracle")


if __name__ == "__main__":
    main()
