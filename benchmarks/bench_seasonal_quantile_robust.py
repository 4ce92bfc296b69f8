"""Stand-alone timing of the seasonal quantile robust kernel (K26,
fm_seasonal_quantile_robust) and of the band decision with a sigma per point
and per side (fm_band_decide_pp_2s) at the headline shapes: 80,000 rows x T =
10,080 fp32 samples (3.2 GB), period 1,440 (seven days at 60 s), and 80,000
rows x 30 current points.

Timed in one process, alternating round by round, device events around
``--iters`` back-to-back launches, all on the same buffers:

  seasonal_quantile  fm_seasonal_quantile_robust: K22's stages up to the
                     floored per-phase scale, then the signed residuals over
                     that scale as keys and two tail ranks by one
                     radix_select_ranks call (one HBM read of the history)
  seasonal_scale     fm_seasonal_scale_robust (K22) on the same rows: the
                     yardstick
  hist_stats         fm_hist_stats: mean, std and finite count, one streaming
                     read of the history
  band_pp_2s         fm_band_decide_pp_2s, sigma_lo and sigma_up [R, n]
  band_pp            fm_band_decide_pp on the same points, sigma [R, n]

Rows are service metrics of different scales under a daily cycle of 60 % of
their level, times log-normal noise exp(0.3 N), with 1 % missing samples and
1 % earlier incidents at x 5: right-skewed, so both sides end on their order
statistic and no row takes the one-sided mean.  The first ``--check-rows``
rows are compared with the numpy oracle before timing.

K26 sweeps the keys about two more times than K22 (one shared first pass plus
two lower passes for each of two ranks, against one three-pass selection); the
line carries the ratio.  Both kernels take the same LDS.

One JSON line is printed and appended to ``--out`` (default
profiles/seasonal_quantile_robust_bench.jsonl): the median per-call
milliseconds of each with their min-max, and the ratios.  Needs a GPU: there
is no CPU fallback.

    python -m benchmarks.bench_seasonal_quantile_robust [--rows 80000] [--T 10080] [--period 1440] [--rounds 5] [--iters 10]
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
    ap.add_argument("--tail-z", type=float, default=2.0)
    ap.add_argument("--horizon", type=int, default=10)
    ap.add_argument("--points", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--check-rows", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "seasonal_quantile_robust_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_seasonal_quantile_robust needs a GPU")
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
    p, iz = MI.quantile_tail_params(a.tail_z)
    ld = (T + 3) // 4 * 4
    gen = torch.Generator(device=dev).manual_seed(0)
    hist = torch.empty((R, ld), dtype=torch.float32, device=dev)
    chunk = 8000
    scale = torch.tensor([1.0, 100.0, 0.1, 30.0], device=dev).repeat((R + 3) // 4)[:R, None]
    col = torch.arange(ld, device=dev, dtype=torch.float32)[None, :]
    level = 1 + 0.6 * torch.sin(col * (2 * math.pi / m))
    for r0 in range(0, R, chunk):
        sl = slice(r0, min(r0 + chunk, R))
        blk = torch.exp(0.3 * torch.randn((sl.stop - r0, ld), generator=gen, device=dev)) * level * scale[sl]
        u = torch.rand(blk.shape, generator=gen, device=dev)
        blk = torch.where(u < 0.01, blk * 5, blk)                                                   # earlier incidents
        blk[u > 0.99] = float("nan")
        hist[sl] = blk
        del blk, u
    Hn = max(H, 1)
    fc26, lo26, up26 = (torch.empty((R, Hn), dtype=torch.float32, device=dev) for _ in range(3))
    st26 = torch.empty((R, 4), dtype=torch.float32, device=dev)
    fc22 = torch.empty((R, Hn), dtype=torch.float32, device=dev)
    sh22 = torch.empty((R, Hn), dtype=torch.float32, device=dev)
    st22 = torch.empty((R, 3), dtype=torch.float32, device=dev)
    hs = torch.empty((R, 3), dtype=torch.float32, device=dev)

    def run_seasonal_quantile():
        LIB.call("fm_seasonal_quantile_robust", ptr(hist), hist.stride(0), T, R, m, J, k, w, float(a.floor), p,
                 float(iz), H, ptr(fc26), ptr(lo26), ptr(up26), Hn, ptr(st26), None, None, stream_of(hist))

    def run_seasonal_scale():
        LIB.call("fm_seasonal_scale_robust", ptr(hist), hist.stride(0), T, R, m, J, k, w, float(a.floor), H, ptr(fc22),
                 ptr(sh22), Hn, ptr(st22), None, None, stream_of(hist))

    def run_hist_stats():
        LIB.call("fm_hist_stats", ptr(hist), hist.stride(0), T, R, ptr(hs), stream_of(hist))

    # the band decisions: n current points a row, centre and sigmas of the magnitude of the rows
    M = 4
    cur = (torch.randn((R, n), generator=gen, device=dev) * 0.2 + 1) * scale
    ctr = torch.ones((R, n), device=dev) * scale
    sig_lo = (0.05 + 0.02 * torch.rand((R, n), generator=gen, device=dev)) * scale
    sig_up = (0.08 + 0.04 * torch.rand((R, n), generator=gen, device=dev)) * scale
    thr = torch.full((M,), 3.0, device=dev)
    bound = torch.full((M,), 3, dtype=torch.int32, device=dev)
    minlb = torch.zeros((M,), device=dev)

    def run_band_pp_2s():
        SM.band_decide_pp_2s(cur, ctr, sig_lo, sig_up, M, thr, bound, minlb)

    def run_band_pp():
        SM.band_decide_pp(cur, ctr, sig_up, M, thr, bound, minlb)

    variants = {"seasonal_quantile": run_seasonal_quantile, "seasonal_scale": run_seasonal_scale,
                "hist_stats": run_hist_stats, "band_pp_2s": run_band_pp_2s, "band_pp": run_band_pp}
    for f in variants.values():                                # warm every shape the timed window uses
        f()
    torch.cuda.synchronize()
    c = min(a.check_rows, R)
    ref = MI.ref_seasonal_quantile_robust(hist[:c, :T].cpu().numpy(), T, m, H, a.smooth, a.scale_smooth, a.floor,
                                          a.tail_z)
    got = st26[:c].cpu().numpy()
    exact = bool(np.array_equal(got[:, 1], ref[3].astype(np.float32))
                 and np.array_equal(fc26[:c, :H].cpu().numpy(), fc22[:c, :H].cpu().numpy(), equal_nan=True)
                 and np.array_equal(got[:, 0], st22[:c, 0].cpu().numpy(), equal_nan=True))
    rel = lambda x, y: float(np.nanmax(np.abs(x - y) / np.maximum(np.abs(y), 1e-30))) if x.size else 0.0  # noqa: E731
    times: dict[str, list[float]] = {k_: [] for k_ in variants}
    for _ in range(a.rounds):
        for k_, f in variants.items():
            times[k_].append(_timed(f, a.iters))
    med = {k_: statistics.median(v) for k_, v in times.items()}
    lds = _lds(J, m, 2 if m > 2048 else 1)
    rec = {"bench": "seasonal_quantile_robust", "device": torch.cuda.get_device_name(dev), "rows": R, "T": T,
           "period": m, "cycles": J, "halfwidth": k, "scale_halfwidth": w, "floor": a.floor, "tail_z": a.tail_z,
           "horizon": H, "points": n, "rounds": a.rounds, "iters": a.iters,
           "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
           "history_GB": round(R * T * 4 / 1e9, 3),
           "ms": {k_: round(v, 4) for k_, v in med.items()},
           "ms_min_max": {k_: [round(min(v), 4), round(max(v), 4)] for k_, v in times.items()},
           "seasonal_quantile_over_seasonal_scale": round(med["seasonal_quantile"] / med["seasonal_scale"], 3),
           "seasonal_quantile_over_hist_stats": round(med["seasonal_quantile"] / med["hist_stats"], 3),
           "band_pp_2s_over_band_pp": round(med["band_pp_2s"] / med["band_pp"], 3),
           "history_GBps": {k_: round(R * T * 4 / (med[k_] * 1e-3) / 1e9, 1)
                            for k_ in ("seasonal_quantile", "seasonal_scale", "hist_stats")},
           "lds_bytes_per_workgroup": {"seasonal_quantile": lds, "seasonal_scale": lds},
           "workgroups_per_cu_by_lds": LDS_PER_CU // lds,
           "oracle_rows": c, "oracle_n_equal_and_centre_equals_seasonal_scale": exact,
           "oracle_sigma_lo_h_max_rel": rel(lo26[:c, :H].cpu().numpy(), ref[1]),
           "oracle_sigma_up_h_max_rel": rel(up26[:c, :H].cpu().numpy(), ref[2]),
           "oracle_kappa_lo_max_rel": rel(got[:, 2], ref[5]), "oracle_kappa_up_max_rel": rel(got[:, 3], ref[6])}
    line = json.dumps(rec)
    print(line)
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    with outp.open("a") as fh:
        fh.write(line + "\n")
    if not exact:
        raise SystemExit("bench_seasonal_quantile_robust: the kernel differs from the oracle")


if __name__ == "__main__":
    main()
