"""Stand-alone timing of the joint multivariate-normal kernel (K12, fm_mvn)
at the fleet shape: 10,000 groups x K = 8 rows of T = 10,080 fp32 samples,
n = 10 current points.

Timed in one process, alternating round by round, device events around
``--iters`` back-to-back launches:

  mvn_form0   fm_mvn, mean sweep + centred sweep (reads the history twice)
  mvn_form1   fm_mvn, shift from the row tails + one centred sweep
  hist_stats  fm_hist_stats over the same buffer: one streaming read of the
              history, the yardstick
  bivariate   zoo._bivariate over the same rows (pairs (0,1), (2,3), ... with
              its gathered copies)

One JSON line is printed and appended to ``--out`` (default
profiles/mvn_bench.jsonl): the median per-call milliseconds of each, the
ratios against the yardstick and the bivariate path, and the achieved read
rate of the history bytes.  Needs a GPU: there is no CPU fallback.

    python -m benchmarks.bench_mvn [--groups 10000] [--T 10080] [--rounds 5] [--iters 20]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path

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
    ap.add_argument("--groups", type=int, default=10000)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--T", type=int, default=10080)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mvn_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mvn needs a GPU")
    from foremast_amd.models import zoo
    from foremast_amd.ops import misc as MI
    from foremast_amd.ops._lib import LIB, ptr, stream_of

    dev = torch.device("cuda", 0)
    G, K, T, n = a.groups, a.K, a.T, a.n
    R, ld = G * K, (T + 3) // 4 * 4
    gen = torch.Generator(device=dev).manual_seed(0)
    hist = torch.empty((R, ld), dtype=torch.float32, device=dev)
    chunk = 8000
    scale = torch.tensor([100.0, 0.1, 1.0, 30.0, 0.01, 5.0, 1.0, 1000.0], device=dev)[:K].repeat(G)[:, None]
    for r0 in range(0, R, chunk):                              # services' metrics of different scales, 1 % missing
        blk = torch.randn((min(chunk, R - r0), ld), generator=gen, device=dev)
        blk = blk * scale[r0:r0 + chunk] + 5 * scale[r0:r0 + chunk]
        blk[torch.rand(blk.shape, generator=gen, device=dev) < 0.01] = float("nan")
        hist[r0:r0 + chunk] = blk
    cur = (torch.randn((R, n), generator=gen, device=dev) * 2 * scale + 5 * scale).contiguous()
    rows = torch.full((G, 8), -1, dtype=torch.int32)
    rows[:, :K] = torch.arange(R, dtype=torch.int32).reshape(G, K)
    rows = rows.to(dev)
    cuts = MI.mvn_cuts(3.0, 0.8)
    lowered = torch.zeros((G,), dtype=torch.uint8, device=dev)
    tables = zoo.Tables(torch.full((K,), 3.0, device=dev), torch.full((K,), 3, dtype=torch.int32, device=dev),
                        torch.zeros((K,), device=dev), 0.8, 10)
    hs = torch.empty((R, 3), dtype=torch.float32, device=dev)

    NA, NW = K + K * (K + 1) // 2, max(1, (n + 63) // 64)
    cuts_d = torch.from_numpy(cuts).to(dev)
    outs = {f: (torch.empty((G, 2 + NA), device=dev), torch.empty((G, n), device=dev),
                torch.zeros((G, NW), dtype=torch.int64, device=dev), torch.empty((G,), dtype=torch.int32, device=dev),
                torch.empty((G,), dtype=torch.int32, device=dev)) for f in (0, 1)}

    def run_mvn(form):
        params, dist, flags, cnt, valid = outs[form]

        def f():                                               # the launch alone: outputs allocated once
            LIB.call("fm_mvn", ptr(hist), hist.stride(0), T, R, ptr(cur), cur.stride(0), n, ptr(rows), G, K,
                     ptr(cuts_d), ptr(lowered), 10, form, ptr(params), ptr(dist), ptr(flags), NW, ptr(cnt),
                     ptr(valid), stream_of(hist))
            return params, dist
        return f

    variants = {
        "mvn_form0": run_mvn(0),
        "mvn_form1": run_mvn(1),
        "hist_stats": lambda: LIB.call("fm_hist_stats", ptr(hist), hist.stride(0), T, R, ptr(hs), stream_of(hist)),
        "bivariate": lambda: zoo._bivariate(hist, T, cur, K, tables),
    }
    keep = MI.MVN_FORM
    p0, d0 = variants["mvn_form0"]()
    p1, d1 = variants["mvn_form1"]()
    torch.cuda.synchronize()
    fin = torch.isfinite(d0) & torch.isfinite(d1)
    forms_dist_maxdiff = float((d0 - d1)[fin].abs().max().item())
    forms_same_nan = bool((torch.isfinite(d0) == torch.isfinite(d1)).all().item())
    for f in variants.values():                                # warm every shape the timed window uses
        f()
    torch.cuda.synchronize()
    times: dict[str, list[float]] = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, f in variants.items():
            times[k].append(_timed(f, a.iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    hist_bytes = R * T * 4
    rec = {"bench": "mvn", "device": torch.cuda.get_device_name(dev), "groups": G, "K": K, "T": T, "n": n,
           "rounds": a.rounds, "iters": a.iters, "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
           "ms": {k: round(v, 4) for k, v in med.items()},
           "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
           "mvn_form0_over_hist_stats": round(med["mvn_form0"] / med["hist_stats"], 3),
           "mvn_form1_over_hist_stats": round(med["mvn_form1"] / med["hist_stats"], 3),
           "mvn_form0_over_bivariate": round(med["mvn_form0"] / med["bivariate"], 3),
           "mvn_form1_over_bivariate": round(med["mvn_form1"] / med["bivariate"], 3),
           "history_GB": round(hist_bytes / 1e9, 3),
           "history_TBps": {k: round(hist_bytes / (med[k] * 1e-3) / 1e12, 3) for k in ("mvn_form0", "mvn_form1",
                                                                                         "hist_stats")},
           "forms_dist_maxdiff": forms_dist_maxdiff, "forms_same_nan": forms_same_nan,
           "default_form": keep}
    line = json.dumps(rec)
    print(line)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    with out.open("a") as fh:
        fh.write(line + "\n")


if __name__ == "__main__":
    main()
