"""K36 benchmark: the robust prophet fit (ops.lsq.prophet_fit_robust,
fm_lsq_robust_fit) against the plain fit (ops.lsq.prophet_fit, K10) on the same
rows, at the fleet's shape.

Inputs: clean daily-cyclic rows, the same with 1 and with 3 past incidents
(60 samples at +20 sigma) and with 5 % of the samples missing in blocks.  Per
input and per rows-a-workgroup variant (1, 2): the time of a fit at --passes
reweighting passes (default 0 2 5) and the time per pass as the least-squares
slope over them; `plain` is K10 in the same run.

One JSON line per (rows, input) on stdout, appended to --out (default
profiles/prophet_robust_bench.jsonl).  Needs a GPU: no CPU fallback.

    python -m benchmarks.bench_prophet_robust [--rows 40000] [--T 10080] [--rounds 5] [--iters 2]
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

from benchmarks.bench_hw_robust import _clean, _timed  # noqa: E402

VARIANTS = (("clean", 0, 0.0), ("1 incident", 1, 0.0), ("3 incidents", 3, 0.0), ("5% gaps", 0, 0.05))


def _variant(clean: torch.Tensor, incidents: int, gaps: float, length: int = 60, size: float = 20.0):
    R, T = clean.shape
    x = clean.clone()
    gen = torch.Generator(device=x.device).manual_seed(1 + incidents)
    t = torch.arange(T, device=x.device)[None, :]
    for _ in range(incidents):
        s = torch.randint(0, T - length, (R, 1), generator=gen, device=x.device)
        x += size * ((t >= s) & (t < s + length))
    if gaps:
        blk = int(gaps * T) // 4                                # four blocks a row
        for _ in range(4):
            s = torch.randint(1, T - blk, (R, 1), generator=gen, device=x.device)
            x.masked_fill_((t >= s) & (t < s + blk), float("nan"))
    return x


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[40000])
    ap.add_argument("--T", type=int, default=10080)
    ap.add_argument("--k", type=float, default=3.0)
    ap.add_argument("--passes", type=int, nargs="+", default=[0, 2, 5])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "prophet_robust_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_prophet_robust needs a GPU")
    from foremast_amd.ops import lsq as LQ

    dev = torch.device("cuda", 0)
    T, H = a.T, 10
    if not LQ.lsq_robust_supported(T):
        raise SystemExit(f"T={T} is outside the kernel's range")
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    clean = _clean(max(a.rows), T, 1440, dev)
    for R in a.rows:
        for name, incidents, gaps in VARIANTS:
            x = _variant(clean[:R], incidents, gaps)
            runs = {"plain": lambda: LQ.prophet_fit(x, T, H)}
            for rows in (1, 2):
                for it in a.passes:
                    runs[f"rows{rows}/iters{it}"] = (lambda rows=rows, it=it:
                                                     LQ.prophet_fit_robust(x, T, H, k=a.k, iters=it, rows=rows))
            for fn in runs.values():                           # warm every path at this shape
                fn()
            torch.cuda.synchronize()
            times: dict[str, list[float]] = {k_: [] for k_ in runs}
            for _ in range(a.rounds):
                for k_, fn in runs.items():
                    times[k_].append(_timed(fn, a.iters))
            med = {k_: statistics.median(v) for k_, v in times.items()}
            slope = {f"rows{rows}": round(float(np.polyfit(a.passes, [med[f"rows{rows}/iters{it}"] for it in a.passes],
                                                           1)[0]), 3) for rows in (1, 2)} if len(a.passes) > 1 else {}
            fit, plain = runs[f"rows1/iters{a.passes[-1]}"](), runs["plain"]()
            rec = {"bench": "prophet_robust", "device": torch.cuda.get_device_name(dev), "rows": R, "T": T, "k": a.k,
                   "variant": name, "rounds": a.rounds, "iters": a.iters,
                   "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                   "ms": {k_: round(v, 3) for k_, v in med.items()},
                   "ms_min_max": {k_: [round(min(v), 3), round(max(v), 3)] for k_, v in times.items()},
                   "ms_per_pass": slope,
                   "set_aside_mean": round((fit.nfin - fit.wsum).float().mean().item(), 2),
                   "sigma_mean": {"plain": round(plain.sigma.mean().item(), 3),
                                  "robust": round(fit.sigma.mean().item(), 3)}}
            line = json.dumps(rec)
            print(line, flush=True)
            with outp.open("a") as fh:
                fh.write(line + "\n")
            del x, fit, plain


if __name__ == "__main__":
    main()
