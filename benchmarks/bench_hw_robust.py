"""Stand-alone timing of the Huber-clipped Holt-Winters scan fit (K35,
fm_hw_robust_fit) against the plain scan fit (fm_hw_scan_fit) on the same
tensor.

Shapes: the config-2 grid fit, 40,000 rows x T = 10,080 at m = 1440 with the
default 27 candidates, and 10,000 rows, in one process.  Rows are daily-cyclic
metrics with N(0, 1) noise carrying, per variant, 0, 1 or 3 past incidents of
30 steps (+40 sigma, at a random place after the second season) or a permanent
level shift of +40 sigma in the second half.  Per shape and variant,
alternating round by round, device events around ``--iters`` back-to-back
calls:

  scan        es_fit(method="scan", prune=0): the yardstick
  robust      es_fit_robust with the thresholds given (the fit alone)
  robust+clip es_fit_robust computing its thresholds (hw_robust_clip: the
              seasonal differences in torch + K13)

and one extra robust fit with the attempt counters on
(fm_hw_robust_set_probe): the mean attempts per season lap over all (row,
candidate pair)s, and the largest.

One JSON line per (shape, variant) is printed and appended to ``--out``
(default profiles/hw_robust_bench.jsonl).  Needs a GPU: no CPU fallback.

    python -m benchmarks.bench_hw_robust [--rows 40000 10000] [--T 10080] [--m 1440] [--rounds 5] [--iters 2]
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

VARIANTS = (("clean", 0, False), ("1 incident", 1, False), ("3 incidents", 3, False), ("level shift", 0, True))


def _timed(fn, iters: int) -> float:
    """ms per call: device events around ``iters`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _clean(R: int, T: int, m: int, dev) -> torch.Tensor:
    gen = torch.Generator(device=dev).manual_seed(0)
    t = torch.arange(T, device=dev, dtype=torch.float32)
    x = torch.empty((R, T), dtype=torch.float32, device=dev)
    for r0 in range(0, R, 8000):
        n = min(8000, R - r0)
        x[r0:r0 + n] = 100 + 20 * torch.sin(2 * torch.pi * t / m)[None, :] + torch.randn((n, T), generator=gen,
                                                                                          device=dev)
    return x


def _variant(clean: torch.Tensor, m: int, incidents: int, shift: bool, length: int = 30, size: float = 40.0):
    R, T = clean.shape
    x = clean.clone()
    gen = torch.Generator(device=x.device).manual_seed(1 + incidents + 10 * shift)
    t = torch.arange(T, device=x.device)[None, :]
    for _ in range(incidents):
        s = torch.randint(2 * m, T - length, (R, 1), generator=gen, device=x.device)
        x += size * ((t >= s) & (t < s + length))
    if shift:
        s = torch.randint(T // 2, T - m, (R, 1), generator=gen, device=x.device)
        x += size * (t >= s)
    return x


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[40000, 10000])
    ap.add_argument("--T", type=int, default=10080)
    ap.add_argument("--m", type=int, default=1440)
    ap.add_argument("--k", type=float, default=3.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=2)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "hw_robust_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hw_robust needs a GPU")
    from foremast_amd.ops import smoothing as SM
    from foremast_amd.ops._lib import LIB

    dev = torch.device("cuda", 0)
    T, m, H = a.T, a.m, 10
    G = SM.default_grid(2).shape[0]
    if not (SM.hw_robust_supported(T, G, m) and SM.hw_scan_supported(T, G, m)):
        raise SystemExit(f"T={T}, m={m} is outside the kernels' range")
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    clean = _clean(max(a.rows), T, m, dev)
    for R in a.rows:
        for name, incidents, shift in VARIANTS:
            x = _variant(clean[:R], m, incidents, shift)
            clip = SM.hw_robust_clip(x, T, m, a.k)
            runs = {"scan": lambda: SM.es_fit(x, T, 2, H, m, method="scan", prune=0.0),
                    "robust": lambda: SM.es_fit_robust(x, T, H, m, clip=clip),
                    "robust+clip": lambda: SM.es_fit_robust(x, T, H, m, k=a.k)}
            for fn in runs.values():                           # warm every path at this shape
                fn()
            probe = torch.zeros((R, 16, 2), dtype=torch.int32, device=dev)
            LIB.call("fm_hw_robust_set_probe", probe.data_ptr())
            try:
                fit = runs["robust"]()
                torch.cuda.synchronize()
            finally:
                LIB.call("fm_hw_robust_set_probe", None)
            att, laps = probe[:, :, 0].sum().item(), probe[:, :, 1].sum().item()
            per_pair = probe[:, :, 0].float() / probe[:, :, 1].clamp(min=1).float()
            plain = runs["scan"]()
            times: dict[str, list[float]] = {k_: [] for k_ in runs}
            for _ in range(a.rounds):
                for k_, fn in runs.items():
                    times[k_].append(_timed(fn, a.iters))
            med = {k_: statistics.median(v) for k_, v in times.items()}
            best = fit.best.long()[:, None]
            rec = {"bench": "hw_robust", "device": torch.cuda.get_device_name(dev), "rows": R, "T": T, "m": m, "G": G,
                   "k": a.k, "variant": name, "rounds": a.rounds, "iters": a.iters,
                   "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
                   "ms": {k_: round(v, 3) for k_, v in med.items()},
                   "ms_min_max": {k_: [round(min(v), 3), round(max(v), 3)] for k_, v in times.items()},
                   "robust_over_scan": round(med["robust"] / med["scan"], 2),
                   "clip_ms": round(med["robust+clip"] - med["robust"], 3),
                   "attempts_per_lap": round(att / max(laps, 1), 3),
                   "attempts_per_lap_max_pair": round(per_pair.max().item(), 2),
                   "winner_nclip_mean": round(fit.nclip.gather(1, best).float().mean().item(), 1),
                   "sigma_mean": {"scan": round(plain.sigma.mean().item(), 3),
                                  "robust": round(fit.sigma.mean().item(), 3)}}
            line = json.dumps(rec)
            print(line, flush=True)
            with outp.open("a") as fh:
                fh.write(line + "\n")
            del x, clip, probe, fit, plain


if __name__ == "__main__":
    main()
