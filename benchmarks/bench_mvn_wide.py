"""Stand-alone timing of the joint detector's wide tier (K37, fm_mvn_wide) at
T = 10,080 fp32 samples, n = 10 current points, over three fleets of about
80,000 member rows: 5,000 groups x K = 16, 2,500 x K = 32, 6,667 x K = 12.

Timed in one process, alternating round by round, device events around
``--iters`` back-to-back launches:

  wide         fm_mvn_wide, every group whole
  wide_robust  fm_mvn_wide_robust (the statistics of fm_robust_stats made once,
               outside the timed window): the counting sweep's cost is its
               difference to ``wide``
  wide_flush2, wide_flush32
               fm_mvn_wide with the fp32 tile flushed to fp64 every 2 / 32
               tiles instead of every 8
  chunks8      the same rows through fm_mvn in chunks of 8 (K12: the same bytes
               for a different, weaker answer)
  hist_stats   fm_hist_stats over the same buffer: one streaming read

One JSON line per shape is printed and appended to ``--out`` (default
profiles/mvn_wide_bench.jsonl): median and [min, max] milliseconds per call,
the ratios, and the two floors computed from the shape: the MFMA floor (T / 2
instructions of 16 passes x 4 cycles per group, over the SIMDs at ``--mhz``)
and the byte floor (the members' history over ``--tbps``).  Needs a GPU: there
is no CPU fallback.

    python -m benchmarks.bench_mvn_wide [--T 10080] [--rounds 5] [--iters 10]
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

SHAPES = ((5000, 16), (2500, 32), (6667, 12))


def _timed(fn, iters: int) -> float:
    """ms per call: device events around ``iters`` launches."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _shape(G: int, K: int, T: int, n: int, a, dev) -> dict:
    from foremast_amd.ops import misc as MI
    from foremast_amd.ops._lib import LIB, ptr, stream_of

    R, ld = G * K, (T + 3) // 4 * 4
    gen = torch.Generator(device=dev).manual_seed(0)
    hist = torch.empty((R, ld), dtype=torch.float32, device=dev)
    scale = torch.tensor([10.0, 0.1, 1.0, 3.0, 0.01, 5.0, 1.0, 0.3], device=dev).repeat((R + 7) // 8)[:R, None]
    for r0 in range(0, R, 8000):                               # metrics of different scales, 0.1 % missing
        blk = torch.randn((min(8000, R - r0), ld), generator=gen, device=dev)
        blk = blk * scale[r0:r0 + 8000] + 5 * scale[r0:r0 + 8000]
        blk[torch.rand(blk.shape, generator=gen, device=dev) < 0.001] = float("nan")
        hist[r0:r0 + 8000] = blk
    cur = (torch.randn((R, n), generator=gen, device=dev) * 2 * scale + 5 * scale).contiguous()
    ids = torch.arange(R, dtype=torch.int32).reshape(G, K)
    rows = torch.full((G, 32), -1, dtype=torch.int32)
    rows[:, :K] = ids
    rows = rows.to(dev)
    chunks = []                                                # (rows [g, 8], k) of the narrow tier
    for c0 in range(0, K, 8):
        k = min(8, K - c0)
        r8 = torch.full((G, 8), -1, dtype=torch.int32)
        r8[:, :k] = ids[:, c0:c0 + k]
        chunks.append((r8.to(dev), k))
    wcuts = torch.from_numpy(MI.mvn_cuts(3.0, 0.8, 32)).to(dev)
    ncuts = torch.from_numpy(MI.mvn_cuts(3.0, 0.8)).to(dev)
    lowered = torch.zeros((G,), dtype=torch.uint8, device=dev)
    NW = max(1, (n + 63) // 64)

    def outs(k):
        return (torch.empty((G, 2 + k + k * (k + 1) // 2), device=dev), torch.empty((G, n), device=dev),
                torch.zeros((G, NW), dtype=torch.int64, device=dev), torch.empty((G,), dtype=torch.int32, device=dev),
                torch.empty((G,), dtype=torch.int32, device=dev))

    wo, co = outs(K), [outs(k) for _, k in chunks]
    rejected = torch.empty((G,), dtype=torch.int32, device=dev)
    stats = torch.empty((R, 3), dtype=torch.float32, device=dev)
    LIB.call("fm_robust_stats", ptr(hist), hist.stride(0), T, R, ptr(stats), stream_of(hist))
    hs = torch.empty((R, 3), dtype=torch.float32, device=dev)
    head = (ptr(hist), hist.stride(0), T, R, ptr(cur), cur.stride(0), n)
    tail = (ptr(wo[0]), ptr(wo[1]), ptr(wo[2]), NW, ptr(wo[3]), ptr(wo[4]))

    def wide(flush=None):
        if flush is None:
            return lambda: LIB.call("fm_mvn_wide", *head, ptr(rows), G, K, ptr(wcuts), ptr(lowered), 10, *tail,
                                    stream_of(hist))
        return lambda: LIB.call("fm_mvn_wide_flush", *head, ptr(rows), G, K, ptr(wcuts), ptr(lowered), 10, flush,
                                *tail, stream_of(hist))

    def chunks8():
        for (r8, k), o in zip(chunks, co):
            LIB.call("fm_mvn", *head, ptr(r8), G, k, ptr(ncuts), ptr(lowered), 10, MI.MVN_FORM, ptr(o[0]), ptr(o[1]),
                     ptr(o[2]), NW, ptr(o[3]), ptr(o[4]), stream_of(hist))

    variants = {
        "wide": wide(),
        "wide_robust": lambda: LIB.call("fm_mvn_wide_robust", *head, ptr(rows), G, K, ptr(wcuts), ptr(lowered), 10,
                                        ptr(stats), MI.MVN_REJECT, *tail, ptr(rejected), stream_of(hist)),
        "wide_flush2": wide(2),
        "wide_flush32": wide(32),
        "chunks8": chunks8,
        "hist_stats": lambda: LIB.call("fm_hist_stats", ptr(hist), hist.stride(0), T, R, ptr(hs), stream_of(hist)),
    }
    dists = {}
    for k in ("wide_flush2", "wide_flush32", "wide"):          # the distances of the three intervals
        variants[k]()
        dists[k] = wo[1].clone()
    flush_maxdiff = max(float(torch.nan_to_num(dists[k] - dists["wide"]).abs().max().item())
                        for k in ("wide_flush2", "wide_flush32"))
    for f in variants.values():                                # warm every shape the timed window uses
        f()
    torch.cuda.synchronize()
    times: dict[str, list[float]] = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, f in variants.items():
            times[k].append(_timed(f, a.iters))
    med = {k: statistics.median(v) for k, v in times.items()}
    simds = torch.cuda.get_device_properties(dev).multi_processor_count * 4
    mfma_floor = G * (T / 2) * 64 / simds / (a.mhz * 1e3)      # ms
    byte_floor = R * T * 4 / (a.tbps * 1e12) * 1e3             # ms
    return {"bench": "mvn_wide", "device": torch.cuda.get_device_name(dev), "groups": G, "K": K, "T": T, "n": n,
            "rounds": a.rounds, "iters": a.iters, "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()),
            "ms": {k: round(v, 4) for k, v in med.items()},
            "ms_min_max": {k: [round(min(v), 4), round(max(v), 4)] for k, v in times.items()},
            "wide_over_chunks8": round(med["wide"] / med["chunks8"], 3),
            "wide_over_hist_stats": round(med["wide"] / med["hist_stats"], 3),
            "counting_sweep_ms": round(med["wide_robust"] - med["wide"], 4),
            "flush_dist_maxdiff": flush_maxdiff,
            "simds": simds, "mhz": a.mhz, "tbps": a.tbps,
            "mfma_floor_ms": round(mfma_floor, 4), "byte_floor_ms": round(byte_floor, 4),
            "wide_over_mfma_floor": round(med["wide"] / mfma_floor, 3),
            "wide_over_byte_floor": round(med["wide"] / byte_floor, 3),
            "history_GB": round(R * T * 4 / 1e9, 3)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=10080)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--mhz", type=float, default=2400.0, help="engine clock of the MFMA floor")
    ap.add_argument("--tbps", type=float, default=8.0, help="memory bandwidth of the byte floor")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mvn_wide_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mvn_wide needs a GPU")
    dev = torch.device("cuda", 0)
    out = Path(a.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    for G, K in SHAPES:
        line = json.dumps(_shape(G, K, a.T, a.n, a, dev))
        print(line, flush=True)
        with out.open("a") as fh:
            fh.write(line + "\n")
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
