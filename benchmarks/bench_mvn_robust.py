"""Stand-alone timing of the robust joint detector (K13 + K17,
fm_robust_stats + fm_mvn_robust) at the fleet shape: 10,000 groups x K = 8
rows of T = 10,080 fp32 samples (3.2 GB), n = 10 current points.

Timed in one process, alternating round by round, device events around
``--iters`` back-to-back launches, all on the same buffer:

  robust_op    fm_robust_stats over the whole buffer, then fm_mvn_robust: what
               ops/misc.py mvn_robust launches
  mvn_robust   fm_mvn_robust alone, the statistics given: one centred sweep
               about the medians (a second one for groups behind the guard)
  mvn          fm_mvn form 1 (K12): shift from the row tails + one centred sweep
  hist_stats   fm_hist_stats: one streaming read of the history, the yardstick

Rows of a group share a common factor (correlation about 0.4), have different
scales, 1 % missing samples, and three 35-sample joint incidents per group in
which members 0 and 1 are raised by 10 of their standard deviations.  The
first ``--check-groups`` groups are compared with the numpy oracle before
timing, by the bounds of tests/test_mvn_robust_ops.py.

One JSON line is printed and appended to ``--out`` (default
profiles/mvn_robust_bench.jsonl): the median per-call milliseconds of each
with their min-max, and the ratios.  Needs a GPU: there is no CPU fallback.

    python -m benchmarks.bench_mvn_robust [--groups 10000] [--T 10080] [--rounds 5] [--iters 10]
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

STRIP = 2e-3


def _timed(fn, iters: int) -> float:
    """ms per call: device events around ``iters`` launches."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def _unpack(words: np.ndarray, n: int) -> np.ndarray:
    w = np.ascontiguousarray(words).view(np.uint64)
    return np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")[:, :n].astype(bool)


def check_against_oracle(got, ref, lowered, cuts, n: int) -> dict:
    """The kernel's outputs against the oracle's by the GPU tests' bounds."""
    gp, gd, gf, gc, gv, gr = got
    rp, rd, rf, rc, rv, rr = ref
    has = rp[:, 0] > 1
    fin = np.isfinite(rd)
    used = cuts[lowered.astype(int), rp[:, 1].astype(int)][:, None]
    with np.errstate(invalid="ignore"):
        near = fin & (np.abs(rd - used) <= STRIP * used)
    gfl, rfl = _unpack(gf, n), _unpack(rf, n)
    res = {
        "n_k_rejected_valid_equal": bool(np.array_equal(gp[:, :2], rp[:, :2]) and np.array_equal(gr, rr)
                                         and np.array_equal(gv, rv)),
        "moments_close": bool(np.allclose(gp[has, 2:], rp[has, 2:], rtol=1e-4, atol=1e-5)),
        "nan_inf_pattern_equal": bool(np.array_equal(np.isnan(gd), np.isnan(rd))
                                      and np.array_equal(np.isposinf(gd), np.isposinf(rd))),
        "dist_close": bool(np.allclose(gd[fin], rd[fin], rtol=1e-3, atol=1e-3)),
        "flags_equal_outside_strip": bool(np.array_equal(gfl[~near], rfl[~near])
                                          and np.abs(gc - rc).sum() <= near.sum()),
        "in_strip": int(near.sum()), "present": int(np.isfinite(rd).sum() + np.isposinf(rd).sum()),
        "rejected_mean": float(rr.mean()), "fell_back": int(((rr == 0) & (rp[:, 0] > 0)).sum()),
    }
    res["ok"] = all(v for v in res.values() if isinstance(v, bool))
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--groups", type=int, default=10000)
    ap.add_argument("--K", type=int, default=8)
    ap.add_argument("--T", type=int, default=10080)
    ap.add_argument("--n", type=int, default=10)
    ap.add_argument("--reject", type=float, default=3.5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--check-groups", type=int, default=256)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "mvn_robust_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mvn_robust needs a GPU")
    from foremast_amd.ops import misc as MI
    from foremast_amd.ops._lib import LIB, ptr, stream_of

    dev = torch.device("cuda", 0)
    G, K, T, n = a.groups, a.K, a.T, a.n
    R, ld = G * K, (T + 3) // 4 * 4
    gen = torch.Generator(device=dev).manual_seed(0)
    hist = torch.empty((R, ld), dtype=torch.float32, device=dev)
    scale = torch.tensor([100.0, 0.1, 1.0, 30.0, 0.01, 5.0, 1.0, 1000.0], device=dev)[:K]
    cols = torch.arange(ld, device=dev)[None, None, :]
    chunk = 1000                                               # groups per block of the generator
    for g0 in range(0, G, chunk):
        gs = min(chunk, G - g0)
        z = torch.randn((gs, K, ld), generator=gen, device=dev)
        common = torch.randn((gs, 1, ld), generator=gen, device=dev)
        blk = 0.6 * common + 0.8 * z                           # unit variance, correlation 0.36
        starts = torch.randint(0, T - 35, (gs, 3), generator=gen, device=dev)
        inc = torch.zeros((gs, 1, ld), dtype=torch.bool, device=dev)
        for i in range(3):
            t0 = starts[:, i, None, None]
            inc |= (cols >= t0) & (cols < t0 + 35)
        blk[:, :2] += 10.0 * inc                               # the joint incidents, on members 0 and 1
        blk = blk * scale[None, :, None] + 5 * scale[None, :, None]
        blk[torch.rand(blk.shape, generator=gen, device=dev) < 0.01] = float("nan")
        hist[g0 * K:(g0 + gs) * K] = blk.reshape(gs * K, ld)
        del z, common, blk, inc
    sc = scale.repeat(G)[:, None]
    cur = (torch.randn((R, n), generator=gen, device=dev) * 2 * sc + 5 * sc).contiguous()
    rows = torch.full((G, 8), -1, dtype=torch.int32)
    rows[:, :K] = torch.arange(R, dtype=torch.int32).reshape(G, K)
    rows = rows.to(dev)
    cuts = MI.mvn_cuts(3.0, 0.8)
    cuts_d = torch.from_numpy(cuts).to(dev)
    lowered = torch.zeros((G,), dtype=torch.uint8, device=dev)
    NA, NW = K + K * (K + 1) // 2, max(1, (n + 63) // 64)
    mk = lambda: (torch.empty((G, 2 + NA), device=dev), torch.empty((G, n), device=dev),
                  torch.zeros((G, NW), dtype=torch.int64, device=dev), torch.empty((G,), dtype=torch.int32, device=dev),
                  torch.empty((G,), dtype=torch.int32, device=dev))
    o17, o12 = mk(), mk()
    rejected = torch.zeros((G,), dtype=torch.int32, device=dev)
    stats = torch.empty((R, 3), dtype=torch.float32, device=dev)
    hs = torch.empty((R, 3), dtype=torch.float32, device=dev)

    def run_stats():
        LIB.call("fm_robust_stats", ptr(hist), hist.stride(0), T, R, ptr(stats), stream_of(hist))

    def run_k17():                                             # the launch alone: outputs allocated once
        p, d, f, c, v = o17
        LIB.call("fm_mvn_robust", ptr(hist), hist.stride(0), T, R, ptr(cur), cur.stride(0), n, ptr(rows), G, K,
                 ptr(cuts_d), ptr(lowered), 10, ptr(stats), float(a.reject), ptr(p), ptr(d), ptr(f), NW, ptr(c),
                 ptr(v), ptr(rejected), stream_of(hist))

    def run_op():
        run_stats()
        run_k17()

    def run_k12():
        p, d, f, c, v = o12
        LIB.call("fm_mvn", ptr(hist), hist.stride(0), T, R, ptr(cur), cur.stride(0), n, ptr(rows), G, K, ptr(cuts_d),
                 ptr(lowered), 10, 1, ptr(p), ptr(d), ptr(f), NW, ptr(c), ptr(v), stream_of(hist))

    def run_hist_stats():
        LIB.call("fm_hist_stats", ptr(hist), hist.stride(0), T, R, ptr(hs), stream_of(hist))

    variants = {"robust_op": run_op, "mvn_robust": run_k17, "mvn": run_k12, "hist_stats": run_hist_stats}
    for f in variants.values():                                # warm every shape the timed window uses
        f()
    torch.cuda.synchronize()
    kg = min(a.check_groups, G)
    ref = MI.ref_mvn_robust(hist[:kg * K, :T].cpu().numpy(), cur[:kg * K].cpu().numpy(), rows[:kg].cpu().numpy(), K,
                            cuts, np.zeros(kg, np.uint8), 10, a.reject)
    got = tuple(t[:kg].cpu().numpy() for t in o17) + (rejected[:kg].cpu().numpy(),)
    chk = check_against_oracle(got, ref, np.zeros(kg, np.uint8), cuts, n)
    times: dict[str, list[float]] = {k_: [] for k_ in variants}
    for _ in range(a.rounds):
        for k_, f in variants.items():
            times[k_].append(_timed(f, a.iters))
    med = {k_: statistics.median(v) for k_, v in times.items()}
    rec = {"bench": "mvn_robust", "device": torch.cuda.get_device_name(dev), "groups": G, "K": K, "T": T, "n": n,
           "reject": a.reject, "rounds": a.rounds, "iters": a.iters,
           "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "history_GB": round(R * T * 4 / 1e9, 3),
           "ms": {k_: round(v, 4) for k_, v in med.items()},
           "ms_min_max": {k_: [round(min(v), 4), round(max(v), 4)] for k_, v in times.items()},
           "robust_op_over_mvn": round(med["robust_op"] / med["mvn"], 3),
           "mvn_robust_over_mvn": round(med["mvn_robust"] / med["mvn"], 3),
           "mvn_robust_over_hist_stats": round(med["mvn_robust"] / med["hist_stats"], 3),
           "history_TBps": {k_: round(R * T * 4 / (med[k_] * 1e-3) / 1e12, 3) for k_ in ("mvn_robust", "mvn",
                                                                                         "hist_stats")},
           "rejected_mean_all": float(rejected.float().mean().item()),
           "groups_fell_back": int(((rejected == 0) & (o17[0][:, 0] > 0)).sum().item()),
           "oracle_groups": kg, "oracle": chk}
    line = json.dumps(rec)
    print(line)
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    with outp.open("a") as fh:
        fh.write(line + "\n")
    if not chk["ok"]:
        raise SystemExit("bench_mvn_robust: the kernel differs from the oracle")


if __name__ == "__main__":
    main()
