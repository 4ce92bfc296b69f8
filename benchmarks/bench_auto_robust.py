"""Stand-alone timing of ``auto_robust`` at the headline shape: 80,000 rows x
T = 10,080 fp32 samples (3.2 GB), period = hold-out = 1,440 (seven days at
60 s, one day held out).  The fleet is six equal parts, one per row shape the
six candidates exist for (row r has shape r % 6: flat, level shift, drift,
daily cycle, daily cycle with noise that grows with the level, drift plus
daily cycle), with 0.5 % missing samples.

Three comparisons, each timed in one process, alternating round by round,
device events around ``--iters`` back-to-back calls on the same buffers:

  holdout_score   K23 (fm_holdout_score through MI.holdout_score) over the six
                  candidates' forecasts and sigmas: 6 streams of R x L floats
  hist_stats      fm_hist_stats over 6 L columns of the same rows: the same
                  number of bytes, the project's streaming yardstick

  auto_select     zoo.auto_select: the six fits on columns [0, T - L) and K23
  fit:<model>     each candidate's fit alone, as auto_select calls it

  decide_auto     zoo.decide("auto_robust") with every row's choice remembered
                  (an AutoChoices memory, looked up per call): one fit per
                  model over the rows that chose it, then the band decision
  decide_seasonal zoo.decide("seasonal_robust") on the same rows

The first ``--check-rows`` rows of K23's outputs are compared with the numpy
contract before timing.  One JSON line is printed and appended to ``--out``
(default profiles/auto_robust_bench.jsonl): median milliseconds per call with
their min-max, and the ratios.  Needs a GPU: there is no CPU fallback.

    python -m benchmarks.bench_auto_robust [--rows 80000] [--T 10080] [--period 1440] [--rounds 5] [--iters 3]
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


def _timed(fn, iters: int) -> float:
    """ms per call: device events around ``iters`` calls."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def make_fleet(R: int, T: int, m: int, dev, seed: int = 0) -> torch.Tensor:
    """[R, ld] histories, row r of shape r % 6 (ld = T rounded up to 4)."""
    ld = (T + 3) // 4 * 4
    gen = torch.Generator(device=dev).manual_seed(seed)
    hist = torch.empty((R, ld), dtype=torch.float32, device=dev)
    t = torch.arange(ld, device=dev, dtype=torch.float32)[None, :]
    w = torch.sin(t * (2 * math.pi / m))
    step = (t >= 3 * m + m // 3).float()
    shape = torch.arange(R, device=dev) % 6
    pick = lambda *v: torch.tensor(v, device=dev)[shape][:, None]    # noqa: E731
    a_w, a_t, a_s = pick(0., 0., 0., 40., 80., 40.), pick(0., 0., 10. / m, 0., 0., 10. / m), pick(0., 40., 0., 0., 0., 0.)
    rel = pick(0., 0., 0., 0., 0.08, 0.)
    for r0 in range(0, R, 8000):
        sl = slice(r0, min(r0 + 8000, R))
        lvl = 100 + a_w[sl] * w + a_t[sl] * t + a_s[sl] * step
        e = torch.randn((sl.stop - r0, ld), generator=gen, device=dev)
        blk = lvl + torch.where(rel[sl] > 0, rel[sl] * lvl, torch.full_like(lvl, 2.0)) * e
        blk[torch.rand(blk.shape, generator=gen, device=dev) > 0.995] = float("nan")
        hist[sl] = blk
        del lvl, e, blk
    return hist


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--T", type=int, default=10080)
    ap.add_argument("--period", type=int, default=1440)
    ap.add_argument("--points", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--check-rows", type=int, default=240)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "auto_robust_bench.jsonl"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_auto_robust needs a GPU")
    from foremast_amd.models import zoo
    from foremast_amd.models.cache import AutoChoices
    from foremast_amd.ops import misc as MI
    from foremast_amd.ops._lib import LIB, ptr, stream_of

    dev = torch.device("cuda", 0)
    R, T, m, n = a.rows, a.T, a.period, a.points
    L = m
    if T < 2 * L or MI.seasonal_cycles(T - L, m) < 2:
        raise SystemExit(f"T = {T}, period = {m}: the fitted part must hold two cycles")
    hist = make_fleet(R, T, m, dev)
    names = zoo.AUTO_CANDIDATES
    par = (5, m, 4.0, 2, 3, 30, 0.1)             # smooth, block, shift threshold, min blocks, trend min blocks, scale smooth, floor
    kw = dict(period=m, holdout=L, block=m)

    fits = {nm: (lambda ci=ci: zoo._auto_fit(ci, hist, T - L, L, m, *par)) for ci, nm in enumerate(names)}
    got = [f() for f in fits.values()]
    fcs, sigmas = [g[0] for g in got], [g[1] for g in got]
    held = hist[:, T - L:T]
    wide = [t for t in fcs + sigmas if t.dim() == 2 and t.shape[1] > 1 and t.stride(1) == 1]
    streams = 1 + len(wide)
    k23_bytes = 4 * R * L * streams
    hs_cols = min(streams * L, hist.shape[1]) // 4 * 4
    hs = torch.empty((R, 3), dtype=torch.float32, device=dev)

    def run_k23():
        return MI.holdout_score(held, fcs, sigmas)

    def run_hist_stats():
        LIB.call("fm_hist_stats", ptr(hist), hist.stride(0), hs_cols, R, ptr(hs), stream_of(hist))

    def run_select():
        return zoo.auto_select(hist, T, **kw)

    # the decisions: n current points a row (the last n samples again), four metric types
    M = 4
    cur = hist[:, T - n:T].contiguous()
    hor = torch.arange(1, n + 1, device=dev).repeat(R, 1)
    tables = zoo.Tables(torch.full((M,), 3.0, device=dev), torch.full((M,), 3, dtype=torch.int32, device=dev),
                        torch.zeros((M,), device=dev), 0.8, 10)
    choice = run_select()[0]
    memory = AutoChoices(capacity=R)
    keys, t_last = list(range(R)), np.zeros(R)
    memory.remember(keys, t_last, choice.cpu().numpy())

    def run_decide_auto():
        ctx = zoo.AutoContext(memory, keys, t_last)
        dec = zoo.decide("auto_robust", hist, T, cur, hor, M, tables, auto=ctx, **kw)
        assert ctx.selected == 0
        return dec

    def run_decide_seasonal():
        return zoo.decide("seasonal_robust", hist, T, cur, hor, M, tables, period=m)

    variants = {"holdout_score": run_k23, "hist_stats": run_hist_stats, "auto_select": run_select,
                **{f"fit:{nm}": f for nm, f in fits.items()}, "decide_auto": run_decide_auto,
                "decide_seasonal": run_decide_seasonal}
    for f in variants.values():                                # warm every shape the timed window uses
        f()
    torch.cuda.synchronize()

    # K23 against the contract on the first rows
    c = min(a.check_rows, R)
    score, cnt, nx, pick = (t[:c].cpu().numpy() for t in run_k23())
    cpu = lambda t: t[:c].cpu().numpy() if t.dim() == 2 else t[:c, None].cpu().numpy()    # noqa: E731
    r_score, r_n, r_nx = MI.ref_holdout_score(held[:c].cpu().numpy(), [cpu(t) for t in fcs], [cpu(t) for t in sigmas])
    r_pick = MI.ref_auto_pick(r_score, r_n, r_nx)
    fin = np.isfinite(r_score)
    err = float(np.max(np.abs(score[fin] - r_score[fin]), initial=0.0))
    ok = bool(np.array_equal(cnt, r_n) and np.array_equal(nx, r_nx) and np.array_equal(pick, r_pick) and err < 1e-5)

    times: dict[str, list[float]] = {k_: [] for k_ in variants}
    for _ in range(a.rounds):
        for k_, f in variants.items():
            times[k_].append(_timed(f, a.iters))
    med = {k_: statistics.median(v) for k_, v in times.items()}
    fit_sum = sum(med[f"fit:{nm}"] for nm in names)
    counts = torch.bincount(choice.long(), minlength=len(names)).tolist()
    own = float((choice.cpu() == (torch.arange(R) % 6).to(torch.int32)).float().mean())
    rec = {"bench": "auto_robust", "device": torch.cuda.get_device_name(dev), "rows": R, "T": T, "period": m,
           "holdout": L, "points": n, "rounds": a.rounds, "iters": a.iters,
           "time": time.strftime("%Y-%m-%dT%H:%M:%SZ", time.gmtime()), "history_GB": round(R * T * 4 / 1e9, 3),
           "ms": {k_: round(v, 4) for k_, v in med.items()},
           "ms_min_max": {k_: [round(min(v), 4), round(max(v), 4)] for k_, v in times.items()},
           "k23_streams": streams, "k23_GB": round(k23_bytes / 1e9, 3),
           "k23_GBps": round(k23_bytes / (med["holdout_score"] * 1e-3) / 1e9, 1),
           "hist_stats_GB": round(4 * R * hs_cols / 1e9, 3),
           "hist_stats_GBps": round(4 * R * hs_cols / (med["hist_stats"] * 1e-3) / 1e9, 1),
           "k23_over_hist_stats": round(med["holdout_score"] / med["hist_stats"], 3),
           "fits_sum_ms": round(fit_sum, 4), "auto_select_over_fits_sum": round(med["auto_select"] / fit_sum, 3),
           "decide_auto_over_decide_seasonal": round(med["decide_auto"] / med["decide_seasonal"], 3),
           "rows_per_model": dict(zip(names, counts)), "rows_that_chose_their_shapes_model": round(own, 4),
           "oracle_rows": c, "oracle_score_max_abs_err": err, "oracle_equal": ok}
    line = json.dumps(rec)
    print(line)
    outp = Path(a.out)
    outp.parent.mkdir(parents=True, exist_ok=True)
    with outp.open("a") as fh:
        fh.write(line + "\n")
    if not ok:
        raise SystemExit("bench_auto_robust: K23 differs from the contract")


if __name__ == "__main__":
    main()
