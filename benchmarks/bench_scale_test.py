#!/usr/bin/env python3
"""The pairwise scale test (K27): the kernel alone, and the steady resident
tick with and without it, one GPU, one process.

K27 alone (``fm_pairwise_scale``: the tier kernel and its finishing pass, with
the p-values of a tick handed through) over ``--rows`` rows at 30 + 30, 64 + 64
and 512 + 512 samples (wave tier), and the workgroup tier at 4096 + 4096 over
``--wide-rows`` rows; beside it K19 (``fm_pairwise_effect``) at 64 + 64 over
the same rows.

The tick: ``score_resident`` over a static ``ResidentHistory`` (T = 10,080,
8 metrics, 10,000 services, 5 pods x 10 points per side: bench.py's headline
shape), every row's history statistics in the cache.  Variants alternate round
by round: ``test_off`` (the default configuration, the reference point),
``test_on`` (``ML_PAIRWISE_SCALE_TEST=BROWN_FORSYTHE``) and ``gate_on`` (the
effect gate, ``ML_PAIRWISE_MIN_SHIFT=0.02`` + ``ML_PAIRWISE_DIRECTIONAL=1``).  A
round times ``--inner`` back-to-back ticks between two device events.

One JSON line per measurement (median of the rounds, their min / max) is
printed and appended to ``--out``."""
from __future__ import annotations

import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from benchmarks.bench_effect_gate import ALIASES, setup, timed  # noqa: E402
from foremast_amd.config import BrainConfig  # noqa: E402
from foremast_amd.engine.scorer import CanaryScorer  # noqa: E402
from foremast_amd.ops import canary as C  # noqa: E402

WAVE = ((30, 30), (64, 64), (512, 512))
WIDE = ((4096, 4096),)


def _windows(rows: int, n_cur: int, n_base: int, dev, seed: int):
    """Baseline N(100, 5); every other current row with twice the spread."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    k = 1.0 + (torch.arange(rows) % 2).to(torch.float32)[:, None]
    cur = (100 + 5 * k * torch.randn((rows, n_cur), generator=g)).to(dev)
    base = (100 + 5 * torch.randn((rows, n_base), generator=g)).to(dev)
    return cur, base, torch.rand((rows, C.N_TESTS), generator=g).to(dev)


def k27_alone(dev, rows: int, wide_rows: int, rounds: int, warmup: int, inner: int) -> list[dict]:
    out = []
    test = C.ScaleTest("BROWN_FORSYTHE")
    for shapes, R, tier in ((WAVE, rows, "wave"), (WIDE, wide_rows, "wide")):
        for n_cur, n_base in shapes:
            cur, base, pv = _windows(R, n_cur, n_base, dev, 27)
            buf = C.alloc_scale(R, dev)
            var = {"k27": lambda: C.pairwise_scale(cur, base, test, pv, out=buf)}
            if (n_cur, n_base) == (64, 64):
                bound = torch.ones((len(ALIASES),), dtype=torch.int32, device=dev)
                gate = C.EffectGate(min_shift=0.02, directional=True)
                ebuf = C.alloc_effect(R, dev)
                var["k19"] = lambda: C.pairwise_effect(cur, base, gate, bound, len(ALIASES), pv, out=ebuf)
            it = inner if n_cur + n_base <= 128 else max(1, inner // 10)
            res = timed(var, rounds, warmup, it)
            torch.cuda.synchronize()
            out.append({"bench": "scale_test_k27_alone", "tier": tier, "rows": R, "n_cur": n_cur, "n_base": n_base,
                        "flagged": round(float(buf.scale_diff.float().mean()), 4), "inner": it, "ms_per_launch": res})
            del cur, base, pv, buf
            torch.cuda.empty_cache()
    return out


def tick_variants(dev, st, rm, cur, base) -> dict:
    def scorer(**kw):
        cfg = BrainConfig(**kw)
        cfg.min_historical_points = 10
        return CanaryScorer(ALIASES, cfg, device=dev, xcd_balance=False)
    off, on = scorer(), scorer(pairwise_scale_test="BROWN_FORSYTHE")
    gate = scorer(pairwise_min_shift=0.02, pairwise_directional=True)
    return {"test_off": lambda: off.score_resident(st.view(), rm, cur, base),
            "test_on": lambda: on.score_resident(st.view(), rm, cur, base),
            "gate_on": lambda: gate.score_resident(st.view(), rm, cur, base)}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--modes", default="k27,tick", help="comma list of k27, tick")
    ap.add_argument("--rows", type=int, default=80000)
    ap.add_argument("--wide-rows", type=int, default=2000)
    ap.add_argument("--services", type=int, default=10000)
    ap.add_argument("--hist", type=int, default=10080)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=os.path.join("profiles", "scale_test_bench.jsonl"))
    ap.add_argument("--label", default="")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scale_test.py measures on a GPU; none is visible")
    dev = torch.device("cuda", 0)
    modes = [m for m in a.modes.split(",") if m]
    common = {"label": a.label, "rounds": a.rounds, "device": torch.cuda.get_device_name(dev)}
    lines = []
    if "k27" in modes:
        lines += [{**ln, **common} for ln in k27_alone(dev, a.rows, a.wide_rows, a.rounds, a.warmup, a.inner)]
    if "tick" in modes:
        st, rm, cur, base = setup(a.services, 5, 10, a.hist, dev)
        res = timed(tick_variants(dev, st, rm, cur, base), a.rounds, a.warmup, a.inner)
        lines.append({"bench": "scale_test_tick", "services": a.services, "metrics": len(ALIASES), "hist": a.hist,
                      "n_cur": cur.shape[1], "n_base": base.shape[1], "inner": a.inner, **common, "ms_per_tick": res})
    for ln in lines:
        s = json.dumps(ln)
        print(s, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
            with open(a.out, "a") as f:
                f.write(s + "\n")


if __name__ == "__main__":
    main()
