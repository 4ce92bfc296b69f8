#!/usr/bin/env python3
"""Per-workgroup start/end of the role-split front kernel (rebuild
csrc/kernels/tick_front.hip with -DFM_FRONT_TIMING:
``python tools/build_native.py --variant NAME:tick_front:-DFM_FRONT_TIMING``,
load the variant through FOREMAST_HIP_LIB): which role ends the
kernel at a given shard size, when the late history workgroups start, and how
a pairwise workgroup's time splits between its rank-test rows and its
p-values (the barrier between the two is the third mark), when the rank-test
phase ends per dispatch age class (the pairwise workgroup ids in fifths) and
per XCD, and how many rows each pairwise workgroup took (the fourth mark;
with the dynamic row queue, ``FM_FRONT_DYN_Q`` > 0, that is what the queue
dealt; they must sum to R).  The launches
measured are the scorer's steady ticks: with the row-statistics cache on
(the default) that is the ``front_hot_wgs`` shape, with ``FM_HIST_CACHE=0``
the streaming ``front_wgs`` shape given in WGS.
Prints one JSON object per shape (times in us from the first start)."""
from __future__ import annotations

import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from foremast_amd.config import BrainConfig  # noqa: E402
from foremast_amd.engine.scorer import CanaryScorer  # noqa: E402
from foremast_amd.ops import canary as C  # noqa: E402
from foremast_amd.ops._lib import LIB  # noqa: E402

ALIASES = ["error5xx", "latency", "traffic", "error4xx", "cpu", "memory", "tomcat_threads", "jvm_heap"]


MARKS = 4   # start, end, rows -> p-values barrier, rows taken (kFtMarks in tick_front.hip)


def pct(a, q):
    return round(float(np.percentile(a, q)), 1) if len(a) else None


def main() -> None:
    dev = torch.device("cuda", 0)
    cfg = BrainConfig()
    cfg.min_historical_points = 10
    for S in [int(x) for x in os.environ.get("SHAPES", "1250,10000").split(",")]:
        for wgs in [tuple(float(v) for v in w.split(":")) for w in os.environ.get("WGS", "1:4,1:3").split(",")]:
            h, b, c = C.synth_fleet(S, 8, 10080, 5, 10, 0, device=dev)
            sc = CanaryScorer(ALIASES, cfg, device=dev, front_wgs=wgs)
            front, decide, _ = sc.split_launchers(h, b, c, 10080)
            for _ in range(20):
                front()
            torch.cuda.synchronize()
            cus = torch.cuda.get_device_properties(dev).multi_processor_count
            R = S * 8
            hot = bool(sc.hist_cache)           # steady ticks expect every row in the cache
            nP, nH = sc._front_grid(not hot)
            nP = min(nP, (R + 3) // 4) if nP > 0 else (R + 3) // 4
            nH = min(nH if nH > 0 else ((R + 255) // 256 if hot else R), R)
            # the host's plan of the pairwise rows (the queue may raise nP); with
            # the queue a steady launch puts the history workgroups first
            plan = (ctypes.c_int64 * 4)()
            LIB.call("fm_front_plan", R, nP, sc._q_ranges, int(hot), ctypes.cast(plan, ctypes.c_void_p))
            s_static, pool0, q_eff, nP = (int(v) for v in plan)
            hfirst = hot and q_eff > 0
            n = nP + nH
            buf = (ctypes.c_ulonglong * (MARKS * n))()
            LIB.call("fm_front_timing_read", ctypes.cast(buf, ctypes.c_void_p), MARKS * n)
            t = np.frombuffer(buf, dtype=np.uint64).astype(np.float64).reshape(n, MARKS) / 100.0   # 100 MHz -> us
            took = t[:, 3] * 100.0                  # (a count, not a time)
            t = t[:, :3]
            t0 = t[:, 0].min()
            t -= t0
            psl, hsl = (slice(nH, n), slice(0, nH)) if hfirst else (slice(0, nP), slice(nP, n))
            p, hh, took = t[psl], t[hsl], took[psl]
            assert int(took.sum()) == R, (int(took.sum()), R)
            # rank-phase end by dispatch age class (pairwise ids in fifths) and by
            # XCD (workgroup ids are dealt round-robin over the 8 XCDs)
            cls = np.minimum(np.arange(nP) // max(nP // 5, 1), 4)
            pxcd = (np.arange(n)[psl]) & 7
            by_class = [{"start": pct(p[cls == k, 0], 50), "rank_end_p50": pct(p[cls == k, 2], 50),
                         "rank_end_max": pct(p[cls == k, 2], 100), "rows_p50": pct(took[cls == k], 50)}
                        for k in range(5) if (cls == k).any()]
            by_xcd = [{"rank_end_p50": pct(p[pxcd == x, 2], 50), "rank_end_max": pct(p[pxcd == x, 2], 100),
                       "rows_p50": pct(took[pxcd == x], 50)} for x in range(8) if (pxcd == x).any()]
            rows_us, pval_us = p[:, 2] - p[:, 0], p[:, 1] - p[:, 2]
            # per-XCD end of the history role (workgroups are dealt round-robin
            # over the 8 XCDs; the history queue splits rows into 8 XCD ranges),
            # over REPS further launches: is the late XCD always the same one?
            xe = []
            for _ in range(int(os.environ.get("REPS", "6"))):
                front()
                torch.cuda.synchronize()
                LIB.call("fm_front_timing_read", ctypes.cast(buf, ctypes.c_void_p), MARKS * n)
                tt = np.frombuffer(buf, dtype=np.uint64).astype(np.float64).reshape(n, MARKS)[:, :3] / 100.0
                tt -= tt[:, 0].min()
                hx = tt[hsl]
                xid = np.arange(nH) & 7
                xe.append([round(float(hx[xid == x, 1].max()), 1) for x in range(8)])
            print(json.dumps({"services": S, "wgs": wgs, "history_end_us_per_xcd": xe}), flush=True)
            print(json.dumps({
                "services": S, "wgs": wgs, "hot": hot, "nP": nP, "nH": nH,
                "plan": {"static_rows_per_wave": s_static, "pool0": pool0, "ranges": q_eff, "history_first": hfirst},
                "rows_taken": {"min": pct(took, 0), "p10": pct(took, 10), "p50": pct(took, 50), "p90": pct(took, 90),
                               "max": pct(took, 100)},
                "rank_end_by_age_class": by_class, "rank_end_by_xcd": by_xcd,
                "kernel_us": round(float(t[:, 1].max()), 1),
                "pairwise_end_us": {"p50": pct(p[:, 1], 50), "p90": pct(p[:, 1], 90), "max": pct(p[:, 1], 100)},
                "pairwise_rows_phase_us": {"p50": pct(rows_us, 50), "max": pct(rows_us, 100)},
                "pairwise_pvalue_phase_us": {"p50": pct(pval_us, 50), "max": pct(pval_us, 100)},
                "pairwise_pvalue_start_us": {"p50": pct(p[:, 2], 50), "max": pct(p[:, 2], 100)},
                "history_start_us": {"p50": pct(hh[:, 0], 50), "p90": pct(hh[:, 0], 90), "max": pct(hh[:, 0], 100)},
                "history_end_us": {"p10": pct(hh[:, 1], 10), "p50": pct(hh[:, 1], 50), "max": pct(hh[:, 1], 100)},
            }), flush=True)


if __name__ == "__main__":
    main()
