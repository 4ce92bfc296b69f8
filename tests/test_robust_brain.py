"""robust_moving_average_all / robust_moving_average through the brain: the
resident fast path equals the general path, ml_algorithmN selects them per
metric type, and a canary job reaches a verdict whose reported band is the
oracle's median + k * sigma."""
import dataclasses
import html
import json

import numpy as np
import pytest

from foremast_amd.api import crd
from foremast_amd.ops import misc as MI

from test_brain_e2e import PODS, _setup
from test_brain_e2e import _metrics as _e2e_metrics
from test_fastpath_models import FAULTS, _brain, _compare, _submit


def _parity(algo, cycles, device):
    a = _brain(True, algo, FAULTS, device)
    b = _brain(False, algo, FAULTS, device)
    ids = _submit(a[2], "static")
    assert ids == _submit(b[2], "static")
    for cyc in range(cycles):
        ra, rb = a[3].run_once(), b[3].run_once()
        assert ra["claimed"] == rb["claimed"]
        if cyc == 0:
            assert ra["fast_jobs"] == len(ids)               # every job took the fast path
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60
    assert crd.PHASE_UNHEALTHY in {a[2].get_status(j).status for j in ids}    # the injected faults are seen


def test_robust_all_fast_path_equals_general_path(device="cpu"):
    _parity("robust_moving_average_all", 4, device)


def test_robust_window_fast_path_equals_general_path(device="cpu"):
    _parity("robust_moving_average", 3, device)


def test_robust_per_metric_algorithm_fast_path_equals_general_path():
    """ml_algorithmN: latency judged by the median / MAD band, the rest by the
    global mean / std model."""
    def brains(resident):
        got = _brain(resident, "moving_average_all", FAULTS)
        cfg = got[3].cfg
        cfg.metric_rules["latency"] = dataclasses.replace(cfg.rule_for("latency"),
                                                          algorithm="robust_moving_average_all")
        assert cfg.algorithm_for("latency") == "robust_moving_average_all"
        assert cfg.algorithm_for("cpu") == "moving_average_all"
        return got
    a, b = brains(True), brains(False)
    ids = _submit(a[2], "static")
    assert ids == _submit(b[2], "static")
    for cyc in range(3):
        a[3].run_once(), b[3].run_once()
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60


def _e2e(device):
    faults = {"7687b9f4d7-aaaa1": 8.0}
    clock, store, client, brain, exp = _setup(faults=faults, algorithm="robust_moving_average_all", device=device)
    jid = client.start_analyzing("default", "demo", PODS, _e2e_metrics(), 10, "canary")
    r = brain.run_once()
    assert r["claimed"] == 1 and r["rows"] == 3
    st = client.get_status(jid)
    assert st.status == crd.PHASE_UNHEALTHY
    reasons = {x["name"]: x for x in json.loads(html.unescape(st.reason))}
    assert set(st.anomaly) == {"error5xx", "latency", "cpu"}  # an 8x pod fault moves every metric of the pod
    assert set(reasons) == set(st.anomaly)
    # the same job's rows from an identical second setup: the oracle's band on each faulted metric
    clock2, store2, client2, brain2, _ = _setup(faults=faults, algorithm="robust_moving_average_all", device="cpu")
    client2.start_analyzing("default", "demo", PODS, _e2e_metrics(), 10, "canary")
    rows = brain2._fetch_job(store2.claim("w0", 1, 90, now=clock2())[0], clock2()).rows
    diff = brain2.score_rows(rows)["diff"]
    seen = 0
    for i, row in enumerate(rows):
        if row.alias not in reasons:
            continue
        hist = np.asarray(row.hist, np.float32)[None, :]
        center, sigma, n = MI.ref_robust_stats(hist, hist.shape[1])
        k = np.float32(brain.cfg.rule_for(row.alias).threshold)
        if diff is not None and diff[i]:
            k = k * np.float32(brain.cfg.pairwise_threshold_factor)
        upper = float(center[0] + k * sigma[0])
        assert reasons[row.alias]["upper"] == pytest.approx(upper, rel=1e-5), row.alias
        assert all(v > upper for v in reasons[row.alias]["values"]), row.alias
        seen += 1
    assert seen == len(reasons)


def test_robust_brain_end_to_end():
    _e2e("cpu")


@pytest.mark.gpu
def test_gpu_robust_all_fast_path_equals_general_path():
    test_robust_all_fast_path_equals_general_path(device="cuda")


@pytest.mark.gpu
def test_gpu_robust_window_fast_path_equals_general_path():
    test_robust_window_fast_path_equals_general_path(device="cuda")


@pytest.mark.gpu
def test_gpu_robust_brain_end_to_end(cuda):
    _e2e(cuda)
