"""seasonal_robust through the brain: the resident fast path equals the
general path, ml_algorithmN selects it per metric type, a canary job reaches
a verdict whose reported band is the oracle's profile + k * sigma at each
point's horizon, and HPA_FORECAST_ALGORITHM=seasonal_robust publishes the load
forecast of an HPA job."""
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

ALGO = "seasonal_robust"


def _parity(kind, cycles, device):
    a = _brain(True, ALGO, FAULTS, device)
    b = _brain(False, ALGO, FAULTS, device)
    ids = _submit(a[2], kind)
    assert ids == _submit(b[2], kind)
    for cyc in range(cycles):
        ra, rb = a[3].run_once(), b[3].run_once()
        assert ra["claimed"] == rb["claimed"]
        if cyc == 0:
            assert ra["fast_jobs"] == len(ids)               # every job took the fast path
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60
    assert crd.PHASE_UNHEALTHY in {a[2].get_status(j).status for j in ids}    # the injected faults are seen


@pytest.mark.parametrize("kind", ["static", "continuous"])
def test_seasonal_fast_path_equals_general_path(kind, device="cpu"):
    _parity(kind, 4, device)


def test_seasonal_per_metric_algorithm_fast_path_equals_general_path(device="cpu"):
    """ml_algorithmN: latency judged by the seasonal median / MAD model, the
    rest by the global mean / std model."""
    def brains(resident):
        got = _brain(resident, "moving_average_all", FAULTS, device)
        cfg = got[3].cfg
        cfg.metric_rules["latency"] = dataclasses.replace(cfg.rule_for("latency"), algorithm="seasonal_mad")
        assert cfg.algorithm_for("latency") == "seasonal_mad" and cfg.algorithm_for("cpu") == "moving_average_all"
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
    clock, store, client, brain, exp = _setup(faults=faults, algorithm=ALGO, device=device)
    jid = client.start_analyzing("default", "demo", PODS, _e2e_metrics(), 10, "canary")
    r = brain.run_once()
    assert r["claimed"] == 1 and r["rows"] == 3
    st = client.get_status(jid)
    assert st.status == crd.PHASE_UNHEALTHY
    reasons = {x["name"]: x for x in json.loads(html.unescape(st.reason))}
    assert reasons and set(reasons) == set(st.anomaly)
    # the same job's rows from an identical second setup: the oracle's band at each flagged point's horizon
    clock2, store2, client2, brain2, _ = _setup(faults=faults, algorithm=ALGO, device="cpu")
    client2.start_analyzing("default", "demo", PODS, _e2e_metrics(), 10, "canary")
    rows = brain2._fetch_job(store2.claim("w0", 1, 90, now=clock2())[0], clock2()).rows
    diff = brain2.score_rows(rows)["diff"]
    m = brain.cfg.seasonal_period_for(brain.step)
    assert m == 1440
    seen = 0
    for i, row in enumerate(rows):
        if row.alias not in reasons:
            continue
        hist = np.asarray(row.hist, np.float32)[None, :]
        assert MI.seasonal_cycles(hist.shape[1], m) >= 2      # a week of history: the seasonal model, not its fallback
        k = np.float32(brain.cfg.rule_for(row.alias).threshold)
        if diff is not None and diff[i]:
            k = k * np.float32(brain.cfg.pairwise_threshold_factor)
        got = reasons[row.alias]
        hor = np.maximum(1, np.rint((np.asarray(row.cur_t) - row.hist_t_last) / brain.step)).astype(np.int64)
        fc, sigma, n, _ = MI.ref_seasonal_robust(hist, hist.shape[1], m, int(hor.max()), brain.cfg.seasonal_smooth)
        upper = (fc[0, hor - 1] + k * sigma[0]).astype(np.float64)
        want = set(zip(got["ts"], got["values"]))             # (a row holds the points of both pods: times repeat)
        flagged = [j for j in range(len(row.cur)) if (float(row.cur_t[j]), float(row.cur[j])) in want]
        assert len(flagged) == len(got["ts"]) > 0, row.alias
        # the reason carries the band of the row's first flagged point; every flagged point is above its own
        assert got["upper"] == pytest.approx(upper[flagged[0]], rel=1e-5), row.alias
        assert all(row.cur[j] > upper[j] for j in flagged), row.alias
        seen += 1
    assert seen == len(reasons)


def test_seasonal_brain_end_to_end():
    _e2e("cpu")


def _hpa(device):
    clock, store, client, brain, exp = _setup(device=device)
    brain.cfg.hpa_forecast_algorithm = ALGO
    jid = client.start_analyzing("default", "demo", None, _e2e_metrics(), 10, "hpa", ["cpu", "latency"])
    for _ in range(2):
        r = brain.run_once()
        assert r["outcome"] == {"hpa_scored": 1}
        clock.t += 30
    st = client.get_status(jid)
    assert st.status == crd.PHASE_RUNNING and len(st.hpa_logs) == 2
    v = exp.sample("foremastbrain:namespace_app_pod_http_server_requests_latency_forecast_max", "default", "demo")
    assert v is not None and np.isfinite(v)


def test_seasonal_hpa_forecast_algorithm():
    _hpa("cpu")


def test_seasonal_hpa_fast_path_equals_general_path(device="cpu"):
    """HPA jobs scored by seasonal_robust with the same model as the published
    forecast: logs, bands and forecast gauges equal on both paths."""
    a = _brain(True, ALGO, FAULTS, device)
    b = _brain(False, ALGO, FAULTS, device)
    for x in (a, b):
        x[3].cfg.hpa_forecast_algorithm = ALGO
    ids = _submit(a[2], "hpa")
    assert ids == _submit(b[2], "hpa")
    for cyc in range(3):
        a[3].run_once(), b[3].run_once()
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60
    assert all(a[1].hpalogs(j) for j in ids)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["static", "continuous"])
def test_gpu_seasonal_fast_path_equals_general_path(kind):
    test_seasonal_fast_path_equals_general_path(kind, device="cuda")


@pytest.mark.gpu
def test_gpu_seasonal_per_metric_algorithm_fast_path_equals_general_path():
    test_seasonal_per_metric_algorithm_fast_path_equals_general_path(device="cuda")


@pytest.mark.gpu
def test_gpu_seasonal_brain_end_to_end(cuda):
    _e2e(cuda)


@pytest.mark.gpu
def test_gpu_seasonal_hpa_forecast_algorithm(cuda):
    _hpa(cuda)


@pytest.mark.gpu
def test_gpu_seasonal_hpa_fast_path_equals_general_path():
    test_seasonal_hpa_fast_path_equals_general_path(device="cuda")
