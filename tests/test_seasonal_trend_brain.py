"""seasonal_trend_robust through the brain: the resident fast path equals the
general path, ml_algorithmN selects it per metric type, a canary job on a
service whose memory drifts and cycles completes healthy while a fault that
hides in trend_robust's band is caught, and
HPA_FORECAST_ALGORITHM=seasonal_trend_robust publishes the profile carried
along the line of an HPA job."""
import dataclasses

import numpy as np
import pytest

from foremast_amd.api import crd
from foremast_amd.models import zoo
from foremast_amd.ops import misc as MI

from test_brain_e2e import _setup
from test_brain_e2e import _metrics as _e2e_metrics
from test_fastpath_models import FAULTS, _brain, _compare, _submit
from test_trend_brain import _drift_job

ALGO = "seasonal_trend_robust"
ARGS = {"period": 1440, "smooth": 5, "trend_min_blocks": 3}


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
def test_seasonal_trend_fast_path_equals_general_path(kind, device="cpu"):
    _parity(kind, 4, device)


def test_seasonal_trend_per_metric_algorithm_fast_path_equals_general_path(device="cpu"):
    """ml_algorithmN: memory judged by this model, the rest by the global
    mean / std model."""
    def brains(resident):
        got = _brain(resident, "moving_average_all", FAULTS, device)
        cfg = got[3].cfg
        cfg.metric_rules["memory"] = dataclasses.replace(cfg.rule_for("memory"), algorithm="robust_stl")
        assert cfg.algorithm_for("memory") == "robust_stl" and cfg.algorithm_for("cpu") == "moving_average_all"
        assert got[3]._model_args(cfg.algorithm_for("memory")) == ARGS
        assert got[3]._model_args("moving_average_all") == {} and got[3]._seasonal_trend_args("trend_robust") == {}
        return got
    a, b = brains(True), brains(False)
    ids = _submit(a[2], "static")
    assert ids == _submit(b[2], "static")
    for cyc in range(3):
        a[3].run_once(), b[3].run_once()
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60


# ------------------------------------------------------------------- drift
# Factor on the new pods' memory from T0 on, picked on the CPU reference at the memory threshold of 5: over the 22
# current points it reaches z = 15.6 .. 16.6 under this model (sigma 2.30) and z = 3.05 .. 3.23 under trend_robust
# (sigma 16.8: the daily cycle).  The healthy points reach z = 3.3 .. 4.1 here, not 0: DriftingMemory multiplies
# the cycle by the drift, and the part of the amplitude that grew since the middle of the week is not in the
# additive profile (docs/BRAIN_SPEC.md, known limits).
FAULT = 1.25


def _e2e(device):
    # the memory of the new pods is 25 % up at T0, on top of the drift and the daily cycle
    status, st = _drift_job({"memory_usage_bytes": FAULT}, ALGO, device)
    assert status == "completed_unhealth" and st.status == crd.PHASE_UNHEALTHY and set(st.anomaly) == {"memory"}
    status, st = _drift_job({}, ALGO, device)
    assert status == "completed_health" and st.status == crd.PHASE_HEALTHY, st.reason


def test_seasonal_trend_brain_end_to_end():
    _e2e("cpu")
    # the cycle stays in trend_robust's sigma: the same fault completes healthy under it
    status, st = _drift_job({"memory_usage_bytes": FAULT}, "trend_robust", "cpu")
    assert status == "completed_health" and st.status == crd.PHASE_HEALTHY, st.reason


# --------------------------------------------------------------------- HPA
def _hpa(device):
    clock, store, client, brain, exp = _setup(device=device)
    brain.cfg.hpa_forecast_algorithm = ALGO
    brain.cfg.hpa_forecast_steps = 15
    jid = client.start_analyzing("default", "demo", None, _e2e_metrics(), 10, "hpa", ["cpu", "latency"])
    r = brain.run_once()
    assert r["outcome"] == {"hpa_scored": 1}
    st = client.get_status(jid)
    assert st.status == crd.PHASE_RUNNING and len(st.hpa_logs) == 1
    # the published peak is the contract's forecast over the same rows
    clock2, store2, client2, brain2, _ = _setup(device="cpu")
    client2.start_analyzing("default", "demo", None, _e2e_metrics(), 10, "hpa", ["cpu", "latency"])
    rows = brain2._fetch_job(store2.claim("w0", 1, 90, now=clock2())[0], clock2()).rows
    seen = 0
    for row in rows:
        if row.alias not in ("cpu", "latency"):
            continue
        hist = np.asarray(row.hist, np.float32)[None, :]
        T = hist.shape[1]
        assert zoo.seasonal_start(T, 1440) == T - MI.seasonal_cycles(T, 1440) * 1440
        fc, s, n, slope, nb, _ = MI.ref_seasonal_trend_robust(hist, T, 1440, 15)
        assert nb[0] >= 3 and slope[0] != 0
        name = {"cpu": "cpu_usage_seconds_total", "latency": "http_server_requests_latency"}[row.alias]
        v = exp.sample(f"foremastbrain:namespace_app_pod_{name}_forecast_max", "default", "demo")
        assert v == pytest.approx(float(fc.max()), rel=1e-5), row.alias
        seen += 1
    assert seen == 2


def test_seasonal_trend_hpa_forecast_algorithm():
    _hpa("cpu")


def test_seasonal_trend_hpa_fast_path_equals_general_path(device="cpu"):
    """HPA jobs scored by seasonal_trend_robust with the same model as the
    published forecast: logs, bands and forecast gauges equal on both paths."""
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
    assert any("forecast_max" in str(k) for k in a[4].table.index)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["static", "continuous"])
def test_gpu_seasonal_trend_fast_path_equals_general_path(kind):
    test_seasonal_trend_fast_path_equals_general_path(kind, device="cuda")


@pytest.mark.gpu
def test_gpu_seasonal_trend_per_metric_algorithm_fast_path_equals_general_path():
    test_seasonal_trend_per_metric_algorithm_fast_path_equals_general_path(device="cuda")


@pytest.mark.gpu
def test_gpu_seasonal_trend_brain_end_to_end(cuda):
    _e2e(cuda)


@pytest.mark.gpu
def test_gpu_seasonal_trend_hpa_forecast_algorithm(cuda):
    _hpa(cuda)


@pytest.mark.gpu
def test_gpu_seasonal_trend_hpa_fast_path_equals_general_path():
    test_seasonal_trend_hpa_fast_path_equals_general_path(device="cuda")
