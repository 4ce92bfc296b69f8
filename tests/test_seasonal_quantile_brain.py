"""seasonal_quantile_robust through the brain: the resident fast path equals
the general path (the band decision takes a pair of sigmas per point on both),
ml_algorithmN selects it per metric type, and
HPA_FORECAST_ALGORITHM=seasonal_quantile_robust publishes the load forecast of
an HPA job, whose forecast uses the centre alone."""
import dataclasses

import numpy as np
import pytest

from foremast_amd.api import crd

from test_brain_e2e import _metrics as _e2e_metrics
from test_brain_e2e import _setup
from test_fastpath_models import FAULTS, _brain, _compare, _submit

ALGO = "seasonal_quantile_robust"


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
def test_seasonal_quantile_fast_path_equals_general_path(kind, device="cpu"):
    _parity(kind, 4, device)


def test_seasonal_quantile_per_metric_algorithm_fast_path_equals_general_path(device="cpu"):
    """ml_algorithmN: latency judged by the asymmetric per-phase band, the rest
    by the global mean / std model."""
    def brains(resident):
        got = _brain(resident, "moving_average_all", FAULTS, device)
        cfg = got[3].cfg
        cfg.metric_rules["latency"] = dataclasses.replace(cfg.rule_for("latency"), algorithm="seasonal_skew_robust")
        assert cfg.algorithm_for("latency") == "seasonal_skew_robust" and cfg.algorithm_for("cpu") == "moving_average_all"
        return got
    a, b = brains(True), brains(False)
    ids = _submit(a[2], "static")
    assert ids == _submit(b[2], "static")
    for cyc in range(3):
        a[3].run_once(), b[3].run_once()
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60


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


def test_seasonal_quantile_hpa_forecast_algorithm():
    _hpa("cpu")


def test_seasonal_quantile_hpa_fast_path_equals_general_path(device="cpu"):
    """HPA jobs scored by seasonal_quantile_robust with the same model as the
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


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["static", "continuous"])
def test_gpu_seasonal_quantile_fast_path_equals_general_path(kind):
    test_seasonal_quantile_fast_path_equals_general_path(kind, device="cuda")


@pytest.mark.gpu
def test_gpu_seasonal_quantile_per_metric_algorithm_fast_path_equals_general_path():
    test_seasonal_quantile_per_metric_algorithm_fast_path_equals_general_path(device="cuda")


@pytest.mark.gpu
def test_gpu_seasonal_quantile_hpa_forecast_algorithm(cuda):
    _hpa(cuda)
