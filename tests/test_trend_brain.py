"""trend_robust through the brain: the resident fast path equals the general
path, ml_algorithmN selects it per metric type, a canary job on a service
whose memory drifts steadily completes healthy while a fault on top of the
drift is caught, and HPA_FORECAST_ALGORITHM=trend_robust publishes the
extrapolated line of an HPA job."""
import dataclasses

import numpy as np
import pytest

from foremast_amd.api import crd
from foremast_amd.config import BrainConfig
from foremast_amd.controller.analyst import AnalystClient
from foremast_amd.engine.brain import Brain
from foremast_amd.engine.exporter import BrainExporter
from foremast_amd.engine.sources import SourceRouter, SyntheticSource
from foremast_amd.models import zoo
from foremast_amd.ops import misc as MI
from foremast_amd.service.app import create_app
from foremast_amd.service.store import MemoryStore

from test_brain_e2e import PODS, T0, Clock, _setup
from test_brain_e2e import _metrics as _e2e_metrics
from test_fastpath_models import FAULTS, _brain, _compare, _submit

ALGO = "trend_robust"


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
def test_trend_fast_path_equals_general_path(kind, device="cpu"):
    _parity(kind, 4, device)


def test_trend_per_metric_algorithm_fast_path_equals_general_path(device="cpu"):
    """ml_algorithmN: memory judged by the trend model, the rest by the global
    mean / std model."""
    def brains(resident):
        got = _brain(resident, "moving_average_all", FAULTS, device)
        cfg = got[3].cfg
        cfg.metric_rules["memory"] = dataclasses.replace(cfg.rule_for("memory"), algorithm="repeated_median")
        assert cfg.algorithm_for("memory") == "repeated_median" and cfg.algorithm_for("cpu") == "moving_average_all"
        assert got[3]._model_args(cfg.algorithm_for("memory")) == {"block": 1440, "trend_min_blocks": 3}
        assert got[3]._model_args("moving_average_all") == {} and got[3]._trend_args("shift_robust") == {}
        return got
    a, b = brains(True), brains(False)
    ids = _submit(a[2], "static")
    assert ids == _submit(b[2], "static")
    for cyc in range(3):
        a[3].run_once(), b[3].run_once()
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60


def test_trend_settings_from_the_environment():
    cfg = BrainConfig.from_env({"ML_ALGORITHM": "robust_trend", "TREND_BLOCK": "288", "TREND_MIN_BLOCKS": "4"})
    assert zoo.canonical(cfg.ml_algorithm) == ALGO and (cfg.trend_block, cfg.trend_min_blocks) == (288, 4)
    brain = Brain(MemoryStore(), cfg, device="cpu", sources=SourceRouter.synthetic_only(), worker_id="w0")
    assert brain._model_args(cfg.ml_algorithm) == {"block": 288, "trend_min_blocks": 4}
    assert brain._seasonal_args(cfg.ml_algorithm) == {} and brain._shift_args(cfg.ml_algorithm) == {}


# ------------------------------------------------------------------- drift
DRIFT_PER_DAY = 0.15                                         # of the level a week before T0: the week doubles it


class DriftingMemory(SyntheticSource):
    """The synthetic fleet with every memory series growing linearly: a leak
    between restarts.  The factor depends on the sample's time only, so a
    sample reads the same from any window."""

    def many(self, keys, noise_keys, fault_keys, t, stream=0):
        v = super().many(keys, noise_keys, fault_keys, t, stream)
        grow = (1.0 + DRIFT_PER_DAY * (np.asarray(t, np.float64) - (T0 - 7 * 86400.0)) / 86400.0)
        mem = np.array([k.startswith("memory") for k in keys], bool)
        return np.where(mem[:, None], v * grow[None, :], v).astype(np.float32)


def _mem_metrics():
    return crd.Metrics("prometheus", "http://prom/api/v1/", [
        crd.Monitoring("memory_usage_bytes", "gauge", "memory"),
        crd.Monitoring("cpu_usage_seconds_total", "gauge", "cpu"),
    ])


def _drift_job(faults, algorithm, device):
    clock = Clock()
    store = MemoryStore()
    client = AnalystClient.for_app(create_app(store), clock=clock)
    cfg = BrainConfig()
    cfg.ml_algorithm = "moving_average_all"
    cfg.metric_rules["memory"] = dataclasses.replace(cfg.rule_for("memory"), algorithm=algorithm)
    src = SourceRouter(synthetic=DriftingMemory(faults=faults, fault_after=T0, noise=0.005), force="synthetic")
    brain = Brain(store, cfg, device=device, sources=src, clock=clock, exporter=BrainExporter(), worker_id="w0")
    jid = client.start_analyzing("default", "demo", PODS[:1], _mem_metrics(), 10, "rollingUpdate")
    r = brain.run_once()
    assert r["claimed"] == 1 and r["rows"] == 2
    if client.get_status(jid).status == crd.PHASE_RUNNING:   # healthy so far: the verdict comes at the end time
        clock.t += 11 * 60
        brain.run_once()
    return store.get(jid).status, client.get_status(jid)


def _e2e(device):
    # the memory of the new pods doubles at T0, on top of the drift (the daily cycle stays in sigma, so the band
    # is about +- 80 % of the level: a limit of the model, docs/BRAIN_SPEC.md)
    status, st = _drift_job({"memory_usage_bytes": 2.0}, ALGO, device)
    assert status == "completed_unhealth" and st.status == crd.PHASE_UNHEALTHY and set(st.anomaly) == {"memory"}
    status, st = _drift_job({}, ALGO, device)
    assert status == "completed_health" and st.status == crd.PHASE_HEALTHY, st.reason


def test_trend_brain_end_to_end():
    _e2e("cpu")


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
    # the published peak is the extrapolated line of the oracle over the same rows
    clock2, store2, client2, brain2, _ = _setup(device="cpu")
    client2.start_analyzing("default", "demo", None, _e2e_metrics(), 10, "hpa", ["cpu", "latency"])
    rows = brain2._fetch_job(store2.claim("w0", 1, 90, now=clock2())[0], clock2()).rows
    seen = 0
    for row in rows:
        if row.alias not in ("cpu", "latency"):
            continue
        hist = np.asarray(row.hist, np.float32)[None, :]
        T = hist.shape[1]
        s0 = zoo.trend_start(T)
        c, s, n, slope, nb = MI.ref_trend_robust(hist[:, s0:], T - s0, 1440)
        assert nb[0] >= 3 and slope[0] != 0
        line = c[0] + slope[0] * np.arange(1, 16, dtype=np.float32)
        name = {"cpu": "cpu_usage_seconds_total", "latency": "http_server_requests_latency"}[row.alias]
        v = exp.sample(f"foremastbrain:namespace_app_pod_{name}_forecast_max", "default", "demo")
        assert v == pytest.approx(float(line.max()), rel=1e-5), row.alias
        seen += 1
    assert seen == 2


def test_trend_hpa_forecast_algorithm():
    _hpa("cpu")


def test_trend_hpa_fast_path_equals_general_path(device="cpu"):
    """HPA jobs scored by trend_robust with the same model as the published
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
    assert any("forecast_max" in str(k) for k in a[4].table.index)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["static", "continuous"])
def test_gpu_trend_fast_path_equals_general_path(kind):
    test_trend_fast_path_equals_general_path(kind, device="cuda")


@pytest.mark.gpu
def test_gpu_trend_per_metric_algorithm_fast_path_equals_general_path():
    test_trend_per_metric_algorithm_fast_path_equals_general_path(device="cuda")


@pytest.mark.gpu
def test_gpu_trend_brain_end_to_end(cuda):
    _e2e(cuda)


@pytest.mark.gpu
def test_gpu_trend_hpa_forecast_algorithm(cuda):
    _hpa(cuda)


@pytest.mark.gpu
def test_gpu_trend_hpa_fast_path_equals_general_path():
    test_trend_hpa_fast_path_equals_general_path(device="cuda")
