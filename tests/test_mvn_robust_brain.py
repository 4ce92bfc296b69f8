"""robust_multivariate through the brain: jobs whose history holds earlier
joint incidents are scored by the new model on the resident fast path and on
the general path with equal results, a canary job reaches a verdict that names
every member metric, ml_algorithmN selects it per metric type, and the HPA
load forecast refuses it (it is not a forecaster)."""
import dataclasses

import numpy as np
import pytest

from foremast_amd.api import crd
from foremast_amd.controller.analyst import AnalystClient
from foremast_amd.engine.brain import Brain
from foremast_amd.engine.exporter import BrainExporter
from foremast_amd.engine.sources import SourceRouter, SyntheticSource
from foremast_amd.ops import misc as MI
from foremast_amd.service.app import create_app
from foremast_amd.service.store import MemoryStore

from test_brain_e2e import PODS
from test_brain_e2e import _metrics as _e2e_metrics
from test_fastpath_models import FAULTS, T0, Clock, _cfg, _compare, _submit

ALGO = "robust_multivariate"


class IncidentSource(SyntheticSource):
    """The synthetic series with a past that holds incidents: on each of the
    last three days latency and the 5xx rate of every app were four times
    their level for 35 minutes."""

    def many(self, keys, noise_keys, fault_keys, t, stream=0):
        v = np.array(super().many(keys, noise_keys, fault_keys, t, stream), np.float32)
        tt = np.asarray(t, np.float64)
        inc = np.zeros(len(tt), bool)
        for day in (1, 2, 3):
            t0 = T0 - day * 86400.0 + day * 3600.0
            inc |= (tt >= t0) & (tt < t0 + 35 * 60.0)
        hit = np.array([("latency" in k) or ("errors_5xx" in k) for k in keys], bool)
        if hit.any() and inc.any():
            v[np.ix_(hit, inc)] *= np.float32(4.0)
        return v


def _brain(resident, faults, device="cpu", fault_after=T0 + 120, algo=ALGO):
    clock = Clock()
    store = MemoryStore()
    client = AnalystClient.for_app(create_app(store), clock=clock)
    exp = BrainExporter()
    src = SourceRouter(synthetic=IncidentSource(faults=faults, fault_after=fault_after), force="synthetic")
    brain = Brain(store, _cfg(algo), device=device, sources=src, clock=clock, exporter=exp, worker_id="w0",
                  resident_history=resident)
    return clock, store, client, brain, exp


def _watch(monkeypatch):
    """Record what the op set aside on every call the brain makes."""
    seen = []
    real = MI.mvn_robust

    def spy(*a, **kw):
        out = real(*a, **kw)
        seen.append((int(out[5].sum()), float(a[8] if len(a) > 8 else kw.get("reject", MI.MVN_REJECT))))
        return out
    monkeypatch.setattr(MI, "mvn_robust", spy)
    return seen


def test_robust_mvn_fast_path_equals_general_path(monkeypatch, device="cpu"):
    seen = _watch(monkeypatch)
    a, b = _brain(True, FAULTS, device), _brain(False, FAULTS, device)
    ids = _submit(a[2], "static")
    assert ids == _submit(b[2], "static")
    for cyc in range(4):
        ra, rb = a[3].run_once(), b[3].run_once()
        assert ra["claimed"] == rb["claimed"]
        if cyc == 0:
            assert ra["fast_jobs"] == len(ids)               # every job took the fast path
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60
    assert crd.PHASE_UNHEALTHY in {a[2].get_status(j).status for j in ids}    # the injected faults are seen
    # both paths went through the new model, with the configured limit, and it set the past incidents aside
    assert len(seen) >= 8 and all(n > 0 and r == 3.5 for n, r in seen)


def test_robust_mvn_per_metric_algorithm_fast_path_equals_general_path(monkeypatch):
    """ml_algorithmN: latency and the 5xx rate judged jointly by the robust
    model, the rest by the global model; ML_MULTIVARIATE_REJECT reaches it."""
    seen = _watch(monkeypatch)

    def brains(resident):
        got = _brain(resident, FAULTS, algo="moving_average_all")
        cfg = got[3].cfg
        cfg.multivariate_reject = 5.0
        for m in ("latency", "error5xx"):
            cfg.metric_rules[m] = dataclasses.replace(cfg.rule_for(m), algorithm="robust_mvn")
        return got
    a, b = brains(True), brains(False)
    ids = _submit(a[2], "static")
    assert ids == _submit(b[2], "static")
    for cyc in range(3):
        a[3].run_once(), b[3].run_once()
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60
    assert seen and all(n > 0 and r == 5.0 for n, r in seen)


@pytest.mark.gpu
def test_gpu_robust_mvn_fast_path_equals_general_path(monkeypatch):
    test_robust_mvn_fast_path_equals_general_path(monkeypatch, device="cuda")


def _e2e(device):
    clock, store, client, brain, exp = _brain(False, {"7687b9f4d7-aaaa1": 8.0}, device, fault_after=0.0)
    jid = client.start_analyzing("default", "demo", PODS, _e2e_metrics(), 10, "canary")
    r = brain.run_once()
    assert r["claimed"] == 1 and r["rows"] == 3
    st = client.get_status(jid)
    # an 8x fault on a canary pod breaks the joint distribution: a verdict, with every member named
    assert st.status == crd.PHASE_UNHEALTHY
    assert set(st.anomaly) == {"error5xx", "latency", "cpu"}
    stamps = {tuple(v["values"][0::2]) for v in st.anomaly.values()}
    assert len(stamps) == 1                                   # the group's flagged points, on every member


def test_robust_mvn_brain_end_to_end():
    _e2e("cpu")


@pytest.mark.gpu
def test_gpu_robust_mvn_brain_end_to_end(cuda):
    _e2e(cuda)


@pytest.mark.parametrize("resident", [True, False])
def test_hpa_forecast_refuses_the_robust_joint_model(resident, caplog):
    clock, store, client, brain, exp = _brain(resident, {}, algo="moving_average_all")
    brain.cfg.hpa_forecast_algorithm = "robust_mvn"
    client.start_analyzing("default", "demo", None, _e2e_metrics(), 10, "hpa", ["cpu", "latency"])
    with caplog.at_level("WARNING"):
        r = brain.run_once()
    assert r["outcome"] == {"hpa_scored": 1}                  # the job is scored; only the forecast is skipped
    assert "HPA forecast skipped" in caplog.text and "not a forecasting model" in caplog.text
    assert exp.sample("foremastbrain:namespace_app_pod_http_server_requests_latency_forecast_max", "default",
                      "demo") is None
