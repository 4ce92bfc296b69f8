"""quantile_robust through the brain: ml_algorithmN selects it for a skewed
latency metric next to a metric under the default model, the resident fast
path equals the general path, the published band is asymmetric about the
median, a clean canary closes healthy under it and unhealthy under
robust_moving_average_all, and a canary whose latency collapses is flagged."""
import numpy as np
import pytest

from foremast_amd.api import crd
from foremast_amd.config import BOUND_BOTH, BrainConfig, MetricRule
from foremast_amd.controller.analyst import AnalystClient
from foremast_amd.engine.brain import Brain
from foremast_amd.engine.exporter import BrainExporter
from foremast_amd.engine.sources import SourceRouter, SyntheticSource
from foremast_amd.service.app import create_app
from foremast_amd.service.store import MemoryStore

from test_fastpath_models import T0, Clock, _compare, _pods

ALGO = "quantile_robust"
LATENCY = "http_server_requests_latency"
SKEW, THR = 0.5, 2.5
# the model's band of 100 exp(0.5 N) at thr = 2.5, z0 = 2 (100 -+ 1.25 x the distance to the 2.3 % quantiles)
# and the median / MAD band of the same history (sigma = 1.4826 x 33.5)
Q_LOWER, Q_UPPER = 100 - 1.25 * (100 - 100 * np.exp(-1.0)), 100 + 1.25 * (100 * np.exp(1.0) - 100)
MAD_UPPER = 100 + THR * 1.4826 * 33.5


class SkewedLatency(SyntheticSource):
    """The synthetic generator with every latency series replaced by 100
    exp(0.5 z): z is the generator's own standard-normal noise of that sample
    (recovered from its value), the injected faults multiply as before.  A
    sample still reads the same from any window and any query."""

    def many(self, keys, noise_keys, fault_keys, t, stream=0):
        v = super().many(keys, noise_keys, fault_keys, t, stream)
        lat = [i for i, k in enumerate(keys) if k.startswith(LATENCY)]
        if lat and len(t):
            pick = lambda a: [a[i] for i in lat]
            args = (pick(keys), pick(noise_keys), pick(fault_keys), t, stream)
            noisy = SyntheticSource(self.step, None, 0.0, self.noise, self.seed).many(*args).astype(np.float64)
            flat = SyntheticSource(self.step, None, 0.0, 0.0, self.seed).many(*args).astype(np.float64)
            z = (noisy / flat - 1.0) / self.noise
            v = v.copy()
            v[lat] = (100.0 * np.exp(SKEW * z) * (v[lat] / noisy)).astype(np.float32)
        return v


def _metrics():
    return crd.Metrics("prometheus", "http://prom/api/v1/", [crd.Monitoring(LATENCY, "gauge", "latency"),
                                                             crd.Monitoring("cpu_usage_seconds_total", "gauge", "cpu")])


def _brain(resident, faults, device="cpu", latency_algo="skew_robust"):
    clock = Clock()
    store = MemoryStore()
    client = AnalystClient.for_app(create_app(store), clock=clock)
    exp = BrainExporter()
    cfg = BrainConfig.from_env({"ML_ALGORITHM": "moving_average_all", "ML_THRESHOLD": "5",
                                "metric_type_threshold_count": "1",
                                "metric_type0": "latency", "threshold0": str(THR), "bound0": str(BOUND_BOTH),
                                "min_lower_bound0": "0", "ml_algorithm0": latency_algo})
    assert cfg.rule_for("latency") == MetricRule(THR, BOUND_BOTH, 0.0, latency_algo)
    src = SourceRouter(synthetic=SkewedLatency(faults=faults, fault_after=T0 + 120), force="synthetic")
    brain = Brain(store, cfg, device=device, sources=src, clock=clock, exporter=exp, worker_id="w0",
                  resident_history=resident)
    return clock, store, client, brain, exp


FAULTS = {"canary1-7687b9f4daaaaaaaaa-p0000": 0.15, "roll1-7687b9f4daaaaaaaaa-p0001": 4.0}


def _submit(client):
    ids = []
    for j in range(4):
        app = f"canary{j}"
        ids.append(client.start_analyzing("default", app, [_pods(app, 2, "7687b9f4d"), _pods(app, 2, "5db89899b")],
                                          _metrics(), 10, "canary"))
    for j in range(2):
        ids.append(client.start_analyzing("default", f"roll{j}", [_pods(f"roll{j}", 2, "7687b9f4d")], _metrics(), 10,
                                          "rollingUpdate"))
    return ids


def test_quantile_per_metric_algorithm_fast_path_equals_general_path(device="cpu"):
    """latency under ml_algorithm0 = skew_robust, cpu under the global mean /
    std model: statuses, reasons with their bounds, anomaly maps and gauges
    are the same on both paths, cycle by cycle, and the latency band both
    publish is the asymmetric one."""
    a, b = _brain(True, FAULTS, device), _brain(False, FAULTS, device)
    assert a[3].cfg.algorithm_for("latency") == "skew_robust" and a[3].cfg.algorithm_for("cpu") == "moving_average_all"
    ids = _submit(a[2])
    assert ids == _submit(b[2])
    for cyc in range(4):
        ra, rb = a[3].run_once(), b[3].run_once()
        assert ra["claimed"] == rb["claimed"]
        if cyc == 0:
            assert ra["fast_jobs"] == len(ids)               # every job took the fast path
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60
    assert crd.PHASE_UNHEALTHY in {a[2].get_status(j).status for j in ids}    # the injected faults are seen
    for x in (a, b):
        for app in ("canary0", "roll0"):
            up = x[4].sample(f"foremastbrain:namespace_app_pod_{LATENCY}_upper", "default", app)
            lo = x[4].sample(f"foremastbrain:namespace_app_pod_{LATENCY}_lower", "default", app)
            assert up == pytest.approx(Q_UPPER, rel=0.1) and lo == pytest.approx(Q_LOWER, rel=0.25)
            assert up - 100 > 2 * (100 - lo) and lo > 0       # asymmetric about the median of 100, above zero


CLEAN_APP = "shop3"


def _canary(algo, faults, device, app=CLEAN_APP):
    """One canary job on ``app`` with latency judged by ``algo`` -> (status
    after the first cycle, status at the end, the job's final status
    document)."""
    clock, store, client, brain, exp = _brain(False, faults, device, algo)
    pods = [_pods(app, 2, "7687b9f4d"), _pods(app, 2, "5db89899b")]
    jid = client.start_analyzing("default", app, pods, _metrics(), 10, "canary")
    assert brain.run_once()["claimed"] == 1
    first = client.get_status(jid).status
    clock.t += 11 * 60
    brain.run_once()
    st = client.get_status(jid)
    return first, st.status, st


def test_clean_skewed_window_is_healthy_where_median_mad_flags_it(device="cpu"):
    """A canary without a fault whose latency window holds a sample in the
    ordinary right tail of the history, above the median / MAD band and inside
    the quantile band: healthy under quantile_robust, unhealthy under
    robust_moving_average_all.  (Of the applications shop0 .. shop11 eight
    close healthy under quantile_robust and one under the median / MAD band;
    this is one of the seven that differ.)"""
    assert MAD_UPPER < Q_UPPER
    assert _canary(ALGO, {}, device)[:2] == (crd.PHASE_RUNNING, crd.PHASE_HEALTHY)
    first, last, st = _canary("robust_moving_average_all", {}, device)
    assert last == crd.PHASE_UNHEALTHY
    flagged = [v for k, a in st.anomaly.items() if "latency" in k for v in a["values"][1::2]]
    assert flagged and all(MAD_UPPER * 0.9 < v < Q_UPPER * 0.9 for v in flagged)


def test_collapsed_latency_is_flagged(device="cpu"):
    """The canary pods of the same application answer at 0.15 of its latency
    (median 15): below the quantile band's lower edge (21; 37 once the canary's
    distribution differs and the threshold is lowered to 2.0), while the
    median / MAD band has no lower edge above zero to cross."""
    faults = {"7687b9f4d": 0.15}
    first, last, st = _canary(ALGO, faults, device)
    assert (first, last) == (crd.PHASE_UNHEALTHY, crd.PHASE_UNHEALTHY)
    flagged = [v for k, a in st.anomaly.items() if "latency" in k for v in a["values"][1::2]]
    assert len(flagged) >= 10 and all(v < 100 * np.exp(-1.0) * 1.1 for v in flagged)
    assert _canary("robust_moving_average_all", faults, device)[:2] == (crd.PHASE_RUNNING, crd.PHASE_HEALTHY)


@pytest.mark.gpu
def test_gpu_quantile_per_metric_algorithm_fast_path_equals_general_path():
    test_quantile_per_metric_algorithm_fast_path_equals_general_path(device="cuda")


@pytest.mark.gpu
def test_gpu_clean_skewed_window_is_healthy_where_median_mad_flags_it(cuda):
    test_clean_skewed_window_is_healthy_where_median_mad_flags_it(device=cuda)


@pytest.mark.gpu
def test_gpu_collapsed_latency_is_flagged(cuda):
    test_collapsed_latency_is_flagged(device=cuda)
