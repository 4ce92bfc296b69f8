"""multivariate_normal through the brain: the resident fast path equals the
general path, a canary job reaches a verdict whose anomaly map names every
member metric of the flagged group, and the joint threshold's config."""
import dataclasses

import pytest

from foremast_amd.api import crd
from foremast_amd.config import BrainConfig

from test_brain_e2e import PODS, _setup
from test_brain_e2e import _metrics as _e2e_metrics
from test_fastpath_models import FAULTS, _brain, _compare, _submit


def _parity(algo, kind, device):
    a = _brain(True, algo, FAULTS, device)
    b = _brain(False, algo, FAULTS, device)
    ids = _submit(a[2], kind)
    assert ids == _submit(b[2], kind)
    for cyc in range(4):
        ra, rb = a[3].run_once(), b[3].run_once()
        assert ra["claimed"] == rb["claimed"]
        if cyc == 0:
            assert ra["fast_jobs"] == len(ids)               # every job took the fast path
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60
    return a, b, ids


def test_mvn_fast_path_equals_general_path(device="cpu"):
    a, b, ids = _parity("multivariate_normal", "static", device)
    assert crd.PHASE_UNHEALTHY in {a[2].get_status(j).status for j in ids}    # the injected faults are seen


def test_mvn_per_metric_algorithm_fast_path_equals_general_path():
    """ml_algorithmN: two of a job's four metrics judged jointly, the rest by
    the global model."""
    def brains(resident):
        got = _brain(resident, "moving_average_all", FAULTS)
        cfg = got[3].cfg
        for m in ("latency", "cpu"):
            cfg.metric_rules[m] = dataclasses.replace(cfg.rule_for(m), algorithm="multivariate_normal")
        return got
    a, b = brains(True), brains(False)
    ids = _submit(a[2], "static")
    assert ids == _submit(b[2], "static")
    for cyc in range(3):
        a[3].run_once(), b[3].run_once()
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60


@pytest.mark.gpu
def test_gpu_mvn_fast_path_equals_general_path():
    test_mvn_fast_path_equals_general_path(device="cuda")


def _e2e(device):
    clock, store, client, brain, exp = _setup(faults={"7687b9f4d7-aaaa1": 8.0}, algorithm="multivariate_normal",
                                              device=device)
    jid = client.start_analyzing("default", "demo", PODS, _e2e_metrics(), 10, "canary")
    r = brain.run_once()
    assert r["claimed"] == 1 and r["rows"] == 3
    st = client.get_status(jid)
    # an 8x fault on a canary pod breaks the joint distribution: a verdict, with every member named
    assert st.status == crd.PHASE_UNHEALTHY
    assert set(st.anomaly) == {"error5xx", "latency", "cpu"}
    stamps = {tuple(v["values"][0::2]) for v in st.anomaly.values()}
    assert len(stamps) == 1                                   # the group's flagged points, on every member


def test_mvn_brain_end_to_end():
    _e2e("cpu")


@pytest.mark.gpu
def test_gpu_mvn_brain_end_to_end(cuda):
    _e2e(cuda)


def test_multivariate_threshold_config():
    c = BrainConfig.from_env({"ML_ALGORITHM": "multivariate_normal", "ML_THRESHOLD": "2.5"})
    assert c.multivariate_threshold is None and c.mvn_threshold() == 2.5
    c = BrainConfig.from_env({"ML_THRESHOLD": "2.5", "ML_MULTIVARIATE_THRESHOLD": "4"})
    assert c.multivariate_threshold == 4.0 and c.mvn_threshold() == 4.0 and c.threshold == 2.5
    assert BrainConfig().multivariate_threshold is None and BrainConfig().mvn_threshold() == BrainConfig().threshold
