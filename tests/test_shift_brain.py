"""shift_robust through the brain: the resident fast path equals the general
path, ml_algorithmN selects it per metric type, and a canary job on a service
whose level changed for good three days ago completes healthy, where the
whole-history median / MAD model rolls it back, while a regression of the
canary alone is still caught."""
import dataclasses

import pytest

from foremast_amd.api import crd
from foremast_amd.config import BrainConfig
from foremast_amd.controller.analyst import AnalystClient
from foremast_amd.engine.brain import Brain
from foremast_amd.engine.exporter import BrainExporter
from foremast_amd.engine.sources import SourceRouter
from foremast_amd.models import zoo
from foremast_amd.service.app import create_app
from foremast_amd.service.store import MemoryStore

from test_brain_e2e import PODS, T0, Clock
from test_brain_e2e import _metrics as _e2e_metrics
from test_fastpath_models import FAULTS, _brain, _compare, _submit

ALGO = "shift_robust"


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
def test_shift_fast_path_equals_general_path(kind, device="cpu"):
    _parity(kind, 4, device)


def test_shift_per_metric_algorithm_fast_path_equals_general_path(device="cpu"):
    """ml_algorithmN: latency judged by the level-shift model, the rest by the
    global mean / std model."""
    def brains(resident):
        got = _brain(resident, "moving_average_all", FAULTS, device)
        cfg = got[3].cfg
        cfg.metric_rules["latency"] = dataclasses.replace(cfg.rule_for("latency"), algorithm="level_shift")
        assert cfg.algorithm_for("latency") == "level_shift" and cfg.algorithm_for("cpu") == "moving_average_all"
        assert got[3]._model_args(cfg.algorithm_for("latency")) == {"block": 1440, "shift_threshold": 4.0,
                                                                    "min_blocks": 2}
        assert got[3]._model_args("moving_average_all") == {}
        return got
    a, b = brains(True), brains(False)
    ids = _submit(a[2], "static")
    assert ids == _submit(b[2], "static")
    for cyc in range(3):
        a[3].run_once(), b[3].run_once()
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60


# every series of the app (its pods' names and its own queries carry "demo") rose tenfold three days ago: far
# enough that no sample of the new level falls inside the old level's daily swing
SHIFT = {"demo": 10.0}
CANARY = "7687b9f4d7-aaaa1"


def _job(faults, algorithm, device):
    clock = Clock()
    store = MemoryStore()
    client = AnalystClient.for_app(create_app(store), clock=clock)
    cfg = BrainConfig()
    cfg.ml_algorithm = algorithm
    src = SourceRouter.synthetic_only(faults=faults, fault_after=T0 - 3 * 86400.0)
    brain = Brain(store, cfg, device=device, sources=src, clock=clock, exporter=BrainExporter(), worker_id="w0")
    jid = client.start_analyzing("default", "demo", PODS, _e2e_metrics(), 10, "canary")
    r = brain.run_once()
    assert r["claimed"] == 1 and r["rows"] == 3
    if client.get_status(jid).status == crd.PHASE_RUNNING:   # healthy so far: the verdict comes at the end time
        clock.t += 11 * 60
        brain.run_once()
    return client.get_status(jid)


def _e2e(device):
    st = _job(SHIFT, ALGO, device)
    assert st.status == crd.PHASE_HEALTHY, st.reason
    # the whole-history median still sits on the old level: every point of the new normal is an anomaly
    st = _job(SHIFT, "robust_moving_average_all", device)
    assert st.status == crd.PHASE_UNHEALTHY and st.anomaly
    # a regression of one canary pod on top of the new level is still seen
    st = _job({**SHIFT, CANARY: 8.0}, ALGO, device)
    assert st.status == crd.PHASE_UNHEALTHY and st.anomaly


def test_shift_brain_end_to_end():
    _e2e("cpu")


def test_shift_settings_from_the_environment():
    cfg = BrainConfig.from_env({"ML_ALGORITHM": "shift_mad", "SHIFT_BLOCK": "288", "SHIFT_THRESHOLD": "6",
                                "SHIFT_MIN_BLOCKS": "3"})
    assert zoo.canonical(cfg.ml_algorithm) == ALGO
    assert (cfg.shift_block, cfg.shift_threshold, cfg.shift_min_blocks) == (288, 6.0, 3)
    brain = Brain(MemoryStore(), cfg, device="cpu", sources=SourceRouter.synthetic_only(), worker_id="w0")
    assert brain._model_args(cfg.ml_algorithm) == {"block": 288, "shift_threshold": 6.0, "min_blocks": 3}
    assert brain._seasonal_args(cfg.ml_algorithm) == {}       # (what an HPA forecast call is given)
    cfg = BrainConfig.from_env({})
    assert (cfg.shift_block, cfg.shift_threshold, cfg.shift_min_blocks) == (0, 4.0, 2)
    assert cfg.shift_block_for(60.0) == 1440


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["static", "continuous"])
def test_gpu_shift_fast_path_equals_general_path(kind):
    test_shift_fast_path_equals_general_path(kind, device="cuda")


@pytest.mark.gpu
def test_gpu_shift_per_metric_algorithm_fast_path_equals_general_path():
    test_shift_per_metric_algorithm_fast_path_equals_general_path(device="cuda")


@pytest.mark.gpu
def test_gpu_shift_brain_end_to_end(cuda):
    _e2e(cuda)
