"""auto_robust through the brain: a cycle over jobs whose metrics have the six
shapes reports the six models and sees an anomaly on each, the choice is
remembered between cycles (and selected again after AUTO_RESELECT of new
history), ml_algorithmN and AUTO_CANDIDATES configure it, and the resident fast
path equals the general path."""
import dataclasses
import urllib.parse
import zlib

import numpy as np
import pytest

from foremast_amd.api import crd
from foremast_amd.config import BrainConfig
from foremast_amd.controller.analyst import AnalystClient
from foremast_amd.engine import sources as S
from foremast_amd.engine.brain import Brain
from foremast_amd.engine.exporter import BrainExporter
from foremast_amd.models import zoo
from foremast_amd.service.app import create_app
from foremast_amd.service.store import MemoryStore

from test_fastpath_models import FAULTS, Clock, T0, _brain, _compare, _submit

ALGO = "auto_robust"
STEP = 900.0                        # 96 samples a day: a 7-day history is 672 samples
M96 = 96
APPS = ("flat", "shift", "trend", "seasonal", "scale", "strend")     # in candidate order
NEVER = float("inf")


class ShapeSource:
    """One series per application, shaped by the application's name: the six
    histories of tests/test_auto_ops.py on the grid of multiples of STEP, a
    sample being a function of its time alone.  After ``fault_after`` every
    sample lies ``fault`` higher."""
    local = True

    def __init__(self, fault_after=NEVER, fault=300.0):
        self.fault_after, self.fault = fault_after, fault
        self.k0 = int(round((T0 - 7 * 86400.0) / STEP))           # the sample a history fetched at T0 starts near

    def values(self, app, metric, t):
        k = np.rint(t / STEP).astype(np.int64)
        i = (k - self.k0).astype(np.float64)
        e = np.array([np.random.default_rng([zlib.crc32(f"{metric}|{app}".encode()), int(j)]).standard_normal()
                      for j in k])
        w = np.sin(2 * np.pi * i / M96)
        lvl = 100 + 80 * w
        v = {"flat": 100 + 2 * e, "shift": 100 + 2 * e + 40 * (i >= 3 * M96 + M96 // 3), "trend": 100 + 10 * i / M96 + 2 * e,
             "seasonal": 100 + 40 * w + 2 * e, "scale": lvl + 0.08 * lvl * e, "strend": 100 + 40 * w + 10 * i / M96 + 2 * e}[app]
        return (v + self.fault * (t > self.fault_after)).astype(np.float32)

    def fetch(self, url):
        qs = dict(urllib.parse.parse_qsl(url.split("?", 1)[1]))
        q, start, end = qs.get("query", ""), float(qs.get("start", 0)), float(qs.get("end", 0))
        t = STEP * np.arange(np.ceil(start / STEP - 1e-9), np.floor(end / STEP + 1e-9) + 1)
        metric = q.split("{")[0]
        return [S.Series({"__name__": metric}, t, self.values(S._app_of(q), metric, t))]


def _metrics(n=1):
    ms = [crd.Monitoring("http_server_requests_latency", "gauge", "latency"),
          crd.Monitoring("cpu_usage_seconds_total", "gauge", "cpu")]
    return crd.Metrics("prometheus", "http://prom/api/v1/", ms[:n])


def _shape_brain(cfg=None, fault_after=NEVER, n_metrics=1, device="cpu"):
    clock, store = Clock(), MemoryStore()
    client = AnalystClient.for_app(create_app(store), clock=clock)
    if cfg is None:
        cfg = BrainConfig()
        cfg.ml_algorithm = ALGO
    cfg.threshold = 6.0
    cfg.metric_rules = {k: dataclasses.replace(r, threshold=6.0) for k, r in cfg.metric_rules.items()}
    exp = BrainExporter()
    brain = Brain(store, cfg, device=device, sources=S.SourceRouter(synthetic=ShapeSource(fault_after), force="synthetic"),
                  clock=clock, exporter=exp, worker_id="w0", resident_history=False, step=STEP, watch_minutes=150.0)
    ids = [client.start_analyzing("prod", app, None, _metrics(n_metrics), 600, "continuous") for app in APPS]
    return (clock, store, client, brain, exp), ids


def _rows_of(got, ids):
    clock, store, client, brain, exp = got
    docs = {d.id: d for d in store.claim("w0", len(ids), 90, now=clock())}
    rows = []
    for j, jid in enumerate(ids):
        wk = brain._fetch_job(docs[jid], clock())
        for r in wk.rows:
            r.job, r.series = j, f"prod/{docs[jid].app_name}"
            rows.append(r)
    return rows


def test_six_shapes_score_under_six_models_and_each_sees_its_anomaly():
    got, ids = _shape_brain(fault_after=T0 - 4.5 * STEP)          # the last five current points lie 300 higher
    brain = got[3]
    rows = _rows_of(got, ids)
    assert len(rows) == 6 and 660 <= len(rows[0].hist) <= 672
    out = brain.score_rows(rows)
    assert out["algorithms"] == [ALGO] * 6
    assert out["auto_choice"] == list(zoo.AUTO_CANDIDATES)
    assert brain.auto_rows == {name: 1 for name in zoo.AUTO_CANDIDATES} and brain.auto_selected == 6
    for i, r in enumerate(rows):
        late = r.cur_t > T0 - 4.5 * STEP
        assert 3 <= late.sum() < len(late)
        np.testing.assert_array_equal(out["flags"][i][:len(late)], late, err_msg=APPS[i])
    # the same rows again: nothing is selected, the decision is the same
    brain.auto_rows, brain.auto_selected = {}, 0
    again = brain.score_rows(rows)
    assert brain.auto_selected == 0 and again["auto_choice"] == out["auto_choice"]
    for k in ("upper", "lower", "count", "score", "valid", "flags"):
        np.testing.assert_array_equal(again[k], out[k], err_msg=k)


def test_choices_are_remembered_between_cycles():
    a, ids = _shape_brain(fault_after=T0 + 0.5 * STEP)   # first seen by the third cycle's window
    b, ids_b = _shape_brain(fault_after=T0 + 0.5 * STEP)   # first seen by the third cycle's window
    assert ids == ids_b
    for cyc in range(3):
        if cyc:
            b[3].auto_choices.clear()                            # b forgets: it selects in every cycle
        ra, rb = a[3].run_once(), b[3].run_once()
        assert ra["claimed"] == rb["claimed"] == 6 and ra["rows"] == 6
        assert a[3].auto_rows == b[3].auto_rows == {name: 1 for name in zoo.AUTO_CANDIDATES}, (cyc, a[3].auto_rows)
        assert a[3].auto_selected == (6 if cyc == 0 else 0) and b[3].auto_selected == 6
        _compare(a, b, ids, cyc)
        status = {a[1].get(j).status for j in ids}
        assert status == ({"completed_unhealth"} if cyc == 2 else {"preprocess_completed"}), (cyc, status)
        a[0].t += STEP
        b[0].t += STEP
    assert len(a[3].auto_choices) == 6


def test_a_day_of_new_history_selects_again():
    cfg = BrainConfig.from_env({"ML_ALGORITHM": "auto", "AUTO_RESELECT": str(2 * STEP)})
    assert cfg.auto_reselect == 2 * STEP and BrainConfig().auto_reselect == 86400.0
    got, ids = _shape_brain(cfg)
    clock, brain = got[0], got[3]
    selected = []
    for _ in range(4):
        brain.run_once()
        selected.append(brain.auto_selected)
        clock.t += STEP
    assert selected == [6, 0, 6, 0]


def test_auto_choices_memory_is_bounded_and_ages():
    from foremast_amd.models.cache import AutoChoices
    mem = AutoChoices(capacity=2, reselect_seconds=100.0)
    mem.remember(["a", "b"], [10.0, 10.0], [3, 4])
    np.testing.assert_array_equal(mem.lookup(["a", "b", "c"], [50.0, 110.0, 0.0]), [3, -1, -1])
    mem.remember(["a", "b", "c"], [0, 120.0, 120.0], [0, 5, 1], fresh=[False, True, True])
    assert len(mem) == 2 and "a" not in mem.entries               # the oldest entry left
    np.testing.assert_array_equal(mem.lookup(["b", "c"], [130.0, 219.9]), [5, 1])
    none = AutoChoices(capacity=0)
    none.remember(["a"], [0.0], [1])
    assert len(none) == 0 and none.lookup(["a"], [0.0])[0] == -1


def test_per_metric_auto_robust_beside_another_model():
    env = {"ML_ALGORITHM": "moving_average_all", "metric_type_threshold_count": "2",
           "metric_type0": "latency", "threshold0": "6", "bound0": "3", "ml_algorithm0": "auto_select",
           "metric_type1": "cpu", "threshold1": "6", "bound1": "1"}
    cfg = BrainConfig.from_env(env)
    assert zoo.canonical(cfg.algorithm_for("latency")) == ALGO and cfg.algorithm_for("cpu") == "moving_average_all"
    got, ids = _shape_brain(cfg, n_metrics=2)
    brain = got[3]
    out = brain.score_rows(_rows_of(got, ids))
    assert out["algorithms"] == [ALGO, "moving_average_all"] * 6
    assert out["auto_choice"] == [x for name in zoo.AUTO_CANDIDATES for x in (name, None)]
    assert brain.auto_rows == {name: 1 for name in zoo.AUTO_CANDIDATES}


def test_auto_candidates_subset_and_unknown_name():
    cfg = BrainConfig.from_env({"ML_ALGORITHM": ALGO, "AUTO_CANDIDATES": "seasonal_robust, robust_moving_average_all",
                                "AUTO_HOLDOUT": "48", "AUTO_MARGIN": "0.1", "AUTO_ZCAP": "6"})
    assert (cfg.auto_holdout, cfg.auto_margin, cfg.auto_zcap) == (48, 0.1, 6.0)
    got, ids = _shape_brain(cfg)
    brain = got[3]
    kw = brain._auto_args(ALGO)
    assert kw["holdout"] == 48 and kw["margin"] == 0.1 and kw["zcap"] == 6.0 and kw["period"] == M96
    assert brain._auto_args("seasonal_robust") == {}
    out = brain.score_rows(_rows_of(got, ids))
    assert set(out["auto_choice"]) == {"robust_moving_average_all", "seasonal_robust"}
    assert out["auto_choice"][0] == "robust_moving_average_all" and out["auto_choice"][3] == "seasonal_robust"
    with pytest.raises(ValueError):
        Brain(MemoryStore(), BrainConfig.from_env({"AUTO_CANDIDATES": "seasonal_robust,holt_winters"}),
              sources=S.SourceRouter.synthetic_only())


# ------------------------------------------------------------------ the resident fast path
def _parity(kind, cycles, device):
    a = _brain(True, ALGO, FAULTS, device)
    b = _brain(False, ALGO, FAULTS, device)
    ids = _submit(a[2], kind)
    assert ids == _submit(b[2], kind)
    for cyc in range(cycles):
        ra, rb = a[3].run_once(), b[3].run_once()
        assert ra["claimed"] == rb["claimed"]
        if cyc == 0:
            assert ra["fast_jobs"] == len(ids)                   # every job took the fast path
            rows = sum(a[3].auto_rows.values())
            assert rows > 0 and a[3].auto_selected == rows and a[3].auto_rows == b[3].auto_rows
        else:
            assert a[3].auto_selected == 0 and b[3].auto_selected == 0 and a[3].auto_rows == b[3].auto_rows
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60
    assert crd.PHASE_UNHEALTHY in {a[2].get_status(j).status for j in ids}    # the injected faults are seen


@pytest.mark.parametrize("kind", ["static", "continuous"])
def test_auto_fast_path_equals_general_path(kind, device="cpu"):
    _parity(kind, 3, device)


def test_auto_hpa_forecast_algorithm(device="cpu"):
    from test_brain_e2e import _metrics as e2e_metrics
    from test_brain_e2e import _setup
    clock, store, client, brain, exp = _setup(device=device)
    brain.cfg.hpa_forecast_algorithm = ALGO
    client.start_analyzing("default", "demo", None, e2e_metrics(), 10, "hpa", ["cpu", "latency"])
    for _ in range(2):
        assert brain.run_once()["outcome"] == {"hpa_scored": 1}
        clock.t += 30
    v = exp.sample("foremastbrain:namespace_app_pod_http_server_requests_latency_forecast_max", "default", "demo")
    assert v is not None and np.isfinite(v)


def test_auto_hpa_fast_path_equals_general_path(device="cpu"):
    """HPA jobs scored by auto_robust, the published forecast by auto_robust
    too: logs, bands, forecast gauges and counters equal on both paths."""
    a = _brain(True, ALGO, FAULTS, device)
    b = _brain(False, ALGO, FAULTS, device)
    for x in (a, b):
        x[3].cfg.hpa_forecast_algorithm = ALGO
    ids = _submit(a[2], "hpa")
    assert ids == _submit(b[2], "hpa")
    for cyc in range(3):
        a[3].run_once(), b[3].run_once()
        _compare(a, b, ids, cyc)
        assert a[3].auto_rows == b[3].auto_rows and sum(a[3].auto_rows.values()) == 12
        assert a[3].auto_selected == b[3].auto_selected == (12 if cyc == 0 else 0)
        a[0].t += 60
        b[0].t += 60
    assert all(a[1].hpalogs(j) for j in ids)


@pytest.mark.gpu
def test_gpu_auto_hpa_fast_path_equals_general_path():
    test_auto_hpa_fast_path_equals_general_path(device="cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["static", "continuous"])
def test_gpu_auto_fast_path_equals_general_path(kind):
    test_auto_fast_path_equals_general_path(kind, device="cuda")


@pytest.mark.gpu
def test_gpu_auto_hpa_forecast_algorithm(cuda):
    test_auto_hpa_forecast_algorithm(device=cuda)
