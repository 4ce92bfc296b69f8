"""The pairwise effect gate through ``Brain.run_once`` (in-memory store).

A canary whose pods run 1 % above the baseline pods -- N(100, 1) on both sides,
100 points per side (10 pods x 10 samples) -- is "different" to every rank test, so every row's
threshold is lowered to 0.8 of itself, and one current point that sits between
the lowered and the full band makes the job unhealthy.  With
``ML_PAIRWISE_MIN_SHIFT=0.02`` the 1 % shift is no difference, the threshold
stays, and the same job is healthy.  The only difference between the runs is
the environment handed to ``BrainConfig``.  Likewise a 5 % *drop* on upper-only
metrics with and without ``ML_PAIRWISE_DIRECTIONAL``."""
import zlib

import numpy as np
import pytest

from foremast_amd.api import crd
from foremast_amd.config import BrainConfig
from foremast_amd.controller.analyst import AnalystClient
from foremast_amd.engine.brain import Brain
from foremast_amd.engine.exporter import BrainExporter
from foremast_amd.engine.sources import SourceRouter, SyntheticSource
from foremast_amd.ops import reference as ref
from foremast_amd.service.app import create_app
from foremast_amd.service.store import MemoryStore

from test_brain_e2e import T0, Clock, _metrics

SEED = 7
CANARY, BASE = "7687b9f4d7", "5db89899b5"
PODS = [[f"demo-{CANARY}-aaa{k:02d}" for k in range(10)], [f"demo-{BASE}-bbb{k:02d}" for k in range(10)]]
SPIKE_POD = PODS[0][4]
SPIKE_T = float(np.floor((T0 + 300.0) / 60.0) * 60.0)       # a grid time inside the job's current window
HIST_SD = 4.0           # history N(100, 4): the current windows stay well inside 0.8 x the tightest band (2 sigma)


class ShiftedCanary(SyntheticSource):
    """History (app level) N(100, HIST_SD), baseline pods N(100, 1), canary
    pods N(100, 1) + offset; counter-based noise, so a sample is the same in
    whichever window and batch it is asked for.  A 10-minute window holds 11
    grid samples; every 11th grid sample of a pod is missing (NaN), so any
    window has exactly 10 finite samples per pod: 100 per side.  ``spikes``:
    metric -> the value of one canary pod's sample at SPIKE_T."""

    def __init__(self, offset, spikes=None):
        super().__init__()
        self.offset, self.spikes = float(offset), dict(spikes or {})

    def prepare(self, keys, noise_keys, fault_keys):
        return None

    def many(self, keys, noise_keys, fault_keys, t, stream=0):
        tt = np.asarray(t, np.float64)
        kh = np.array([zlib.crc32(k.encode()) ^ SEED for k in noise_keys], np.uint32)[:, None]
        ti = ((tt / self.step).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)[None, :]
        h1 = ref.hash3(kh, ti, np.uint32(0xE4FEC7))
        h2 = ref.hash_u32(h1 ^ np.uint32(0x68E31DA4)).reshape(h1.shape)
        z = np.sqrt(-2.0 * np.log(ref.u01(h1).astype(np.float64))) * np.cos(2 * np.pi * ref.u01(h2).astype(np.float64))
        gap = (tt / self.step).astype(np.int64) % 11 == 0
        assert not gap[tt == SPIKE_T].any()
        out = np.empty((len(keys), len(tt)), np.float32)
        for i, nk in enumerate(noise_keys):
            metric, who = nk.split("|")
            if CANARY in who:
                v = 100.0 + z[i] + self.offset
                if who == SPIKE_POD and metric in self.spikes:
                    v = np.where(tt == SPIKE_T, self.spikes[metric], v)
                v = np.where(gap, np.nan, v)
            elif BASE in who:
                v = np.where(gap, np.nan, 100.0 + z[i])
            else:
                v = 100.0 + HIST_SD * z[i]
            out[i] = v
        return out


def _env(algo, **settings):
    env = {"ML_ALGORITHM": algo}
    env.update({k: str(v) for k, v in settings.items()})
    return env


def _setup(env, offset, spikes=None, device="cpu", resident=True):
    clock = Clock()
    store = MemoryStore()
    client = AnalystClient.for_app(create_app(store), clock=clock)
    cfg = BrainConfig.from_env(env)
    cfg.hpalog_async = 0
    src = SourceRouter(synthetic=ShiftedCanary(offset, spikes), force="synthetic")
    brain = Brain(store, cfg, device=device, sources=src, clock=clock, exporter=BrainExporter(), worker_id="w0",
                  resident_history=resident)
    return clock, store, client, brain


def _rows(env, offset, spikes=None):
    clock, store, client, brain = _setup(env, offset, spikes)
    client.start_analyzing("default", "demo", PODS, _metrics(), 10, "canary")
    rows = brain._fetch_job(store.claim("w0", 1, 90, now=clock())[0], clock()).rows
    return brain, rows


def _spikes(algo, offset, gate, aliases):
    """Per metric of ``aliases`` the value half way between the band under the
    lowered threshold (ungated scoring of the spike-less rows: every row is
    "different") and under the full one (gated scoring of the same rows)."""
    b0, rows = _rows(_env(algo), offset)
    b1, rows1 = _rows(_env(algo, **gate), offset)
    lo, full = b0.score_rows(rows), b1.score_rows(rows1)
    assert lo["diff"].all() and not full["diff"].any()
    out = {}
    for i, r in enumerate(rows):
        up_lo, up_full = float(lo["upper"][i].reshape(-1)[0]), float(full["upper"][i].reshape(-1)[0])
        assert up_lo < up_full, r.alias                     # the gate kept the threshold from being lowered
        assert np.nanmax(r.cur) < up_lo - 0.5                     # no ordinary point near either band
        if r.alias in aliases:
            out[r.base_metric.replace("namespace_app_pod_", "")] = 0.5 * (up_lo + up_full)
    return out


def _preconditions(algo, offset, spikes, max_rel):
    """On the reference, over the very rows the brain scores: ungated, every
    row is "different" (ALL six tests, p < 0.05), and every |shift| / |base_med|
    is below ``max_rel`` (or, for max_rel None, every shift is negative)."""
    _, rows = _rows(_env(algo), offset, spikes)
    cur = np.stack([r.cur for r in rows]).astype(np.float32)
    base = np.stack([r.base for r in rows]).astype(np.float32)
    assert cur.shape == base.shape == (3, 110)
    assert (np.isfinite(cur).sum(1) == 100).all() and (np.isfinite(base).sum(1) == 100).all()
    c = BrainConfig()
    _, _, diff = ref.pairwise_tests(cur, base, 63, 0, c.pairwise_threshold, c.min_mann_white, c.min_wilcoxon,
                                    c.min_kruskal)
    assert diff.all()
    eff, _ = ref.pairwise_effect(cur, base)
    rel = np.abs(eff[:, 1]) / np.abs(eff[:, 2])
    if max_rel is not None:
        assert (rel < max_rel).all() and (rel > 0.005).all(), rel
    else:
        assert (eff[:, 1] < 0).all() and (rel > 0.03).all(), eff


def _verdict(env, offset, spikes, device="cpu", resident=True):
    clock, store, client, brain = _setup(env, offset, spikes, device, resident)
    jid = client.start_analyzing("default", "demo", PODS, _metrics(), 10, "canary")
    r = brain.run_once()
    assert r["claimed"] == 1 and r["rows"] == 3
    if resident:
        assert r["fast_jobs"] == 1
    first = store.get(jid).status
    if first.startswith("completed"):
        return first, client.get_status(jid)
    clock.t += 11 * 60
    brain.run_once()
    return store.get(jid).status, client.get_status(jid)


GATE = {"ML_PAIRWISE_MIN_SHIFT": 0.02}
ALL3 = ("error5xx", "latency", "cpu")


def _one_percent(algo, device="cpu", resident=True):
    spikes = _spikes(algo, 1.0, GATE, ALL3)
    assert len(spikes) == 3
    _preconditions(algo, 1.0, spikes, 0.02)
    s0, st0 = _verdict(_env(algo), 1.0, spikes, device, resident)
    assert s0 == "completed_unhealth" and st0.status == crd.PHASE_UNHEALTHY
    assert set(st0.anomaly) == set(ALL3)
    s1, st1 = _verdict(_env(algo, **GATE), 1.0, spikes, device, resident)
    assert s1 == "completed_health" and st1.status == crd.PHASE_HEALTHY, st1.reason
    return s0, s1


def test_one_percent_shift_is_unhealthy_ungated_and_healthy_gated():
    _one_percent("moving_average_all")


def test_one_percent_shift_general_path():
    _one_percent("moving_average_all", resident=False)


def test_one_percent_shift_op_by_op_model():
    _one_percent("robust_moving_average")


def _drop(algo, device="cpu"):
    """bound = 1 (upper only): a 5 % drop lowers the threshold unless the gate
    is directional; the two-sided latency row keeps its lowered threshold
    either way (no spike there)."""
    gate = {"ML_PAIRWISE_DIRECTIONAL": 1}
    b, rows = _rows(_env(algo), -5.0)
    b1, rows1 = _rows(_env(algo, **gate), -5.0)
    lo, full = b.score_rows(rows), b1.score_rows(rows1)
    assert lo["diff"].all()
    assert [bool(d) for d in full["diff"]] == [BrainConfig().rule_for(r.alias).bound == 3 for r in rows]
    spikes = {}
    for i, r in enumerate(rows):
        up_lo, up_full = float(lo["upper"][i].reshape(-1)[0]), float(full["upper"][i].reshape(-1)[0])
        if BrainConfig().rule_for(r.alias).bound == 1:
            assert up_lo < up_full
            spikes[r.base_metric.replace("namespace_app_pod_", "")] = 0.5 * (up_lo + up_full)
        else:
            assert up_lo == up_full
    assert len(spikes) == 2
    _preconditions(algo, -5.0, spikes, None)
    s0, st0 = _verdict(_env(algo), -5.0, spikes, device)
    assert s0 == "completed_unhealth" and set(st0.anomaly) == {"error5xx", "cpu"}
    s1, _ = _verdict(_env(algo, **gate), -5.0, spikes, device)
    assert s1 == "completed_health"


def test_directional_gate_ignores_a_drop_on_upper_only_metrics():
    _drop("moving_average_all")


@pytest.mark.gpu
def test_gpu_resident_fast_path_gives_the_cpu_verdicts(cuda):
    assert _one_percent("moving_average_all", device=cuda) == _one_percent("moving_average_all")
    _drop("moving_average_all", device=cuda)
