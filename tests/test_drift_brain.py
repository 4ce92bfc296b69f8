"""The drift test through ``Brain.run_once`` and ``Brain.score_rows`` (in-memory store).

History N(100, 5).  Every canary pod creeps from 100 to 113.5 over the job's
10-minute window; every baseline sample is drawn uniformly from the same range,
in no order.  Both windows then have the same pooled distribution, no test of
``ALL`` sees a difference, and the threshold stays: 113.5 lies inside 3 sigma
(115) and outside 0.8 x 3 sigma (112), so the job is healthy with the test off
and unhealthy with ``ML_PAIRWISE_DRIFT_TEST=MANN_KENDALL``, which finds the
trend and lowers the threshold."""
import zlib

import numpy as np
import pytest

from foremast_amd.config import BrainConfig
from foremast_amd.controller.analyst import AnalystClient
from foremast_amd.engine.brain import Brain, Row
from foremast_amd.engine.exporter import BrainExporter
from foremast_amd.engine.scorer import CanaryScorer
from foremast_amd.engine.sources import SourceRouter, SyntheticSource
from foremast_amd.ops import reference as ref
from foremast_amd.service.store import MemoryStore
from foremast_amd.service.app import create_app

from test_brain_e2e import T0, Clock
from test_effect_brain import BASE, CANARY, PODS, SEED
from test_scale_brain import _metrics

ON = {"ML_PAIRWISE_DRIFT_TEST": "MANN_KENDALL"}
TOP = 13.5


class CreepingCanary(SyntheticSource):
    """Counter-based noise as test_scale_brain.JitteryCanary; every 11th grid
    sample of a pod is missing, so a 10-minute window has 10 finite samples per pod."""

    def prepare(self, keys, noise_keys, fault_keys):
        return None

    def many(self, keys, noise_keys, fault_keys, t, stream=0):
        tt = np.asarray(t, np.float64)
        kh = np.array([zlib.crc32(k.encode()) ^ SEED for k in noise_keys], np.uint32)[:, None]
        ti = ((tt / self.step).astype(np.int64) & 0xFFFFFFFF).astype(np.uint32)[None, :]
        h1 = ref.hash3(kh, ti, np.uint32(0xE4FEC7))
        h2 = ref.hash_u32(h1 ^ np.uint32(0x68E31DA4)).reshape(h1.shape)
        u1, u2 = ref.u01(h1).astype(np.float64), ref.u01(h2).astype(np.float64)
        z = np.sqrt(-2.0 * np.log(u1)) * np.cos(2 * np.pi * u2)
        gap = (tt / self.step).astype(np.int64) % 11 == 0
        creep = TOP * np.clip((tt - T0) / 600.0, 0.0, 1.0)
        out = np.empty((len(keys), len(tt)), np.float32)
        for i, nk in enumerate(noise_keys):
            _, who = nk.split("|")
            if CANARY in who:
                out[i] = np.where(gap, np.nan, 100.0 + creep + 0.05 * z[i])
            elif BASE in who:
                out[i] = np.where(gap, np.nan, 100.0 + TOP * u2[i])
            else:
                out[i] = 100.0 + 5.0 * z[i]
        return out


def _setup(env, device="cpu"):
    clock, store = Clock(), MemoryStore()
    client = AnalystClient.for_app(create_app(store), clock=clock)
    cfg = BrainConfig.from_env({"ML_ALGORITHM": "moving_average_all", **env})
    cfg.hpalog_async = 0
    brain = Brain(store, cfg, device=device, sources=SourceRouter(synthetic=CreepingCanary(), force="synthetic"),
                  clock=clock, exporter=BrainExporter(), worker_id="w0")
    return clock, store, client, brain


def _verdict(env, device="cpu"):
    clock, store, client, brain = _setup(env, device)
    jid = client.start_analyzing("default", "demo", PODS, _metrics(), 10, "canary")
    r = brain.run_once()
    assert r["claimed"] == 1 and r["rows"] == 1 and r["fast_jobs"] == 1
    if not store.get(jid).status.startswith("completed"):
        clock.t += 11 * 60
        brain.run_once()
    return store.get(jid).status, client.get_status(jid).reason


def test_preconditions_on_the_rows_the_brain_scores():
    clock, store, client, brain = _setup({})
    client.start_analyzing("default", "demo", PODS, _metrics(), 10, "canary")
    row, = brain._fetch_job(store.claim("w0", 1, 90, now=clock())[0], clock()).rows
    c = BrainConfig()
    _, _, diff = ref.pairwise_tests(row.cur[None], row.base[None], 63, 0, c.pairwise_threshold, c.min_mann_white,
                                    c.min_wilcoxon, c.min_kruskal)
    assert not diff.any() and row.cur_pods.tolist() == [11] * 10
    d, counts, _, pod_n, k = ref.pairwise_drift(row.cur[None], np.cumsum(row.cur_pods)[None], row.base[None],
                                                c.min_drift_points)
    assert ref.drift_verdict(d, c.pairwise_threshold).all() and k[0] == 10 and (pod_n == 10).all()
    assert counts[0, 0, 0] == counts[0, 0, 1] == 450 and abs(d[0, 4]) < 2 and d[0, 1] < 1e-6


def test_creeping_canary_is_unhealthy_only_with_the_setting():
    assert _verdict({})[0] == "completed_health"
    assert _verdict({"ML_PAIRWISE_DRIFT_TEST": "OFF"})[0] == "completed_health"
    status, reason = _verdict(ON)
    assert status == "completed_unhealth" and "error4xx" in reason, reason


@pytest.mark.gpu
def test_gpu_resident_fast_path_gives_the_cpu_verdicts(cuda):
    assert _verdict({}, cuda) == _verdict({})
    assert _verdict(ON, cuda) == _verdict(ON)


def _score(env, cur, base):
    rng = np.random.default_rng(1)
    brain = Brain(MemoryStore(), BrainConfig.from_env({"ML_ALGORITHM": "moving_average_all", **env}), device="cpu",
                  resident_history=False)
    row = Row(0, "error4xx", "m", rng.normal(100, 5, 600).astype(np.float32), 0.0, cur, np.zeros(0), base,
              cur_pods=np.asarray([len(cur)], np.int64))
    return brain.score_rows([row])["diff"].tolist()


def test_a_common_ramp_stays_healthy_with_the_setting():
    rng = np.random.default_rng(2)
    ramp = np.linspace(98, 102, 60)
    cur, base = ((ramp + rng.normal(0, 1, 60)).astype(np.float32) for _ in range(2))
    flat = (100 + rng.normal(0, 1, 60)).astype(np.float32)
    assert _score(ON, cur, base) == [0] and _score({}, cur, base) == [0]
    assert _score(ON, cur, flat) == [1]                        # the same canary against a baseline that does not ramp


def test_unknown_setting_stops_the_brain_and_the_scorer_refuses():
    import torch
    with pytest.raises(ValueError, match="drift test"):
        Brain(MemoryStore(), BrainConfig.from_env({"ML_PAIRWISE_DRIFT_TEST": "THEIL_SEN"}), device="cpu")
    with pytest.raises(ValueError, match="min_points"):
        Brain(MemoryStore(), BrainConfig.from_env({**ON, "MIN_DRIFT_DATA_POINTS": "2"}), device="cpu")
    with pytest.raises(ValueError, match="min_tau"):
        Brain(MemoryStore(), BrainConfig.from_env({**ON, "ML_PAIRWISE_DRIFT_MIN_TAU": "2"}), device="cpu")
    # the scorer's rows carry no pod boundaries: it refuses a tick with a baseline and ticks without one as ever
    rng = np.random.default_rng(3)
    hist, cur, base = (torch.from_numpy(rng.normal(100, 5, (1, n)).astype(np.float32)) for n in (600, 80, 80))
    on, off = (CanaryScorer(["error4xx"], BrainConfig.from_env(e), device="cpu") for e in (ON, {}))
    with pytest.raises(ValueError, match="ML_PAIRWISE_DRIFT_TEST"):
        on.score(hist, base, cur, 600)
    with pytest.raises(ValueError, match="ML_PAIRWISE_DRIFT_TEST"):
        CanaryScorer(["error4xx"], BrainConfig.from_env(ON), device="cpu", mode="fused")
    assert torch.equal(on.score(hist, None, cur, 600).packed, off.score(hist, None, cur, 600).packed)
