"""The per-pod test through ``Brain.run_once`` on the fast path (in-memory store).

History N(100, 5); every baseline pod and nine of the ten canary pods sit at
100 +- 2, the tenth canary pod at 113 +- 0.1.  The pooled tests of ``ALL`` do not
all see the one pod in ten, so the threshold stays: 113 lies inside 3 sigma
(115) and outside 0.8 x 3 sigma (112), and the job is healthy with the test off
and unhealthy with ``ML_PAIRWISE_POD_TEST=KRUSKAL_DUNN``.  A job without a
baseline ends the same with the setting on as with it off."""
import zlib

import numpy as np
import pytest

from foremast_amd.config import BrainConfig
from foremast_amd.controller.analyst import AnalystClient
from foremast_amd.engine.brain import Brain
from foremast_amd.engine.exporter import BrainExporter
from foremast_amd.engine.sources import SourceRouter, SyntheticSource
from foremast_amd.ops import reference as ref
from foremast_amd.service.app import create_app
from foremast_amd.service.store import MemoryStore

from test_brain_e2e import Clock
from test_effect_brain import BASE, CANARY, PODS, SEED
from test_scale_brain import _metrics

ON = {"ML_PAIRWISE_POD_TEST": "KRUSKAL_DUNN"}
BAD_POD = 4


class OneBadPod(SyntheticSource):
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
        z = np.sqrt(-2.0 * np.log(ref.u01(h1).astype(np.float64))) * np.cos(2 * np.pi * ref.u01(h2).astype(np.float64))
        gap = (tt / self.step).astype(np.int64) % 11 == 0
        out = np.empty((len(keys), len(tt)), np.float32)
        for i, nk in enumerate(noise_keys):
            _, who = nk.split("|")
            if CANARY in who and int(who[-2:]) == BAD_POD:
                out[i] = np.where(gap, np.nan, 113.0 + 0.1 * z[i])
            elif CANARY in who or BASE in who:
                out[i] = np.where(gap, np.nan, 100.0 + 2.0 * z[i])
            else:
                out[i] = 100.0 + 5.0 * z[i]
        return out


def _setup(env, resident=True):
    clock, store = Clock(), MemoryStore()
    client = AnalystClient.for_app(create_app(store), clock=clock)
    cfg = BrainConfig.from_env({"ML_ALGORITHM": "moving_average_all", **env})
    cfg.hpalog_async = 0
    brain = Brain(store, cfg, device="cpu", sources=SourceRouter(synthetic=OneBadPod(), force="synthetic"), clock=clock,
                  exporter=BrainExporter(), worker_id="w0", resident_history=resident)
    return clock, store, client, brain


def _verdict(env, pods=PODS, strategy="canary", resident=True):
    clock, store, client, brain = _setup(env, resident)
    jid = client.start_analyzing("default", "demo", pods, _metrics(), 10, strategy)
    r = brain.run_once()
    assert r["claimed"] == 1 and r["rows"] == 1 and (not resident or r["fast_jobs"] == 1)
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
    pods, *_ = ref.pairwise_pods(row.cur[None], np.cumsum(row.cur_pods)[None], row.base[None], c.min_pod_points)
    assert ref.pods_verdict(pods, c.pairwise_threshold).all() and pods[0, 4] == BAD_POD and pods[0, 5] == 10


@pytest.mark.parametrize("resident", [True, False])
def test_one_bad_pod_is_unhealthy_only_with_the_setting(resident):
    assert _verdict({}, resident=resident)[0] == "completed_health"
    status, reason = _verdict(ON, resident=resident)
    assert status == "completed_unhealth" and "error4xx" in reason, reason


@pytest.mark.parametrize("strategy", ["rollingUpdate", "continuous", "canary"])
def test_a_job_without_a_baseline_ends_as_with_the_setting_off(strategy):
    assert _verdict(ON, PODS[:1], strategy) == _verdict({}, PODS[:1], strategy)
