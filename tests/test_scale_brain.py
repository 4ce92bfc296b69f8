"""The pairwise scale test through ``Brain.run_once`` (in-memory store).

History N(100, 5); the baseline pods sit at 100 +- 5 and the canary pods at
100 +- 13 (half of the pods on either side, a little noise on top), so both
windows have the same median and mean, no location test of ``ALL`` sees a
difference, and the threshold stays.  At the metric's default threshold 3, 113
lies inside 3 sigma (115) and outside 0.8 x 3 sigma (112): the job is healthy
with the test off and unhealthy with ``ML_PAIRWISE_SCALE_TEST=BROWN_FORSYTHE``,
which finds the spread 2.6 times the baseline's and lowers the threshold.  The
only difference between the runs is the environment handed to ``BrainConfig``."""
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

from test_brain_e2e import Clock
from test_effect_brain import BASE, CANARY, PODS, SEED

HIST_SD, BASE_AMP, CUR_AMP, NOISE = 5.0, 5.0, 13.0, 0.1
ON = {"ML_PAIRWISE_SCALE_TEST": "BROWN_FORSYTHE"}


def _metrics():
    # error4xx: default threshold 3, upper bound only
    return crd.Metrics("prometheus", "http://prom/api/v1/", [
        crd.Monitoring("http_server_requests_errors_4xx", "gauge", "error4xx")])


class JitteryCanary(SyntheticSource):
    """History (app level) N(100, HIST_SD); pod k of a side sits at 100 + amp
    (k even) or 100 - amp (k odd) with NOISE N(0, 1) on top, amp = BASE_AMP for
    the baseline pods and CUR_AMP for the canary pods; counter-based noise, so
    a sample is the same in whichever window and batch it is asked for.  Every
    11th grid sample of a pod is missing (NaN), so a 10-minute window has
    exactly 10 finite samples per pod: 50 high and 50 low per side."""

    def __init__(self, cur_amp=CUR_AMP):
        super().__init__()
        self.cur_amp = float(cur_amp)

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
            if CANARY in who or BASE in who:
                amp = self.cur_amp if CANARY in who else BASE_AMP
                sign = 1.0 if int(who[-2:]) % 2 == 0 else -1.0
                out[i] = np.where(gap, np.nan, 100.0 + sign * amp + NOISE * z[i])
            else:
                out[i] = 100.0 + HIST_SD * z[i]
        return out


def _env(algo, **settings):
    env = {"ML_ALGORITHM": algo}
    env.update({k: str(v) for k, v in settings.items()})
    return env


def _setup(env, device="cpu", resident=True, amp=CUR_AMP):
    clock = Clock()
    store = MemoryStore()
    client = AnalystClient.for_app(create_app(store), clock=clock)
    cfg = BrainConfig.from_env(env)
    cfg.hpalog_async = 0
    src = SourceRouter(synthetic=JitteryCanary(amp), force="synthetic")
    brain = Brain(store, cfg, device=device, sources=src, clock=clock, exporter=BrainExporter(), worker_id="w0",
                  resident_history=resident)
    return clock, store, client, brain


def _rows(env, amp):
    clock, store, client, brain = _setup(env, amp=amp)
    client.start_analyzing("default", "demo", PODS, _metrics(), 10, "canary")
    return brain, brain._fetch_job(store.claim("w0", 1, 90, now=clock())[0], clock()).rows


def _preconditions(algo, amp):
    """On the references, over the very rows the brain scores: the same median,
    no location verdict, a scale verdict; every canary sample between the
    lowered and the full band (above) or far inside (below)."""
    b0, rows = _rows(_env(algo), amp)
    b1, rows1 = _rows(_env(algo, **ON), amp)
    cur = np.stack([r.cur for r in rows]).astype(np.float32)
    base = np.stack([r.base for r in rows]).astype(np.float32)
    assert cur.shape == base.shape == (1, 110)
    assert (np.isfinite(cur).sum(1) == 100).all() and (np.isfinite(base).sum(1) == 100).all()
    c = BrainConfig()
    assert c.rule_for(rows[0].alias).threshold == 3.0
    _, _, diff = ref.pairwise_tests(cur, base, 63, 0, c.pairwise_threshold, c.min_mann_white, c.min_wilcoxon,
                                    c.min_kruskal)
    assert not diff.any()
    s = ref.pairwise_scale(cur, base, c.min_scale_points)
    assert ref.scale_verdict(s, c.pairwise_threshold).all() and s[0, 1] < 1e-6 and abs(s[0, 2] - amp / BASE_AMP) < 0.1
    assert abs(s[0, 3] - s[0, 4]) < 0.5 and abs(s[0, 3] - 100) < 0.5
    full, low = b0.score_rows(rows), b1.score_rows(rows1)
    assert not full["diff"].any() and low["diff"].all()
    up_full, up_low = float(full["upper"][0].reshape(-1)[0]), float(low["upper"][0].reshape(-1)[0])
    hi = cur[0][cur[0] > 100]
    assert len(hi) == 50 and up_low + 0.2 < hi.min() and hi.max() < up_full - 0.2, (up_low, hi.min(), hi.max(), up_full)


def _verdict(env, device="cpu", resident=True, amp=CUR_AMP):
    clock, store, client, brain = _setup(env, device, resident, amp)
    jid = client.start_analyzing("default", "demo", PODS, _metrics(), 10, "canary")
    r = brain.run_once()
    assert r["claimed"] == 1 and r["rows"] == 1
    if resident:
        assert r["fast_jobs"] == 1
    first = store.get(jid).status
    if first.startswith("completed"):
        return first, client.get_status(jid)
    clock.t += 11 * 60
    brain.run_once()
    return store.get(jid).status, client.get_status(jid)


def _jitter(algo, device="cpu", resident=True, amp=CUR_AMP):
    _preconditions(algo, amp)
    s0, st0 = _verdict(_env(algo), device, resident, amp)
    assert s0 == "completed_health" and st0.status == crd.PHASE_HEALTHY, st0.reason
    s0b, _ = _verdict(_env(algo, ML_PAIRWISE_SCALE_TEST="OFF"), device, resident, amp)
    assert s0b == s0
    s1, st1 = _verdict(_env(algo, **ON), device, resident, amp)
    assert s1 == "completed_unhealth" and st1.status == crd.PHASE_UNHEALTHY
    assert set(st1.anomaly) == {"error4xx"} and "error4xx" in st1.reason, st1.reason
    return s0, s1, sorted(st1.anomaly)


def test_jittery_canary_is_healthy_without_and_unhealthy_with_the_scale_test():
    _jitter("moving_average_all")


def test_jittery_canary_general_path_agrees_with_the_fast_path():
    assert _jitter("moving_average_all", resident=False) == _jitter("moving_average_all")


def test_jittery_canary_op_by_op_model():
    """The rolling median/MAD band of this model is tighter than the whole history's: canary pods at 100 +- 9."""
    _jitter("robust_moving_average", amp=9.0)


def test_a_wrong_setting_stops_the_brain_at_start_up():
    for bad in ({"ML_PAIRWISE_SCALE_TEST": "ANSARI"}, dict(ON, ML_PAIRWISE_SCALE_MIN_RATIO="0.9")):
        with pytest.raises(ValueError):
            _setup(_env("moving_average_all", **bad))


@pytest.mark.gpu
def test_gpu_resident_fast_path_gives_the_cpu_verdicts(cuda):
    assert _jitter("moving_average_all", device=cuda) == _jitter("moving_average_all")
    assert _jitter("robust_moving_average", device=cuda, amp=9.0) == _jitter("robust_moving_average", amp=9.0)
