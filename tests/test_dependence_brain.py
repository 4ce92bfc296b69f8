"""The dependence gate through ``Brain.run_once`` (the fast path's op-by-op
route), ``Brain.score_rows`` (the general path) and ``CanaryScorer``.

History N(100, 5).  The 4 canary and the 4 baseline pods are one AR(1) process
(rho = 0.8) around 113.5, 31 samples a pod: nothing differs, yet at this seed
``ALL`` calls the canary "different", which lowers the threshold from 3 sigma
(114.9) to 0.8 x 3 sigma (111.9), below the samples: unhealthy.  Under
``ML_PAIRWISE_DEPENDENCE=RANK_ACF`` the verdict is cleared and the job healthy;
the same canary 0.25 higher (a real shift, inside 3 sigma) keeps its verdict."""
import zlib

import numpy as np
import pytest
import torch

from foremast_amd.config import BrainConfig
from foremast_amd.controller.analyst import AnalystClient
from foremast_amd.engine.brain import Brain, Row
from foremast_amd.engine.exporter import BrainExporter
from foremast_amd.engine.scorer import CanaryScorer
from foremast_amd.engine.sources import SourceRouter, SyntheticSource
from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref
from foremast_amd.service.app import create_app
from foremast_amd.service.store import MemoryStore

from test_brain_e2e import Clock
from test_effect_brain import BASE, CANARY
from test_scale_brain import _metrics

ON = {"ML_PAIRWISE_DEPENDENCE": "RANK_ACF"}
PODS = [[f"demo-{CANARY}-aaa{k:02d}" for k in range(4)], [f"demo-{BASE}-bbb{k:02d}" for k in range(4)]]


class AutocorrelatedCanary(SyntheticSource):
    """Counter-based noise as test_drift_brain.CreepingCanary; a pod's series is AR(1) as a 40-term moving average."""

    def __init__(self, shift=0.0):
        super().__init__()
        self.shift = float(shift)

    def prepare(self, keys, noise_keys, fault_keys):
        return None

    def many(self, keys, noise_keys, fault_keys, t, stream=0):
        kh = np.array([zlib.crc32(k.encode()) ^ 1 for k in noise_keys], np.uint32)[:, None]
        ti = (np.asarray(t, np.float64) / self.step).astype(np.int64)

        def z(idx):
            h1 = ref.hash3(kh, (idx & 0xFFFFFFFF).astype(np.uint32)[None, :], np.uint32(0xE4FEC7))
            h2 = ref.hash_u32(h1 ^ np.uint32(0x68E31DA4)).reshape(h1.shape)
            return np.sqrt(-2.0 * np.log(ref.u01(h1).astype(np.float64))) * np.cos(2 * np.pi * ref.u01(h2).astype(np.float64))

        ar, white = sum(0.8 ** j * z(ti - j) for j in range(40)) * 0.6, z(ti)
        out = np.empty((len(keys), len(ti)), np.float32)
        for i, nk in enumerate(noise_keys):
            who = nk.split("|")[1]
            out[i] = (113.5 + self.shift * (CANARY in who) + 0.45 * ar[i] if CANARY in who or BASE in who
                      else 100.0 + 5.0 * white[i])
        return out


def _both_paths(env, shift=0.0, device="cpu"):
    """(the job's end through run_once's fast path, the general path's diff of the row that job fetches)."""
    out = []
    for general in (False, True):
        clock, store = Clock(), MemoryStore()
        client = AnalystClient.for_app(create_app(store), clock=clock)
        cfg = BrainConfig.from_env({"ML_ALGORITHM": "moving_average_all", **env})
        cfg.hpalog_async = 0
        brain = Brain(store, cfg, device=device, clock=clock, exporter=BrainExporter(), worker_id="w0",
                      sources=SourceRouter(synthetic=AutocorrelatedCanary(shift), force="synthetic"))
        jid = client.start_analyzing("default", "demo", PODS, _metrics(), 30, "canary")
        if general:
            row, = brain._fetch_job(store.claim("w0", 1, 90, now=clock())[0], clock()).rows
            assert row.cur_pods.tolist() == [31] * 4 and len(row.base) == 124
            assert row.cur.max() < 114.9          # inside 3 sigma of this history (114.93): only a verdict flags it
            out.append(brain.score_rows([row])["diff"].tolist())
        else:
            r = brain.run_once()
            assert r["claimed"] == 1 and r["rows"] == 1 and r["fast_jobs"] == 1
            if not store.get(jid).status.startswith("completed"):
                clock.t += 31 * 60
                brain.run_once()
            out.append(store.get(jid).status)
    return tuple(out)


def test_gate_clears_the_false_verdict_on_the_fast_path_and_the_general_path():
    assert _both_paths({}) == _both_paths({"ML_PAIRWISE_DEPENDENCE": "OFF"}) == ("completed_unhealth", [1])
    assert _both_paths(ON) == ("completed_health", [0])
    assert _both_paths(ON, shift=0.25) == _both_paths({}, shift=0.25) == ("completed_unhealth", [1])


@pytest.mark.gpu
def test_gpu_gives_the_cpu_verdicts(cuda):
    for env, shift in (({}, 0.0), (ON, 0.0), (ON, 0.25)):
        assert _both_paths(env, shift, cuda) == _both_paths(env, shift)


def _score(env, cur, base):
    rng = np.random.default_rng(1)
    brain = Brain(MemoryStore(), BrainConfig.from_env({"ML_ALGORITHM": "moving_average_all", **env}), device="cpu",
                  resident_history=False)
    row = Row(0, "error4xx", "m", rng.normal(100, 5, 600).astype(np.float32), 0.0, cur, np.zeros(0), base,
              cur_pods=np.asarray([30] * 4, np.int64))
    return brain.score_rows([row])["diff"].tolist()


def test_a_drift_verdict_survives_the_gate_and_off_is_the_identity():
    from test_dependence_ops import _ar1
    rng = np.random.default_rng(1)
    cur = (100 + _ar1(rng, 0.7, (4, 30)).reshape(120)).astype(np.float32)
    base = (100 + _ar1(rng, 0.7, (120,))).astype(np.float32)
    creep = (cur + np.tile(np.linspace(-1.5, 1.5, 30), 4)).astype(np.float32)     # every pod creeps; the level stays
    assert _score({}, cur, base) == [1] and _score(ON, cur, base) == [0] and _score(ON, creep, base) == [0]
    assert _score({**ON, "ML_PAIRWISE_DRIFT_TEST": "MANN_KENDALL"}, creep, base) == [1]
    d = torch.tensor([1], dtype=torch.int8)
    seg = torch.tensor([[30, 60, 90, 120]], dtype=torch.int32)
    assert C.dependence_diff(d, torch.from_numpy(cur)[None], seg, torch.from_numpy(base)[None],
                             C.DependenceGate("OFF")) is d


def test_wrong_settings_stop_the_brain_and_the_scorer_refuses():
    for bad in ({"ML_PAIRWISE_DEPENDENCE": "NEWEY_WEST"}, {"ML_PAIRWISE_ACF_MAX_LAG": "17"}, {"MIN_ACF_DATA_POINTS": "3"}):
        with pytest.raises(ValueError):
            Brain(MemoryStore(), BrainConfig.from_env(bad), device="cpu")
    rng = np.random.default_rng(3)
    hist, cur, base = (torch.from_numpy(rng.normal(100, 5, (1, n)).astype(np.float32)) for n in (600, 80, 80))
    on, off = (CanaryScorer(["error4xx"], BrainConfig.from_env(e), device="cpu") for e in (ON, {}))
    with pytest.raises(ValueError, match="ML_PAIRWISE_DEPENDENCE"):
        on.score(hist, base, cur, 600)
    with pytest.raises(ValueError, match="ML_PAIRWISE_DEPENDENCE"):
        CanaryScorer(["error4xx"], BrainConfig.from_env(ON), device="cpu", mode="fused")
    assert torch.equal(on.score(hist, None, cur, 600).packed, off.score(hist, None, cur, 600).packed)
