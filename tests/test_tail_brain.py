"""The tail test through ``Brain.run_once`` and ``Brain.score_rows`` (in-memory store).

History N(100, 5); error4xx, threshold 3, upper bound only.  Both windows of a
job hold 100 + SD z with z standard normal from a fixed-seed table, 300 finite
samples a side, so samples between 0.8 x 3 sigma (112) and 3 sigma (115) occur
on both sides and the job's health hangs on the pairwise verdict alone.  The
stretched canary's upper fifth lies 0.6 SD further out (a lognormal(4, 0.3)
latency whose upper fifth is stretched by 1.2, in log units): no test of
``ALL`` sees a difference, ``ML_PAIRWISE_TAIL_TEST=EXCEEDANCE`` does and lowers
the threshold."""
import numpy as np
import pytest

from foremast_amd.config import BrainConfig
from foremast_amd.controller.analyst import AnalystClient
from foremast_amd.engine.brain import Brain
from foremast_amd.engine.exporter import BrainExporter
from foremast_amd.engine.scorer import CanaryScorer
from foremast_amd.engine.sources import SourceRouter, SyntheticSource
from foremast_amd.ops import reference as ref
from foremast_amd.service.app import create_app
from foremast_amd.service.store import MemoryStore

from test_brain_e2e import Clock
from test_effect_brain import BASE, CANARY, PODS
from test_scale_brain import _metrics

ON = {"ML_PAIRWISE_TAIL_TEST": "EXCEEDANCE"}
SD, WINDOW_MIN = 4.0, 30
KINDS = ("stretched", "halved", "spike", "collapsed")


class TailCanary(SyntheticSource):
    """Pod k of a side reads row k of a fixed-seed table of standard normals by
    the sample's grid index; every 31st grid sample of a pod is missing, so a
    30-minute window has 30 finite samples per pod.  The canary's z are changed
    by ``kind`` relative to the canary's own quantiles over the whole table."""

    def __init__(self, kind):
        super().__init__()
        rng = np.random.default_rng(32)
        self.z = rng.standard_normal((2, 10, 4096))
        c = self.z[0]
        if kind == "stretched":                                # the upper fifth moves out by 0.6
            c[c > np.quantile(c, 0.8)] += 0.6
        if kind == "halved":                                   # the spread halves about the median: harmless
            c *= 0.5
        if kind == "collapsed":                                # the lower fifth drops by 0.6: the metric judges no lower bound
            c[c < np.quantile(c, 0.2)] -= 0.6
        self.kind = kind

    def prepare(self, keys, noise_keys, fault_keys):
        return None

    def many(self, keys, noise_keys, fault_keys, t, stream=0):
        tt = np.asarray(t, np.float64)
        ti = (tt / self.step).astype(np.int64)
        out = np.empty((len(keys), len(tt)), np.float32)
        hist = np.random.default_rng(5).standard_normal(4096)
        for i, nk in enumerate(noise_keys):
            _, who = nk.split("|")
            if CANARY in who or BASE in who:
                z = self.z[0 if CANARY in who else 1, int(who[-2:])][ti % 4096]
                out[i] = np.where(ti % 31 == 0, np.nan, 100.0 + SD * z)
            else:
                out[i] = 100.0 + 5.0 * hist[ti % 4096]
        return out


def _setup(env, kind, device="cpu"):
    clock, store = Clock(), MemoryStore()
    client = AnalystClient.for_app(create_app(store), clock=clock)
    cfg = BrainConfig.from_env({"ML_ALGORITHM": "moving_average_all", **env})
    cfg.hpalog_async = 0
    brain = Brain(store, cfg, device=device, sources=SourceRouter(synthetic=TailCanary(kind), force="synthetic"),
                  clock=clock, exporter=BrainExporter(), worker_id="w0")
    return clock, store, client, brain


def _verdict(env, kind, device="cpu"):
    clock, store, client, brain = _setup(env, kind, device)
    jid = client.start_analyzing("default", "demo", PODS, _metrics(), WINDOW_MIN, "canary")
    r = brain.run_once()
    assert r["claimed"] == 1 and r["rows"] == 1 and r["fast_jobs"] == 1
    if not store.get(jid).status.startswith("completed"):
        clock.t += (WINDOW_MIN + 1) * 60
        brain.run_once()
    return store.get(jid).status, client.get_status(jid).reason


def _row(kind):
    clock, store, client, brain = _setup({}, kind)
    client.start_analyzing("default", "demo", PODS, _metrics(), WINDOW_MIN, "canary")
    row, = brain._fetch_job(store.claim("w0", 1, 90, now=clock())[0], clock()).rows
    if kind == "spike":                                        # one sample x 100: noise, not a regression
        row.cur[int(np.flatnonzero(np.isfinite(row.cur))[7])] *= 100
    return brain, row


@pytest.mark.parametrize("kind", KINDS)
def test_preconditions_on_the_rows_the_brain_scores(kind):
    """K4 says "same" on every fixture; the reference tail p-value is clear of
    the threshold: below it for the stretched canary, above it (or no test at
    all on the side the metric judges) for the rest."""
    _, row = _row(kind)
    c = BrainConfig()
    assert np.isfinite(row.cur).sum() == np.isfinite(row.base).sum() == 300
    _, _, diff = ref.pairwise_tests(row.cur[None], row.base[None], 63, 0, c.pairwise_threshold, c.min_mann_white,
                                    c.min_wilcoxon, c.min_kruskal)
    tail, which, J, _, counts = ref.pairwise_tail(row.cur[None], row.base[None], (9000, 9500, 9900), "BOUND", [1],
                                                  c.min_tail_data_points, c.min_tail_points)
    assert not counts[0, 1].any() and J[0] >= 2                # error4xx: the upper side alone
    if kind == "stretched":
        assert not diff.any() and tail[0, 0] < 0.01 and tail[0, 2] > 0.03
    else:
        assert tail[0, 0] > 0.2
    if kind == "collapsed":                                    # the lower side would see it
        assert ref.pairwise_tail(row.cur[None], row.base[None], (9000, 9500, 9900), "LOWER")[0][0, 0] < 0.01


@pytest.mark.parametrize("kind", KINDS)
def test_only_the_stretched_tail_is_different_with_the_setting(kind):
    brain, row = _row(kind)
    on = Brain(MemoryStore(), BrainConfig.from_env({"ML_ALGORITHM": "moving_average_all", **ON}), device="cpu",
               resident_history=False)
    off, with_it = brain.score_rows([row])["diff"].tolist(), on.score_rows([row])["diff"].tolist()
    assert with_it == ([1] if kind == "stretched" else off)


def test_stretched_canary_is_unhealthy_only_with_the_setting():
    assert _verdict({}, "stretched")[0] == "completed_health"
    assert _verdict({"ML_PAIRWISE_TAIL_TEST": "OFF"}, "stretched")[0] == "completed_health"
    status, reason = _verdict(ON, "stretched")
    assert status == "completed_unhealth" and "error4xx" in reason, reason
    for kind in ("halved", "collapsed"):
        assert _verdict(ON, kind)[0] == "completed_health"


@pytest.mark.gpu
def test_gpu_resident_fast_path_gives_the_cpu_verdicts(cuda):
    assert _verdict({}, "stretched", cuda) == _verdict({}, "stretched")
    assert _verdict(ON, "stretched", cuda) == _verdict(ON, "stretched")


def test_unknown_setting_stops_the_brain_and_the_scorer_refuses():
    import torch
    for bad, what in (({"ML_PAIRWISE_TAIL_TEST": "HILL"}, "tail test"), ({**ON, "ML_PAIRWISE_TAIL_SIDES": "INNER"}, "sides"),
                      ({**ON, "ML_PAIRWISE_TAIL_QUANTILES": "0.99,0.9"}, "quantiles"),
                      ({**ON, "MIN_TAIL_DATA_POINTS": "1"}, "min_points"), ({**ON, "MIN_TAIL_POINTS": "0"}, "min_tail"),
                      ({**ON, "ML_PAIRWISE_TAIL_MIN_EXCESS": "1"}, "min_excess")):
        with pytest.raises(ValueError, match=what):
            Brain(MemoryStore(), BrainConfig.from_env(bad), device="cpu")
    rng = np.random.default_rng(3)
    hist, cur, base = (torch.from_numpy(rng.normal(100, 5, (1, n)).astype(np.float32)) for n in (600, 80, 80))
    on, off = (CanaryScorer(["error4xx"], BrainConfig.from_env(e), device="cpu") for e in (ON, {}))
    with pytest.raises(ValueError, match="ML_PAIRWISE_TAIL_TEST"):
        on.score(hist, base, cur, 600)
    with pytest.raises(ValueError, match="ML_PAIRWISE_TAIL_TEST"):
        CanaryScorer(["error4xx"], BrainConfig.from_env(ON), device="cpu", mode="fused")
    assert torch.equal(on.score(hist, None, cur, 600).packed, off.score(hist, None, cur, 600).packed)
