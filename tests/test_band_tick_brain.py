"""The brain's route for static groups judged by the static band models with
quantile_robust among them, alone or per metric next to a default: the resident
tick over the store's band-record cache (CanaryScorer(model="band_mix"), K25)
gives the verdicts of the general path and of the op-by-op route it replaces
(FM_BAND_TICK=0); sliding groups and mean + robust mixes keep the op-by-op
route."""
import dataclasses

import numpy as np
import pytest
import torch

from foremast_amd.api import crd
from foremast_amd.engine.fp_models import ModelsMixin

from test_fastpath_models import FAULTS, _brain, _compare, _metrics, _pods, _submit

Q, ROBUST, MEAN = "quantile_robust", "robust_moving_average_all", "moving_average_all"
# (global algorithm, per-metric overrides) -> the codes of error5xx, latency, cpu, memory
FLEETS = {"all_quantile": (Q, {}, (2, 2, 2, 2)),
          "latency": (MEAN, {"latency": Q}, (0, 2, 0, 0)),
          "latency_cpu": (MEAN, {"latency": Q, "cpu": ROBUST}, (0, 2, 1, 0))}


def _fleet_brain(resident, fleet, device):
    algo, rules, _ = FLEETS[fleet]
    x = _brain(resident, algo, FAULTS, device)
    cfg = x[3].cfg
    for alias, a in rules.items():
        cfg.metric_rules[alias] = dataclasses.replace(cfg.rule_for(alias), algorithm=a)
    return x


def _spy(monkeypatch):
    """Counts the groups that enter the op-by-op model path."""
    seen = []
    real = ModelsMixin._score_models

    def spy(self, works, now, ga, store):
        seen.append(works[0].plan.algos)
        return real(self, works, now, ga, store)
    monkeypatch.setattr(ModelsMixin, "_score_models", spy)
    return seen


def _run(monkeypatch, brain, tick: bool):
    if tick:
        monkeypatch.delenv("FM_BAND_TICK", raising=False)
    else:
        monkeypatch.setenv("FM_BAND_TICK", "0")
    try:
        return brain[3].run_once()
    finally:
        monkeypatch.delenv("FM_BAND_TICK", raising=False)


def _parity(monkeypatch, fleet, device):
    a = _fleet_brain(True, fleet, device)                     # the resident band tick
    b = _fleet_brain(False, fleet, device)                    # the general path
    c = _fleet_brain(True, fleet, device)                     # the fast path's op-by-op route
    ids = _submit(a[2], "static")
    assert ids == _submit(b[2], "static") == _submit(c[2], "static")
    seen = _spy(monkeypatch)
    for cyc in range(4):
        before = a[3].fast.band_ticks
        ra = _run(monkeypatch, a, True)
        assert a[3].fast.band_ticks > before and not seen, cyc    # ticked, and no group went op by op
        rb = b[3].run_once()
        rc = _run(monkeypatch, c, False)
        assert seen and c[3].fast.band_ticks == 0
        seen.clear()
        assert ra["claimed"] == rb["claimed"] == rc["claimed"]
        if cyc == 0:
            assert ra["fast_jobs"] == len(ids) == rc["fast_jobs"]
        _compare(a, b, ids, cyc)
        _compare(a, c, ids, cyc)
        for x in (a, b, c):
            x[0].t += 60
    assert crd.PHASE_UNHEALTHY in {a[2].get_status(j).status for j in ids}    # the injected faults are seen
    assert {k[1] for k in a[3].fast.scorers} == {"band_mix"}   # scorers are keyed by (aliases, model)
    assert {sc.codes for sc in a[3].fast.scorers.values()} == {FLEETS[fleet][2]}
    assert a[3].fast.robust_ticks == 0
    return a


@pytest.mark.parametrize("fleet", list(FLEETS))
def test_static_band_jobs_tick_resident_with_the_same_verdicts(monkeypatch, fleet):
    a = _parity(monkeypatch, fleet, "cpu")
    assert a[3].fast.static.bcache is not None


@pytest.mark.gpu
@pytest.mark.parametrize("fleet", list(FLEETS))
def test_gpu_static_band_jobs_tick_resident_with_the_same_verdicts(monkeypatch, cuda, fleet):
    a = _parity(monkeypatch, fleet, "cuda")
    st = a[3].fast.static
    T = st.view().T
    assert st.bcache.T == T and st.bcache.dirty == 0
    v = st.bcache.valid
    tagged = v != 0
    assert int(tagged.sum()) > 0 and bool(((v[tagged] & 0x0FFFFFFF) == T).all())
    assert {int(c) - 1 for c in (v[tagged] >> 28).unique()} == set(FLEETS[fleet][2])
    assert not bool((st.cache.valid != 0).any()) and not bool((st.rcache.valid != 0).any())


def _other_routes(monkeypatch, device):
    seen = _spy(monkeypatch)
    # a continuous job's window slides every cycle: no cache to keep
    a = _brain(True, Q, FAULTS, device)
    b = _brain(False, Q, FAULTS, device)
    ids = _submit(a[2], "continuous")
    assert ids == _submit(b[2], "continuous")
    for cyc in range(3):
        a[3].run_once(), b[3].run_once()
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60
    assert a[3].fast.band_ticks == 0 and seen and all(set(al) == {Q} for al in seen)
    seen.clear()
    # a static mean + robust mix: no quantile_robust metric, the route it had
    m = _brain(True, MEAN, FAULTS, device)
    cfg = m[3].cfg
    cfg.metric_rules["latency"] = dataclasses.replace(cfg.rule_for("latency"), algorithm=ROBUST)
    _submit(m[2], "static")
    for _ in range(2):
        m[3].run_once()
        m[0].t += 60
    assert m[3].fast.band_ticks == 0 and m[3].fast.robust_ticks == 0
    assert seen and all(set(al) == {MEAN, ROBUST} for al in seen)
    seen.clear()
    # quantile_robust next to a model that is no static band model
    f = _brain(True, MEAN, FAULTS, device)
    cfg = f[3].cfg
    cfg.metric_rules["latency"] = dataclasses.replace(cfg.rule_for("latency"), algorithm=Q)
    cfg.metric_rules["cpu"] = dataclasses.replace(cfg.rule_for("cpu"), algorithm="shift_robust")
    _submit(f[2], "static")
    f[3].run_once()
    assert f[3].fast.band_ticks == 0 and seen


def test_sliding_groups_and_other_mixes_keep_the_op_by_op_route(monkeypatch):
    _other_routes(monkeypatch, "cpu")


@pytest.mark.gpu
def test_gpu_sliding_groups_and_other_mixes_keep_the_op_by_op_route(monkeypatch, cuda):
    _other_routes(monkeypatch, "cuda")


@pytest.mark.gpu
def test_gpu_arrival_is_computed_once_and_cached(monkeypatch, cuda):
    """A job that arrives in cycle 3 brings rows without a valid tag into a
    tick shaped for hits; after the cycle every row of the group carries its
    tag and the verdicts are the op-by-op route's."""
    a = _fleet_brain(True, "latency_cpu", "cuda")
    c = _fleet_brain(True, "latency_cpu", "cuda")
    ids = _submit(a[2], "static")
    assert ids == _submit(c[2], "static")
    for cyc in range(4):
        if cyc == 2:
            for x in (a, c):
                ids.append(x[2].start_analyzing("default", "late", [_pods("late", 2, "7687b9f4d"),
                                                                     _pods("late", 2, "5db89899b")],
                                                _metrics(4), 10, "canary"))
            assert ids[-1] == ids[-2]
            ids.pop()
        _run(monkeypatch, a, True)
        _run(monkeypatch, c, False)
        _compare(a, c, ids, cyc)
        if cyc >= 2:
            fast = a[3].fast
            st = fast.static
            T = st.view().T
            late = fast.works[ids[-1]]
            mapped = np.concatenate([ga.rowmap for ga in fast._garr.values()])
            rows = np.unique(mapped)
            assert len(rows) >= 8 and np.isin(late.rows, mapped).all()
            v = st.bcache.valid[torch.from_numpy(rows.astype(np.int64)).to(st.device)]
            assert bool((v != 0).all()) and bool(((v & 0x0FFFFFFF) == T).all()), cyc
        for x in (a, c):
            x[0].t += 60
    assert a[3].fast.band_ticks >= 4 and c[3].fast.band_ticks == 0
