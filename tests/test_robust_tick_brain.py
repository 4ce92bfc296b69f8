"""The brain's route for static robust_moving_average_all groups: the resident
tick over the store's robust row-statistics cache (CanaryScorer(model=...))
gives the verdicts of the general path and of the op-by-op route it replaces
(FM_ROBUST_TICK=0); sliding and mixed-algorithm groups keep the op-by-op
route."""
import dataclasses

import numpy as np
import pytest
import torch

from foremast_amd.engine.fp_models import ModelsMixin

from test_fastpath_models import FAULTS, _brain, _compare, _metrics, _pods, _submit

ROBUST = "robust_moving_average_all"


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
        monkeypatch.delenv("FM_ROBUST_TICK", raising=False)
    else:
        monkeypatch.setenv("FM_ROBUST_TICK", "0")
    try:
        return brain[3].run_once()
    finally:
        monkeypatch.delenv("FM_ROBUST_TICK", raising=False)


def _parity(monkeypatch, device):
    a = _brain(True, ROBUST, FAULTS, device)                  # the resident robust tick
    b = _brain(False, ROBUST, FAULTS, device)                 # the general path
    c = _brain(True, ROBUST, FAULTS, device)                  # the fast path's op-by-op route
    ids = _submit(a[2], "static")
    assert ids == _submit(b[2], "static") == _submit(c[2], "static")
    seen = _spy(monkeypatch)
    for cyc in range(4):
        before = a[3].fast.robust_ticks
        ra = _run(monkeypatch, a, True)
        assert a[3].fast.robust_ticks > before and not seen, cyc   # ticked, and no group went op by op
        rb = b[3].run_once()
        rc = _run(monkeypatch, c, False)
        assert seen and c[3].fast.robust_ticks == 0
        seen.clear()
        assert ra["claimed"] == rb["claimed"] == rc["claimed"]
        if cyc == 0:
            assert ra["fast_jobs"] == len(ids) == rc["fast_jobs"]
        _compare(a, b, ids, cyc)
        _compare(a, c, ids, cyc)
        for x in (a, b, c):
            x[0].t += 60
    from foremast_amd.api import crd
    assert crd.PHASE_UNHEALTHY in {a[2].get_status(j).status for j in ids}    # the injected faults are seen
    assert {k[1] for k in a[3].fast.scorers} == {ROBUST}       # scorers are keyed by (aliases, model)
    return a


def test_static_robust_jobs_tick_resident_with_the_same_verdicts(monkeypatch):
    a = _parity(monkeypatch, "cpu")
    assert a[3].fast.static.rcache is not None


@pytest.mark.gpu
def test_gpu_static_robust_jobs_tick_resident_with_the_same_verdicts(monkeypatch, cuda):
    a = _parity(monkeypatch, "cuda")
    st = a[3].fast.static
    assert st.rcache.T == st.view().T and st.rcache.dirty == 0
    assert int((st.rcache.valid == st.view().T).sum()) > 0 and not bool((st.cache.valid != 0).any())


def _other_routes(monkeypatch, device):
    seen = _spy(monkeypatch)
    # a continuous job's window slides every cycle: no cache to keep
    a = _brain(True, ROBUST, FAULTS, device)
    b = _brain(False, ROBUST, FAULTS, device)
    ids = _submit(a[2], "continuous")
    assert ids == _submit(b[2], "continuous")
    for cyc in range(3):
        a[3].run_once(), b[3].run_once()
        _compare(a, b, ids, cyc)
        a[0].t += 60
        b[0].t += 60
    assert a[3].fast.robust_ticks == 0 and seen and all(set(al) == {ROBUST} for al in seen)
    seen.clear()
    # a static group with two models among its metrics
    m = _brain(True, "moving_average_all", FAULTS, device)
    cfg = m[3].cfg
    cfg.metric_rules["latency"] = dataclasses.replace(cfg.rule_for("latency"), algorithm=ROBUST)
    _submit(m[2], "static")
    for _ in range(2):
        m[3].run_once()
        m[0].t += 60
    assert m[3].fast.robust_ticks == 0 and seen and all(len(set(al)) == 2 for al in seen)


def test_sliding_and_mixed_groups_keep_the_op_by_op_route(monkeypatch):
    _other_routes(monkeypatch, "cpu")


@pytest.mark.gpu
def test_gpu_sliding_and_mixed_groups_keep_the_op_by_op_route(monkeypatch, cuda):
    _other_routes(monkeypatch, "cuda")


@pytest.mark.gpu
def test_gpu_arrival_is_selected_once_and_cached(monkeypatch, cuda):
    """A job that arrives in cycle 3 brings rows without a valid tag into a
    tick shaped for hits; after the cycle every row of the group is tagged and
    the verdicts are the op-by-op route's."""
    a = _brain(True, ROBUST, FAULTS, "cuda")
    c = _brain(True, ROBUST, FAULTS, "cuda")
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
            assert bool((st.rcache.valid[torch.from_numpy(rows.astype(np.int64)).to(st.device)] == T).all()), cyc
        for x in (a, c):
            x[0].t += 60
    assert a[3].fast.robust_ticks >= 4 and c[3].fast.robust_ticks == 0
