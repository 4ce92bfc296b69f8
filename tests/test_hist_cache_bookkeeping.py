"""Host bookkeeping of the row-statistics cache of a static ResidentHistory
(engine/resident.py RowStatsCache): every writer of a row clears exactly that
row's validity word, growing the store keeps the words, and a sliding store
has no cache.  Runs on the CPU: the words are marked valid by hand, as the
statistics kernel would."""
from types import SimpleNamespace

import numpy as np
import torch

from foremast_amd.engine.resident import ResidentHistory

T = 40
TAG = 40


def _store(n: int) -> tuple[ResidentHistory, np.ndarray]:
    st = ResidentHistory(T, "cpu")
    rows, new = st.rows_for([("k", i) for i in range(n)], owner=("ns", "app"))
    assert new.all()
    rng = np.random.default_rng(1)
    st.write_static(rows, [rng.normal(size=T).astype(np.float32) for _ in rows], np.zeros(len(rows)))
    return st, rows


def _mark_valid(st: ResidentHistory) -> None:
    st.cache.valid.fill_(TAG)
    st.cache.ticked(TAG)


def _cleared(st: ResidentHistory) -> list[int]:
    return torch.nonzero(st.cache.valid == 0).flatten().tolist()


def test_write_static_clears_exactly_the_written_rows():
    st, rows = _store(12)
    assert len(st.cache) == st.buf.shape[0]
    assert _cleared(st) == list(range(len(st.cache)))        # nothing computed yet
    _mark_valid(st)
    assert not st.cache.expect_miss(TAG, 12)
    w = rows[[2, 5, 7]]
    st.write_static(w, [np.ones(T, np.float32)] * 3, np.zeros(3))
    assert _cleared(st) == sorted(int(r) for r in w)
    assert st.cache.dirty == 3


def test_release_clears_exactly_the_released_rows():
    st, rows = _store(12)
    _mark_valid(st)
    assert st.release([("k", 3), ("k", 9), ("absent", 0)]) == 2
    assert _cleared(st) == sorted(int(rows[i]) for i in (3, 9))
    # the freed slots are reused by new keys, written, and stay invalid until the next tick
    r2, new = st.rows_for([("n", 0), ("n", 1)])
    assert new.all() and set(r2.tolist()) == {int(rows[3]), int(rows[9])}
    st.write_static(r2, [np.zeros(T, np.float32)] * 2, np.zeros(2))
    assert _cleared(st) == sorted(r2.tolist())


def test_checkpoint_restore_clears_exactly_the_restored_rows():
    from foremast_amd.engine.fp_history import load_history
    st, rows = _store(12)
    _mark_valid(st)
    keys = [["k", 1], ["k", 4], ["r", 0]]                    # two rows overwritten in place, one new
    vals = torch.arange(3 * T, dtype=torch.float32).reshape(3, T)
    t = {"static.values": vals, "static.last_t": torch.zeros(3, dtype=torch.float64),
         "static.nlen": torch.full((3,), T, dtype=torch.int64)}
    meta = {"static.keys": keys, "static.owners": [["ns", "app"]] * 3}
    fp = SimpleNamespace(static=st, sliding=None, cycle=0, history_s=0.0)
    assert load_history(fp, t, meta, now=0.0) == 3
    want = sorted([int(rows[1]), int(rows[4]), st.slot[("r", 0)]])
    assert _cleared(st) == want
    assert torch.equal(st.buf[int(rows[1]), :T], vals[0]) and torch.equal(st.buf[st.slot[("r", 0)], :T], vals[2])


def test_grow_preserves_the_words_and_the_statistics():
    st, rows = _store(12)
    _mark_valid(st)
    st.cache.stats.copy_(torch.arange(len(st.cache) * 3, dtype=torch.float32).reshape(-1, 3))
    before_v, before_s = st.cache.valid.clone(), st.cache.stats.clone()
    n0 = len(st.cache)
    st.rows_for([("g", i) for i in range(n0 + 50)])          # forces _grow
    assert st.buf.shape[0] > n0 and len(st.cache) == st.buf.shape[0]
    assert torch.equal(st.cache.valid[:n0], before_v) and torch.equal(st.cache.stats[:n0], before_s)
    assert not st.cache.valid[n0:].any()                     # new rows start invalid


def test_sliding_store_has_no_cache():
    st = ResidentHistory(T, "cpu", sliding=True, slack=8, capacity=16)
    assert st.cache is None and st.view().cache is None
    st.advance(T * 60.0)
    rows, _ = st.rows_for([("s", 0), ("s", 1)])
    st.write_sliding_dense(rows, np.arange(T) * 60.0 + 60.0, np.ones((2, T), np.float32))
    st.touch(rows)                                           # a no-op, not an allocation
    st.release([("s", 0)])
    assert st.cache is None and st.view().cache is None


def test_view_length_change_expects_misses():
    st, rows = _store(4)
    st.cache.ticked(st.view().T)
    assert not st.cache.expect_miss(st.view().T, 4)
    assert st.cache.expect_miss(st.view().T + 1, 4)          # max_len grew: the tag differs everywhere
