"""Device-resident history rows of the brain (HBM as the series cache).

The reference brain re-queries the whole 7-day history of every metric of
every job on every cycle (foremast-barrelman/pkg/client/metrics/metricsquery.go:93-99
builds a now-7d..now ``historical`` query; the brain re-reads it per cycle,
docs/guides/design.md:31-43).  At fleet scale that is 80k x 10,080 samples =
3.2 GB per cycle, i.e. ~60 ms of host->device copy before any scoring.  Here
each history row is fetched ONCE and stays in device memory (288 GB of HBM3E
holds ~90x the 10k x 8 fleet); a cycle only appends the samples that arrived
since the row's newest one, and the scoring kernels read the rows in place
through a row map (the ``rowmap`` of ``fm_tick_front`` / ``fm_hist_stats_cached``).

Two layouts:

* ``static`` — a row is a fixed window written once, LEFT-aligned (samples
  from column 0, NaN after): the absolute-time ``historical`` query of a
  canary / rolling update job never changes while the job is re-examined.
  The scored view is ``[0, longest row)``, so a complete row holds no missing
  sample inside the view and the row-stats kernel keeps its unmasked fast
  path (right-aligned rows carried up to 3 NaN of alignment padding in front
  of every 7-day window, which sent every row down the masked path).
* ``sliding`` — every row lives on one global time grid (column c = time
  t0 + c*step) and the window is the last ``T`` columns before "now".  When
  time advances the window start moves right (a view offset, no data moved);
  the columns that fall out of the window are overwritten with NaN, and the
  buffer is compacted back to column 0 only when its right-hand slack runs
  out (once every ``slack`` steps).  Continuous / HPA jobs, whose queries use
  the ``START_TIME``/``END_TIME`` placeholders, live here; each cycle fetches
  only ``(last_t, now]``.

moving_average_all (the deployed default, foremast-brain.yaml:24-25) skips
non-finite samples, so a row's statistics depend only on which samples sit in
its window, not on their column: both layouts reproduce the per-cycle
re-fetch exactly, and the statistics kernels read rows in place.  Models
whose output depends on sample position (exponential smoothing /
Holt-Winters, Prophet, LSTM, bivariate) read each row right-aligned at its
newest sample: ``fm_gather_cols`` (csrc/kernels/gather.hip) copies exactly
the columns a model needs (``nlen`` locates a static row's end; a sliding
row ends at the window end), so a cached fit advanced over k new samples
moves k columns per row, not the 7-day window.  ``nfin`` counts each row's
finite samples in the window (the ``MIN_HISTORICAL_DATA_POINT_TO_MEASURE``
gate) without reading the row.
"""
from __future__ import annotations

import math
from dataclasses import dataclass

import numpy as np
import torch

from . import native_rt


def _ceil4(x: int) -> int:
    return (x + 3) // 4 * 4


class RowStatsCache:
    """Per-row (mean, std, n) -- or, in a store's second cache, the robust
    (median, sigma, n) -- of a history tensor whose rows are written once
    and scored many times, kept by the statistics kernels themselves
    (csrc/include/fm_row_stats.h): ``stats[p]`` are the three floats the
    kernel computed for physical row ``p``, ``valid[p]`` the view length they
    were computed for (0 = invalid).  Whoever writes a row clears its word,
    on the stream of the write (:meth:`touch` / :meth:`invalidate`); the next
    tick recomputes exactly those rows.

    ``dirty`` is the host's count of words cleared since the last tick.  It
    only shapes that tick's launch (:meth:`expect_miss`); what is recomputed
    is decided on the device, word by word.

    ``width=4`` is the cache of the static band models' records (K25,
    ``ops.misc.band_stats_cached``): (centre, sigma_lo, sigma_up, n) per row,
    16-byte entries, the word a tag of model and view length.  Such a cache
    also remembers the ``quantile_robust`` tail parameter its entries were made
    with (:meth:`rekey`)."""

    def __init__(self, rows: int, device, width: int = 3):
        self.device = torch.device(device)
        self.width = int(width)
        self.stats = torch.empty((rows, self.width), dtype=torch.float32, device=self.device)
        self.valid = torch.zeros((rows,), dtype=torch.int32, device=self.device)
        self.dirty = rows
        self.T = 0                                  # view length of the last tick
        self.z0: float | None = None                # width 4: tail parameter of the quantile_robust entries

    def __len__(self) -> int:
        return self.valid.numel()

    def grow(self, rows: int) -> None:
        """More rows; the existing entries stay (the row data is copied)."""
        n = len(self)
        if rows <= n:
            return
        stats = torch.empty((rows, self.width), dtype=torch.float32, device=self.device)
        valid = torch.zeros((rows,), dtype=torch.int32, device=self.device)
        stats[:n].copy_(self.stats)
        valid[:n].copy_(self.valid)
        self.stats, self.valid = stats, valid

    def touch(self, idx: torch.Tensor) -> None:
        """Rows ``idx`` (int64, on the device) were written on the current stream."""
        self.valid.index_fill_(0, idx, 0)
        self.dirty += int(idx.numel())

    def invalidate(self, stream: int | None = None) -> None:
        """Every row, on ``stream`` (a raw stream handle; default: the current
        torch stream)."""
        if self.valid.is_cuda:
            from ..ops._lib import LIB, ptr, stream_of
            LIB.call("fm_hist_cache_invalidate", ptr(self.valid), len(self),
                     stream_of(self.valid) if stream is None else stream)
        else:
            self.valid.zero_()
        self.dirty = max(self.dirty, len(self))

    def rekey(self, z0: float) -> None:
        """The next tick makes its ``quantile_robust`` records with the tail
        parameter ``z0``: entries made with another one are stale, and the tag
        does not tell them apart, so everything is invalidated (on the current
        stream)."""
        z0 = float(z0)
        if self.z0 is not None and self.z0 != z0:
            self.invalidate()
        self.z0 = z0

    def expect_miss(self, T: int, rows: int) -> bool:
        """Whether the tick over ``rows`` rows of a view of length ``T`` should
        be shaped for streaming history (many misses) rather than for hits."""
        return self.T != T or self.dirty * 16 > rows

    def ticked(self, T: int) -> None:
        self.T, self.dirty = T, 0


@dataclass
class HistView:
    """What a scoring launch needs: the buffer view (16-B aligned rows), its
    leading dimension, the logical history length and the row map; for a
    static store also the row-statistics caches of the buffer: ``cache``
    holds (mean, std, n), ``rcache`` the robust (median, sigma, n), ``bcache``
    the static band models' records (centre, sigma_lo, sigma_up, n)."""
    hist: torch.Tensor        # [rows, >= T] view into the resident buffer
    ld: int
    T: int
    cache: RowStatsCache | None = None
    rcache: RowStatsCache | None = None
    bcache: RowStatsCache | None = None


class ResidentHistory:
    def __init__(self, T: int, device, step: float = 60.0, sliding: bool = False, slack: int = 1024,
                 capacity: int = 0):
        self.T = int(T)
        self.step = float(step)
        self.sliding = sliding
        self.device = torch.device(device)
        # static rows: T rounded up to a multiple of 4 columns (NaN on the left);
        # sliding rows: the window may start up to 3 columns early (aligned view)
        self.width = _ceil4(self.T) if not sliding else _ceil4(self.T + 3) + _ceil4(max(4, slack))
        self.buf = torch.empty((0, self.width), dtype=torch.float32, device=self.device)
        # static rows are written once and re-scored every cycle: their
        # statistics are cached per row; a sliding window moves every cycle
        self.cache = None if sliding else RowStatsCache(0, self.device)
        # the robust model's (median, sigma, n) of the same rows (K18): a cache
        # of its own, with its own view length and dirty count -- a fleet may
        # tick some groups with each model
        self.rcache = None if sliding else RowStatsCache(0, self.device)
        # the band records of a per-metric mix of the static band models (K25)
        self.bcache = None if sliding else RowStatsCache(0, self.device, width=4)
        self.slot: dict = {}
        self.free: list[int] = []
        self.last_t = np.zeros(0, np.float64)       # time of each row's newest sample (-inf: none)
        self.nlen = np.zeros(0, np.int64)           # static: columns written (the row's right end)
        self.nfin = np.zeros(0, np.int64)           # finite samples inside the window (history gate)
        self.used = np.zeros(0, np.int64)           # cycle of last use (eviction)
        self.occ = np.zeros(0, bool)                # row holds a key
        self.keys: list = []
        # per row, for history checkpoints (set when a job's plan claims the
        # row): the key and the owner (namespace, app) as ready UTF-8 JSON and
        # the owner's service_owner(.., 16) block -- a save lists its rows
        # with array passes and C-level joins, no per-job Python
        self.kjson: list = []
        self.ojson: list = []
        self.oblk = np.zeros(0, np.int16)
        self.owned = np.zeros(0, bool)
        self.kdone = np.zeros(0, bool)              # kjson[r] is encoded
        self.t0: float | None = None                # sliding: time of column 0
        self.e = 0                                  # sliding: exclusive end column of the window
        self.ws = 0                                 # sliding: first column inside the window
        if capacity:
            self._grow(capacity)
        self.compactions = 0
        self._gone = None                           # (device, pinned) finite counts of retired columns
        self.bytes_in = 0
        self.max_len = 0                            # static: longest row written (view length)
        self.dense_rows = 0                         # sliding rows whose history arrived as one grid block
        self._dense_pin = None                      # [2 x (pinned staging buffer, event of its last upload), next]

    # ------------------------------------------------------------------ rows
    def __len__(self) -> int:
        return len(self.slot)

    def _grow(self, need: int) -> None:
        cap = self.buf.shape[0]
        if need <= cap:
            return
        new_cap = max(need, int(cap * 1.5) + 256)
        nb = torch.full((new_cap, self.width), float("nan"), dtype=torch.float32, device=self.device)
        if cap:
            nb[:cap].copy_(self.buf)
        self.buf = nb
        if self.cache is not None:
            self.cache.grow(new_cap)
        if self.rcache is not None:
            self.rcache.grow(new_cap)
        if self.bcache is not None:
            self.bcache.grow(new_cap)
        self.free.extend(range(new_cap - 1, cap - 1, -1))
        self.last_t = np.concatenate([self.last_t, np.full(new_cap - cap, -np.inf)])
        self.nlen = np.concatenate([self.nlen, np.zeros(new_cap - cap, np.int64)])
        self.nfin = np.concatenate([self.nfin, np.zeros(new_cap - cap, np.int64)])
        self.used = np.concatenate([self.used, np.zeros(new_cap - cap, np.int64)])
        self.occ = np.concatenate([self.occ, np.zeros(new_cap - cap, bool)])
        self.keys.extend([None] * (new_cap - cap))
        self.kjson.extend([None] * (new_cap - cap))
        self.ojson.extend([None] * (new_cap - cap))
        self.oblk = np.concatenate([self.oblk, np.zeros(new_cap - cap, np.int16)])
        self.owned = np.concatenate([self.owned, np.zeros(new_cap - cap, bool)])
        self.kdone = np.concatenate([self.kdone, np.zeros(new_cap - cap, bool)])

    OWNER_BLOCKS = 16

    def rows_for(self, keys: list, cycle: int = 0, owner=None) -> tuple[np.ndarray, np.ndarray]:
        """Row index of every key (allocating missing ones) and a mask of the
        rows that were just allocated (need a full history fetch).  ``owner``
        ((namespace, app), or one per key) is recorded on rows that have none
        yet (history checkpoints order and re-shard rows by it)."""
        out = np.empty(len(keys), np.int32)
        new = np.zeros(len(keys), bool)
        missing = [i for i, k in enumerate(keys) if k not in self.slot]
        if missing:
            self._grow(len(self.slot) + len(missing))
            for i in missing:
                k = keys[i]
                if k in self.slot:          # duplicate key within this call
                    continue
                r = self.free.pop()
                self.slot[k] = r
                self.keys[r] = k
                self.occ[r] = True
                self.last_t[r] = -np.inf
                new[i] = True
        for i, k in enumerate(keys):
            out[i] = self.slot[k]
        self.used[out] = cycle
        if owner is not None and not self.owned[out].all():
            self._own(out, keys, owner)
        return out, new

    def _own(self, rows, keys, owner) -> None:
        """Record the owner of rows that have none (its JSON and block once per
        distinct owner); a row's key JSON is encoded by the first history
        save that needs it (:meth:`key_json`), not on the claiming cycle."""
        import json
        from ..parallel.dist import service_owner
        enc = json.JSONEncoder(separators=(",", ":")).encode
        memo: dict = {}
        one = isinstance(owner, tuple)
        for i, r in enumerate(rows.tolist()):
            if self.owned[r]:
                continue
            o = owner if one else tuple(owner[i])
            oj = memo.get(o)
            if oj is None:
                oj = memo[o] = (enc([o[0], o[1]]).encode(), service_owner(o[0], o[1], self.OWNER_BLOCKS))
            self.kjson[r] = None
            self.kdone[r] = False
            self.ojson[r], self.oblk[r] = oj
            self.owned[r] = True

    def key_json(self, rows: np.ndarray) -> list:
        """UTF-8 JSON of the keys of ``rows`` (encoded once per row, then kept)."""
        import json
        enc = json.JSONEncoder(separators=(",", ":")).encode
        kj, keys = self.kjson, self.keys
        for r in rows[~self.kdone[rows]].tolist():
            kj[r] = enc(list(keys[r])).encode()
        self.kdone[rows] = True
        return kj

    def get(self, key):
        return self.slot.get(key)

    def release(self, keys) -> int:
        rows = [self.slot.pop(k) for k in keys if k in self.slot]
        if rows:
            idx = torch.as_tensor(rows, dtype=torch.int64, device=self.device)
            self.buf.index_fill_(0, idx, float("nan"))
            self.touch(idx)
            for r in rows:
                self.keys[r] = None
                self.kjson[r] = self.ojson[r] = None
                self.last_t[r] = -np.inf
            self.owned[rows] = False
            self.kdone[rows] = False
            self.nlen[rows] = 0
            self.nfin[rows] = 0
            self.occ[rows] = False
            self.free.extend(rows)
        return len(rows)

    def evict_idle(self, cycle: int, max_idle: int) -> int:
        """Drop rows not used for more than ``max_idle`` cycles."""
        idle = np.flatnonzero(self.occ & (cycle - self.used > max_idle))
        if len(idle) == 0:
            return 0
        return self.release([self.keys[r] for r in idle])

    # ------------------------------------------------------------------ writes
    def write_static(self, rows: np.ndarray, values: list[np.ndarray], t_last: np.ndarray) -> None:
        """Static rows: left-align each series into its row (one packed
        host->device copy, one scatter of whole rows)."""
        assert not self.sliding
        if len(rows) == 0:
            return
        packed = native_rt.pack_left(values, self.width, self.width)
        self.max_len = max(self.max_len, min(self.width, max((len(v) for v in values), default=0)))
        src = torch.from_numpy(packed)
        if self.device.type == "cuda":
            src = src.pin_memory().to(self.device, non_blocking=True)
        idx = torch.as_tensor(rows, dtype=torch.int64).to(self.device)
        self.buf.index_copy_(0, idx, src)
        self.touch(idx)
        self.last_t[rows] = t_last
        self.nlen[rows] = [min(len(v), self.width) for v in values]
        self.nfin[rows] = [int(np.isfinite(np.asarray(v[:self.width], np.float32)).sum()) for v in values]
        self.bytes_in += packed.nbytes

    def touch(self, rows) -> None:
        """Rows whose data was just written on the current stream: their
        cached statistics are stale.  Every writer of a static ``buf`` row
        calls this (write_static, release, the checkpoint restore)."""
        if self.cache is not None and len(rows):
            idx = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(np.asarray(rows), dtype=torch.int64)
            idx = idx.to(self.device)
            self.cache.touch(idx)
            self.rcache.touch(idx)
            self.bcache.touch(idx)

    def view(self) -> HistView:
        if not self.sliding:
            return HistView(self.buf, self.width, max(1, self.max_len), self.cache, self.rcache, self.bcache)
        vs = max(0, self.ws // 4 * 4)
        return HistView(self.buf[:, vs:], self.width, self.e - vs)

    def view_until(self, t_end: float | None) -> HistView:
        """Sliding view whose logical length stops at the grid point <= t_end
        (a merged sliding group's grid also holds its current window)."""
        v = self.view()
        if not self.sliding or t_end is None or self.t0 is None:
            return v
        vs = max(0, self.ws // 4 * 4)
        e = int(self.col(math.floor(t_end / self.step + 1e-9) * self.step)) + 1
        return HistView(v.hist, v.ld, max(0, min(self.e, e) - vs))

    # ------------------------------------------------------------------ sliding grid
    def col(self, t) -> np.ndarray:
        return np.rint((np.asarray(t, np.float64) - self.t0) / self.step).astype(np.int64)

    def advance(self, t_end: float, t_start: float | None = None) -> None:
        """Move the window to the samples in ``[t_start, t_end]`` (grid
        points; at most ``T`` columns ending at the last grid point <= t_end)."""
        assert self.sliding
        t_last = math.floor(t_end / self.step) * self.step
        t_first = None if t_start is None else math.ceil(t_start / self.step) * self.step
        if self.t0 is None:
            self.t0 = t_last - (self.T - 1) * self.step
            self.e = self.ws = 0

        def target() -> tuple[int, int]:
            e = int(self.col(t_last)) + 1
            ws = e - self.T if t_first is None else max(e - self.T, int(self.col(t_first)))
            return e, ws
        e_new, ws_new = target()
        if e_new < self.e or (e_new == self.e and ws_new <= self.ws):
            return
        if e_new > self.width:
            self._compact(ws_new)
            e_new, ws_new = target()
        # columns that leave the window (those before the aligned view start
        # included) must read as missing
        lo, hi = max(0, self.ws), max(0, ws_new)
        if hi > lo and self.buf.shape[0]:
            # finite samples leaving the window no longer count (history gate)
            hi = min(hi, self.width)
            if self.device.type == "cuda":
                from ..ops._lib import LIB, ptr, stream_of
                R = self.buf.shape[0]
                if self._gone is None or self._gone[0].numel() < R:
                    self._gone = (torch.empty((R,), dtype=torch.int32, device=self.device),
                                  torch.empty((R,), dtype=torch.int32).pin_memory())
                gd, gh = self._gone
                LIB.call("fm_grid_retire", ptr(self.buf), self.buf.stride(0), R, lo, hi, ptr(gd), stream_of(self.buf))
                gh[:R].copy_(gd[:R], non_blocking=True)
                torch.cuda.current_stream(self.device).synchronize()
                gone = gh[:R].numpy()
            else:
                gone = torch.isfinite(self.buf[:, lo:hi]).sum(1).numpy()
                self.buf[:, lo:hi] = float("nan")
            self.nfin -= gone.astype(np.int64)
        self.e, self.ws = e_new, max(ws_new, 0)

    def _compact(self, ws_new: int) -> None:
        """Shift the live columns back to column 0 (rows in chunks, so the
        temporary stays small) and NaN the freed tail."""
        vs = max(0, ws_new // 4 * 4)
        keep = self.e - vs                       # live columns after the shift
        if self.buf.shape[0] and keep > 0:
            for r0 in range(0, self.buf.shape[0], 4096):
                blk = self.buf[r0:r0 + 4096]
                tmp = blk[:, vs:self.e].clone()
                blk[:, :keep] = tmp
                blk[:, keep:] = float("nan")
        elif self.buf.shape[0]:
            self.buf.fill_(float("nan"))
        self.t0 += vs * self.step
        self.e -= vs
        self.ws = max(0, self.ws - vs)
        self.compactions += 1

    def window_start_t(self) -> float:
        return self.t0 + self.ws * self.step

    def write_sliding(self, rows: np.ndarray, times: list[np.ndarray], values: list[np.ndarray]) -> None:
        """Scatter the samples of each row onto the grid (samples outside the
        current window are dropped); rows' ``last_t`` advance."""
        assert self.sliding and self.t0 is not None
        if len(rows) == 0:
            return
        lens = np.fromiter((len(t) for t in times), np.int64, len(times))
        if lens.sum() == 0:
            return
        self.write_sliding_flat(np.repeat(np.asarray(rows, np.int64), lens), np.concatenate(times),
                                np.concatenate(values).astype(np.float32, copy=False))

    def write_sliding_dense(self, rows: np.ndarray, t: np.ndarray, V: np.ndarray) -> None:
        """Rows with NO sample yet (new jobs' history): ``V[i, k]`` is row
        ``rows[i]``'s sample at grid time ``t[k]`` (consecutive grid points,
        NaN = missing).  The block goes to the device in one copy and one
        row-scatter of a column range; ``last_t`` / ``nfin`` from array passes
        -- no per-sample scatter (a new job's 7-day window is 10,080 samples
        per metric)."""
        assert self.sliding and self.t0 is not None
        rows = np.asarray(rows, np.int64)
        if not len(rows) or not len(t):
            return
        c = self.col(t)
        if len(c) > 1 and not (np.diff(c) == 1).all():
            ok = np.isfinite(V)
            self.write_sliding_flat(np.repeat(rows, ok.sum(1)), np.broadcast_to(t, V.shape)[ok], V[ok])
            return
        a, b = max(int(c[0]), self.ws), min(int(c[-1]) + 1, self.e)
        if b <= a:
            return
        V = V[:, a - int(c[0]):b - int(c[0])]
        fin = np.isfinite(V)
        cnt = fin.sum(1)
        has = cnt > 0
        last = V.shape[1] - 1 - np.argmax(fin[:, ::-1], axis=1)
        self.nfin[rows] = cnt
        self.last_t[rows] = np.where(has, self.t0 + (a + last) * self.step, -np.inf)
        if self.device.type == "cuda":
            # one reusable pinned staging buffer (a pinned allocation per block
            # costs more than the copy); the previous block's upload must have
            # left it before it is refilled
            o = (V.size + 1) // 2 * 2                # (the int64 rows start 8-byte aligned)
            n = o + len(rows) * 2
            # two staging buffers used in turn: a cycle's blocks (one per
            # metric) fill one while the previous one's upload runs
            pins = self._dense_pin
            if pins is None:
                pins = self._dense_pin = [None, None, 0]
            k = pins[2]
            pins[2] ^= 1
            st = pins[k]
            if st is None or st[0].numel() < n:
                if st is not None:
                    st[1].synchronize()
                st = pins[k] = (torch.empty((int(n * 1.25) + 1024,), dtype=torch.float32).pin_memory(),
                                torch.cuda.Event())
            else:
                st[1].synchronize()
            hv = st[0][:V.size].numpy().reshape(V.shape)
            np.copyto(hv, V, casting="unsafe")
            hi = st[0][o:o + 2 * len(rows)].view(torch.int64).numpy()
            hi[:] = rows
            blk = st[0][:V.size].view(V.shape).to(self.device, non_blocking=True)
            idx = st[0][o:o + 2 * len(rows)].view(torch.int64).to(self.device, non_blocking=True)
            st[1].record()
        else:
            blk = torch.from_numpy(np.ascontiguousarray(V, np.float32))
            idx = torch.from_numpy(rows)
        self.buf[idx, a:b] = blk
        self.bytes_in += blk.numel() * 4
        self.dense_rows += len(rows)

    def write_sliding_flat(self, r: np.ndarray, t: np.ndarray, v: np.ndarray) -> None:
        """:meth:`write_sliding` for samples already flattened (row per sample)."""
        assert self.sliding and self.t0 is not None
        if len(r) == 0:
            return
        n = len(r)
        if self.device.type == "cuda":
            # indices and values in ONE pinned buffer, one host->device copy
            hb = torch.empty((3 * n,), dtype=torch.int32).pin_memory()
            hn = hb.numpy()
            of, ov = hn[:2 * n].view(np.int64), hn[2 * n:].view(np.float32)
        else:
            of, ov = np.empty(n, np.int64), np.empty(n, np.float32)
        k = native_rt.sliding_prep(r, t, v, self.t0, self.step, self.ws, self.e, self.width, self.last_t, self.nfin,
                                   of, ov)
        if k is not None:                                  # the one-pass native form
            if k:
                if self.device.type == "cuda":
                    db = hb.to(self.device, non_blocking=True)
                    flat, vals = db[:2 * n].view(torch.int64)[:k], db[2 * n:].view(torch.float32)[:k]
                else:
                    flat, vals = torch.from_numpy(of[:k]), torch.from_numpy(ov[:k])
                self.buf.view(-1).index_copy_(0, flat, vals)
                self.bytes_in += 12 * k
            return
        c = self.col(t)
        ok = (c >= self.ws) & (c < self.e) & np.isfinite(v)
        r, c, v, t = r[ok], c[ok], v[ok], t[ok]
        if len(r):
            lt = self.last_t[r]
            fl = np.isfinite(lt)
            prev = np.where(fl, self.col(np.where(fl, lt, self.t0)), -1)
            if np.bincount(r).max() <= 1:                 # one sample per row (a 60-s poll): plain indexing
                self.nfin[r] += c > prev
                self.last_t[r] = np.maximum(lt, t)
            else:
                np.add.at(self.nfin, r[c > prev], 1)      # new columns only (a re-sent sample counts once)
                np.maximum.at(self.last_t, r, t)
            n = len(r)
            if self.device.type == "cuda":
                # indices and values in ONE pinned buffer, one host->device copy
                hb = torch.empty((3 * n,), dtype=torch.int32).pin_memory()
                hn = hb.numpy()
                hn[:2 * n].view(np.int64)[:] = r * self.width + c
                hn[2 * n:].view(np.float32)[:] = v
                db = hb.to(self.device, non_blocking=True)
                flat, vals = db[:2 * n].view(torch.int64), db[2 * n:].view(torch.float32)
            else:
                flat = torch.from_numpy(r * self.width + c)
                vals = torch.from_numpy(np.ascontiguousarray(v))
            self.buf.view(-1).index_copy_(0, flat, vals)
            self.bytes_in += v.nbytes + 8 * len(r)
