"""Host-side mirror of io.buoyant.telemetry (reference: telemetry/core/src/main/scala/
io/buoyant/telemetry/{Metric,MetricsTree,MetricsTreeStatsReceiver}.scala), with
Metric.Stat backed by the MI355X engine instead of a per-Stat BucketedHistogram.

Names, argument meaning and error behaviour follow the reference:
  * MetricsTree.resolve / try_resolve / children / metric / mk_counter / mk_stat /
    register_gauge / deregister_gauge / prune (MetricsTree.scala:10-120); a type
    conflict raises ValueError ("non-stat metric already exists"), the analogue of
    IllegalArgumentException (MetricsTree.scala:82,92,103,112).
  * Metric.Stat.add / peek / snapshot / reset / summary / snapshotted_summary /
    starting_at (Metric.scala:22-70); HistogramSummary has the 11 fields of
    Metric.scala:76-88.
What changes is *where* the arithmetic runs: Stat.add appends (series id, value)
to a per-thread staging batch; batches go to the GPU through the C-ABI
(l5dh_ingest); StatEngine.snapshot_all is the batched form of the timer's
per-Stat snapshot()+reset() walk (AdminMetricsExportTelemeter.scala:154-162).
"""
from __future__ import annotations

import threading
import time
from contextlib import contextmanager
from dataclasses import dataclass
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from .javamap import reference_child_order


@dataclass(frozen=True)
class HistogramSummary:
    """Metric.HistogramSummary (Metric.scala:76-88)."""
    count: int
    min: int
    max: int
    sum: int
    p50: int
    p90: int
    p95: int
    p99: int
    p9990: int
    p9999: int
    avg: float

    @staticmethod
    def from_record(rec) -> "HistogramSummary":
        return HistogramSummary(int(rec["count"]), int(rec["min"]), int(rec["max"]), int(rec["sum"]),
                                int(rec["p50"]), int(rec["p90"]), int(rec["p95"]), int(rec["p99"]),
                                int(rec["p9990"]), int(rec["p9999"]), float(rec["avg"]))


@dataclass(frozen=True)
class BucketAndCount:
    """finagle-core BucketAndCount(lowerLimit, upperLimit, count)."""
    lower: int
    upper: int
    count: int


class StatEngine:
    """Series registry + batched ingest in front of one HistogramEngine (one GPU).

    Each thread stages Stat.add calls in its own (ids, values) batch; a full batch,
    or any snapshot/peek/reset, flushes every thread's batch to the GPU.
    """

    def __init__(self, capacity: int = 1 << 16, device: int = 0, batch: int = 1 << 16, engine=None):
        if engine is None:
            from .engine import HistogramEngine
            engine = HistogramEngine(capacity, device)
        self.engine = engine
        self.capacity = int(engine.max_series)
        self.batch = int(batch)
        self._lock = threading.Lock()
        self._next = 0
        self._free: List[int] = []
        self._limits = None
        self._tls = threading.local()
        self._buffers: List["_Staging"] = []
        # lifetime cumulative buckets (enable_le): cuts, their exact labels, the counters
        self.le_cuts: Optional[np.ndarray] = None
        self.le_labels: Optional[np.ndarray] = None
        self.le_buckets: Optional[np.ndarray] = None
        self.le_sums: Optional[np.ndarray] = None
        # configured quantiles (enable_quantiles): the q, their labels, the last interval's values
        self.quantile_q: Optional[np.ndarray] = None
        self.quantile_labels: Optional[List[str]] = None
        self.quantile_values: Optional[np.ndarray] = None
        # the sliding window over ended intervals (enable_window): a window.Window of the engine
        self.window = None
        # the counters.CounterEngine opened over this StatEngine (it sets this): grow takes it along
        self.counters = None

    # registry (MetricsTree.mkStat assigns the id; MetricsTree.prune releases it)
    def register(self) -> int:
        with self._lock:
            if self._free:
                return self._free.pop()
            if self._next >= self.capacity:
                raise RuntimeError(f"histogram engine full: {self.capacity} series")
            sid = self._next
            self._next += 1
            return sid

    def release(self, sid: int) -> None:
        """Return a pruned Stat's id (MetricsPruningModule.scala:14-39 prunes closed
        clients' subtrees).  Its staged samples are flushed and its row is cleared
        on the GPU before the id can be handed out again, so a new Stat starts empty."""
        self.flush()
        self.engine.snapshot(first=sid, count=1, reset=True)
        if self.le_cuts is not None:  # the id's lifetime buckets end with its Stat
            self.le_buckets[sid] = 0
            self.le_sums[sid] = 0
        if self.quantile_q is not None:
            self.quantile_values[sid] = 0
        if self.window is not None:  # the id's kept intervals end with its Stat too
            self.window.forget(sid)
        with self._lock:
            self._free.append(sid)

    @property
    def registered(self) -> int:
        """Series ids currently held by Stats."""
        return self._next - len(self._free)

    # growth and restart: the open interval moves as sparse rows (export_sparse -> import_sparse)
    def grow(self, capacity: int) -> None:
        """Make room for ``capacity`` series: a larger HistogramEngine takes over the open
        interval of this one (its rows leave with export_sparse(reset=True) and enter with
        import_sparse, so they cost what the data costs, not 7192 B per series), the ids
        held by Stats stay valid, and register() succeeds again.  The lifetime ``le``
        counters and the last interval's quantile values are kept and extended with zero
        rows; a sliding window moves to the new engine as it is (Window.move_to: no copy), its
        new ids reading as empty, and so does a CounterEngine opened over this StatEngine
        (CounterEngine.move_to: its values and ids stay).  Adds from other threads wait for the swap; snapshot calls must not run beside
        it.  Tunables set on the old engine (HistogramEngine.set_param) are not carried over."""
        capacity = int(capacity)
        self.flush()
        def refuse_smaller():
            if capacity <= self.capacity:
                raise ValueError(f"grow: capacity {capacity} is not above {self.capacity}")

        with self._staging_held(first=refuse_smaller):  # every thread's adds wait until the new engine is in place
            old = self.engine
            new = type(old)(capacity, old.device)
            try:
                row_off, entries, totals = old.export_sparse(first=0, count=self._next, reset=True)
                new.import_sparse(row_off, entries, totals, first=0)
                if self.window is not None:
                    self.window.move_to(new)
                if self.counters is not None:
                    self.counters.move_to(new)
            except Exception:
                new.close()
                raise
            self.engine, self.capacity = new, int(new.max_series)
            if self.le_cuts is not None:
                self.le_buckets, self.le_sums = self._more_rows(self.le_buckets), self._more_rows(self.le_sums)
            if self.quantile_q is not None:
                self.quantile_values = self._more_rows(self.quantile_values)
            old.close()

    @contextmanager
    def _staging_held(self, first=None):
        """Every thread's staging lock held and its batch flushed: self._lock (held
        throughout: a thread's first add, which registers its batch, waits too), then each
        batch's lock in list order.  No add can fall between the engine calls made inside.
        ``first`` runs under self._lock alone, before any staging lock is taken (a refusal)."""
        with self._lock:
            if first is not None:
                first()
            bufs = list(self._buffers)
            for st in bufs:
                st.lock.acquire()
            try:
                for st in bufs:
                    self._flush_locked(st)
                yield
            finally:
                for st in bufs:
                    st.lock.release()

    def _more_rows(self, a: np.ndarray) -> np.ndarray:
        """A per-series side array extended with zero rows to the capacity."""
        return np.concatenate([a, np.zeros((self.capacity - a.shape[0],) + a.shape[1:], a.dtype)])

    def _start_le(self, cuts: np.ndarray, labels: np.ndarray) -> None:
        """The lifetime ``le`` counters of these cuts, all zero."""
        self.le_cuts, self.le_labels = cuts, labels
        self.le_buckets = np.zeros((self.capacity, len(cuts) + 1), np.uint64)
        self.le_sums = np.zeros(self.capacity, np.int64)

    def checkpoint(self, reset: bool = False) -> Dict[str, np.ndarray]:
        """The open interval and the registry as numpy arrays (np.savez takes the dict as it
        is): the sparse rows and totals of every id handed out so far, the next id, the
        free list, the ``le`` cuts, labels and lifetime counters, and the configured
        quantiles with the last interval's values (``quantile_q`` is empty when
        enable_quantiles was not called).  ``reset`` ends the interval here (what a process
        does before it stops).  The sliding window (enable_window) is not carried: its kept
        intervals stay on the device and end with the process."""
        self.flush()
        with self._lock:
            n = self._next
            row_off, entries, totals = self.engine.export_sparse(first=0, count=n, reset=reset)
            le = self.le_cuts is not None
            K1 = self.le_buckets.shape[1] if le else 1
            qt = self.quantile_q is not None
            return {
                "row_off": row_off, "entries": entries, "totals": totals,
                "next": np.array([n], np.int64), "free": np.array(self._free, np.uint32),
                "le_cuts": self.le_cuts.copy() if le else np.zeros(0, np.uint32),
                "le_labels": self.le_labels.copy() if le else np.zeros(0, np.int64),
                "le_buckets": self.le_buckets[:n].copy() if le else np.zeros((0, K1), np.uint64),
                "le_sums": self.le_sums[:n].copy() if le else np.zeros(0, np.int64),
                "quantile_q": self.quantile_q.copy() if qt else np.zeros(0, np.float64),
                "quantile_values": self.quantile_values[:n].copy() if qt else np.zeros((0, 0), np.int64),
            }

    def restore(self, ckpt) -> None:
        """Take over a checkpoint: on a fresh StatEngine (no id handed out yet) of at least
        the checkpoint's ids.  Afterwards the engine reports what the checkpointed one
        did, and register() continues where it stopped.  A checkpoint written before the
        configured quantiles existed (no ``quantile_q``) restores with them off.  A checkpoint
        holds no sliding window: enable_window starts an empty one."""
        from . import _native as N
        n = int(np.asarray(ckpt["next"]).reshape(-1)[0])
        with self._lock:
            if self._next != 0 or self._free:
                raise RuntimeError("restore needs a fresh StatEngine")
            if n > self.capacity:
                raise ValueError(f"restore: the checkpoint holds {n} series, the engine {self.capacity}")
            row_off = np.ascontiguousarray(ckpt["row_off"], np.uint64)
            entries = np.ascontiguousarray(ckpt["entries"]).view(N.BUCKET_ENTRY_DTYPE).reshape(-1)
            totals = np.ascontiguousarray(ckpt["totals"], np.int64)
            if row_off.size != n + 1 or totals.size != n or int(row_off[-1]) != entries.size:
                raise ValueError("restore: the checkpoint's arrays do not belong together")
            self.engine.import_sparse(row_off, entries, totals, first=0)
            self._next = n
            self._free = [int(x) for x in np.asarray(ckpt["free"]).reshape(-1)]
            cuts = np.asarray(ckpt["le_cuts"], np.uint32).reshape(-1)
            if cuts.size:
                self._start_le(cuts.copy(), np.asarray(ckpt["le_labels"], np.int64).reshape(-1).copy())
                self.le_buckets[:n] = np.asarray(ckpt["le_buckets"], np.uint64).reshape(n, cuts.size + 1)
                self.le_sums[:n] = np.asarray(ckpt["le_sums"], np.int64).reshape(-1)
            qs = np.asarray(ckpt["quantile_q"], np.float64).reshape(-1) if "quantile_q" in ckpt else np.zeros(0)
            if qs.size:
                self.enable_quantiles(qs)
                self.quantile_values[:n] = np.asarray(ckpt["quantile_values"], np.int64).reshape(n, qs.size)

    def _staging(self) -> "_Staging":
        st = getattr(self._tls, "st", None)
        if st is None:
            st = _Staging(self.batch)
            self._tls.st = st
            with self._lock:
                self._buffers.append(st)
        return st

    def add(self, sid: int, value: float) -> None:
        st = self._staging()
        with st.lock:
            st.ids[st.n] = sid
            st.vals[st.n] = value
            st.n += 1
            if st.n == self.batch:
                self._flush_locked(st)

    def _flush_locked(self, st: "_Staging") -> None:
        if st.n:
            n, st.n = st.n, 0  # cleared first: a failed call is never re-sent (no double count)
            self.engine.ingest(st.ids[:n], st.vals[:n])

    def flush(self) -> None:
        with self._lock:
            bufs = list(self._buffers)
        for st in bufs:
            with st.lock:
                self._flush_locked(st)

    # snapshot paths
    def summary(self, sid: int, reset: bool = False) -> HistogramSummary:
        self.flush()
        rec = self.engine.snapshot(first=sid, count=1, reset=reset)[0]
        return HistogramSummary.from_record(rec)

    def peek(self, sid: int) -> List[BucketAndCount]:
        self.flush()
        return [BucketAndCount(int(b["lower"]), int(b["upper"]), int(b["count"])) for b in self.engine.peek(sid)]

    def reset_series(self, sid: int) -> List[BucketAndCount]:
        """Metric.Stat.reset (Metric.scala:44-51): bucketAndCounts + clear as ONE
        engine call (snapshot of one series with its counts and reset), so no sample
        flushed by another thread can fall between the two."""
        self.flush()
        _, counts = self.engine.snapshot(first=sid, count=1, reset=True, with_counts=True)
        if self._limits is None:
            from . import _native
            self._limits = _native.limits()
        L = self._limits
        row = counts[0]
        return [BucketAndCount(0 if b == 0 else int(L[b - 1]), int(L[b]) if b < len(L) else 2147483647, int(row[b]))
                for b in np.flatnonzero(row > 0)]

    def snapshot_all(self, reset: bool = True) -> np.ndarray:
        """Summaries of every series in one fused GPU pass (snapshot + reset)."""
        self.flush()
        return self.engine.snapshot(first=0, count=self.capacity, reset=reset)

    def snapshot_all_rollup(self, group_of, ngroups: int, reset: bool = True):
        """(series summaries, group summaries) of every series from ONE engine call:
        the exact rollups of the groups named by ``group_of`` (uint32 [capacity], entry
        = group or NO_GROUP; linkerd_amd.rollup.plan_rollup) and the per-series
        snapshot (+ reset) see exactly the same samples."""
        self.flush()
        groups, series = self.engine.rollup(group_of, ngroups, first=0, count=self.capacity, reset=reset,
                                            with_series=True)
        return series, groups

    # exact top-k of the open interval
    def top(self, k: int, by="p99", order: str = "largest", min_count: int = 1, group=None, g: int = 0):
        """HistogramEngine.top over the whole capacity after flushing every thread's staged
        adds; nothing is reset.  Released ids have zero rows, so with min_count >= 1 they
        never rank."""
        self.flush()
        return self.engine.top(k, by, order=order, min_count=min_count, group=group, g=g, first=0,
                               count=self.capacity, reset=False)

    # cumulative `le` buckets (Prometheus histogram counters)
    def enable_le(self, bounds) -> None:
        """Keep lifetime cumulative bucket counters at ``bounds`` (snapped down to exact
        labels and deduplicated: HistogramEngine.le_cuts): le_buckets uint64
        [capacity][K+1] -- the K cuts, then +Inf -- and le_sums int64 [capacity], fed by
        snapshot_all_le.  Calling it again starts the counters anew."""
        cuts, labels = self.engine.le_cuts(bounds)
        if not 1 <= len(cuts) <= 64:
            raise ValueError(f"enable_le: {len(cuts)} distinct cuts, 1..64 are supported")
        self._start_le(cuts, labels)

    def snapshot_all_le(self, reset: bool = True) -> np.ndarray:
        """snapshot_all plus the interval's cumulative buckets, from ONE engine call that
        adds them to the lifetime counters: the buckets, the summaries and the reset see
        exactly the same samples.  reset=False only looks: the counters stay as they are
        (the same samples would be added again by the next call)."""
        if self.le_cuts is None:
            raise RuntimeError("snapshot_all_le needs enable_le(bounds) first")
        self.flush()
        if not reset:
            return self.engine.snapshot(first=0, count=self.capacity, reset=False)
        return self.engine.le_counts(self.le_cuts, first=0, count=self.capacity, reset=True, with_series=True,
                                     accumulate_into=(self.le_buckets, self.le_sums))[2]

    # configurable quantiles (any q, beside the summary's six)
    def enable_quantiles(self, qs) -> None:
        """Report the exact quantiles ``qs`` of every series per interval: quantile_q
        (float64, ascending), quantile_labels (their Java Double.toString, the
        exposition's ``quantile`` label) and quantile_values int64 [capacity][K], written
        by snapshot_all_quantiles.  1..64 distinct values in [0, 1], none of the eight the
        summary block prints already (0, 0.5, 0.9, 0.95, 0.99, 0.999, 0.9999, 1): those
        would duplicate a series of the exposition.  Calling it again starts anew."""
        from .javafmt import double_to_string
        q = np.sort(np.asarray(qs, np.float64).reshape(-1))
        if not 1 <= q.size <= 64:
            raise ValueError(f"enable_quantiles: {q.size} quantiles, 1..64 are supported")
        if not np.all((q >= 0.0) & (q <= 1.0)):  # (NaN fails both)
            raise ValueError("enable_quantiles: every quantile must be in [0, 1]")
        if np.unique(q).size != q.size:
            raise ValueError("enable_quantiles: duplicate quantiles")
        taken = sorted(set(q.tolist()) & {0.0, 0.5, 0.9, 0.95, 0.99, 0.999, 0.9999, 1.0})
        if taken:
            raise ValueError(f"enable_quantiles: {taken} are quantiles of the summary block already")
        self.quantile_q = q
        self.quantile_labels = [double_to_string(float(x)) for x in q]
        self.quantile_values = np.zeros((self.capacity, q.size), np.int64)

    def snapshot_all_quantiles(self, reset: bool = True) -> np.ndarray:
        """snapshot_all plus the interval's configured quantiles, which overwrite
        quantile_values (quantiles do not accumulate).  With enable_le on, the same call
        also feeds the lifetime ``le`` counters: every staging lock is held (as grow holds
        them) over the two engine calls -- quantiles(reset=False), then
        le_counts(reset=True, with_series=True) -- so no add can fall between them and
        both see exactly the same samples.  reset=False only looks and leaves the ``le``
        counters alone, as snapshot_all_le does."""
        if self.quantile_q is None:
            raise RuntimeError("snapshot_all_quantiles needs enable_quantiles(qs) first")
        if not reset or self.le_cuts is None:
            self.flush()
            self.quantile_values, summaries = self.engine.quantiles(
                self.quantile_q, first=0, count=self.capacity, reset=reset, with_series=True)
            return summaries
        with self._staging_held():
            self.quantile_values = self.engine.quantiles(self.quantile_q, first=0, count=self.capacity, reset=False)
            return self.engine.le_counts(self.le_cuts, first=0, count=self.capacity, reset=True,
                                         with_series=True, accumulate_into=(self.le_buckets, self.le_sums))[2]


    # exact sliding-window summaries over the last W ended intervals
    def enable_window(self, slots: int) -> None:
        """Keep the last ``slots`` (1..64) ended intervals on the device (window.Window), fed
        by push_window and read by window_summaries.  Calling it again starts anew."""
        from .window import Window
        if self.window is not None:
            self.window.close()
            self.window = None
        self.window = Window(self.engine, slots)

    def push_window(self) -> np.ndarray:
        """snapshot_all(reset=True) whose interval is also kept in the window's next slot,
        from ONE engine call.  With enable_le / enable_quantiles on, every staging lock is
        held (as snapshot_all_quantiles holds them) over the engine calls -- the quantiles
        and the ``le`` buckets without a reset, then the push -- so no add can fall between
        them and all of them see exactly the same samples."""
        if self.window is None:
            raise RuntimeError("push_window needs enable_window(slots) first")
        if self.le_cuts is None and self.quantile_q is None:
            self.flush()
            return self.window.push(self.capacity, with_series=True)
        with self._staging_held():
            if self.quantile_q is not None:
                self.quantile_values = self.engine.quantiles(self.quantile_q, first=0, count=self.capacity, reset=False)
            if self.le_cuts is not None:
                self.engine.le_counts(self.le_cuts, first=0, count=self.capacity, reset=False,
                                      accumulate_into=(self.le_buckets, self.le_sums))
            return self.window.push(self.capacity, with_series=True)

    def window_summaries(self, last: int, include_open: bool = False) -> np.ndarray:
        """Summaries of every series over the ``last`` most recent pushed intervals (+ the open
        one with ``include_open``, after flushing every thread's staged adds): what each Stat
        would report had it received all their samples.  Nothing is reset."""
        if self.window is None:
            raise RuntimeError("window_summaries needs enable_window(slots) first")
        if include_open:
            self.flush()
        return self.window.summaries(last, first=0, count=self.capacity, include_open=include_open)


class _Staging:
    def __init__(self, n: int):
        self.lock = threading.Lock()
        self.ids = np.zeros(n, dtype=np.uint32)
        self.vals = np.zeros(n, dtype=np.float32)
        self.n = 0


class Metric:
    """sealed trait Metric (Metric.scala:8-89)."""

    class _None:
        def __repr__(self):
            return "Metric.None"

    NONE = _None()

    class Counter:
        """Metric.Counter (Metric.scala:14-20): AtomicLong.  With ``counters`` (a
        counters.CounterEngine) the value lives on the GPU under ``counter_id``: incr stages
        the add (its delta an Int, as the reference's parameter), get is exact and current."""

        def __init__(self, counters=None):
            # with a CounterEngine, the monitor of Stat._lock: incr reads the id and stages its
            # add under it, and _release takes the id away under it
            self._lock = threading.Lock()
            self._value = 0  # (device-backed: the last value, once the id has been handed back)
            self._counters = counters
            self.counter_id = counters.register() if counters is not None else None

        def incr(self, delta: int = 1) -> None:
            with self._lock:
                if self._counters is None:
                    self._value += int(delta)
                elif self.counter_id is not None:  # (pruned: like adding to a counter no exporter reads any more)
                    self._counters.incr(self.counter_id, delta)

        def get(self) -> int:
            ce, cid = self._counters, self.counter_id  # read once
            if ce is None or cid is None:
                return self._value
            v = ce.bulk_value(cid)  # (a host writer's scrape: one bulk read, not one per counter)
            return ce.get(cid) if v is None else v

        def _release(self) -> None:
            """MetricsTree.prune: hand the counter id back.  The id is taken under the
            counter's lock, so every incr that saw it has already staged its add;
            CounterEngine.release then flushes those and writes 0 before the id is handed out
            again.  The counter keeps its last value."""
            ce = self._counters
            if ce is None:
                return
            with self._lock:
                cid = self.counter_id
                if cid is None:
                    return
                self._value = ce.get(cid)
                self.counter_id = None
            ce.release(cid)

    class Stat:
        """Metric.Stat (Metric.scala:22-70) over the GPU engine."""

        def __init__(self, engine: Optional[StatEngine] = None):
            self._engine = engine
            # the per-Stat monitor of Metric.scala:30-33: add() reads the id and stages
            # its sample under it, and _release() takes the id away under it, so once
            # _release has run no add can stage the old id (which may be re-issued)
            self._lock = threading.Lock()
            self.series_id = engine.register() if engine is not None else None
            self._summary_snapshot: Optional[HistogramSummary] = None
            self._reset_time = time.time()

        def _eng(self) -> StatEngine:
            if self._engine is None:
                from ._native import NativeLibraryMissing
                raise NativeLibraryMissing("Metric.Stat needs a StatEngine (GPU); none attached")
            return self._engine

        @property
        def starting_at(self) -> float:
            return self._reset_time

        def add(self, value: float) -> None:
            with self._lock:
                sid = self.series_id  # read once
                if sid is None and self._engine is not None:
                    return  # pruned: like adding to a histogram no exporter reads any more
                self._eng().add(sid, value)

        def peek(self) -> List[BucketAndCount]:
            if self.series_id is None and self._engine is not None:
                return []
            return self._eng().peek(self.series_id)

        def _release(self) -> None:
            """MetricsTree.prune: hand the series id back to the engine.  The id is
            taken under the Stat's lock, so every add that saw it has already staged its
            sample; StatEngine.release then flushes those and clears the row before the
            id is handed out again."""
            with self._lock:
                sid, self.series_id = self.series_id, None
            if self._engine is not None and sid is not None:
                self._engine.release(sid)

        def snapshot(self) -> HistogramSummary:
            self._summary_snapshot = self.summary
            return self._summary_snapshot

        def reset(self) -> Tuple[List[BucketAndCount], float]:
            eng = self._eng()
            buckets = [] if self.series_id is None else eng.reset_series(self.series_id)
            now = time.time()
            delta = now - self._reset_time
            self._reset_time = now
            return buckets, delta

        @property
        def summary(self) -> HistogramSummary:
            if self.series_id is None and self._engine is not None:
                return HistogramSummary(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0)
            return self._eng().summary(self.series_id, reset=False)

        @property
        def snapshotted_summary(self) -> Optional[HistogramSummary]:
            return self._summary_snapshot

        def _set_snapshot(self, summary: HistogramSummary, reset_time: Optional[float] = None) -> None:
            """Used by the batched snapshot driver (one GPU pass for all Stats)."""
            self._summary_snapshot = summary
            if reset_time is not None:
                self._reset_time = reset_time

    class Gauge:
        """Metric.Gauge (Metric.scala:72-74)."""

        def __init__(self, f: Callable[[], float]):
            self._f = f

        def get(self) -> float:
            return float(np.float32(self._f()))


class MetricsTree:
    """MetricsTree.Impl (MetricsTree.scala:38-120)."""

    def __init__(self, engine: Optional[StatEngine] = None, counters=None):
        self._engine = engine
        self._counters = counters  # a counters.CounterEngine: mk_counter makes device-backed counters
        self._trees: Dict[str, "MetricsTree"] = {}  # insertion order
        self._order: Optional[List[str]] = None
        self._tlock = threading.Lock()
        self._mlock = threading.Lock()
        self._metric = Metric.NONE

    @property
    def children(self) -> Dict[str, "MetricsTree"]:
        """Children in the reference's iteration order (ConcurrentHashMap ->
        immutable Map, MetricsTree.scala:44-45; linkerd_amd.javamap)."""
        with self._tlock:
            if self._order is None or len(self._order) != len(self._trees):
                self._order = reference_child_order(list(self._trees))
            return {k: self._trees[k] for k in self._order}

    def _get_or_mk(self, k: str) -> "MetricsTree":
        with self._tlock:
            t = self._trees.get(k)
            if t is None:
                t = MetricsTree(self._engine, self._counters)
                self._trees[k] = t
            return t

    def resolve(self, scope: Sequence[str]) -> "MetricsTree":
        t = self
        for name in scope:
            t = t._get_or_mk(name)
        return t

    def try_resolve(self, scope: Sequence[str]) -> Optional["MetricsTree"]:
        t = self
        for name in scope:
            with t._tlock:
                t = t._trees.get(name)
            if t is None:
                return None
        return t

    @property
    def metric(self):
        return self._metric

    def mk_counter(self) -> Metric.Counter:
        with self._mlock:
            m = self._metric
            if isinstance(m, Metric.Counter):
                return m
            if m is Metric.NONE:
                self._metric = Metric.Counter(self._counters)
                return self._metric
            raise ValueError("non-counter metric already exists")

    def mk_stat(self) -> Metric.Stat:
        with self._mlock:
            m = self._metric
            if isinstance(m, Metric.Stat):
                return m
            if m is Metric.NONE:
                self._metric = Metric.Stat(self._engine)
                return self._metric
            raise ValueError("non-stat metric already exists")

    def register_gauge(self, f: Callable[[], float]) -> None:
        with self._mlock:
            if self._metric is Metric.NONE or isinstance(self._metric, Metric.Gauge):
                self._metric = Metric.Gauge(f)
                return
            raise ValueError("non-gauge metric already exists")

    def deregister_gauge(self) -> None:
        with self._mlock:
            if self._metric is Metric.NONE:
                return
            if isinstance(self._metric, Metric.Gauge):
                self._metric = Metric.NONE
                return
            raise ValueError("non-gauge metric already exists")

    def prune(self) -> None:
        with self._tlock:
            kids = list(self._trees.values())
            self._trees.clear()
            self._order = None
        for k in kids:
            k.prune()
        with self._mlock:
            m, self._metric = self._metric, Metric.NONE
        if isinstance(m, (Metric.Stat, Metric.Counter)):
            m._release()

    def walk(self, prefix: Tuple[str, ...] = ()):
        """Depth-first (path, tree) pairs."""
        yield prefix, self
        for name, child in self.children.items():
            yield from child.walk(prefix + (name,))


class MetricsTreeStatsReceiver:
    """MetricsTreeStatsReceiver (MetricsTreeStatsReceiver.scala:8-28)."""

    def __init__(self, tree: MetricsTree):
        self.tree = tree

    def counter(self, *name: str) -> Metric.Counter:
        return self.tree.resolve(name).mk_counter()

    def stat(self, *name: str) -> Metric.Stat:
        return self.tree.resolve(name).mk_stat()

    def add_gauge(self, *name: str, f: Callable[[], float]):
        self.tree.resolve(name).register_gauge(f)

    def remove_gauge(self, *name: str) -> None:
        self.tree.resolve(name).deregister_gauge()

    def prune(self, *name: str) -> None:
        self.tree.resolve(name).prune()

    def scope(self, *namespaces: str) -> "MetricsTreeStatsReceiver":
        return MetricsTreeStatsReceiver(self.tree.resolve(namespaces))


def snapshot_histograms(tree: MetricsTree, engine: StatEngine) -> int:
    """Batched AdminMetricsExportTelemeter.snapshotHistograms (:154-162): one fused
    GPU snapshot + reset of every series, then each Stat's snapshottedSummary is set.
    Returns the number of Stats updated."""
    return _set_snapshots(tree, engine.snapshot_all)


def live_stats(tree: MetricsTree):
    """(path, Stat) of every Stat of ``tree`` that holds a series id, depth-first."""
    for path, t in tree.walk():
        m = t.metric
        if isinstance(m, Metric.Stat) and m.series_id is not None:
            yield path, m


def _set_snapshots(tree: MetricsTree, snapshot_all) -> int:
    """One resetting snapshot of every series (a StatEngine.snapshot_all*), then each
    Stat's snapshottedSummary and reset time are set from it."""
    now = time.time()
    summaries = snapshot_all(reset=True)
    n = 0
    for n, (_, m) in enumerate(live_stats(tree), 1):
        m._set_snapshot(HistogramSummary.from_record(summaries[m.series_id]), now)
    return n


def snapshot_histograms_le(tree: MetricsTree, engine: StatEngine) -> int:
    """snapshot_histograms plus the cumulative `le` buckets: the same fused snapshot +
    reset, whose interval is also added to the engine's lifetime bucket counters
    (StatEngine.enable_le) by the same engine call.  Returns the number of Stats updated."""
    return _set_snapshots(tree, engine.snapshot_all_le)


def snapshot_histograms_quantiles(tree: MetricsTree, engine: StatEngine) -> int:
    """snapshot_histograms plus the configured quantiles (StatEngine.enable_quantiles) of
    the same interval -- and, with enable_le, the lifetime `le` counters fed by it.  Returns
    the number of Stats updated."""
    return _set_snapshots(tree, engine.snapshot_all_quantiles)


def snapshot_histograms_window(tree: MetricsTree, engine: StatEngine) -> int:
    """snapshot_histograms whose interval is also kept in the engine's sliding window
    (StatEngine.enable_window) -- and, with enable_le / enable_quantiles, feeds those from
    the same samples.  The tick of a process that answers "p99 over the last five minutes".
    Returns the number of Stats updated."""
    return _set_snapshots(tree, lambda reset: engine.push_window())


def window_stats(tree: MetricsTree, engine: StatEngine, last: int, include_open: bool = False) -> dict:
    """{Stat: HistogramSummary} over the ``last`` most recent pushed intervals (+ the open
    one with ``include_open``), for the Stats of ``tree`` that have a series id.  Nothing is
    reset and no Stat's snapshottedSummary changes.  The reference has no such query."""
    summaries = engine.window_summaries(last, include_open=include_open)
    return {m: HistogramSummary.from_record(summaries[m.series_id]) for _, m in live_stats(tree)}


def top_stats(tree: MetricsTree, engine: StatEngine, k: int, by="p99", order: str = "largest", min_count: int = 1,
              scope: Sequence[str] = ()) -> list:
    """The ``k`` Stats of the open interval with the largest (``order="smallest"``:
    smallest) ``by`` -- a HistogramSummary field name, or a float q for the exact
    q-quantile -- as (path tuple, HistogramSummary[, q value]) in rank order.  The
    selection runs on the GPU (StatEngine.top); nothing is reset and no Stat's
    snapshottedSummary changes.  ``scope`` restricts the candidates to the Stats under
    that subtree (an unknown one has none): one member map built from the tree, members
    0 and everything else NO_GROUP.  The reference has no such query; paths are relative
    to ``tree``'s root, as in flattenMetricsTree."""
    from ._native import NO_GROUP
    scope = tuple(scope)
    paths = {m.series_id: path for path, m in live_stats(tree)}  # the id -> path map, from one walk
    group = None
    if scope or int(min_count) < 1:  # (min_count = 0 admits empty rows: then only rows that Stats own)
        group = np.full(engine.capacity, NO_GROUP, dtype=np.uint32)
        for sid, path in paths.items():
            if path[:len(scope)] == scope:
                group[sid] = 0
    res = engine.top(k, by, order=order, min_count=min_count, group=group, g=0)
    ids, summ = res[0], res[1]
    out = []
    for j, sid in enumerate(ids.tolist()):
        path = paths.get(sid)
        if path is None:
            continue  # (a Stat registered after the walk)
        item = (path, HistogramSummary.from_record(summ[j]))
        out.append(item + (int(res[2][j]),) if len(res) > 2 else item)
    return out
