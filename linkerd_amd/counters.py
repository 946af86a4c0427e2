"""Counters on the device (the l5dh_counters_* calls): Metric.Counter (Metric.scala:14-20, an
AtomicLong behind ``incr(delta: Int)``) batched into an engine's counter space, over a
HistogramEngine's argument rules.

A CounterEngine owns ``int64 values[capacity]`` in the device memory of an engine's context
and a registry of counter ids.  ``incr`` stages (id, delta) per thread, as StatEngine stages
samples; a full batch, and every read, sends the staged adds to the GPU in one call
(l5dh_counters_add).  Every sum is a two's-complement sum that wraps like a Java long, so the
order of adds never shows.  ``device_values`` is the live array as a torch tensor: the device
renderers take it as ``counters``, so a scrape prints the counters from where they live.

Every argument is checked before the library is called.
"""
from __future__ import annotations

import ctypes
import threading
from contextlib import contextmanager
from typing import Dict, List, Optional

import numpy as np

from . import _native as N

INT32_MIN, INT32_MAX = -(1 << 31), (1 << 31) - 1


class _Staging:
    def __init__(self, n: int):
        self.lock = threading.Lock()
        self.ids = np.zeros(n, dtype=np.uint32)
        self.deltas = np.zeros(n, dtype=np.int32)
        self.n = 0


class _DeviceArray:
    """``n`` int64 at a device address, as torch reads it (``__cuda_array_interface__``)."""

    def __init__(self, ptr: int, n: int):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": "<i8", "data": (ptr, False), "version": 2,
                                         "strides": None}


def _integer(x, name: str) -> int:
    if isinstance(x, bool) or not isinstance(x, (int, np.integer)):
        raise TypeError(f"{name}: {x!r} is not an integer")
    return int(x)


class CounterEngine:
    """The counter space of ``engine`` -- a HistogramEngine without one, or a StatEngine, whose
    engine is meant and whose ``grow`` then takes the counters along -- with room for
    ``capacity`` counters; ``batch`` adds are staged per thread before they are sent."""

    def __init__(self, engine, capacity: int, batch: int = 1 << 16):
        capacity, batch = _integer(capacity, "capacity"), _integer(batch, "batch")
        if capacity < 1 or capacity > N.MAX_COUNTERS:
            raise ValueError(f"capacity must be in [1, {N.MAX_COUNTERS}], got {capacity}")
        if batch < 1 or batch > 1 << 30:
            raise ValueError(f"batch must be in [1, 2^30], got {batch}")
        self._owner = engine if hasattr(engine, "engine") else None  # a StatEngine
        eng = engine.engine if self._owner is not None else engine
        if not hasattr(eng, "_ctx") or not eng._ctx:
            raise ValueError("an open HistogramEngine (or a StatEngine) is needed")
        if self._owner is not None and getattr(self._owner, "counters", None) is not None:
            raise ValueError("the StatEngine already has a CounterEngine")
        self.engine = eng
        self.capacity = capacity
        self.batch = batch
        self._lock = threading.Lock()
        self._next = 0
        self._free: List[int] = []
        self._tls = threading.local()
        self._buffers: List[_Staging] = []
        self._bulk = threading.local()  # .values: one scrape's bulk read on this thread (bulk_reads)
        self._view = None  # (address, capacity, tensor) of device_values
        eng._check(eng._lib.l5dh_counters_open(eng._ctx, capacity), "l5dh_counters_open")
        self._open = True
        if self._owner is not None:
            self._owner.counters = self

    # -- lifecycle -----------------------------------------------------------
    def _eng(self):
        if not self._open:
            raise RuntimeError("the counter engine is closed")
        return self.engine

    def close(self) -> None:
        """Free the space (closing the engine frees it too)."""
        if self._open:
            self._open = False
            self._view = None
            if self._owner is not None and getattr(self._owner, "counters", None) is self:
                self._owner.counters = None
            if self.engine._ctx:
                self.engine._check(self.engine._lib.l5dh_counters_close(self.engine._ctx), "l5dh_counters_close")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- registry (MetricsTree.mk_counter takes the id; MetricsTree.prune hands it back) ----------
    def register(self) -> int:
        self._eng()
        with self._lock:
            if self._free:
                return self._free.pop()
            if self._next >= self.capacity:
                raise RuntimeError(f"counter engine full: {self.capacity} counters")
            cid = self._next
            self._next += 1
            return cid

    def _cid(self, cid) -> int:
        cid = _integer(cid, "counter id")
        if cid < 0 or cid >= self.capacity:
            raise ValueError(f"counter id {cid} outside [0, {self.capacity})")
        return cid

    def release(self, cid: int) -> None:
        """Hand a pruned counter's id back: its staged adds are flushed and its value is
        written 0 before the id can be handed out again, so a new counter starts at 0."""
        eng, cid = self._eng(), self._cid(cid)
        self.flush()
        eng._check(eng._lib.l5dh_counters_write(eng._ctx, cid, 1, None), "l5dh_counters_write")
        with self._lock:
            self._free.append(cid)

    @property
    def registered(self) -> int:
        """Counter ids currently held."""
        return self._next - len(self._free)

    # -- the hot path ---------------------------------------------------------------
    def _staging(self) -> _Staging:
        st = getattr(self._tls, "st", None)
        if st is None:
            st = _Staging(self.batch)
            self._tls.st = st
            with self._lock:
                self._buffers.append(st)
        return st

    def incr(self, cid: int, delta: int = 1) -> None:
        """Metric.Counter.incr(delta: Int): staged; a delta outside int32 is a ValueError."""
        delta = int(delta)
        if delta < INT32_MIN or delta > INT32_MAX:
            raise ValueError(f"delta {delta} is not an Int (incr(delta: Int), Metric.scala:17)")
        st = self._staging()
        with st.lock:
            st.ids[st.n] = cid
            st.deltas[st.n] = delta
            st.n += 1
            if st.n == self.batch:
                self._flush_locked(st)

    def _flush_locked(self, st: _Staging) -> None:
        if st.n:
            n, st.n = st.n, 0  # cleared first: a failed call is never re-sent (no double count)
            eng = self._eng()
            eng._check(eng._lib.l5dh_counters_add(eng._ctx, st.ids.ctypes.data, st.deltas.ctypes.data, n),
                       "l5dh_counters_add")

    def flush(self) -> None:
        self._eng()
        with self._lock:
            bufs = list(self._buffers)
        for st in bufs:
            with st.lock:
                self._flush_locked(st)

    @contextmanager
    def _staging_held(self):
        """Every thread's staging lock held and its batch flushed (StatEngine._staging_held):
        no add can fall between the engine calls made inside."""
        with self._lock:
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

    def add(self, ids, deltas=None) -> None:
        """A caller's batch as it is: ids uint32 (int32), deltas int32 or None (1 each); numpy,
        or torch tensors on the engine's GPU.  l5dh_ingest's contract: queued when it returns."""
        eng = self._eng()
        n = int(ids.size) if isinstance(ids, np.ndarray) else int(ids.numel())
        if deltas is not None:
            nd = int(deltas.size) if isinstance(deltas, np.ndarray) else int(deltas.numel())
            if nd != n:
                raise ValueError("ids and deltas differ in length")
        if n > 1 << 30:
            raise ValueError("a batch holds at most 2^30 adds")
        ip = eng._buf(ids, (np.uint32, np.int32), "ids")
        dp = eng._buf(deltas, (np.int32,), "deltas")
        eng._check(eng._lib.l5dh_counters_add(eng._ctx, ip, dp, n), "l5dh_counters_add")

    # -- reads ------------------------------------------------------------------------------
    def get(self, cid: int) -> int:
        """The counter's exact current value: flushes, then reads 8 bytes."""
        eng, cid = self._eng(), self._cid(cid)
        self.flush()
        out = np.zeros(1, np.int64)
        eng._check(eng._lib.l5dh_counters_read(eng._ctx, cid, 1, out.ctypes.data), "l5dh_counters_read")
        return int(out[0])

    def values(self) -> np.ndarray:
        """Every value, int64 [capacity], from one flush and one copy."""
        self.flush()
        return self._read(0, self.capacity)

    def read(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """values()'s range [first, first + count)."""
        first, count = self._range(first, count)
        self.flush()
        return self._read(first, count)

    def _read(self, first: int, count: int) -> np.ndarray:
        eng = self._eng()
        out = np.zeros(count, np.int64)
        eng._check(eng._lib.l5dh_counters_read(eng._ctx, first, count, out.ctypes.data if count else None),
                   "l5dh_counters_read")
        return out

    def write(self, first: int, values=None, count: Optional[int] = None) -> None:
        """Set [first, first + count) to ``values`` (int64; numpy, or a torch tensor on the
        engine's GPU), or to 0 with values=None."""
        eng = self._eng()
        if values is not None and count is None:
            count = int(values.size) if isinstance(values, np.ndarray) else int(values.numel())
        first, count = self._range(first, count)
        vp = eng._buf(values, (np.int64,), "values", count)
        self.flush()
        eng._check(eng._lib.l5dh_counters_write(eng._ctx, first, count, vp), "l5dh_counters_write")

    def _range(self, first, count):
        first = _integer(first, "first")
        count = self.capacity - first if count is None else _integer(count, "count")
        if first < 0 or count < 0 or first + count > self.capacity:
            raise ValueError(f"counter range [{first}, {first + count}) outside [0, {self.capacity})")
        return first, count

    def device_values(self):
        """The live array as a torch int64 tensor [capacity] on the engine's GPU, after a
        flush: what the device renderers of the same engine take as ``counters``.  A view --
        nothing is copied -- valid until the next grow, move_to or close."""
        import torch
        eng = self._eng()
        self.flush()
        p, m = ctypes.c_void_p(), ctypes.c_uint32(0)
        eng._check(eng._lib.l5dh_counters_values(eng._ctx, ctypes.byref(p), ctypes.byref(m)), "l5dh_counters_values")
        if self._view is None or self._view[:2] != (p.value, m.value):
            t = torch.as_tensor(_DeviceArray(p.value, m.value), device=torch.device("cuda", eng.device))
            self._view = (p.value, m.value, t)
        return self._view[2]

    @contextmanager
    def bulk_reads(self):
        """One values() now; until the block ends, this thread's reads of single counters
        (Metric.Counter.get) are answered from it.  A host writer's scrape: one copy, no
        device read per counter."""
        self._bulk.values = self.values()
        try:
            yield self._bulk.values
        finally:
            self._bulk.values = None

    def bulk_value(self, cid: int) -> Optional[int]:
        """The value of ``cid`` in this thread's open bulk_reads block, None without one."""
        v = getattr(self._bulk, "values", None)
        return None if v is None else int(v[cid])

    def rollup(self, group_of, ngroups: int, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """Label rollups of counters: int64 [ngroups], the wrapping sum per group of the
        counters [first, first + count) under the map ``group_of`` (uint32 [count]: a group
        below ngroups, or NO_GROUP).  An empty group reads 0."""
        eng = self._eng()
        ngroups = _integer(ngroups, "ngroups")
        if ngroups < 1 or ngroups > N.MAX_COUNTERS:
            raise ValueError(f"ngroups must be in [1, {N.MAX_COUNTERS}], got {ngroups}")
        first, count = self._range(first, count)
        if isinstance(group_of, np.ndarray):
            if group_of.dtype.kind not in "iu":
                raise TypeError(f"group_of: dtype {group_of.dtype} is not an integer type")
            if group_of.size and (group_of.min() < 0 or group_of.max() >= 2 ** 32):
                raise ValueError("group_of must fit uint32")
            group_of = np.ascontiguousarray(group_of.astype(np.uint32, copy=False))
        gp = eng._buf(group_of, (np.uint32, np.int32), "group_of", count)
        self.flush()
        out = np.zeros(ngroups, np.int64)
        eng._check(eng._lib.l5dh_counters_rollup(eng._ctx, first, count, gp if count else None, ngroups,
                                                 out.ctypes.data), "l5dh_counters_rollup")
        return out

    # -- growth, hand-over, restart ---------------------------------------------------------
    def grow(self, capacity: int) -> None:
        """Room for ``capacity`` counters: the values are kept, the new ones read 0."""
        eng = self._eng()
        capacity = _integer(capacity, "capacity")
        if capacity < self.capacity or capacity > N.MAX_COUNTERS:
            raise ValueError(f"grow: capacity {capacity} outside [{self.capacity}, {N.MAX_COUNTERS}]")
        with self._staging_held():
            eng._check(eng._lib.l5dh_counters_resize(eng._ctx, capacity), "l5dh_counters_resize")
            self.capacity = capacity
            self._view = None

    def move_to(self, engine) -> None:
        """Hand the space to ``engine``: another HistogramEngine on the same GPU that has no
        counters.  The pointer moves, nothing is copied.  This is how StatEngine.grow keeps
        its counters."""
        eng = self._eng()
        if engine is eng:
            raise ValueError("move_to: the counters already belong to this engine")
        if not hasattr(engine, "_ctx") or not engine._ctx:
            raise ValueError("move_to: an open HistogramEngine is needed")
        if engine.device != eng.device:
            raise ValueError(f"move_to: the counters are on cuda:{eng.device}, the engine on cuda:{engine.device}")
        with self._staging_held():
            rc = eng._lib.l5dh_counters_move(eng._ctx, engine._ctx)
            if rc != 0:  # (the refusals that concern the target are in its error text)
                msg = eng._lib.l5dh_last_error(engine._ctx) or eng._lib.l5dh_last_error(eng._ctx)
                raise N.L5dhError(rc, "l5dh_counters_move", msg.decode() if msg else "")
            self.engine = engine
            self._view = None

    def checkpoint(self) -> Dict[str, np.ndarray]:
        """The values of every id handed out so far, the next id and the free list, as numpy
        arrays (np.savez takes the dict as it is)."""
        with self._staging_held():
            n = self._next
            return {"counter_values": self._read(0, n),
                    "counter_next": np.array([n], np.int64), "counter_free": np.array(self._free, np.uint32)}

    def restore(self, ckpt) -> None:
        """Take over a checkpoint: on a fresh CounterEngine (no id handed out yet) of at
        least the checkpoint's ids."""
        eng = self._eng()
        n = int(np.asarray(ckpt["counter_next"]).reshape(-1)[0])
        values = np.ascontiguousarray(np.asarray(ckpt["counter_values"], np.int64).reshape(-1))
        free = [int(x) for x in np.asarray(ckpt["counter_free"]).reshape(-1)]
        with self._lock:
            if self._next != 0 or self._free:
                raise RuntimeError("restore needs a fresh CounterEngine")
            if n < 0 or n > self.capacity:
                raise ValueError(f"restore: the checkpoint holds {n} counters, the engine {self.capacity}")
            if values.size != n or any(f >= n for f in free) or len(set(free)) != len(free):
                raise ValueError("restore: the checkpoint's arrays do not belong together")
            if n:
                eng._check(eng._lib.l5dh_counters_write(eng._ctx, 0, n, values.ctypes.data), "l5dh_counters_write")
            self._next, self._free = n, free

    # -- what the kernels counted ---------------------------------------------------------------
    def info(self) -> dict:
        """max_counters and the add kernels' statistics since the space was opened: adds
        applied, those that went through an LDS claim table (lds_adds) or took a global
        atomic of their own (global_adds), and the dropped invalid ids."""
        eng = self._eng()
        m = ctypes.c_uint32(0)
        a, l, g, d = (ctypes.c_uint64(0) for _ in range(4))
        eng._check(eng._lib.l5dh_counters_info(eng._ctx, ctypes.byref(m), ctypes.byref(a), ctypes.byref(l),
                                               ctypes.byref(g), ctypes.byref(d)), "l5dh_counters_info")
        return {"max_counters": m.value, "adds": a.value, "lds_adds": l.value, "global_adds": g.value,
                "dropped": d.value}

    def kernel_time(self, reset: bool = False):
        """(device ms, launches) of the counter kernels since the last reset (PARAM_TIMING)."""
        return self._eng().kernel_time(N.K_COUNTERS, reset)
