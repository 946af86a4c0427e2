"""Exact sliding-window summaries over the last W ended intervals (the l5dh_window_* calls),
over a HistogramEngine's argument rules.

A Window is a ring of at most 64 slots that belongs to an engine's context.  ``push`` ends the
open interval -- a resetting snapshot whose sparse rows stay on the device in the ring's next
slot, the oldest being overwritten once the ring is full -- and ``summaries`` sums, per series,
the rows of the ``last`` most recent slots and optionally the open interval's live row.  The
histogram of a union of intervals is the element-wise integer sum of their bucket rows, so a
window summary is byte for byte what one Stat would report had it received every sample of
those intervals: "p99 over the last five minutes", exact.

The results are what every other row source returns -- summaries, dense rows, exact totals,
as numpy arrays or in caller buffers (numpy, or torch tensors on the engine's GPU) -- so they
feed HistogramEngine.top_summaries, render_summaries, quantiles_dense, le_counts_dense and
rollup_dense unchanged.  Every argument is checked before the library is called.
"""
from __future__ import annotations

import ctypes
from typing import Optional

import numpy as np

from . import _native as N


class Window:
    """The ring of ``slots`` ended intervals of ``engine`` (a HistogramEngine without one)."""

    def __init__(self, engine, slots: int):
        slots = int(slots)
        if slots < 1 or slots > N.WINDOW_MAX:
            raise ValueError(f"slots must be in [1, {N.WINDOW_MAX}], got {slots}")
        self.engine = engine
        self.slots = slots
        self.filled = 0  # slots that hold an interval: min(pushes, slots)
        engine._check(engine._lib.l5dh_window_open(engine._ctx, slots), "l5dh_window_open")
        self._open = True

    # -- lifecycle -----------------------------------------------------------
    def _eng(self):
        if not self._open:
            raise RuntimeError("the window is closed")
        return self.engine

    def close(self) -> None:
        """Free the ring (closing the engine frees it too)."""
        if self._open:
            self._open = False
            if self.engine._ctx:
                self.engine._check(self.engine._lib.l5dh_window_close(self.engine._ctx), "l5dh_window_close")

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def move_to(self, engine) -> None:
        """Hand the whole ring to ``engine``: another HistogramEngine on the same GPU that
        has no window and holds at least as many series as the largest pushed interval.
        Pointers move, nothing is copied; series the old engine did not have read as empty.
        This is how StatEngine.grow keeps its window."""
        eng = self._eng()
        if engine is eng:
            raise ValueError("move_to: the window already belongs to this engine")
        if not hasattr(engine, "_ctx") or not engine._ctx:
            raise ValueError("move_to: an open HistogramEngine is needed")
        if engine.device != eng.device:
            raise ValueError(f"move_to: the window is on cuda:{eng.device}, the engine on cuda:{engine.device}")
        rc = eng._lib.l5dh_window_move(eng._ctx, engine._ctx)
        if rc != 0:  # (the refusals that concern the target are in its error text)
            msg = eng._lib.l5dh_last_error(engine._ctx) or eng._lib.l5dh_last_error(eng._ctx)
            raise N.L5dhError(rc, "l5dh_window_move", msg.decode() if msg else "")
        self.engine = engine

    # -- the interval's end ----------------------------------------------------
    def _count(self, count: Optional[int]) -> int:
        eng = self._eng()
        count = eng.max_series if count is None else int(count)
        if count < 0 or count > eng.max_series:
            raise ValueError(f"count={count} outside [0, {eng.max_series}]")
        return count

    def push_into(self, series=None, count: Optional[int] = None) -> None:
        """End the interval of series [0, count) (None: every series) into the ring's next
        slot.  ``series`` (int64 [count*11] or the numpy summary dtype; numpy, or a torch
        tensor on the engine's GPU; None: not wanted) receives the interval's summaries, what
        snapshot(0, count, reset=True) reports -- from the same state, under one hold of the
        context's lock."""
        count = self._count(count)
        eng = self.engine
        sp = eng._summ_buf(series, count, "series")
        eng._check(eng._lib.l5dh_window_push(eng._ctx, count, sp), "l5dh_window_push")
        self.filled = min(self.filled + 1, self.slots)

    def push(self, count: Optional[int] = None, with_series: bool = False):
        """push_into; with ``with_series`` the interval's summaries are returned (numpy)."""
        count = self._count(count)
        series = np.zeros(count, dtype=N.SUMMARY_DTYPE) if with_series else None
        self.push_into(series, count)
        return series

    # -- the query ------------------------------------------------------------------
    def _last(self, last, include_open: bool) -> int:
        if isinstance(last, bool) or not isinstance(last, (int, np.integer)):
            raise TypeError(f"last: {last!r} is not an integer")
        last = int(last)
        if last < 0 or last > self.filled:
            raise ValueError(f"last={last}: the ring holds {self.filled} intervals")
        if last == 0 and not include_open:
            raise ValueError("last=0 sums nothing without include_open")
        return last

    def summaries_into(self, last: int, summaries=None, counts=None, totals=None, first: int = 0,
                       count: Optional[int] = None, include_open: bool = False) -> None:
        """The window of series [first, first+count) over the ``last`` most recent intervals
        (+ the open one with ``include_open``, which is not changed) into caller buffers
        (numpy, or torch tensors on the engine's GPU; each optional): summaries int64
        [count*11] (or the numpy summary dtype), counts int32 [count][1798], totals int64
        [count].  A bucket sum above 2^31 - 1 raises (ERANGE), the least such series named."""
        eng = self._eng()
        last = self._last(last, include_open)
        first, count = eng._range(first, count)
        sp = eng._summ_buf(summaries, count, "summaries")
        cp = eng._buf(counts, (np.int32,), "counts", count * N.NBUCKETS, writable=True)
        tp = eng._buf(totals, (np.int64,), "totals", count, writable=True)
        eng._check(eng._lib.l5dh_window_query(eng._ctx, first, count, last, int(bool(include_open)), sp, cp, tp),
                   "l5dh_window_query")

    def summaries(self, last: int, first: int = 0, count: Optional[int] = None, include_open: bool = False,
                  with_counts: bool = False, with_totals: bool = False):
        """The window summaries (numpy structured) of series [first, first+count), followed
        by the summed dense rows int32 [count][1798] with ``with_counts`` and the summed exact
        sums int64 [count] with ``with_totals``."""
        first, count = self._eng()._range(first, count)
        out = np.zeros(count, dtype=N.SUMMARY_DTYPE)
        counts = np.zeros((count, N.NBUCKETS), np.int32) if with_counts else None
        totals = np.zeros(count, np.int64) if with_totals else None
        self.summaries_into(last, out, counts, totals, first, count, include_open)
        res = (out,) + ((counts,) if with_counts else ()) + ((totals,) if with_totals else ())
        return res if len(res) > 1 else out

    def forget(self, first: int, count: int = 1) -> None:
        """Series [first, first+count) start their history now: queries ignore, for them,
        every interval pushed so far (a pruned id's past stays out of the next Stat that
        gets the id).  The open interval is not touched."""
        eng = self._eng()
        first, count = eng._range(int(first), int(count))
        eng._check(eng._lib.l5dh_window_forget(eng._ctx, first, count), "l5dh_window_forget")

    # -- what the ring holds -----------------------------------------------------------
    def info(self) -> dict:
        """slots, filled, pushes, entries (8 B each, over the filled slots) and the device
        bytes the ring owns."""
        eng = self._eng()
        s, f = ctypes.c_uint32(0), ctypes.c_uint32(0)
        p, e, b = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        eng._check(eng._lib.l5dh_window_info(eng._ctx, ctypes.byref(s), ctypes.byref(f), ctypes.byref(p),
                                             ctypes.byref(e), ctypes.byref(b)), "l5dh_window_info")
        return {"slots": s.value, "filled": f.value, "pushes": p.value, "entries": e.value, "bytes": b.value}

    def kernel_time(self, reset: bool = False):
        """(device ms, launches) of the query kernel since the last reset (PARAM_TIMING)."""
        return self._eng().kernel_time(N.K_WINDOW, reset)
