"""window.Window against a small recording library of its own (no GPU): every refusal the
class makes before a call reaches the library, and the exact C-ABI call of each accepted
method.  (tests/test_abi.py pins that every l5dh_window_* symbol of the header is exported
and bound.)
"""
import ctypes
import errno

import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd.engine import HistogramEngine
from linkerd_amd.window import Window

S = 6  # series of the engine under the stub
NB = N.NBUCKETS


class StubLib:
    """The entry points Window uses: records (name, args) with pointers as 'ptr' / None."""

    def __init__(self, fail=None):
        self.calls, self.fail = [], dict(fail or {})

    def _rec(self, name, *args):
        self.calls.append((name,) + tuple(a.value if isinstance(a, ctypes.c_void_p) else a for a in args))
        return self.fail.get(name, 0)

    @staticmethod
    def _p(p):
        return "ptr" if p else None

    def l5dh_last_error(self, ctx):
        return b"stub text"

    def l5dh_window_open(self, ctx, slots):
        return self._rec("l5dh_window_open", ctx, slots)

    def l5dh_window_close(self, ctx):
        return self._rec("l5dh_window_close", ctx)

    def l5dh_window_push(self, ctx, count, series):
        return self._rec("l5dh_window_push", ctx, count, self._p(series))

    def l5dh_window_query(self, ctx, first, count, last, include_open, out, counts, totals):
        return self._rec("l5dh_window_query", ctx, first, count, last, include_open, self._p(out), self._p(counts),
                         self._p(totals))

    def l5dh_window_forget(self, ctx, first, count):
        return self._rec("l5dh_window_forget", ctx, first, count)

    def l5dh_window_move(self, a, b):
        return self._rec("l5dh_window_move", a, b)

    def l5dh_window_info(self, ctx, s, f, p, e, b):
        s._obj.value, f._obj.value, p._obj.value, e._obj.value, b._obj.value = 3, 2, 5, 40, 4096
        return self._rec("l5dh_window_info", ctx, *(type(x._obj).__name__ for x in (s, f, p, e, b)))

    def l5dh_kernel_time(self, ctx, kid, ms, n, reset):
        ms._obj.value, n._obj.value = 2.5, 4
        return self._rec("l5dh_kernel_time", ctx, kid, reset)


def stub_engine(lib, max_series=S, ctx=0x1000, device=0):
    e = HistogramEngine.__new__(HistogramEngine)
    e._lib, e._ctx, e.max_series, e.device = lib, ctypes.c_void_p(ctx), max_series, device
    e._stream, e._events, e._render_cap = None, [], {}
    e.nranks, e.rank = 1, 0
    return e


@pytest.fixture
def lib():
    return StubLib()


@pytest.fixture
def win(lib):
    w = Window(stub_engine(lib), 3)
    lib.calls.clear()
    return w


def pushed(win, lib, n=2):
    for _ in range(n):
        win.push()
    lib.calls.clear()
    return win


# ---- accepted calls ----------------------------------------------------------------------------
def test_open_and_close(lib):
    e = stub_engine(lib)
    w = Window(e, np.int64(64))
    assert lib.calls == [("l5dh_window_open", 0x1000, 64)] and w.slots == 64 and w.filled == 0
    w.close()
    w.close()  # (once)
    assert lib.calls[1:] == [("l5dh_window_close", 0x1000)]
    with pytest.raises(RuntimeError, match="closed"):
        w.push()
    e._ctx = ctypes.c_void_p()


def test_context_manager_closes(lib):
    with Window(stub_engine(lib), 1):
        pass
    assert [c[0] for c in lib.calls] == ["l5dh_window_open", "l5dh_window_close"]


def test_push(win, lib):
    assert win.push() is None
    assert lib.calls == [("l5dh_window_push", 0x1000, S, None)] and win.filled == 1
    out = win.push(count=4, with_series=True)
    assert out.dtype == N.SUMMARY_DTYPE and out.shape == (4,)
    assert lib.calls[1] == ("l5dh_window_push", 0x1000, 4, "ptr") and win.filled == 2
    win.push_into(np.zeros(S * 11, np.int64))
    win.push(count=0)
    assert lib.calls[2:] == [("l5dh_window_push", 0x1000, S, "ptr"), ("l5dh_window_push", 0x1000, 0, None)]
    assert win.filled == 3  # (never above the slots)


def test_a_failed_push_fills_nothing(lib):
    lib.fail["l5dh_window_push"] = -errno.ENOMEM
    w = Window(stub_engine(lib), 2)
    with pytest.raises(N.L5dhError, match="ENOMEM.*stub text"):
        w.push()
    assert w.filled == 0


def test_summaries(win, lib):
    pushed(win, lib)
    out = win.summaries(2)
    assert out.dtype == N.SUMMARY_DTYPE and out.shape == (S,)
    assert lib.calls == [("l5dh_window_query", 0x1000, 0, S, 2, 0, "ptr", None, None)]
    out, counts, totals = win.summaries(1, first=1, count=3, include_open=True, with_counts=True, with_totals=True)
    assert out.shape == (3,) and counts.shape == (3, NB) and counts.dtype == np.int32 and totals.dtype == np.int64
    assert lib.calls[1] == ("l5dh_window_query", 0x1000, 1, 3, 1, 1, "ptr", "ptr", "ptr")
    out, totals = win.summaries(0, include_open=True, with_totals=True)
    assert lib.calls[2] == ("l5dh_window_query", 0x1000, 0, S, 0, 1, "ptr", None, "ptr") and totals.shape == (S,)


def test_summaries_into_takes_any_subset_of_buffers(win, lib):
    pushed(win, lib)
    win.summaries_into(np.int32(2), counts=np.zeros((2, NB), np.int32), first=4)
    win.summaries_into(1, totals=np.zeros(S, np.int64))
    win.summaries_into(1, np.zeros(S * 11, np.int64))
    assert lib.calls == [("l5dh_window_query", 0x1000, 4, 2, 2, 0, None, "ptr", None),
                         ("l5dh_window_query", 0x1000, 0, S, 1, 0, None, None, "ptr"),
                         ("l5dh_window_query", 0x1000, 0, S, 1, 0, "ptr", None, None)]


def test_forget_info_and_kernel_time(win, lib):
    win.forget(2)
    win.forget(1, count=5)
    assert lib.calls == [("l5dh_window_forget", 0x1000, 2, 1), ("l5dh_window_forget", 0x1000, 1, 5)]
    lib.calls.clear()
    assert win.info() == {"slots": 3, "filled": 2, "pushes": 5, "entries": 40, "bytes": 4096}
    assert lib.calls == [("l5dh_window_info", 0x1000, "c_uint", "c_uint", "c_ulong", "c_ulong", "c_ulong")]
    assert win.kernel_time(reset=True) == (2.5, 4)
    assert lib.calls[1] == ("l5dh_kernel_time", 0x1000, N.K_WINDOW, 1)


def test_move_to(win, lib):
    pushed(win, lib)
    new = stub_engine(lib, max_series=12, ctx=0x2000)
    win.move_to(new)
    assert lib.calls == [("l5dh_window_move", 0x1000, 0x2000)] and win.engine is new and win.filled == 2
    win.summaries(2, count=12)
    assert lib.calls[1] == ("l5dh_window_query", 0x2000, 0, 12, 2, 0, "ptr", None, None)
    new._ctx = ctypes.c_void_p()


def test_a_refused_move_keeps_the_engine(win, lib):
    lib.fail["l5dh_window_move"] = -errno.EEXIST
    old = win.engine
    with pytest.raises(N.L5dhError, match="EEXIST"):
        win.move_to(stub_engine(lib, ctx=0x2000))
    assert win.engine is old


def test_the_engines_kernel_times_stay_the_eight_phases(lib):
    assert N.K_WINDOW == 8 and N.KERNEL_NAMES[N.K_WINDOW] == "window"
    e = stub_engine(lib)
    assert list(e.kernel_times()) == list(N.KERNEL_NAMES[:8])
    e._ctx = ctypes.c_void_p()


# ---- refusals: nothing reaches the library -----------------------------------------------------------
@pytest.mark.parametrize("slots", [0, 65, -1])
def test_open_refuses_slots(lib, slots):
    with pytest.raises(ValueError, match="slots must be in"):
        Window(stub_engine(lib), slots)
    assert lib.calls == []


REFUSED = {
    "push_count_negative": (lambda w: w.push(count=-1), ValueError, "count=-1 outside"),
    "push_count_large": (lambda w: w.push(count=S + 1), ValueError, "outside"),
    "push_series_small": (lambda w: w.push_into(np.zeros((S - 1) * 11, np.int64)), ValueError, "series"),
    "push_series_dtype": (lambda w: w.push_into(np.zeros(S * 11, np.float64)), TypeError, "series"),
    "last_above_filled": (lambda w: w.summaries(3), ValueError, "holds 2 intervals"),
    "last_negative": (lambda w: w.summaries(-1), ValueError, "last=-1"),
    "last_zero_without_open": (lambda w: w.summaries(0), ValueError, "include_open"),
    "last_not_integer": (lambda w: w.summaries(1.0), TypeError, "not an integer"),
    "last_bool": (lambda w: w.summaries(True), TypeError, "not an integer"),
    "range_first": (lambda w: w.summaries(1, first=S + 1), ValueError, "series range"),
    "range_count": (lambda w: w.summaries(1, first=2, count=S), ValueError, "series range"),
    "summaries_small": (lambda w: w.summaries_into(1, np.zeros(S * 11 - 1, np.int64)), ValueError, "summaries"),
    "summaries_dtype": (lambda w: w.summaries_into(1, np.zeros(S * 11, np.int32)), TypeError, "summaries"),
    "counts_dtype": (lambda w: w.summaries_into(1, counts=np.zeros((S, NB), np.int64)), TypeError, "counts"),
    "counts_small": (lambda w: w.summaries_into(1, counts=np.zeros((S, NB - 1), np.int32)), ValueError, "counts"),
    "counts_not_contiguous": (lambda w: w.summaries_into(1, counts=np.zeros((NB, S), np.int32).T), ValueError,
                              "C-contiguous"),
    "totals_dtype": (lambda w: w.summaries_into(1, totals=np.zeros(S, np.uint64)), TypeError, "totals"),
    "totals_small": (lambda w: w.summaries_into(1, totals=np.zeros(S - 1, np.int64)), ValueError, "totals"),
    "totals_read_only": (lambda w: w.summaries_into(1, totals=np.frombuffer(bytes(8 * S), np.int64)), ValueError,
                         "read-only"),
    "forget_range": (lambda w: w.forget(S), ValueError, "series range"),
    "forget_negative": (lambda w: w.forget(-1), ValueError, "series range"),
    "move_to_itself": (lambda w: w.move_to(w.engine), ValueError, "already belongs"),
    "move_to_not_an_engine": (lambda w: w.move_to(object()), ValueError, "HistogramEngine is needed"),
    "move_to_other_device": (lambda w: w.move_to(stub_engine(w.engine._lib, ctx=0x2000, device=1)), ValueError,
                             "cuda:1"),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_before_the_library(win, lib, name):
    call, exc, text = REFUSED[name]
    pushed(win, lib)
    with pytest.raises(exc, match=text):
        call(win)
    assert lib.calls == []


# ---- StatEngine's side ----------------------------------------------------------------------------
def test_statengine_needs_enable_window():
    from linkerd_amd.telemetry import StatEngine
    se = StatEngine(engine=stub_engine(StubLib()))
    with pytest.raises(RuntimeError, match="enable_window"):
        se.push_window()
    with pytest.raises(RuntimeError, match="enable_window"):
        se.window_summaries(1)
    se.engine._ctx = ctypes.c_void_p()


def test_statengine_window_calls():
    from linkerd_amd.telemetry import StatEngine
    lib = StubLib()
    se = StatEngine(engine=stub_engine(lib))
    se.enable_window(4)
    out = se.push_window()
    assert out.shape == (S,)
    se.window_summaries(1)
    assert lib.calls == [("l5dh_window_open", 0x1000, 4), ("l5dh_window_push", 0x1000, S, "ptr"),
                         ("l5dh_window_query", 0x1000, 0, S, 1, 0, "ptr", None, None)]
    se.enable_window(2)  # again: anew
    assert lib.calls[3:] == [("l5dh_window_close", 0x1000), ("l5dh_window_open", 0x1000, 2)]
    se.engine._ctx = ctypes.c_void_p()
