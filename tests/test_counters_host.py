"""counters.CounterEngine against a small recording library of its own (no GPU): every refusal
the class makes before a call reaches the library, the exact C-ABI call of each accepted method,
the int32 rule of ``delta``, the registry and its free list.  (tests/test_abi.py pins that
every l5dh_counters_* symbol of the header is exported and bound.)
"""
import ctypes
import threading

import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd.counters import CounterEngine
from linkerd_amd.engine import HistogramEngine
from linkerd_amd.telemetry import Metric, MetricsTree

CTX = 0x1000


class StubLib:
    """The entry points CounterEngine uses, over an int64 array of its own: records (name,
    args) with the batches' contents in place of their pointers."""

    def __init__(self, fail=None):
        self.calls, self.fail = [], dict(fail or {})
        self.values = np.zeros(0, np.int64)

    def _rec(self, name, *args):
        self.calls.append((name,) + tuple(a.value if isinstance(a, ctypes.c_void_p) else a for a in args))
        return self.fail.get(name, 0)

    @staticmethod
    def _arr(p, n, ctype):
        return None if not p else list(np.ctypeslib.as_array(ctypes.cast(p, ctypes.POINTER(ctype)), shape=(n,)))

    def l5dh_last_error(self, ctx):
        return b"stub text"

    def l5dh_counters_open(self, ctx, n):
        self.values = np.zeros(n, np.int64)
        return self._rec("l5dh_counters_open", ctx, n)

    def l5dh_counters_close(self, ctx):
        return self._rec("l5dh_counters_close", ctx)

    def l5dh_counters_resize(self, ctx, n):
        rc = self._rec("l5dh_counters_resize", ctx, n)
        if rc == 0:
            self.values = np.concatenate([self.values, np.zeros(n - self.values.size, np.int64)])
        return rc

    def l5dh_counters_add(self, ctx, ids, deltas, n):
        i, d = self._arr(ids, n, ctypes.c_uint32), self._arr(deltas, n, ctypes.c_int32)
        rc = self._rec("l5dh_counters_add", ctx, i, d, n)
        if rc == 0 and n:
            np.add.at(self.values, i, 1 if d is None else np.asarray(d, np.int64))
        return rc

    def l5dh_counters_read(self, ctx, first, count, out):
        rc = self._rec("l5dh_counters_read", ctx, first, count, "ptr" if out else None)
        if rc == 0 and count:
            np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_int64)), shape=(count,))[:] = \
                self.values[first:first + count]
        return rc

    def l5dh_counters_write(self, ctx, first, count, values):
        v = self._arr(values, count, ctypes.c_int64)
        rc = self._rec("l5dh_counters_write", ctx, first, count, v)
        if rc == 0:
            self.values[first:first + count] = 0 if v is None else v
        return rc

    def l5dh_counters_rollup(self, ctx, first, count, group, ngroups, out):
        g = self._arr(group, count, ctypes.c_uint32)
        o = np.ctypeslib.as_array(ctypes.cast(out, ctypes.POINTER(ctypes.c_int64)), shape=(ngroups,))
        o[:] = 0
        for j, gj in enumerate(g or []):
            if gj != N.NO_GROUP:
                o[gj] += self.values[first + j]
        return self._rec("l5dh_counters_rollup", ctx, first, count, g, ngroups, "ptr")

    def l5dh_counters_move(self, a, b):
        return self._rec("l5dh_counters_move", a, b)

    def l5dh_counters_info(self, ctx, m, a, l, g, d):
        m._obj.value, a._obj.value, l._obj.value, g._obj.value, d._obj.value = self.values.size, 9, 7, 2, 1
        return self._rec("l5dh_counters_info", ctx, *(type(x._obj).__name__ for x in (m, a, l, g, d)))

    def l5dh_kernel_time(self, ctx, kid, ms, n, reset):
        ms._obj.value, n._obj.value = 1.5, 3
        return self._rec("l5dh_kernel_time", ctx, kid, reset)


def stub_engine(lib, max_series=6, ctx=CTX, device=0):
    e = HistogramEngine.__new__(HistogramEngine)
    e._lib, e._ctx, e.max_series, e.device = lib, ctypes.c_void_p(ctx), max_series, device
    e._stream, e._events, e._render_cap = None, [], {}
    e.nranks, e.rank = 1, 0
    return e


@pytest.fixture
def lib():
    return StubLib()


@pytest.fixture
def ce(lib):
    c = CounterEngine(stub_engine(lib), 10, batch=4)
    lib.calls.clear()
    yield c
    c.engine._ctx = ctypes.c_void_p()  # (nothing to close behind the stub)


# ---- accepted calls ----------------------------------------------------------------------------
def test_open_and_close(lib):
    e = stub_engine(lib)
    c = CounterEngine(e, np.int64(N.MAX_COUNTERS))
    assert lib.calls == [("l5dh_counters_open", CTX, 1 << 24)] and c.capacity == 1 << 24 and c.batch == 1 << 16
    c.close()
    c.close()  # (once)
    assert lib.calls[1:] == [("l5dh_counters_close", CTX)]
    for use in (c.register, c.flush, c.values, lambda: c.get(0), lambda: c.grow(1 << 24), c.info, c.checkpoint):
        with pytest.raises(RuntimeError, match="closed"):
            use()
    e._ctx = ctypes.c_void_p()


def test_context_manager_closes(lib):
    e = stub_engine(lib)
    with CounterEngine(e, 1):
        pass
    assert [c[0] for c in lib.calls] == ["l5dh_counters_open", "l5dh_counters_close"]
    e._ctx = ctypes.c_void_p()


def test_incr_stages_until_the_batch_is_full(ce, lib):
    for cid, d in ((3, 1), (3, -2), (9, 2 ** 31 - 1)):
        ce.incr(cid, d)
    assert lib.calls == []  # staged
    ce.incr(0, -2 ** 31)  # the fourth: the batch is full
    assert lib.calls == [("l5dh_counters_add", CTX, [3, 3, 9, 0], [1, -2, 2 ** 31 - 1, -2 ** 31], 4)]
    ce.flush()  # nothing staged: no call
    assert len(lib.calls) == 1
    ce.incr(5)
    ce.flush()
    assert lib.calls[1] == ("l5dh_counters_add", CTX, [5], [1], 1)


def test_get_flushes_then_reads_eight_bytes(ce, lib):
    ce.incr(2, 40)
    ce.incr(2, 2)
    assert ce.get(2) == 42
    assert lib.calls == [("l5dh_counters_add", CTX, [2, 2], [40, 2], 2), ("l5dh_counters_read", CTX, 2, 1, "ptr")]


def test_values_is_one_copy(ce, lib):
    ce.incr(9, -1)
    v = ce.values()
    assert v.dtype == np.int64 and v.shape == (10,) and v[9] == -1
    assert [c[0] for c in lib.calls] == ["l5dh_counters_add", "l5dh_counters_read"]
    assert lib.calls[1] == ("l5dh_counters_read", CTX, 0, 10, "ptr")
    lib.calls.clear()
    np.testing.assert_array_equal(ce.read(8, 2), [0, -1])
    assert ce.read(10, 0).size == 0
    assert lib.calls == [("l5dh_counters_read", CTX, 8, 2, "ptr"), ("l5dh_counters_read", CTX, 10, 0, None)]


def test_write(ce, lib):
    ce.write(1, np.array([5, -6], np.int64))
    ce.write(4, None, count=3)
    ce.incr(1, 1)
    ce.write(0, np.array([2 ** 63 - 1], np.int64))  # (a write is ordered after the staged adds)
    assert lib.calls == [("l5dh_counters_write", CTX, 1, 2, [5, -6]), ("l5dh_counters_write", CTX, 4, 3, None),
                         ("l5dh_counters_add", CTX, [1], [1], 1), ("l5dh_counters_write", CTX, 0, 1, [2 ** 63 - 1])]


def test_add_passes_a_batch_as_it_is(ce, lib):
    ce.add(np.array([1, 2, 2], np.uint32), np.array([1, 2, 3], np.int32))
    ce.add(np.array([7], np.uint32))
    ce.add(np.zeros(0, np.uint32))
    assert lib.calls[0] == ("l5dh_counters_add", CTX, [1, 2, 2], [1, 2, 3], 3)
    assert lib.calls[1] == ("l5dh_counters_add", CTX, [7], None, 1)
    assert lib.calls[2][0] == "l5dh_counters_add" and lib.calls[2][4] == 0


def test_rollup(ce, lib):
    ce.write(0, np.arange(10, dtype=np.int64))
    lib.calls.clear()
    ce.incr(0, 100)
    g = np.array([0, 1, N.NO_GROUP, 1], np.int64)
    out = ce.rollup(g, 3, first=0, count=4)
    np.testing.assert_array_equal(out, [100, 1 + 3, 0])
    assert lib.calls == [("l5dh_counters_add", CTX, [0], [100], 1),
                         ("l5dh_counters_rollup", CTX, 0, 4, [0, 1, N.NO_GROUP, 1], 3, "ptr")]
    lib.calls.clear()
    np.testing.assert_array_equal(ce.rollup(np.zeros(0, np.uint32), 2, first=10, count=0), [0, 0])
    assert lib.calls == [("l5dh_counters_rollup", CTX, 10, 0, None, 2, "ptr")]


def test_grow_move_info_kernel_time(ce, lib):
    ce.incr(1, 1)
    ce.grow(20)
    assert ce.capacity == 20
    assert lib.calls == [("l5dh_counters_add", CTX, [1], [1], 1), ("l5dh_counters_resize", CTX, 20)]
    lib.calls.clear()
    ce.grow(20)  # (the same size is a resize too: the library returns at once)
    other = stub_engine(lib, ctx=0x2000)
    old = ce.engine
    ce.incr(2, 2)
    ce.move_to(other)
    assert ce.engine is other
    assert lib.calls == [("l5dh_counters_resize", CTX, 20), ("l5dh_counters_add", CTX, [2], [2], 1),
                         ("l5dh_counters_move", CTX, 0x2000)]
    lib.calls.clear()
    assert ce.info() == {"max_counters": 20, "adds": 9, "lds_adds": 7, "global_adds": 2, "dropped": 1}
    assert lib.calls == [("l5dh_counters_info", 0x2000, "c_uint", "c_ulong", "c_ulong", "c_ulong", "c_ulong")]
    assert ce.kernel_time(reset=True) == (1.5, 3)
    assert lib.calls[1] == ("l5dh_kernel_time", 0x2000, N.K_COUNTERS, 1)
    assert N.K_COUNTERS == 9 and N.KERNEL_NAMES[9] == "counters" and len(N.KERNEL_NAMES) == 10
    old._ctx = ctypes.c_void_p()


def test_a_failing_library_call_raises_and_is_not_resent(lib):
    lib.fail["l5dh_counters_add"] = -22
    c = CounterEngine(stub_engine(lib), 4, batch=2)
    c.incr(0)
    with pytest.raises(N.L5dhError, match="stub text"):
        c.incr(1)
    del lib.fail["l5dh_counters_add"]
    lib.calls.clear()
    c.flush()
    assert lib.calls == []  # the failed batch was dropped, not sent twice
    lib.fail["l5dh_counters_move"] = -17
    with pytest.raises(N.L5dhError):
        c.move_to(stub_engine(lib, ctx=0x2000))
    assert c.engine._ctx.value == CTX
    c.engine._ctx = ctypes.c_void_p()


# ---- refusals before the library is called -------------------------------------------------------
def test_constructor_refusals(lib):
    e = stub_engine(lib)
    for bad in (0, -1, N.MAX_COUNTERS + 1):
        with pytest.raises(ValueError, match="capacity"):
            CounterEngine(e, bad)
    for bad in (1.5, "3", True, None):
        with pytest.raises(TypeError):
            CounterEngine(e, bad)
    for bad in (0, -4, (1 << 30) + 1):
        with pytest.raises(ValueError, match="batch"):
            CounterEngine(e, 4, batch=bad)
    closed = stub_engine(lib, ctx=0)
    with pytest.raises(ValueError, match="open"):
        CounterEngine(closed, 4)
    with pytest.raises(ValueError, match="open"):
        CounterEngine(object(), 4)
    assert lib.calls == []
    e._ctx = ctypes.c_void_p()


def test_delta_must_be_an_int32(ce, lib):
    for bad in (2 ** 31, -2 ** 31 - 1, 2 ** 63, -2 ** 70):
        with pytest.raises(ValueError, match="Int"):
            ce.incr(0, bad)
    ce.incr(0, 2 ** 31 - 1)
    ce.incr(0, -2 ** 31)
    ce.incr(0, np.int32(-7))
    assert ce.get(0) == -8 and lib.calls[0][3] == [2 ** 31 - 1, -2 ** 31, -7]
    # the host Metric.Counter keeps its behaviour: any Python integer
    m = Metric.Counter()
    m.incr(2 ** 40)
    assert m.get() == 2 ** 40 and m.counter_id is None


def test_argument_refusals(ce, lib):
    for call in (lambda: ce.get(10), lambda: ce.get(-1), lambda: ce.release(10), lambda: ce.read(5, 6),
                 lambda: ce.read(-1, 1), lambda: ce.write(9, np.zeros(2, np.int64)), lambda: ce.write(0, None, count=11),
                 lambda: ce.grow(9), lambda: ce.grow(N.MAX_COUNTERS + 1),
                 lambda: ce.rollup(np.zeros(10, np.uint32), 0), lambda: ce.rollup(np.zeros(10, np.uint32), (1 << 24) + 1),
                 lambda: ce.rollup(np.zeros(9, np.uint32), 2),  # a map shorter than the range
                 lambda: ce.rollup(np.full(10, -1, np.int64), 2), lambda: ce.rollup(np.full(10, 2 ** 32, np.int64), 2),
                 lambda: ce.add(np.zeros(3, np.uint32), np.zeros(2, np.int32)),
                 lambda: ce.write(0, np.zeros(2, np.int64), count=3),
                 lambda: ce.move_to(ce.engine), lambda: ce.move_to(stub_engine(lib, ctx=0)),
                 lambda: ce.move_to(stub_engine(lib, ctx=0x2000, device=1))):
        with pytest.raises(ValueError):
            call()
        assert lib.calls == []
    for call in (lambda: ce.get(1.0), lambda: ce.get(True), lambda: ce.grow("20"), lambda: ce.rollup(np.zeros(10), 2),
                 lambda: ce.rollup(np.zeros(10, np.uint32), 2.0), lambda: ce.add(np.zeros(3, np.float32)),
                 lambda: ce.add(np.zeros(3, np.uint32), np.zeros(3, np.int64)), lambda: ce.write(0, np.zeros(2, np.int32)),
                 lambda: ce.add([1, 2])):
        with pytest.raises((TypeError, AttributeError)):
            call()
    assert lib.calls == []


# ---- the registry ----------------------------------------------------------------------------------
def test_registry_and_free_list(lib):
    c = CounterEngine(stub_engine(lib), 3, batch=8)
    lib.calls.clear()
    assert [c.register() for _ in range(3)] == [0, 1, 2] and c.registered == 3
    with pytest.raises(RuntimeError, match="full"):
        c.register()
    c.incr(1, 5)
    c.release(1)  # flushes, then writes 0, then the id is free
    assert lib.calls == [("l5dh_counters_add", CTX, [1], [5], 1), ("l5dh_counters_write", CTX, 1, 1, None)]
    assert c.registered == 2 and lib.values[1] == 0
    c.release(0)
    assert [c.register(), c.register()] == [0, 1]  # the free list is a stack
    assert c.get(1) == 0
    c.engine._ctx = ctypes.c_void_p()


def test_checkpoint_and_restore(lib):
    c = CounterEngine(stub_engine(lib), 8, batch=8)
    for _ in range(5):
        c.register()
    c.incr(0, -3)
    c.incr(4, 2 ** 31 - 1)
    c.release(2)
    lib.calls.clear()
    c.incr(3, 1)
    ck = c.checkpoint()
    assert lib.calls == [("l5dh_counters_add", CTX, [3], [1], 1), ("l5dh_counters_read", CTX, 0, 5, "ptr")]
    np.testing.assert_array_equal(ck["counter_values"], [-3, 0, 0, 1, 2 ** 31 - 1])
    assert ck["counter_next"].tolist() == [5] and ck["counter_free"].tolist() == [2]
    lib2 = StubLib()
    d = CounterEngine(stub_engine(lib2), 6)
    lib2.calls.clear()
    d.restore(ck)
    assert lib2.calls == [("l5dh_counters_write", CTX, 0, 5, [-3, 0, 0, 1, 2 ** 31 - 1])]
    assert d.registered == 4 and d.register() == 2 and d.register() == 5
    with pytest.raises(RuntimeError, match="fresh"):
        d.restore(ck)
    small = CounterEngine(stub_engine(StubLib()), 4)
    with pytest.raises(ValueError, match="holds 5"):
        small.restore(ck)
    with pytest.raises(ValueError, match="belong"):
        CounterEngine(stub_engine(StubLib()), 8).restore(dict(ck, counter_free=np.array([7], np.uint32)))
    for x in (c, d, small):
        x.engine._ctx = ctypes.c_void_p()


# ---- Metric.Counter over a CounterEngine ------------------------------------------------------------
def test_tree_counters_hold_ids_and_prune_hands_them_back(lib):
    c = CounterEngine(stub_engine(lib), 4, batch=16)
    tree = MetricsTree(counters=c)
    a, b = tree.resolve(["rt", "x", "a"]).mk_counter(), tree.resolve(["rt", "x", "b"]).mk_counter()
    assert (a.counter_id, b.counter_id) == (0, 1) and tree.resolve(["rt", "x", "a"]).mk_counter() is a
    a.incr()
    a.incr(41)
    b.incr(-1)
    lib.calls.clear()
    assert a.get() == 42 and b.get() == -1
    assert lib.calls[0] == ("l5dh_counters_add", CTX, [0, 0, 1], [1, 41, -1], 3)
    with pytest.raises(ValueError, match="Int"):
        a.incr(2 ** 31)
    lib.calls.clear()
    tree.resolve(["rt", "x"]).prune()
    assert a.counter_id is None and b.counter_id is None and c.registered == 0
    assert ("l5dh_counters_write", CTX, 0, 1, None) in lib.calls and ("l5dh_counters_write", CTX, 1, 1, None) in lib.calls
    assert a.get() == 42  # (its last value; no exporter reads it any more)
    lib.calls.clear()
    a.incr(5)  # pruned: nothing is staged for an id that was handed back
    c.flush()
    assert lib.calls == [] and a.get() == 42
    n = tree.resolve(["new"]).mk_counter()
    assert n.counter_id in (0, 1) and n.get() == 0
    # a tree without a CounterEngine is as before
    plain = MetricsTree().resolve(["c"]).mk_counter()
    plain.incr(3)
    assert plain.get() == 3 and plain.counter_id is None
    c.engine._ctx = ctypes.c_void_p()


def test_bulk_reads_answer_get_without_a_call_per_counter(lib):
    c = CounterEngine(stub_engine(lib), 4, batch=16)
    tree = MetricsTree(counters=c)
    ms = [tree.resolve([f"c{i}"]).mk_counter() for i in range(4)]
    for i, m in enumerate(ms):
        m.incr(i + 1)
    lib.calls.clear()
    with c.bulk_reads():
        assert [m.get() for m in ms] == [1, 2, 3, 4]
        seen = []
        t = threading.Thread(target=lambda: seen.append(c.bulk_value(0)))  # another thread has no bulk block
        t.start()
        t.join()
        assert seen == [None]
    assert [x[0] for x in lib.calls] == ["l5dh_counters_add", "l5dh_counters_read"]  # one flush, one copy
    assert c.bulk_value(0) is None
    c.engine._ctx = ctypes.c_void_p()
