"""HistogramEngine's whole Python face against a recording library (no GPU): for every
public method the exact C-ABI calls it makes -- their order, every argument, the words an
input pointer leads to after the Python layer's conversions, the event handoffs -- and for
every refused input the exception class, its message, and that the library saw nothing.

The expected traces (tests/golden/engine_calls.json) were written by this module's
``__main__`` from the engine.py of the commit before the argument layer was unified, and
are never written again from a later one: they pin what that file did, copy by copy.
"""
import ctypes
import errno
import json
import os
import zlib
from types import SimpleNamespace

import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd.engine import QUERY, HistogramEngine
from linkerd_amd.prometheus import NameTable

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_calls.json")
S = 6  # series of the engine under the stub
NB = N.NBUCKETS


# ---- the recording library ---------------------------------------------------------------------
def _v(x):
    """A scalar argument as JSON holds it (a context / handle by its value)."""
    if isinstance(x, ctypes.c_void_p):
        return x.value
    if isinstance(x, (bool, np.bool_)):
        return int(x)
    if isinstance(x, np.integer):
        return int(x)
    if isinstance(x, np.floating):
        return float(x)
    assert x is None or isinstance(x, (int, float)), type(x)
    return x


def _p(p):
    """An output (or unconverted input) pointer: NULL or not."""
    return "ptr" if p else None


def _ref(r):
    """A byref: the ctypes type behind it."""
    return "byref:" + type(r._obj).__name__


def _w(p, ctype, n):
    """An input pointer: NULL, or the n words behind it."""
    if not p:
        return None
    return ["ptr"] + list((ctype * int(n)).from_address(int(p)))


def _arr(a):
    """A ctypes array argument: its element type and, for pointers, how many are set."""
    if a is None:
        return None
    vals = list(a)
    if a._type_ is ctypes.c_void_p:
        return [a._type_.__name__, len(vals), sum(1 for v in vals if v)]
    return [a._type_.__name__, len(vals)]


def _set(p, ctype, i, value):
    ctypes.cast(p, ctypes.POINTER(ctype))[i] = value


class RecordingLib:
    """Every l5dh_* entry point: records (name, normalised args) and answers so that the
    two-call methods complete.  ``fail`` maps an entry point to the code it returns;
    ``erange_once`` makes the first fitting export / render call report a larger size."""

    def __init__(self, winners=3, fail=None, erange_once=False):
        self.calls, self.winners, self.fail = [], winners, dict(fail or {})
        self.erange_once = erange_once
        self.sparse_n, self.text_n = 3, 10
        self._last = {}

    def _rec(self, name, *args):
        # (a retry repeats its inputs: words equal to the entry point's previous call are recorded as "same")
        last = self._last.get(name, ())
        same = [isinstance(a, list) and len(a) > 4 and i < len(last) and a == last[i] for i, a in enumerate(args)]
        self.calls.append([name] + ["same" if eq else a for eq, a in zip(same, args)])
        self._last[name] = args
        return self.fail.get(name, 0)

    # lifecycle, plumbing
    def l5dh_open(self, ref, max_series, mask):
        rc = self._rec("l5dh_open", _ref(ref), _v(max_series), _v(mask))
        if rc == 0:
            ref._obj.value = 0x1000
        return rc

    def l5dh_close(self, ctx):
        return self._rec("l5dh_close", _v(ctx))

    def l5dh_last_error(self, ctx):
        self._rec("l5dh_last_error", _v(ctx))
        return b"stub"

    def l5dh_sync(self, ctx):
        return self._rec("l5dh_sync", _v(ctx))

    def l5dh_set_stream(self, ctx, h):
        return self._rec("l5dh_set_stream", _v(ctx), _v(h))

    def l5dh_wait_event(self, ctx, ev):
        return self._rec("l5dh_wait_event", _v(ctx), _p(ev))

    def l5dh_set_param(self, ctx, param, value):
        return self._rec("l5dh_set_param", _v(ctx), _v(param), _v(value))

    def l5dh_kernel_time(self, ctx, kid, ms, n, reset):
        ms._obj.value, n._obj.value = 1.5 + kid, 2 + kid
        return self._rec("l5dh_kernel_time", _v(ctx), _v(kid), _ref(ms), _ref(n), _v(reset))

    def l5dh_tile_totals(self, ctx, out, n):
        for i in range(n):
            out[i] = 7 + i
        return self._rec("l5dh_tile_totals", _v(ctx), type(out).__name__, _v(n))

    def l5dh_partition_redos(self, ctx, a, b, k):
        a._obj.value, b._obj.value, k._obj.value = 1, 2, 3
        return self._rec("l5dh_partition_redos", _v(ctx), _ref(a), _ref(b), _ref(k))

    def l5dh_merge_bytes(self, ctx, d, e, s):
        d._obj.value, e._obj.value, s._obj.value = 30, 20, 10
        return self._rec("l5dh_merge_bytes", _v(ctx), _ref(d), _ref(e), _ref(s))

    # ingest, snapshot, dense state
    def l5dh_ingest(self, ctx, sp, vp, n):
        return self._rec("l5dh_ingest", _v(ctx), _w(sp, ctypes.c_uint32, n), _w(vp, ctypes.c_float, n), _v(n))

    def l5dh_ingest_async(self, ctx, sp, vp, n, ticket):
        ticket._obj.value = 41
        return self._rec("l5dh_ingest_async", _v(ctx), _w(sp, ctypes.c_uint32, n), _w(vp, ctypes.c_float, n), _v(n),
                         _ref(ticket))

    def l5dh_ingest_wait(self, ctx, ticket):
        return self._rec("l5dh_ingest_wait", _v(ctx), _v(ticket))

    def l5dh_snapshot(self, ctx, first, count, out, counts, reset):
        return self._rec("l5dh_snapshot", _v(ctx), _v(first), _v(count), _p(out), _p(counts), _v(reset))

    def l5dh_peek(self, ctx, series, out, cap, n):
        n._obj.value = 3
        return self._rec("l5dh_peek", _v(ctx), _v(series), _p(out), _v(cap), _ref(n))

    def l5dh_export_state(self, ctx, first, count, counts, totals, reset):
        return self._rec("l5dh_export_state", _v(ctx), _v(first), _v(count), _p(counts), _p(totals), _v(reset))

    def l5dh_import_state(self, ctx, first, count, counts, totals):
        return self._rec("l5dh_import_state", _v(ctx), _v(first), _v(count), _p(counts), _p(totals))

    def l5dh_summarize_dense(self, ctx, counts, totals, n, out):
        return self._rec("l5dh_summarize_dense", _v(ctx), _p(counts), _p(totals), _v(n), _p(out))

    # sparse state
    def l5dh_export_sparse(self, ctx, first, count, row_off, entries, cap, n, totals, reset):
        rc = self._rec("l5dh_export_sparse", _v(ctx), _v(first), _v(count), _p(row_off), _p(entries), _v(cap), _ref(n),
                       _p(totals), _v(reset))
        if rc == 0 and entries and self.erange_once:
            self.erange_once, self.sparse_n = False, self.sparse_n + 2  # (samples arrived after the size query)
            rc = -errno.ERANGE
        elif rc == 0 and (entries or row_off) and cap < self.sparse_n:
            rc = -errno.ERANGE
        n._obj.value = self.sparse_n
        return rc

    def l5dh_import_sparse(self, ctx, series, first, n, row_off, entries, totals):
        offs = _w(row_off, ctypes.c_uint64, n + 1)
        return self._rec("l5dh_import_sparse", _v(ctx), _w(series, ctypes.c_uint32, n), _v(first), _v(n), offs,
                         _w(entries, ctypes.c_uint32, 2 * offs[-1]) if offs else _p(entries), _p(totals))

    # per-row queries
    def l5dh_rollup(self, ctx, first, count, group, ngroups, summ, counts, totals, series, reset):
        return self._rec("l5dh_rollup", _v(ctx), _v(first), _v(count), _w(group, ctypes.c_uint32, count), _v(ngroups),
                         _p(summ), _p(counts), _p(totals), _p(series), _v(reset))

    def l5dh_rollup_dense(self, ctx, dcounts, dtotals, n, group, ngroups, summ, counts, totals):
        return self._rec("l5dh_rollup_dense", _v(ctx), _p(dcounts), _p(dtotals), _v(n), _w(group, ctypes.c_uint32, n),
                         _v(ngroups), _p(summ), _p(counts), _p(totals))

    def l5dh_le_cuts(self, bounds, n, cuts, le):
        b = _w(bounds, ctypes.c_double, n)
        rc = self._rec("l5dh_le_cuts", b, _v(n), _p(cuts), _p(le))
        for i in range(n if rc == 0 else 0):
            _set(cuts, ctypes.c_uint32, i, int(b[1 + i]) // 10)
            _set(le, ctypes.c_int64, i, int(b[1 + i]) // 10 * 10)
        return rc

    def l5dh_le(self, ctx, first, count, cuts, K, le, sums, accumulate, series, reset):
        return self._rec("l5dh_le", _v(ctx), _v(first), _v(count), _w(cuts, ctypes.c_uint32, K), _v(K), _p(le), _p(sums),
                         _v(accumulate), _p(series), _v(reset))

    def l5dh_le_dense(self, ctx, dcounts, dtotals, n, cuts, K, le, sums, accumulate):
        return self._rec("l5dh_le_dense", _v(ctx), _p(dcounts), _p(dtotals), _v(n), _w(cuts, ctypes.c_uint32, K), _v(K),
                         _p(le), _p(sums), _v(accumulate))

    def l5dh_quantiles(self, ctx, first, count, q, K, out, series, reset):
        return self._rec("l5dh_quantiles", _v(ctx), _v(first), _v(count), _w(q, ctypes.c_double, K), _v(K), _p(out),
                         _p(series), _v(reset))

    def l5dh_quantiles_dense(self, ctx, dcounts, n, q, K, out):
        return self._rec("l5dh_quantiles_dense", _v(ctx), _p(dcounts), _v(n), _w(q, ctypes.c_double, K), _v(K), _p(out))

    def _winners(self, k, ids, top, qo, n_out):
        m = min(self.winners, k)
        _set(n_out, ctypes.c_uint32, 0, m)
        for j in range(m):
            _set(ids, ctypes.c_uint32, j, 10 + j)
            if top:
                _set(top, ctypes.c_int64, j * 11, 100 + j)
            if qo:
                _set(qo, ctypes.c_int64, j, 1000 + j)

    def l5dh_top(self, ctx, first, count, by, q, order, min_count, group, g, k, ids, top, qo, n_out, series, reset):
        rc = self._rec("l5dh_top", _v(ctx), _v(first), _v(count), _v(by), _v(q), _v(order), _v(min_count),
                       _w(group, ctypes.c_uint32, count), _v(g), _v(k), _p(ids), _p(top), _p(qo), _p(n_out), _p(series),
                       _v(reset))
        if rc == 0:
            self._winners(k, ids, top, qo, n_out)
        return rc

    def l5dh_top_summaries(self, ctx, values, n, by, order, min_count, group, g, k, ids, top, n_out):
        rc = self._rec("l5dh_top_summaries", _v(ctx), _w(values, ctypes.c_int64, 11 * n), _v(n), _v(by), _v(order),
                       _v(min_count), _w(group, ctypes.c_uint32, n), _v(g), _v(k), _p(ids), _p(top), _p(n_out))
        if rc == 0:
            self._winners(k, ids, top, None, n_out)
        return rc

    # renders
    def _names(self, ref, n):
        nm = ref._obj
        assert isinstance(nm, N.Names)
        key_off, lab_off = _w(nm.key_off, ctypes.c_uint64, n + 1), _w(nm.lab_off, ctypes.c_uint64, n + 1)
        return [_ref(ref), _w(nm.index, ctypes.c_uint32, n), key_off, _w(nm.key_bytes, ctypes.c_uint8, key_off[-1]),
                lab_off, _w(nm.lab_bytes, ctypes.c_uint8, lab_off[-1])]

    def _text(self, rc, op, cap, ln):
        if rc == 0 and op and self.erange_once and cap >= self.text_n:
            self.erange_once, self.text_n = False, self.text_n + 4  # (the text outgrew the last one)
        ln._obj.value = self.text_n
        if rc != 0 or not op:
            return rc
        if cap < self.text_n:
            return -errno.ERANGE
        ctypes.memmove(op, b"x" * self.text_n, self.text_n)
        return 0

    def l5dh_render_summaries(self, ctx, names, n, values, nvalues, op, cap, ln):
        rc = self._rec("l5dh_render_summaries", _v(ctx), self._names(names, n), _v(n),
                       _w(values, ctypes.c_int64, 11 * nvalues), _v(nvalues), _p(op), _v(cap), _ref(ln))
        return self._text(rc, op, cap, ln)

    def l5dh_render_le(self, ctx, names, n, rows, sums, nvalues, labels, K, op, cap, ln):
        rc = self._rec("l5dh_render_le", _v(ctx), self._names(names, n), _v(n), _p(rows), _p(sums), _v(nvalues),
                       _w(labels, ctypes.c_int64, K), _v(K), _p(op), _v(cap), _ref(ln))
        return self._text(rc, op, cap, ln)

    def l5dh_render_quantiles(self, ctx, names, n, rows, nvalues, q, K, op, cap, ln):
        rc = self._rec("l5dh_render_quantiles", _v(ctx), self._names(names, n), _v(n), _p(rows), _v(nvalues),
                       _w(q, ctypes.c_double, K), _v(K), _p(op), _v(cap), _ref(ln))
        return self._text(rc, op, cap, ln)

    # fleet
    def l5dh_comm_unique_id(self, buf):
        rc = self._rec("l5dh_comm_unique_id", len(buf))
        if rc == 0:
            buf.raw = bytes(range(N.UNIQUE_ID_BYTES))
        return rc

    def l5dh_comm_init_rank(self, ctx, uid, nranks, rank):
        return self._rec("l5dh_comm_init_rank", _v(ctx), [len(uid), zlib.crc32(uid.raw)], _v(nranks), _v(rank))

    def l5dh_comm_init_all(self, ctxs, n):
        return self._rec("l5dh_comm_init_all", _arr(ctxs) + list(ctxs), _v(n))

    def l5dh_comm_init_loopback(self, ctxs, n):
        return self._rec("l5dh_comm_init_loopback", _arr(ctxs) + list(ctxs), _v(n))

    def l5dh_comm_destroy(self, ctx):
        return self._rec("l5dh_comm_destroy", _v(ctx))

    def l5dh_merge(self, ctx, mode, out, counts, totals, first, count):
        first._obj.value, count._obj.value = 1, 2
        return self._rec("l5dh_merge", _v(ctx), _v(mode), _p(out), _p(counts), _p(totals), _ref(first), _ref(count))

    def l5dh_merge_all(self, ctxs, n, mode, outs, counts, totals, firsts, cnts):
        for i in range(n):
            firsts[i], cnts[i] = i, 1
        return self._rec("l5dh_merge_all", _arr(ctxs) + list(ctxs), _v(n), _v(mode), _arr(outs), _arr(counts),
                         _arr(totals), _arr(firsts), _arr(cnts))


def stub_engine(max_series=S, lib=None, ctx=0x1000, **kw):
    """A HistogramEngine over a RecordingLib, built as the other host tests build theirs."""
    e = HistogramEngine.__new__(HistogramEngine)
    e._lib, e._ctx, e.max_series, e.device = lib or RecordingLib(**kw), ctypes.c_void_p(ctx), max_series, 0
    e._stream, e._events, e._render_cap = None, [], {}
    e.nranks, e.rank = 1, 0
    return e


class OnDevice:
    """A CPU tensor that reports itself on cuda:``index``: what _buf sees of a device tensor."""

    def __init__(self, t, index=0):
        self._t, self.is_cuda, self.device, self.dtype = t, True, SimpleNamespace(index=index), t.dtype
        self.shape = t.shape

    def data_ptr(self):
        return self._t.data_ptr()

    def numel(self):
        return self._t.numel()

    def is_contiguous(self):
        return self._t.is_contiguous()


_RECORDS = {str(N.SUMMARY_DTYPE): "summary", str(N.BUCKET_ENTRY_DTYPE): "bucket_entry",
            str(N.BUCKET_COUNT_DTYPE): "bucket_count"}
EMPTY = {"result": None, "error": None, "calls": [], "handoffs": 0, "render_cap": {}}  # (not written to the file)


def _result(r):
    """What a method returned: scalars as they are, arrays by dtype, shape and checksum."""
    if isinstance(r, (tuple, list)):
        return [_result(x) for x in r]
    if isinstance(r, dict):
        return {str(k): _result(v) for k, v in r.items()}
    if isinstance(r, np.ndarray):
        return {"dtype": _RECORDS.get(str(r.dtype), str(r.dtype)), "shape": list(r.shape),
                "crc": zlib.crc32(np.ascontiguousarray(r).tobytes())}
    if isinstance(r, bytes):
        return {"bytes": len(r), "crc": zlib.crc32(r)}
    if isinstance(r, HistogramEngine):
        return "engine"
    return _v(r)


# ---- inputs ----------------------------------------------------------------------------------------
def t(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a))


def dev(a, index=0):
    return OnDevice(t(a), index)


def summ(n):
    a = np.zeros(n, N.SUMMARY_DTYPE)
    a["count"], a["p99"] = np.arange(n) + 1, np.arange(n) * 3
    return a


def words(a):
    return a.view(np.int64).reshape(-1).copy()


def dense(n, extra=0):
    return np.zeros(n * NB + extra, np.int32)


def entries(n):
    a = np.zeros(n, N.BUCKET_ENTRY_DTYPE)
    a["bucket"], a["count"] = np.arange(n) + 5, np.arange(n) + 1
    return a


def ro(a):
    a.flags.writeable = False
    return a


def strided(dtype, n=4):
    return np.zeros((n, 2), dtype)[:, 0]


def names(n=2, index=True, conv=lambda a: a):
    key = [b"key%d" % i for i in range(n)]
    lab = [b'a="%d"' % i for i in range(n)]
    off = lambda parts: np.cumsum([0] + [len(p) for p in parts]).astype(np.uint64)  # noqa: E731
    return NameTable(conv(np.arange(n, dtype=np.uint32)[::-1].copy()) if index else None, conv(off(key)),
                     conv(np.frombuffer(b"".join(key), np.uint8).copy()), conv(off(lab)),
                     conv(np.frombuffer(b"".join(lab), np.uint8).copy()))


ROW_OFF = np.array([0, 1, 3], np.uint64)
G6 = [0, 1, -1, 1, 0, 2]
Q2 = [0.25, 0.995]
u32, i32, i64, u64, f32, f64, u8 = np.uint32, np.int32, np.int64, np.uint64, np.float32, np.float64, np.uint8
z = np.zeros


def two_renders(e):
    return [e.render_summaries(names(), summ(2)), e.render_summaries(names(), summ(2))]


def construct(e):
    with HistogramEngine(9, device=2) as h:
        r = (h.max_series, h.device, h._ctx.value, h._stream, h._events, h._render_cap, h.nranks, h.rank)
    h.close()  # (a second close is no call)
    return r[:3] + (r[3] is None, r[4] == [], r[5] == {}) + r[6:]


def group_of(engines):
    return [(e.nranks, e.rank) for e in engines]


def three(e):
    group = [e, stub_engine(ctx=0x2000, lib=e._lib), stub_engine(ctx=0x3000, lib=e._lib)]
    for other in group[1:]:
        other.close = lambda: None  # (collected whenever: its close must not land in the trace)
    return group


# name -> (call, options of the RecordingLib); every call gets a fresh engine ``e`` of S series
ACCEPTED = {
    "construct_enter_exit_close": (construct, {}),
    "open_fails": (lambda e: HistogramEngine(9, device=1), {"fail": {"l5dh_open": -12}}),
    "check_reports_last_error": (lambda e: e.sync(), {"fail": {"l5dh_sync": -5}}),
    # ingest: ids as lists are not converted (refused below); arrays are
    "ingest_u32_f32": (lambda e: e.ingest(np.array([1, 2, 3], u32), np.array([1, 2.5, 3], f32)), {}),
    "ingest_i64_f64": (lambda e: e.ingest(np.array([1, 2, 2 ** 32 - 1], i64), np.array([1, 2.5, 3], f64)), {}),
    "ingest_i32_ids": (lambda e: e.ingest(np.array([1, 2, 3], i32), np.array([1, 2.5, 3], f32)), {}),
    "ingest_float_ids": (lambda e: e.ingest(np.array([1.0, 2.7, 3.0]), np.array([1, 2, 3], f32)), {}),
    "ingest_strided": (lambda e: e.ingest(np.arange(8, dtype=i64)[::2], np.arange(8, dtype=f32)[::2]), {}),
    "ingest_strided_u32": (lambda e: e.ingest(np.arange(8, dtype=u32)[::2], np.arange(8, dtype=f32)[::2]), {}),
    "ingest_empty": (lambda e: e.ingest(z(0, i64), z(0, f32)), {}),
    "ingest_cpu_torch": (lambda e: e.ingest(t(np.array([4, 5], i32)), t(np.array([1, 2], f32))), {}),
    "ingest_device": (lambda e: e.ingest(dev(np.array([4, 5], i32)), dev(np.array([1, 2], f32))), {}),
    "ingest_async": (lambda e: e.ingest_async(np.array([1, 2], u32), np.array([1, 2], f32)), {}),
    "ingest_async_device": (lambda e: e.ingest_async(dev(np.array([1, 2], u32)), dev(np.array([1, 2], f32))), {}),
    "ingest_wait": (lambda e: e.ingest_wait(np.int64(41)), {}),
    "snapshot": (lambda e: e.snapshot(), {}),
    "snapshot_range_counts": (lambda e: e.snapshot(first=1, count=3, reset=False, with_counts=True), {}),
    "snapshot_into_nothing": (lambda e: e.snapshot_into(), {}),
    "snapshot_into_records": (lambda e: e.snapshot_into(summ(S), dense(S), first=0, reset=False), {}),
    "snapshot_into_words": (lambda e: e.snapshot_into(words(summ(3)), None, first=2, count=3), {}),
    "snapshot_into_device": (lambda e: e.snapshot_into(dev(words(summ(S))), dev(dense(S))), {}),
    "snapshot_into_cpu_torch": (lambda e: e.snapshot_into(t(words(summ(S)))), {}),
    "snapshot_into_read_only_records": (lambda e: e.snapshot_into(ro(summ(S))), {}),  # (records: not checked)
    "peek": (lambda e: e.peek(4), {}),
    "export_state_own": (lambda e: e.export_state(first=1, count=2, reset=True), {}),
    "export_state_buffers": (lambda e: e.export_state(counts=dense(S), totals=z(S, i64)), {}),
    "export_state_counts_only": (lambda e: e.export_state(counts=dev(dense(S))), {}),
    "import_state": (lambda e: e.import_state(dense(2), z(2, i64), first=3), {}),
    "import_state_no_totals_device": (lambda e: e.import_state(dev(dense(2))), {}),
    "export_sparse_size": (lambda e: e.export_sparse_size(1, 2), {}),
    "export_sparse_into_records": (lambda e: e.export_sparse_into(z(S + 1, u64), entries(4), z(S, i64)), {}),
    "export_sparse_into_pairs": (lambda e: e.export_sparse_into(z(3, i64), z((4, 2), u32), first=1, count=2,
                                                                 reset=True), {}),
    "export_sparse_into_odd_pairs": (lambda e: e.export_sparse_into(z(3, i64), z(9, i32), first=1, count=2), {}),
    "export_sparse_into_words64": (lambda e: e.export_sparse_into(z(3, u64), z(5, u64), first=1, count=2), {}),
    "export_sparse_into_device": (lambda e: e.export_sparse_into(dev(z(3, i64)), dev(z(5, i64)), dev(z(2, i64)),
                                                                  first=1, count=2), {}),
    "export_sparse_into_too_small": (lambda e: e.export_sparse_into(z(3, u64), entries(2), first=1, count=2), {}),
    "export_sparse": (lambda e: e.export_sparse(), {}),
    "export_sparse_retry": (lambda e: e.export_sparse(first=1, count=2, reset=True), {"erange_once": True}),
    "export_sparse_fails": (lambda e: e.export_sparse(), {"fail": {"l5dh_export_sparse": -22}}),
    "import_sparse_records": (lambda e: e.import_sparse(ROW_OFF, entries(3), z(2, i64), first=2), {}),
    "import_sparse_pairs": (lambda e: e.import_sparse(ROW_OFF.astype(i64), entries(3).view(u32)), {}),
    "import_sparse_words64": (lambda e: e.import_sparse(ROW_OFF, entries(3).view(u64)), {}),
    "import_sparse_series_i64": (lambda e: e.import_sparse(ROW_OFF, entries(3), series=np.array([1, 4], i64)), {}),
    "import_sparse_series_u32": (lambda e: e.import_sparse(ROW_OFF, entries(3), series=np.array([1, 4], u32)), {}),
    "import_sparse_series_i32": (lambda e: e.import_sparse(ROW_OFF, entries(3), series=np.array([1, 4], i32)), {}),
    "import_sparse_series_strided_i64": (lambda e: e.import_sparse(ROW_OFF, entries(3),
                                                                  series=np.array([1, 0, 4, 0], i64)[::2]), {}),
    "import_sparse_empty_rows": (lambda e: e.import_sparse(z(3, u64), entries(0)), {}),
    "import_sparse_no_entries": (lambda e: e.import_sparse(z(1, u64), None), {}),
    "import_sparse_device": (lambda e: e.import_sparse(dev(ROW_OFF), dev(entries(3).view(u32)), dev(z(2, i64)),
                                                        series=dev(np.array([1, 4], i32))), {}),
    "summarize_dense_own": (lambda e: e.summarize_dense(dense(2), z(2, i64)), {}),
    "summarize_dense_out_words": (lambda e: e.summarize_dense(dense(2).reshape(2, NB), None, out=z(22, i64)), {}),
    "summarize_dense_device": (lambda e: e.summarize_dense(dev(dense(2)), dev(z(2, i64)), out=dev(z(22, i64))), {}),
    # rollups
    "rollup_u32": (lambda e: e.rollup(np.array([0, 1, N.NO_GROUP, 1, 0, 2], u32), 3), {}),
    "rollup_i32": (lambda e: e.rollup(np.array(G6, i32), 3, reset=True, with_counts=True), {}),
    "rollup_i64_range_series": (lambda e: e.rollup(np.array(G6[:4], i64), 3, first=1, count=4, with_series=True), {}),
    "rollup_all_outputs": (lambda e: e.rollup(np.array(G6, i64), 3, with_counts=True, with_series=True), {}),
    "rollup_dense": (lambda e: e.rollup_dense(dense(2), z(2, i64), np.array([1, -1], i32), 2, with_counts=True), {}),
    "rollup_dense_no_totals": (lambda e: e.rollup_dense(dense(2), None, np.array([1, 0], u32), 2), {}),
    "rollup_into_nothing": (lambda e: e.rollup_into(np.array(G6, i32), 3), {}),
    "rollup_into_words": (lambda e: e.rollup_into(np.array(G6, i64)[::-1], 3, z(33, i64), dense(3), z(3, i64),
                                                  z(S * 11, i64), reset=True), {}),
    "rollup_into_device": (lambda e: e.rollup_into(dev(np.array([0, 1, 2, 1, 0, 2], u32)), 3, dev(z(33, i64)),
                                                   dev(dense(3)), dev(z(3, i64)), dev(z(S * 11, i64))), {}),
    "rollup_into_cpu_torch_map": (lambda e: e.rollup_into(t(np.array([0, 1, 2, 1, 0, 2], u32)), 3, summ(3)), {}),
    "rollup_into_dense_device": (lambda e: e.rollup_into(dev(np.array([0, 1], u32)), 2, dev(z(22, i64)),
                                                         dense=(dev(dense(2)), dev(z(2, i64)))), {}),
    # le
    "le_cuts": (lambda e: e.le_cuts([100.0, 25, 104, 7]), {}),
    "le_cuts_static": (lambda e: HistogramEngine.le_cuts(np.array([50, 10], f32)), {}),
    "le_cuts_fails": (lambda e: e.le_cuts([-1.0]), {"fail": {"l5dh_le_cuts": -22}}),
    "le_counts_list": (lambda e: e.le_counts([3, 9, 1797]), {}),
    "le_counts_i64_series": (lambda e: e.le_counts(np.array([3, 9], i64), first=1, count=2, reset=True,
                                                   with_series=True), {}),
    "le_counts_u32": (lambda e: e.le_counts(np.array([[3, 9]], u32)), {}),
    "le_counts_strided_cuts": (lambda e: e.le_counts(np.array([3, 0, 9, 0], u32)[::2]), {}),
    "le_counts_no_cuts": (lambda e: e.le_counts([]), {}),
    "le_counts_torch_cuts": (lambda e: e.le_counts(t(np.array([3, 9], i32))), {}),
    "le_counts_accumulate_into": (lambda e: e.le_counts([3, 9], reset=True, with_series=True,
                                                        accumulate_into=(z((S, 3), u64), z(S, i64))), {}),
    "le_counts_dense": (lambda e: e.le_counts_dense(dense(2), z(2, i64), [3, 9]), {}),
    "le_counts_dense_no_totals": (lambda e: e.le_counts_dense(dense(2).reshape(2, NB), None, np.array([3], u32)), {}),
    "le_counts_into_i64_no_sums": (lambda e: e.le_counts_into([3, 9], z(S * 3, i64), accumulate=1), {}),
    "le_counts_into_device": (lambda e: e.le_counts_into(dev(np.array([3, 9], u32)), dev(z(S * 3, u64)),
                                                         dev(z(S, i64)), dev(z(S * 11, i64)), reset=True), {}),
    "le_counts_into_dense_device": (lambda e: e.le_counts_into([3], dev(z(4, u64)), dev(z(2, i64)),
                                                               dense=(dev(dense(2)), None), accumulate=True), {}),
    # quantiles
    "quantiles_list": (lambda e: e.quantiles(Q2), {}),
    "quantiles_f32_series": (lambda e: e.quantiles(np.array([0.5, 0.25], f32), first=1, count=2, reset=True,
                                                   with_series=True), {}),
    "quantiles_scalar": (lambda e: e.quantiles(0.5), {}),
    "quantiles_torch_q": (lambda e: e.quantiles(t(np.array(Q2))), {}),
    "quantiles_dense": (lambda e: e.quantiles_dense(dense(2), Q2), {}),
    "quantiles_into_device": (lambda e: e.quantiles_into(dev(np.array(Q2)), dev(z(S * 2, i64)), dev(z(S * 11, i64)),
                                                         reset=True), {}),
    "quantiles_into_dense_device": (lambda e: e.quantiles_into(Q2, dev(z(4, i64)), dense=dev(dense(2))), {}),
    # top
    "top_default": (lambda e: e.top(5), {}),
    "top_field_smallest": (lambda e: e.top(2, "avg", order="smallest", min_count=0, first=1, count=4, reset=True), {}),
    "top_quantile_series": (lambda e: e.top(4, 0.995, with_series=True), {}),
    "top_int_quantile": (lambda e: e.top(4, 1), {}),
    "top_limit": (lambda e: e.top(N.TOP_LIMIT, "count"), {}),
    "top_group_u32": (lambda e: e.top(3, group=np.array([0, 1, N.NO_GROUP, 1, 0, 2], u32), g=1), {}),
    "top_group_i32": (lambda e: e.top(3, group=np.array(G6, i32), g=1), {}),
    "top_group_i64": (lambda e: e.top(3, group=np.array(G6, i64), g=np.int64(2)), {}),
    "top_group_torch_i32": (lambda e: e.top(3, group=t(np.array(G6, i32)), g=1), {}),
    "top_group_torch_u32": (lambda e: e.top(3, group=t(np.array(G6, i32).astype(u32)), g=1), {}),
    "top_summaries_records": (lambda e: e.top_summaries(summ(4), 2, "avg", order="smallest", min_count=3,
                                                        group=np.array([0, -1, 0, 0], i64), g=0), {}),
    "top_summaries_words": (lambda e: e.top_summaries(words(summ(4)), 7, "sum"), {}),
    "top_summaries_empty": (lambda e: e.top_summaries(summ(0), 2), {}),
    "top_summaries_empty_words": (lambda e: e.top_summaries(z(0, i64), 2), {}),
    "top_summaries_cpu_torch": (lambda e: e.top_summaries(t(words(summ(4))), 2), {}),
    "top_into_words_q": (lambda e: e.top_into(2, 0.5, z(2, u32), z(1, u32), z(22, i64), z(2, i64), series=summ(S)), {}),
    "top_into_bare": (lambda e: e.top_into(2, "max", z(2, i32), z(1, i32)), {}),
    "top_into_device": (lambda e: e.top_into(2, 0.5, dev(z(2, i32)), dev(z(1, i32)), dev(z(22, i64)), dev(z(2, i64)),
                                             group=dev(np.array(G6, i32)), g=1, series=dev(z(S * 11, i64)),
                                             reset=True), {}),
    "top_into_values_device": (lambda e: e.top_into(2, "p99", dev(z(2, i32)), dev(z(1, i32)), dev(z(22, i64)),
                                                    values=dev(words(summ(4))), group=dev(z(4, u32))), {}),
    "top_fails": (lambda e: e.top(5), {"fail": {"l5dh_top": -22}}),
    # renders
    "render_summaries_records": (lambda e: e.render_summaries(names(), summ(2)), {}),
    "render_summaries_words_no_index": (lambda e: e.render_summaries(names(index=False), words(summ(3))), {}),
    "render_summaries_query": (lambda e: e.render_summaries(names(), summ(2), out=QUERY), {}),
    "render_summaries_out": (lambda e: e.render_summaries(names(), summ(2), out=z(64, u8)), {}),
    "render_summaries_out_too_small": (lambda e: e.render_summaries(names(), summ(2), out=z(4, u8)), {}),
    "render_summaries_device": (lambda e: e.render_summaries(names(conv=dev), dev(words(summ(2))),
                                                             out=dev(z(64, u8))), {}),
    "render_summaries_cpu_torch": (lambda e: e.render_summaries(names(conv=t), t(words(summ(2))), out=t(z(64, u8))), {}),
    "render_summaries_i64_offsets": (lambda e: e.render_summaries(names(conv=lambda a: a.astype(
        {u32: i32, u64: i64}.get(a.dtype.type, a.dtype.type))), summ(2)), {}),
    "render_summaries_retry": (lambda e: e.render_summaries(names(), summ(2)), {"erange_once": True}),
    "render_summaries_twice": (two_renders, {}),
    "render_summaries_fails": (lambda e: e.render_summaries(names(), summ(2)), {"fail": {"l5dh_render_summaries": -22}}),
    "render_le": (lambda e: e.render_le(names(), z((2, 3), u64), z(2, i64), [10, 20]), {}),
    "render_le_i64_no_sums_query": (lambda e: e.render_le(names(), z(6, i64), None, np.array([10, 20], i32), out=QUERY),
                                    {}),
    "render_le_out_device": (lambda e: e.render_le(names(conv=dev), dev(z(6, u64)), dev(z(2, i64)),
                                                   dev(np.array([10, 20], i64)), out=dev(z(32, u8))), {}),
    "render_quantiles": (lambda e: e.render_quantiles(names(), z((2, 2), i64), Q2), {}),
    "render_quantiles_query": (lambda e: e.render_quantiles(names(), z(4, i64), np.array(Q2, f32), out=QUERY), {}),
    "render_quantiles_no_q": (lambda e: e.render_quantiles(names(), z(4, i64), [], out=QUERY), {}),
    "render_quantiles_out_device": (lambda e: e.render_quantiles(names(conv=dev), dev(z(4, i64)), dev(np.array(Q2)),
                                                                 out=dev(z(32, u8))), {}),
    # fleet
    "comm_unique_id": (lambda e: e.comm_unique_id(), {}),
    "comm_unique_id_fails": (lambda e: e.comm_unique_id(), {"fail": {"l5dh_comm_unique_id": -5}}),
    "comm_init_rank": (lambda e: (e.comm_init_rank(bytes(range(128)), np.int64(4), 3), e.nranks, e.rank), {}),
    "comm_init_all": (lambda e: (HistogramEngine.comm_init_all(three(e)[:2]), e.nranks, e.rank), {}),
    "comm_init_all_ranks": (lambda e: (lambda g: (HistogramEngine.comm_init_all(g), group_of(g)))(three(e)), {}),
    "comm_init_all_fails": (lambda e: HistogramEngine.comm_init_all(three(e)), {"fail": {"l5dh_comm_init_all": -5}}),
    "comm_init_loopback_ranks": (lambda e: (lambda g: (HistogramEngine.comm_init_loopback(g), group_of(g)))(three(e)),
                                 {}),
    "comm_init_loopback_fails": (lambda e: HistogramEngine.comm_init_loopback(three(e)),
                                 {"fail": {"l5dh_comm_init_loopback": -5}}),
    "comm_destroy": (lambda e: (setattr(e, "nranks", 3), e.comm_destroy(), e.nranks, e.rank), {}),
    "merge_rows": (lambda e: (setattr(e, "nranks", 4), e.merge_rows(), e.merge_rows(N.MERGE_ALL_REDUCE)), {}),
    "merge_own": (lambda e: e.merge(), {}),
    "merge_all_reduce_buffers": (lambda e: e.merge(N.MERGE_ALL_REDUCE, out=z(S * 11, i64), counts=dense(S),
                                                   totals=z(S, i64)), {}),
    "merge_device": (lambda e: e.merge(out=dev(z(S * 11, i64)), counts=dev(dense(S)), totals=dev(z(S, i64))), {}),
    "merge_all": (lambda e: HistogramEngine.merge_all(three(e)), {}),
    "merge_all_counts": (lambda e: HistogramEngine.merge_all(three(e)[:2], N.MERGE_ALL_REDUCE, with_counts=True), {}),
    "merge_all_fails": (lambda e: HistogramEngine.merge_all(three(e)), {"fail": {"l5dh_merge_all": -5}}),
    "tile_totals": (lambda e: e.tile_totals(), {}),
    "partition_redos": (lambda e: e.partition_redos(), {}),
    "merge_bytes": (lambda e: e.merge_bytes(), {}),
    "sync": (lambda e: e.sync(), {}),
    "set_stream": (lambda e: (e.set_stream(0), e._stream, e.set_stream(None), e._stream, e.set_stream(77)), {}),
    "set_param": (lambda e: e.set_param(np.int32(N.PARAM_TIMING), True), {}),
    "kernel_time": (lambda e: e.kernel_time(2, reset=True), {}),
    "kernel_times": (lambda e: e.kernel_times(), {}),
}

BAD_DENSE = dense(2, extra=1)
ok_ids, ok_n = (lambda: z(5, u32)), (lambda: z(1, u32))

# calls that must be refused before the library sees anything
REFUSED = {
    # _buf and _range, through the calls that reach them first
    "buf_not_contiguous": lambda e: e.snapshot_into(counts=strided(i32, S * NB)),
    "buf_read_only": lambda e: e.snapshot_into(counts=ro(dense(S))),
    "buf_tensor_not_contiguous": lambda e: e.snapshot_into(counts=t(z((S * NB, 2), i32))[:, 0]),
    "buf_other_device": lambda e: e.snapshot_into(counts=dev(dense(S), index=1)),
    "buf_unsupported_type": lambda e: e.snapshot_into(counts=[0] * (S * NB)),
    "buf_dtype": lambda e: e.snapshot_into(counts=z(S * NB, i64)),
    "buf_torch_dtype": lambda e: e.snapshot_into(counts=t(z(S * NB, np.int16))),
    "buf_too_small": lambda e: e.snapshot_into(counts=dense(S)[1:]),
    "range_past_end": lambda e: e.snapshot(first=4, count=3),
    "range_negative_first": lambda e: e.snapshot_into(first=-1, count=1),
    "range_negative_count": lambda e: e.export_state(first=1, count=-1),
    "summ_buf_few_records": lambda e: e.snapshot_into(summ(S - 1)),
    "summ_buf_strided_records": lambda e: e.snapshot_into(summ(2 * S)[::2]),
    "summ_buf_few_words": lambda e: e.snapshot_into(z(S * 11 - 1, i64)),
    # ingest
    "ingest_list_ids": lambda e: e.ingest([1, 2], np.array([1, 2], f32)),
    "ingest_negative_id": lambda e: e.ingest(np.array([-1, 2]), np.array([1, 2], f32)),
    "ingest_id_past_u32": lambda e: e.ingest(np.array([1, 2 ** 32]), np.array([1, 2], f32)),
    "ingest_lengths": lambda e: e.ingest(np.array([1, 2, 3], u32), np.array([1, 2], f32)),
    "ingest_torch_ids_i64": lambda e: e.ingest(t(np.array([1, 2], i64)), t(np.array([1, 2], f32))),
    "ingest_async_dtype": lambda e: e.ingest_async(np.array([1, 2], i64), np.array([1, 2], f32)),
    "ingest_async_values_dtype": lambda e: e.ingest_async(np.array([1, 2], u32), np.array([1, 2], f64)),
    "ingest_async_strided": lambda e: e.ingest_async(strided(u32), z(4, f32)),
    "ingest_async_lengths": lambda e: e.ingest_async(z(3, u32), z(2, f32)),
    # the seven places that divide by 1798 (and the conveniences in front of them)
    "whole_rows_import_state": lambda e: e.import_state(BAD_DENSE),
    "whole_rows_summarize_dense": lambda e: e.summarize_dense(BAD_DENSE, None),
    "whole_rows_rollup_into": lambda e: e.rollup_into(z(2, u32), 1, dense=(BAD_DENSE, None)),
    "whole_rows_rollup_dense": lambda e: e.rollup_dense(BAD_DENSE, None, z(2, u32), 1),
    "whole_rows_le_counts_into": lambda e: e.le_counts_into([3], z(4, u64), dense=(BAD_DENSE, None)),
    "whole_rows_le_counts_dense": lambda e: e.le_counts_dense(BAD_DENSE, None, [3]),
    "whole_rows_quantiles_into": lambda e: e.quantiles_into(Q2, z(4, i64), dense=BAD_DENSE),
    "whole_rows_quantiles_dense": lambda e: e.quantiles_dense(BAD_DENSE, Q2),
    # dense state
    "import_state_negative_first": lambda e: e.import_state(dense(1), first=-1),
    "import_state_first_past_u32": lambda e: e.import_state(dense(1), first=2 ** 32),
    "import_state_few_totals": lambda e: e.import_state(dense(2), z(1, i64)),
    "import_state_counts_dtype": lambda e: e.import_state(dense(1).astype(u32)),
    "summarize_dense_few_totals": lambda e: e.summarize_dense(dense(2), z(1, i64)),
    "summarize_dense_small_out": lambda e: e.summarize_dense(dense(2), None, out=summ(1)),
    "export_state_small_totals": lambda e: e.export_state(counts=dense(S), totals=z(S - 1, i64)),
    # sparse state
    "export_sparse_into_no_row_off": lambda e: e.export_sparse_into(None, entries(4)),
    "export_sparse_into_no_entries": lambda e: e.export_sparse_into(z(S + 1, u64), None),
    "export_sparse_into_small_row_off": lambda e: e.export_sparse_into(z(S, u64), entries(4)),
    "export_sparse_into_entries_read_only": lambda e: e.export_sparse_into(z(S + 1, u64), ro(entries(4))),
    "export_sparse_into_entries_strided": lambda e: e.export_sparse_into(z(S + 1, u64), entries(8)[::2]),
    "export_sparse_into_entries_dtype": lambda e: e.export_sparse_into(z(S + 1, u64), z(8, f32)),
    "export_sparse_into_range": lambda e: e.export_sparse_into(z(S + 1, u64), entries(4), first=S, count=1),
    "export_sparse_size_range": lambda e: e.export_sparse_size(0, S + 1),
    "export_sparse_range": lambda e: e.export_sparse(first=-1),
    "import_sparse_no_offsets": lambda e: e.import_sparse(z(0, u64), entries(0)),
    "import_sparse_negative_first": lambda e: e.import_sparse(ROW_OFF, entries(3), first=-1),
    "import_sparse_first_past_u32": lambda e: e.import_sparse(ROW_OFF, entries(3), first=2 ** 32),
    "import_sparse_float_series": lambda e: e.import_sparse(ROW_OFF, entries(3), series=np.array([1.0, 4.0])),
    "import_sparse_negative_series": lambda e: e.import_sparse(ROW_OFF, entries(3), series=np.array([-1, 4])),
    "import_sparse_series_past_u32": lambda e: e.import_sparse(ROW_OFF, entries(3), series=np.array([1, 2 ** 32])),
    "import_sparse_series_list": lambda e: e.import_sparse(ROW_OFF, entries(3), series=[1, 4]),
    "import_sparse_few_series": lambda e: e.import_sparse(ROW_OFF, entries(3), series=np.array([1], u32)),
    "import_sparse_many_series": lambda e: e.import_sparse(ROW_OFF, entries(3), series=np.array([1, 2, 3], u32)),
    "import_sparse_few_entries": lambda e: e.import_sparse(ROW_OFF, entries(2)),
    "import_sparse_few_entry_words": lambda e: e.import_sparse(ROW_OFF, z(5, u32)),
    "import_sparse_few_entry_words64": lambda e: e.import_sparse(ROW_OFF, z(2, u64)),
    "import_sparse_series_strided_u32": lambda e: e.import_sparse(ROW_OFF, entries(3),
                                                                  series=np.array([1, 0, 4, 0], u32)[::2]),
    "import_sparse_entries_dtype_f64": lambda e: e.import_sparse(ROW_OFF, z(3, f64)),
    "import_sparse_entries_dtype_f32": lambda e: e.import_sparse(ROW_OFF, z(6, f32)),
    "import_sparse_entries_dtype_c64": lambda e: e.import_sparse(ROW_OFF, z(3, np.complex64)),
    "import_sparse_entries_dtype_u8": lambda e: e.import_sparse(ROW_OFF, z(24, u8)),
    "import_sparse_few_entries_u8": lambda e: e.import_sparse(ROW_OFF, z(16, u8)),
    "import_sparse_row_off_dtype": lambda e: e.import_sparse(ROW_OFF.astype(u32), entries(3)),
    "import_sparse_few_totals": lambda e: e.import_sparse(ROW_OFF, entries(3), z(1, i64)),
    "import_sparse_entries_strided": lambda e: e.import_sparse(ROW_OFF, entries(6)[::2]),
    # group maps: the rollup's rule and the ranking's
    "group_ngroups_zero": lambda e: e.rollup(z(S, u32), 0),
    "group_ngroups_past_limit": lambda e: e.rollup_into(z(S, u32), N.MAX_SERIES + 1),
    "group_ngroups_dense": lambda e: e.rollup_dense(dense(2), None, z(2, u32), -1),
    "group_float_map": lambda e: e.rollup(z(S, f32), 2),
    "group_u16_map": lambda e: e.rollup(z(S, np.uint16), 2),
    "group_below_minus_one": lambda e: e.rollup(np.full(S, -2, i64), 2),
    "group_past_u32": lambda e: e.rollup(np.full(S, 2 ** 32, i64), 2),
    "group_few_entries": lambda e: e.rollup(z(S - 1, u32), 2),
    "group_entries_of_range": lambda e: e.rollup(z(S, u32), 2, first=1, count=3),
    "group_entries_of_dense": lambda e: e.rollup_dense(dense(2), None, z(3, u32), 1),
    "group_list_map": lambda e: e.rollup(G6, 3),
    "group_torch_i32_rollup": lambda e: e.rollup(t(np.array(G6, i32)), 3),
    "group_torch_i64_rollup": lambda e: e.rollup(t(np.array(G6, i64)), 3),
    "group_torch_i64_top": lambda e: e.top(3, group=t(np.array(G6, i64))),
    "group_torch_f32_top": lambda e: e.top(3, group=t(z(S, f32))),
    "group_float_map_top": lambda e: e.top(3, group=z(S, f32)),
    "group_below_minus_one_top": lambda e: e.top(3, group=np.full(S, -2, i32)),
    "group_few_entries_top": lambda e: e.top(3, group=z(S - 1, u32)),
    "group_list_map_top": lambda e: e.top(3, group=G6),
    "group_few_entries_top_summaries": lambda e: e.top_summaries(summ(4), 2, group=z(3, u32)),
    # rollup, le, quantiles: live-or-dense
    "rollup_dense_with_series": lambda e: e.rollup_into(z(2, u32), 1, series=summ(2), dense=(dense(2), None)),
    "rollup_dense_with_reset": lambda e: e.rollup_into(z(2, u32), 1, reset=True, dense=(dense(2), None)),
    "rollup_range": lambda e: e.rollup(z(S, u32), 2, first=3, count=4),
    "rollup_small_summaries": lambda e: e.rollup_into(z(S, u32), 3, summ(2)),
    "rollup_small_series": lambda e: e.rollup_into(z(S, u32), 3, series=summ(S - 1)),
    "rollup_dense_counts_dtype": lambda e: e.rollup_into(z(2, u32), 1, dense=(dense(2).astype(i64), None)),
    "rollup_dense_few_totals": lambda e: e.rollup_into(z(2, u32), 1, dense=(dense(2), z(1, i64))),
    "le_dense_with_series": lambda e: e.le_counts_into([3], z(4, u64), series=summ(2), dense=(dense(2), None)),
    "le_dense_with_reset": lambda e: e.le_counts_into([3], z(4, u64), reset=True, dense=(dense(2), None)),
    "le_no_output": lambda e: e.le_counts_into([3], None),
    "le_small_output": lambda e: e.le_counts_into([3, 9], z(S * 3 - 1, u64)),
    "le_float_cuts": lambda e: e.le_counts(np.array([3.0, 9.0])),
    "le_float_cuts_into": lambda e: e.le_counts_into([3.5], z(S * 2, u64)),
    "le_negative_cuts": lambda e: e.le_counts([-1, 3]),
    "le_cuts_past_u32": lambda e: e.le_counts_dense(dense(1), None, [2 ** 32]),
    "le_torch_cuts_i64": lambda e: e.le_counts(t(np.array([3, 9], i64))),
    "le_range": lambda e: e.le_counts([3], first=5, count=2),
    "le_accumulate_into_small": lambda e: e.le_counts([3], accumulate_into=(z((S, 2), u64), z(S - 1, i64))),
    "quantiles_dense_with_series": lambda e: e.quantiles_into(Q2, z(4, i64), series=summ(2), dense=dense(2)),
    "quantiles_dense_with_reset": lambda e: e.quantiles_into(Q2, z(4, i64), reset=True, dense=dense(2)),
    "quantiles_no_output": lambda e: e.quantiles_into(Q2, None),
    "quantiles_small_output": lambda e: e.quantiles_into(Q2, z(S * 2 - 1, i64)),
    "quantiles_torch_q_f32": lambda e: e.quantiles(t(np.array(Q2, f32))),
    "quantiles_range": lambda e: e.quantiles(Q2, first=S + 1),
    "quantiles_text_q": lambda e: e.quantiles(["a"]),
    # top
    "top_k_zero": lambda e: e.top(0),
    "top_k_past_limit": lambda e: e.top(N.TOP_LIMIT + 1),
    "top_unknown_field": lambda e: e.top(3, "p98"),
    "top_by_none": lambda e: e.top(3, None),
    "top_by_bool": lambda e: e.top(3, True),
    "top_order": lambda e: e.top(3, order="biggest"),
    "top_order_unhashable": lambda e: e.top(3, order=[]),
    "top_range": lambda e: e.top(3, first=3, count=4),
    "top_no_ids": lambda e: e.top_into(5, "p99", None, ok_n()),
    "top_no_n_out": lambda e: e.top_into(5, "p99", ok_ids(), None),
    "top_few_ids": lambda e: e.top_into(5, "p99", z(4, u32), ok_n()),
    "top_small_summaries": lambda e: e.top_into(5, "p99", ok_ids(), ok_n(), summ(4)),
    "top_small_q_values": lambda e: e.top_into(5, 0.5, ok_ids(), ok_n(), q_values=z(4, i64)),
    "top_summaries_quantile": lambda e: e.top_summaries(summ(4), 2, 0.5),
    "top_summaries_unknown_field": lambda e: e.top_summaries(summ(4), 2, "p98"),
    "top_summaries_k_zero": lambda e: e.top_summaries(summ(4), 0),
    "top_summaries_part_words": lambda e: e.top_summaries(z(12, i64), 2),
    "top_summaries_strided_records": lambda e: e.top_summaries(summ(8)[::2], 2),
    "top_summaries_words_dtype": lambda e: e.top_summaries(z(22, u64), 2),
    "top_values_with_reset": lambda e: e.top_into(5, "p99", ok_ids(), ok_n(), values=summ(4), reset=True),
    "top_values_with_series": lambda e: e.top_into(5, "p99", ok_ids(), ok_n(), values=summ(4), series=summ(4)),
    # renders
    "render_summaries_strided_records": lambda e: e.render_summaries(names(), summ(4)[::2]),
    "render_summaries_values_dtype": lambda e: e.render_summaries(names(), z(22, u64)),
    "render_summaries_out_dtype": lambda e: e.render_summaries(names(), summ(2), out=z(64, np.int8)),
    "render_summaries_out_read_only": lambda e: e.render_summaries(names(), summ(2), out=ro(z(64, u8))),
    "render_names_index_dtype": lambda e: e.render_summaries(names(conv=lambda a: a.astype(f32)), summ(2)),
    "render_le_part_rows": lambda e: e.render_le(names(), z(7, u64), None, [10, 20]),
    "render_le_few_sums": lambda e: e.render_le(names(), z(6, u64), z(1, i64), [10, 20]),
    "render_le_rows_dtype": lambda e: e.render_le(names(), z(6, f64), None, [10, 20]),
    "render_le_torch_labels_i32": lambda e: e.render_le(names(), z(6, u64), None, t(np.array([10, 20], i32))),
    "render_quantiles_part_rows": lambda e: e.render_quantiles(names(), z(5, i64), Q2),
    "render_quantiles_rows_dtype": lambda e: e.render_quantiles(names(), z(4, u64), Q2),
    # two things wrong at once: which refusal comes first
    "first_top_reset_then_part_words": lambda e: e.top_into(5, "p99", ok_ids(), ok_n(), values=z(12, i64), reset=True),
    "first_top_part_words_then_group": lambda e: e.top_summaries(z(12, i64), 2, group=z(3, u32)),
    "first_le_dense_cuts_then_rows": lambda e: e.le_counts_dense(BAD_DENSE, None, [3.5]),
    "first_le_into_rows_then_cuts": lambda e: e.le_counts_into([3.5], z(4, u64), dense=(BAD_DENSE, None)),
    "first_quantiles_dense_q_then_rows": lambda e: e.quantiles_dense(BAD_DENSE, ["a"]),
    "first_rollup_rows_then_ngroups": lambda e: e.rollup_dense(BAD_DENSE, None, z(2, u32), 0),
    "first_rollup_range_then_ngroups": lambda e: e.rollup(z(S, u32), 0, first=4, count=4),
    "first_import_state_rows_then_first": lambda e: e.import_state(BAD_DENSE, first=-1),
    "first_import_sparse_first_then_series": lambda e: e.import_sparse(ROW_OFF, entries(3), first=-1,
                                                                       series=np.array([1.0, 4.0])),
    "first_ingest_ids_then_lengths": lambda e: e.ingest(np.array([-1, 2, 3]), z(2, f32)),
    "first_export_sparse_into_range_then_buffers": lambda e: e.export_sparse_into(None, None, first=S, count=1),
    "first_top_k_then_by": lambda e: e.top(0, "p98"),
    "first_top_by_then_range": lambda e: e.top(3, "p98", first=4, count=4),
    # fleet
    "comm_init_rank_short_id": lambda e: e.comm_init_rank(b"short", 2, 0),
    "merge_small_out": lambda e: e.merge(out=summ(S - 1)),
    "merge_small_counts": lambda e: e.merge(counts=dense(S - 1)),
}

# Where the shared helper gave two copies one wording: the class is compared, and that the
# message still names the argument (everything else compares the whole message).
ONE_WORDING = {
    "import_sparse_float_series": "series ids",        # the uint32 coercion's one non-integer message
    # "a dense rollup has" / "dense rows have" / "external summaries have" no series snapshot and ...
    "rollup_dense_with_series": "no series snapshot", "rollup_dense_with_reset": "nothing to reset",
    "le_dense_with_series": "no series snapshot", "le_dense_with_reset": "nothing to reset",
    "quantiles_dense_with_series": "no series snapshot", "quantiles_dense_with_reset": "nothing to reset",
    "top_values_with_series": "no series snapshot", "top_values_with_reset": "nothing to reset",
    "first_top_reset_then_part_words": "nothing to reset",
    "top_summaries_strided_records": "values:",        # "array must be C-contiguous" / "needs N contiguous ..."
    "render_summaries_strided_records": "values:",     # "needs contiguous" / "needs N contiguous summary records"
}


def run_case(call, opts):
    """The trace of one call on a fresh engine: what the library saw (event handoffs
    included, in order), what came back, or the exception."""
    lib = RecordingLib(**opts)
    e = stub_engine(lib=lib)
    e._order_after_torch = lambda: lib.calls.append(["_order_after_torch"])
    load, N.load = N.load, lambda *a: lib  # (the static methods ask _native for the library)
    try:
        try:
            out = {"result": _result(call(e)), "error": None}
        except Exception as ex:  # noqa: BLE001 -- the class is what is recorded
            out = {"result": None, "error": [type(ex).__name__, str(ex)]}
    finally:
        N.load = load
    e._ctx = ctypes.c_void_p()  # (nothing to close)
    out["calls"] = lib.calls
    out["handoffs"] = sum(1 for c in lib.calls if c[0] == "_order_after_torch")
    out["render_cap"] = dict(e._render_cap)
    return {k: v for k, v in json.loads(json.dumps(out)).items() if v != EMPTY[k]}


def all_traces():
    tr = {"accepted": {k: run_case(*v) for k, v in ACCEPTED.items()},
          "refused": {k: run_case(v, {}) for k, v in REFUSED.items()}}
    return tr


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def _whole(trace):
    return {**EMPTY, **trace}


def test_tables_match_the_golden_file(golden):
    assert list(golden["accepted"]) == list(ACCEPTED) and list(golden["refused"]) == list(REFUSED)


@pytest.mark.parametrize("name", list(ACCEPTED))
def test_accepted_call_makes_the_parents_calls(golden, name):
    assert run_case(*ACCEPTED[name]) == golden["accepted"][name]


@pytest.mark.parametrize("name", list(REFUSED))
def test_refused_call_is_refused_as_by_the_parent(golden, name):
    got, want = _whole(run_case(REFUSED[name], {})), _whole(golden["refused"][name])
    assert want["error"] is not None and [c for c in want["calls"] if c[0] != "_order_after_torch"] == []
    if name in ONE_WORDING:
        assert got["error"][0] == want["error"][0]
        assert ONE_WORDING[name] in got["error"][1] and ONE_WORDING[name] in want["error"][1]
        got["error"] = want["error"]
    assert got == want


def test_every_public_method_is_traced(golden):
    public = {n for n, f in vars(HistogramEngine).items() if not n.startswith("_") and callable(getattr(HistogramEngine, n))}
    src = open(__file__).read()
    assert [n for n in sorted(public) if f".{n}(" not in src] == []
    seen = {c[0] for tr in golden["accepted"].values() for c in tr.get("calls", [])}
    entry = {n for n in vars(RecordingLib) if n.startswith("l5dh_")}
    # (l5dh_wait_event is _order_after_torch's, which needs a torch stream: counted above, run on the GPU)
    assert entry - seen == {"l5dh_wait_event"}, "an entry point no accepted call reaches"
    assert entry == {n for n in N.SIGNATURES if n in entry} and seen - entry == {"_order_after_torch"}


def test_the_stub_needs_no_attribute_beyond_the_documented_ones():
    e = stub_engine()
    assert set(vars(e)) == {"_lib", "_ctx", "max_series", "device", "_stream", "_events", "_render_cap", "nranks", "rank"}


if __name__ == "__main__":
    # Writes the expected traces.  Only ever run against the engine.py the traces pin (see
    # the module docstring); a later engine.py is compared with the file, not written to it.
    with open(GOLDEN, "w") as f:  # one case per line
        f.write("{" + ",\n".join(json.dumps(kind) + ": {\n" + ",\n".join(
            json.dumps(k) + ":" + json.dumps(v, separators=(",", ":")) for k, v in cases.items()) + "\n}"
            for kind, cases in all_traces().items()) + "}\n")
    print(GOLDEN, os.path.getsize(GOLDEN), "bytes")
