"""HistogramEngine: Python face of the C-ABI (one context = one GPU shard).

Mirrors what a JVM caller does through JNI: batched Stat.add (``ingest``) and
the timer-driven snapshot+reset (``snapshot``) of
AdminMetricsExportTelemeter.snapshotHistograms
(reference: telemetry/admin-metrics-export/.../AdminMetricsExportTelemeter.scala:154-162),
plus the RCCL fleet merge (``merge``).

Inputs may be numpy arrays (host) or torch tensors on the engine's GPU; outputs
go to numpy (host) or to caller-provided torch tensors (device).  Every buffer is
checked (dtype, device, size) before it reaches the library.  Calls that take a
device tensor first hand the library an event recorded on torch's current stream
(l5dh_wait_event), so the engine's kernels run after the torch work that produced
their inputs; calls with device outputs return once the outputs are written.

Layout: every argument rule stands once, ahead of the methods that use it: ``_buf``
(any buffer), ``_records`` (records of a structured dtype, or the words that stand for
them), ``_rows`` with ``_whole_rows`` (the live range, or external rows), ``_u32`` and
``_member_map``.  A query family is a ``*_into`` method -- rows, buffers, one C call.
"""
from __future__ import annotations

import ctypes
import errno
from typing import Optional, Sequence

import numpy as np

from . import _native as N

_NP_OF_TORCH = {"torch.int32": np.int32, "torch.uint32": np.uint32, "torch.int64": np.int64, "torch.uint64": np.uint64,
                "torch.float32": np.float32, "torch.float64": np.float64, "torch.uint8": np.uint8}


QUERY = object()  # render_summaries / render_le: out=QUERY asks for the text's length only


def _is_torch(x) -> bool:
    return hasattr(x, "data_ptr") and hasattr(x, "is_cuda")


def _numel(x) -> int:
    return int(x.size) if isinstance(x, np.ndarray) else int(x.numel())


def _np_type(x):
    """The numpy scalar type of an array or tensor (None: neither, or a dtype no call takes)."""
    return x.dtype.type if isinstance(x, np.ndarray) else _NP_OF_TORCH.get(str(getattr(x, "dtype", None)))


_RECORD_NOUN = {N.SUMMARY_DTYPE: "summary records", N.BUCKET_ENTRY_DTYPE: "bucket entries"}


def _record_words(x, rec):
    """(word dtypes, words per record) of a plain array ``x`` that stands for records of
    ``rec``: int64 x 11 for a summary; for a bucket entry one 64-bit word, else two uint32."""
    if rec is N.SUMMARY_DTYPE:
        return (np.int64,), 11
    return ((np.uint64, np.int64), 1) if _np_type(x) in (np.uint64, np.int64) else ((np.uint32, np.int32), 2)


def _record_rows(x, rec):
    """(whole records, words left over) of ``x``: a numpy array of ``rec`` itself, or plain words."""
    if isinstance(x, np.ndarray) and x.dtype == rec:
        return int(x.size), 0
    return divmod(_numel(x), _record_words(x, rec)[1])


def _whole_rows(counts, name: str = "dense counts") -> Optional[int]:
    """The rows of external dense counts, which come as whole rows of 1798 buckets (None: none given)."""
    if counts is None:
        return None
    n, part = divmod(_numel(counts), N.NBUCKETS)
    if part:
        raise ValueError(f"{name} must hold whole rows of 1798 buckets")
    return n


def _u32(a: np.ndarray, what: str, not_integer=None) -> np.ndarray:
    """``a`` as uint32, converted after the range check.  not_integer: what a non-integer
    dtype raises -- None (ingest) converts it silently, import_sparse raises ValueError,
    the cuts TypeError (kept apart until one rule is chosen)."""
    if a.dtype == np.dtype(np.uint32):
        return a
    if a.size and not_integer is not None and a.dtype.kind not in "iu":
        raise not_integer(f"{what}: dtype {a.dtype} is not an integer type")
    if a.size and (a.min() < 0 or a.max() >= 2 ** 32):
        raise ValueError(f"{what} must fit uint32")
    return np.ascontiguousarray(a.astype(np.uint32))


class HistogramEngine:
    """Device-resident BucketedHistograms for ``max_series`` series on one GPU."""

    def __init__(self, max_series: int, device: int = 0):
        self._lib = N.load()
        self._ctx = ctypes.c_void_p()
        rc = self._lib.l5dh_open(ctypes.byref(self._ctx), int(max_series), 1 << int(device))
        if rc != 0:
            raise N.L5dhError(rc, "l5dh_open", f"max_series={max_series} device={device}")
        self.max_series = int(max_series)
        self.device = int(device)
        self._stream = None  # external stream handle the context runs on (None: its own)
        self._events = []
        self._render_cap = {}  # bytes of the last text of each render call
        self.nranks, self.rank = 1, 0

    # -- lifecycle -----------------------------------------------------------
    def close(self):
        if self._ctx:
            self._lib.l5dh_close(self._ctx)
            self._ctx = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, where: str):
        if rc != 0:
            msg = self._lib.l5dh_last_error(self._ctx)
            raise N.L5dhError(rc, where, msg.decode() if msg else "")

    # -- buffer checks -------------------------------------------------------
    def _buf(self, x, dtypes: Sequence, name: str, min_numel: int = 0, writable: bool = False) -> Optional[int]:
        """Raw pointer of a C-contiguous numpy array or torch tensor after checking
        dtype, device and size (ctypes passes no type information)."""
        if x is None:
            return None
        if isinstance(x, np.ndarray):
            if not x.flags["C_CONTIGUOUS"]:
                raise ValueError(f"{name}: array must be C-contiguous")
            if writable and not x.flags["WRITEABLE"]:
                raise ValueError(f"{name}: array is read-only")
            dt = x.dtype.type
        elif _is_torch(x):
            if not x.is_contiguous():
                raise ValueError(f"{name}: tensor must be contiguous")
            if x.is_cuda:
                if x.device.index != self.device:
                    raise ValueError(f"{name}: tensor on cuda:{x.device.index}, engine on cuda:{self.device}")
                self._order_after_torch()
            dt = _NP_OF_TORCH.get(str(x.dtype))
        else:
            raise TypeError(f"{name}: unsupported buffer type {type(x)!r}")
        if dt not in tuple(np.dtype(d).type for d in dtypes):
            raise TypeError(f"{name}: dtype {getattr(x, 'dtype', None)} not in {[np.dtype(d).name for d in dtypes]}")
        if _numel(x) < min_numel:
            raise ValueError(f"{name}: {_numel(x)} elements, at least {min_numel} needed")
        return x.data_ptr() if _is_torch(x) else x.ctypes.data

    def _order_after_torch(self):
        """Order the context's next work after everything queued on torch's current
        stream (an event handoff: no host synchronization)."""
        import torch
        cur = torch.cuda.current_stream(self.device)
        if self._stream is not None and int(self._stream) == cur.cuda_stream:
            return  # the context runs on that stream: already in order (a wait would only idle the GPU)
        ev = torch.cuda.Event()
        ev.record(cur)
        self._check(self._lib.l5dh_wait_event(self._ctx, ev.cuda_event), "l5dh_wait_event")
        self._events.append(ev)  # the handle must outlive the enqueued wait
        del self._events[:-4]

    def _range(self, first: int, count: Optional[int]):
        if count is None:
            count = self.max_series - first
        if first < 0 or count < 0 or first + count > self.max_series:
            raise ValueError(f"series range [{first}, {first + count}) outside [0, {self.max_series})")
        return first, count

    def _rows(self, first: int, count: Optional[int], series, reset: bool, external: Optional[int]):
        """(first, count) of a query's rows: the live range [first, first+count), or rows
        0..external of data from outside (dense counts: _whole_rows; summaries), which
        have no series snapshot and nothing to reset."""
        if external is None:
            return self._range(first, count)
        if series is not None or reset:
            raise ValueError("external rows have no series snapshot and nothing to reset")
        return 0, external

    def _records(self, x, rec, name: str, rows: int = 0, writable: bool = False, records_writable=None):
        """Pointer of at least ``rows`` records: a numpy array of the structured dtype
        ``rec``, or a numpy array / torch tensor of the words that stand for them
        (_record_words; _record_rows counts them).  records_writable=False: a record
        array is not asked to be writable (summary outputs never were; kept)."""
        if x is None:
            return None
        if isinstance(x, np.ndarray) and x.dtype == rec:
            w = writable if records_writable is None else records_writable
            if x.size < rows or not x.flags["C_CONTIGUOUS"] or (w and not x.flags["WRITEABLE"]):
                raise ValueError(f"{name}: needs {rows} contiguous{' writable' if w else ''} {_RECORD_NOUN[rec]}")
            return x.ctypes.data
        dtypes, per = _record_words(x, rec)
        return self._buf(x, dtypes, name, rows * per, writable=writable)

    def _summ_buf(self, x, rows: int, name: str):
        """Pointer of a summary output of ``rows`` rows: int64 [rows*11] or the numpy summary dtype."""
        return self._records(x, N.SUMMARY_DTYPE, name, rows, writable=True, records_writable=False)

    # -- hot path ---------------------------------------------------------------
    def ingest(self, series, values) -> None:
        """Batched Metric.Stat.add: values[i] into series[i] (u32 ids, f32 values)."""
        if isinstance(series, np.ndarray):
            series = np.ascontiguousarray(_u32(series, "series ids"))
        if isinstance(values, np.ndarray):
            values = np.ascontiguousarray(values, np.float32)
        sp, vp, n = self._samples(series, values)
        self._check(self._lib.l5dh_ingest(self._ctx, sp, vp, n), "l5dh_ingest")

    def _samples(self, series, values):
        """(series pointer, values pointer, n) of a batch: u32 (i32) ids, f32 values."""
        n = _numel(series)
        if n != _numel(values):
            raise ValueError("series and values differ in length")
        return self._buf(series, (np.uint32, np.int32), "series"), self._buf(values, (np.float32,), "values"), n

    def ingest_async(self, series, values) -> int:
        """l5dh_ingest_async: returns a ticket; the buffers must stay unchanged until
        ingest_wait(ticket) (host numpy buffers must stay referenced by the caller)."""
        for name, x, dts in (("series", series, (np.uint32, np.int32)), ("values", values, (np.float32,))):
            if isinstance(x, np.ndarray) and (x.dtype.type not in dts or not x.flags["C_CONTIGUOUS"]):
                raise TypeError(f"ingest_async: {name} must be C-contiguous {dts[0].__name__} (no conversion copy)")
        sp, vp, n = self._samples(series, values)
        t = ctypes.c_uint64(0)
        self._check(self._lib.l5dh_ingest_async(self._ctx, sp, vp, n, ctypes.byref(t)), "l5dh_ingest_async")
        return t.value

    def ingest_wait(self, ticket: int) -> None:
        self._check(self._lib.l5dh_ingest_wait(self._ctx, int(ticket)), "l5dh_ingest_wait")

    def snapshot(self, first: int = 0, count: Optional[int] = None, reset: bool = True,
                 with_counts: bool = False):
        """Summaries (numpy structured, HistogramSummary field order) and optional
        dense [count][1798] int32 bucket counts, for series [first, first+count)."""
        first, count = self._range(first, count)
        out = np.zeros(count, dtype=N.SUMMARY_DTYPE)
        counts = np.zeros((count, N.NBUCKETS), dtype=np.int32) if with_counts else None
        self.snapshot_into(out, counts, first, count, reset)
        return (out, counts) if with_counts else out

    def snapshot_into(self, summaries=None, counts=None, first: int = 0, count: Optional[int] = None,
                      reset: bool = True) -> None:
        """Snapshot into caller buffers (device tensors stay on the GPU).  summaries:
        int64 [count*11] (or the numpy summary dtype); counts: int32 [count][1798]."""
        first, count = self._range(first, count)
        sp = self._summ_buf(summaries, count, "summaries")
        cp = self._buf(counts, (np.int32,), "counts", count * N.NBUCKETS, writable=True)
        self._check(self._lib.l5dh_snapshot(self._ctx, first, count, sp, cp, int(reset)), "l5dh_snapshot")

    def peek(self, series: int) -> np.ndarray:
        """Metric.Stat.peek: non-empty buckets as (lower, upper, count)."""
        n = ctypes.c_size_t(0)
        self._check(self._lib.l5dh_peek(self._ctx, int(series), None, 0, ctypes.byref(n)), "l5dh_peek")
        out = np.zeros(n.value, dtype=N.BUCKET_COUNT_DTYPE)
        if n.value:
            self._check(self._lib.l5dh_peek(self._ctx, int(series), out.ctypes.data, n.value, ctypes.byref(n)),
                        "l5dh_peek")
        return out

    def export_state(self, first: int = 0, count: Optional[int] = None, reset: bool = False,
                     counts=None, totals=None):
        """Dense state for the fleet merge; fills caller buffers or returns numpy copies."""
        first, count = self._range(first, count)
        own = counts is None and totals is None
        if own:
            counts = np.zeros((count, N.NBUCKETS), dtype=np.int32)
            totals = np.zeros(count, dtype=np.int64)
        cp = self._buf(counts, (np.int32,), "counts", count * N.NBUCKETS, writable=True)
        tp = self._buf(totals, (np.int64,), "totals", count, writable=True)
        self._check(self._lib.l5dh_export_state(self._ctx, first, count, cp, tp, int(reset)), "l5dh_export_state")
        return (counts, totals) if own else None

    # -- state import and sparse export ---------------------------------------------
    def import_state(self, counts, totals=None, first: int = 0) -> None:
        """l5dh_import_state: dense rows (counts int32 [count][1798], totals int64 [count]
        or None: 0 -- what ``export_state`` returns; numpy, or torch tensors on the engine's
        GPU) are added to series [first, first+count): each then reports what it would had
        it also received the samples behind its row.  A bucket sum above 2^31 - 1 raises
        (ERANGE), a negative count raises (EINVAL); a failing import changes nothing."""
        count = _whole_rows(counts, "counts")
        first = self._first_u32(first)
        cp = self._buf(counts, (np.int32,), "counts")
        tp = self._buf(totals, (np.int64,), "totals", count)
        self._check(self._lib.l5dh_import_state(self._ctx, first, count, cp, tp), "l5dh_import_state")

    @staticmethod
    def _first_u32(first) -> int:
        first = int(first)
        if first < 0 or first >= 2 ** 32:
            raise ValueError(f"first={first} does not fit uint32")
        return first

    def export_sparse_size(self, first: int = 0, count: Optional[int] = None) -> int:
        """The entries ``export_sparse`` of the range would write (the size query)."""
        first, count = self._range(first, count)
        n = ctypes.c_size_t(0)
        self._check(self._lib.l5dh_export_sparse(self._ctx, first, count, None, None, 0, ctypes.byref(n), None, 0),
                    "l5dh_export_sparse")
        return n.value

    def export_sparse_into(self, row_off, entries, totals=None, first: int = 0, count: Optional[int] = None,
                           reset: bool = False) -> int:
        """l5dh_export_sparse into caller buffers (numpy, or torch tensors on the engine's
        GPU): row_off uint64 (int64) [count+1], entries (N.BUCKET_ENTRY_DTYPE, or uint32
        [cap][2], or 64-bit words [cap]), totals int64 [count] or None.  Returns the entry
        count; entries too small for it raise ERANGE with nothing written or reset."""
        rc, n = self._export_sparse(row_off, entries, totals, first, count, reset)
        self._check(rc, "l5dh_export_sparse")
        return n

    def _export_sparse(self, row_off, entries, totals, first, count, reset):
        """(return code, entry count) of l5dh_export_sparse into checked caller buffers."""
        first, count = self._range(first, count)
        rp = self._buf(row_off, (np.uint64, np.int64), "row_off", count + 1, writable=True)
        if row_off is None or entries is None:
            raise ValueError("row_off and entries: output buffers are needed (export_sparse_size is the size query)")
        cap = _record_rows(entries, N.BUCKET_ENTRY_DTYPE)[0]
        ep = self._records(entries, N.BUCKET_ENTRY_DTYPE, "entries", writable=True)
        tp = self._buf(totals, (np.int64,), "totals", count, writable=True)
        n = ctypes.c_size_t(0)
        rc = self._lib.l5dh_export_sparse(self._ctx, first, count, rp, ep, cap, ctypes.byref(n), tp, int(reset))
        return rc, n.value

    def export_sparse(self, first: int = 0, count: Optional[int] = None, reset: bool = False):
        """(row_off uint64 [count+1], entries N.BUCKET_ENTRY_DTYPE [row_off[count]], totals
        int64 [count]): the CSR of the non-empty buckets of series [first, first+count), row
        i's entries at entries[row_off[i]:row_off[i+1]] in ascending bucket order.  ``reset``
        clears the range afterwards, atomically with the export."""
        first, count = self._range(first, count)
        row_off, totals = np.zeros(count + 1, np.uint64), np.zeros(count, np.int64)
        # (the size query and the export are two holds of the lock: samples that arrive in
        # between make the buffer too small, and the export is tried again)
        while True:
            entries = np.zeros(max(1, self.export_sparse_size(first, count)), N.BUCKET_ENTRY_DTYPE)
            rc, n = self._export_sparse(row_off, entries, totals, first, count, reset)
            if rc == -errno.ERANGE and n > entries.size:
                continue
            self._check(rc, "l5dh_export_sparse")
            return row_off, entries[:n], totals

    def import_sparse(self, row_off, entries, totals=None, first: int = 0, series=None) -> None:
        """l5dh_import_sparse: CSR rows (what ``export_sparse`` returns) are added to series
        ``series[i]`` (uint32, strictly ascending) or, without a map, first + i.  Invalid rows
        raise (EINVAL) and a bucket sum above 2^31 - 1 raises (ERANGE), the least offender
        named; a failing import changes nothing."""
        n = _numel(row_off) - 1
        if n < 0:
            raise ValueError("row_off: at least one offset (row_off[0] = 0) is needed")
        first = self._first_u32(first)
        if isinstance(series, np.ndarray):
            series = _u32(series, "series ids", not_integer=ValueError)
        sp = self._buf(series, (np.uint32, np.int32), "series", n)
        if series is not None and _numel(series) != n:
            raise ValueError(f"series: {_numel(series)} ids for {n} rows")
        rp = self._buf(row_off, (np.uint64, np.int64), "row_off")
        if isinstance(row_off, np.ndarray) and isinstance(entries, np.ndarray):
            # (the library reads row_off[n] entries: a host array is checked to hold them, counted in
            # bytes so that an array of a dtype no entry has is still _buf's to refuse, as a TypeError)
            have = entries.nbytes // N.BUCKET_ENTRY_DTYPE.itemsize
            if int(np.asarray(row_off).reshape(-1)[n].astype(np.uint64)) > have:
                raise ValueError(f"entries: row_off[{n}] = {int(row_off.reshape(-1)[n])} entries, {have} given")
        ep = self._records(entries, N.BUCKET_ENTRY_DTYPE, "entries") if entries is not None and _numel(entries) else None
        tp = self._buf(totals, (np.int64,), "totals", n)
        self._check(self._lib.l5dh_import_sparse(self._ctx, sp, first, n, rp, ep, tp), "l5dh_import_sparse")

    def summarize_dense(self, counts, totals, out=None):
        n = _whole_rows(counts, "counts")
        cp = self._buf(counts, (np.int32,), "counts")
        tp = self._buf(totals, (np.int64,), "totals", n)
        own = out is None
        if own:
            out = np.zeros(n, dtype=N.SUMMARY_DTYPE)
        op = self._summ_buf(out, n, "out")
        self._check(self._lib.l5dh_summarize_dense(self._ctx, cp, tp, n, op), "l5dh_summarize_dense")
        return out if own else None

    # -- label rollups ------------------------------------------------------------
    @staticmethod
    def _ngroups(ngroups) -> int:
        ngroups = int(ngroups)
        if ngroups < 1 or ngroups > N.MAX_SERIES:
            raise ValueError(f"ngroups must be in [1, {N.MAX_SERIES}], got {ngroups}")
        return ngroups

    @staticmethod
    def _member_map(group, rows: int, unit: str, torch_uint32_only: bool):
        """The uint32 map of ``rows`` rows to groups.  A numpy int32 / int64 map is
        converted, -1 standing for NO_GROUP; a torch tensor is taken as it is.
        torch_uint32_only: the rollup refuses any other tensor dtype here, the ranking
        leaves int32 (the same words) to _buf (kept apart until one rule is chosen)."""
        if isinstance(group, np.ndarray):
            if group.dtype in (np.dtype(np.int32), np.dtype(np.int64)):
                if group.size and (group.min() < -1 or group.max() > N.NO_GROUP):
                    raise ValueError("group: entries must be -1 (no group) or fit uint32")
                group = np.where(group == -1, N.NO_GROUP, group).astype(np.uint32)
            elif group.dtype != np.dtype(np.uint32):
                raise ValueError(f"group: dtype {group.dtype} is not uint32 (or int32 / int64 with -1 for no group)")
            group = np.ascontiguousarray(group)
        elif not _is_torch(group):
            raise ValueError(f"group: unsupported map type {type(group)!r}")
        elif torch_uint32_only and _np_type(group) is not np.uint32:
            raise ValueError(f"group: dtype {group.dtype} is not uint32")
        if _numel(group) != rows:
            raise ValueError(f"group: {_numel(group)} entries for {rows} {unit}")
        return group

    def _group_map(self, group, ngroups: int, count: int):
        """(map, ngroups) of a rollup of ``count`` series: every entry < ngroups or
        NO_GROUP (entries >= ngroups are found on the device)."""
        ngroups = self._ngroups(ngroups)
        return self._member_map(group, count, "series", torch_uint32_only=True), ngroups

    def _dense_rows(self, dcounts, dtotals, count: int):
        """Pointers of external dense rows (counts int32 [count][1798], totals int64 [count] or None)."""
        return self._buf(dcounts, (np.int32,), "dense counts"), self._buf(dtotals, (np.int64,), "dense totals", count)

    def rollup_into(self, group, ngroups: int, summaries=None, counts=None, totals=None, series=None,
                    first: int = 0, count: Optional[int] = None, reset: bool = False, dense=None) -> None:
        """Exact per-group rollup into caller buffers (numpy, or torch tensors on the
        engine's GPU): summaries int64 [ngroups*11] (or the numpy summary dtype), counts
        int32 [ngroups][1798], totals int64 [ngroups].  dense=None sums the live rows of
        series [first, first+count) (l5dh_rollup; ``series`` then receives the per-series
        summaries of the same state and ``reset`` clears the range, atomically with the
        rollup); dense=(counts, totals) sums external dense rows (l5dh_rollup_dense)."""
        dcounts, dtotals = (None, None) if dense is None else dense
        first, count = self._rows(first, count, series, reset, _whole_rows(dcounts))
        group, ngroups = self._group_map(group, ngroups, count)
        gp = self._buf(group, (np.uint32,), "group", count)
        sp = self._summ_buf(summaries, ngroups, "summaries")
        cp = self._buf(counts, (np.int32,), "counts", ngroups * N.NBUCKETS, writable=True)
        tp = self._buf(totals, (np.int64,), "totals", ngroups, writable=True)
        if dense is not None:
            dcp, dtp = self._dense_rows(dcounts, dtotals, count)
            self._check(self._lib.l5dh_rollup_dense(self._ctx, dcp, dtp, count, gp, ngroups, sp, cp, tp),
                        "l5dh_rollup_dense")
            return
        rp = self._summ_buf(series, count, "series")
        self._check(self._lib.l5dh_rollup(self._ctx, first, count, gp, ngroups, sp, cp, tp, rp, int(reset)),
                    "l5dh_rollup")

    def _rollup_numpy(self, group, ngroups, with_counts, with_series, **kw):
        first, count = (0, 0) if "dense" in kw else self._range(kw.get("first", 0), kw.get("count"))
        ngroups = self._ngroups(ngroups)
        out = np.zeros(ngroups, dtype=N.SUMMARY_DTYPE)
        counts = np.zeros((ngroups, N.NBUCKETS), dtype=np.int32) if with_counts else None
        totals = np.zeros(ngroups, dtype=np.int64) if with_counts else None
        series = np.zeros(count, dtype=N.SUMMARY_DTYPE) if with_series else None
        self.rollup_into(group, ngroups, out, counts, totals, series, **kw)
        res = (out,) + ((counts, totals) if with_counts else ()) + ((series,) if with_series else ())
        return res if len(res) > 1 else out

    def rollup(self, group, ngroups: int, first: int = 0, count: Optional[int] = None, reset: bool = False,
               with_counts: bool = False, with_series: bool = False):
        """Exact summaries of the unions of series [first, first+count) named by
        ``group`` (entry i: the group of series first+i, or NO_GROUP / -1): what one Stat
        fed every member's samples would report.  Returns the group summaries, followed
        by (counts [ngroups][1798], totals [ngroups]) with ``with_counts`` and by the
        per-series summaries of the same state with ``with_series``; ``reset`` clears
        the range atomically with both."""
        return self._rollup_numpy(group, ngroups, with_counts, with_series, first=first, count=count, reset=reset)

    def rollup_dense(self, counts, totals, group, ngroups: int, with_counts: bool = False):
        """The same over external dense rows (counts [n][1798] int32, totals [n] int64 or
        None), e.g. the slice a rank received from ``merge``."""
        return self._rollup_numpy(group, ngroups, with_counts, False, dense=(counts, totals))

    # -- cumulative le buckets ------------------------------------------------------
    @staticmethod
    def le_cuts(bounds):
        """(cuts uint32, le int64) of the requested upper bounds (l5dh_le_cuts): each
        bound is snapped down to the largest exact label le = L[c-1] - 1 <= floor(bound);
        bounds that snap to one cut are dropped, and the cuts come back ascending.
        Cut c counts the samples with (long)value <= le.  +Inf gives cut 1797."""
        b = np.ascontiguousarray(np.asarray(bounds, np.float64).reshape(-1))
        cuts, le = np.zeros(b.size, np.uint32), np.zeros(b.size, np.int64)
        rc = N.load().l5dh_le_cuts(b.ctypes.data, b.size, cuts.ctypes.data, le.ctypes.data)
        if rc != 0:
            raise N.L5dhError(rc, "l5dh_le_cuts", "bounds must be >= 0 and not NaN")
        cuts, keep = np.unique(cuts, return_index=True)
        return cuts, le[keep]

    @staticmethod
    def _cuts(cuts):
        """The uint32 cuts of a call: a torch tensor as it is, anything else as a numpy
        array (range and order are checked by the library)."""
        if _is_torch(cuts):
            return cuts
        return np.ascontiguousarray(_u32(np.asarray(cuts).reshape(-1), "cuts", not_integer=TypeError))

    def le_counts_into(self, cuts, le_out, sums=None, series=None, first: int = 0, count: Optional[int] = None,
                       reset: bool = False, accumulate: bool = False, dense=None) -> None:
        """Exact cumulative bucket counts into caller buffers (numpy, or torch tensors on
        the engine's GPU): le_out uint64 (or int64) [count][K+1] -- per series the counts
        at the K cuts (``le_cuts``), then the row's count (the +Inf bucket); sums int64
        [count] the exact sums.  dense=None reads the live rows of series [first,
        first+count) (l5dh_le; ``series`` then receives the per-series summaries of the
        same state and ``reset`` clears the range, atomically with the buckets);
        dense=(counts, totals) reads external dense rows (l5dh_le_dense).  ``accumulate``
        adds to what the outputs hold: lifetime counters across resetting intervals."""
        dcounts, dtotals = (None, None) if dense is None else dense
        first, count = self._rows(first, count, series, reset, _whole_rows(dcounts))
        cuts = self._cuts(cuts)
        K = _numel(cuts)
        kp = self._buf(cuts, (np.uint32, np.int32), "cuts")
        lp = self._buf(le_out, (np.uint64, np.int64), "le_out", count * (K + 1), writable=True)
        if le_out is None:
            raise ValueError("le_out: an output buffer is needed")
        tp = self._buf(sums, (np.int64,), "sums", count, writable=True)
        if dense is not None:
            dcp, dtp = self._dense_rows(dcounts, dtotals, count)
            self._check(self._lib.l5dh_le_dense(self._ctx, dcp, dtp, count, kp, K, lp, tp, int(bool(accumulate))),
                        "l5dh_le_dense")
            return
        rp = self._summ_buf(series, count, "series")
        self._check(self._lib.l5dh_le(self._ctx, first, count, kp, K, lp, tp, int(bool(accumulate)), rp, int(reset)),
                    "l5dh_le")

    def le_counts(self, cuts, first: int = 0, count: Optional[int] = None, reset: bool = False,
                  with_series: bool = False, accumulate_into=None):
        """(le uint64 [count][K+1], sums int64 [count]) of series [first, first+count),
        followed by the per-series summaries of the same state with ``with_series``;
        ``reset`` clears the range atomically with both.  accumulate_into=(le, sums): the
        results are added to these arrays (which are returned) instead of new ones."""
        first, count = self._range(first, count)
        K = _numel(self._cuts(cuts))
        if accumulate_into is not None:
            le, sums = accumulate_into
        else:
            le, sums = np.zeros((count, K + 1), np.uint64), np.zeros(count, np.int64)
        series = np.zeros(count, dtype=N.SUMMARY_DTYPE) if with_series else None
        self.le_counts_into(cuts, le, sums, series, first=first, count=count, reset=reset,
                            accumulate=accumulate_into is not None)
        return (le, sums, series) if with_series else (le, sums)

    def le_counts_dense(self, counts, totals, cuts):
        """The same over external dense rows (counts [n][1798] int32, totals [n] int64 or
        None), e.g. the g_counts of a rollup: cumulative buckets are linear, so these are
        the members' summed buckets."""
        K = _numel(self._cuts(cuts))
        n = _whole_rows(counts)
        le, sums = np.zeros((n, K + 1), np.uint64), np.zeros(n, np.int64)
        self.le_counts_into(cuts, le, sums, dense=(counts, totals))
        return le, sums

    # -- configurable quantiles ------------------------------------------------------
    @staticmethod
    def _q(q):
        """The float64 quantiles of a call: a torch tensor as it is, anything else as a
        numpy array (count and range are checked by the library)."""
        if _is_torch(q):
            return q
        return np.ascontiguousarray(np.asarray(q, np.float64).reshape(-1))

    def quantiles_into(self, q, out, series=None, first: int = 0, count: Optional[int] = None,
                       reset: bool = False, dense=None) -> None:
        """Exact quantiles into caller buffers (numpy, or torch tensors on the engine's
        GPU): out int64 [count][K] -- per series the value of each of the K quantiles
        ``q`` (float64 in [0, 1], any order, duplicates legal; upstream
        BucketedHistogram.percentile).  dense=None reads the live rows of series [first,
        first+count) (l5dh_quantiles; ``series`` then receives the per-series summaries
        of the same state and ``reset`` clears the range, atomically with the
        quantiles); dense=counts reads external dense rows (l5dh_quantiles_dense)."""
        first, count = self._rows(first, count, series, reset, _whole_rows(dense))
        q = self._q(q)
        K = _numel(q)
        qp = self._buf(q, (np.float64,), "q")
        op = self._buf(out, (np.int64,), "out", count * K, writable=True)
        if out is None:
            raise ValueError("out: an output buffer is needed")
        if dense is not None:
            dcp = self._buf(dense, (np.int32,), "dense counts")
            self._check(self._lib.l5dh_quantiles_dense(self._ctx, dcp, count, qp, K, op), "l5dh_quantiles_dense")
            return
        rp = self._summ_buf(series, count, "series")
        self._check(self._lib.l5dh_quantiles(self._ctx, first, count, qp, K, op, rp, int(reset)), "l5dh_quantiles")

    def quantiles(self, q, first: int = 0, count: Optional[int] = None, reset: bool = False,
                  with_series: bool = False):
        """int64 [count][K]: the K quantiles ``q`` of series [first, first+count), followed
        by the per-series summaries of the same state with ``with_series``; ``reset``
        clears the range atomically with both."""
        first, count = self._range(first, count)
        out = np.zeros((count, _numel(self._q(q))), np.int64)
        series = np.zeros(count, dtype=N.SUMMARY_DTYPE) if with_series else None
        self.quantiles_into(q, out, series, first=first, count=count, reset=reset)
        return (out, series) if with_series else out

    def quantiles_dense(self, counts, q):
        """The same over external dense rows (counts [n][1798] int32), e.g. the g_counts of
        a rollup: the exact quantiles of the members' union."""
        K = _numel(self._q(q))
        out = np.zeros((_whole_rows(counts), K), np.int64)
        self.quantiles_into(q, out, dense=counts)
        return out

    # -- exact top-k ------------------------------------------------------------------
    @staticmethod
    def _top_by(by, allow_quantile: bool = True):
        """(by, q) of a ranking: a field name of SUMMARY_FIELDS, or a float q in [0, 1] for
        BucketedHistogram.percentile(q) (live state only)."""
        if isinstance(by, str):
            if by not in N.SUMMARY_FIELDS:
                raise ValueError(f"by: {by!r} is not one of {N.SUMMARY_FIELDS} (or a float quantile)")
            return N.SUMMARY_FIELDS.index(by), 0.0
        if isinstance(by, (float, np.floating)) or (isinstance(by, (int, np.integer)) and not isinstance(by, bool)):
            if not allow_quantile:
                raise ValueError("by: external summaries rank by a field name only (they hold no buckets)")
            return N.BY_QUANTILE, float(by)
        raise ValueError(f"by: {by!r} is neither a field name nor a float quantile")

    @staticmethod
    def _top_order(order) -> int:
        try:
            return {"largest": N.TOP_LARGEST, "smallest": N.TOP_SMALLEST}[order]
        except (KeyError, TypeError):
            raise ValueError(f"order: {order!r} is not 'largest' or 'smallest'") from None

    def top_into(self, k: int, by, ids, n_out, summaries=None, q_values=None, order: str = "largest",
                 min_count: int = 1, group=None, g: int = 0, first: int = 0, count: Optional[int] = None,
                 reset: bool = False, series=None, values=None) -> None:
        """The exact top ``k`` into caller buffers (numpy, or torch tensors on the engine's
        GPU): ids uint32 [k], n_out uint32 [1] (= min(k, candidates)), summaries int64
        [k*11] (or the numpy summary dtype: the winners' whole summaries), q_values int64
        [k] (``by`` a float q).  Only the first n_out entries of each are written.
        values=None ranks the live rows of series [first, first+count) (l5dh_top; ``series``
        then receives the per-series summaries of the same state and ``reset`` clears the
        range, atomically with the ranking); values=<summaries> ranks external summaries
        (l5dh_top_summaries: numpy summary dtype, or int64 [n*11]), ids being row indices.
        A row is a candidate iff its count >= min_count and (group is None or group[i] == g)."""
        k = int(k)
        if k < 1 or k > N.TOP_LIMIT:
            raise ValueError(f"k must be in [1, {N.TOP_LIMIT}], got {k}")
        by_i, q = self._top_by(by, allow_quantile=values is None)
        order_i = self._top_order(order)
        rows, part = (None, 0) if values is None else _record_rows(values, N.SUMMARY_DTYPE)
        first, count = self._rows(first, count, series, reset, rows)
        if part:
            raise ValueError("values must hold whole summaries of 11 words")
        if group is not None:
            group = self._member_map(group, count, "rows", torch_uint32_only=False)
        gp = self._buf(group, (np.uint32, np.int32), "group", count)  # (a torch int32 map: the same words)
        ip = self._buf(ids, (np.uint32, np.int32), "ids", k, writable=True)
        np_ = self._buf(n_out, (np.uint32, np.int32), "n_out", 1, writable=True)
        if ids is None or n_out is None:
            raise ValueError("ids and n_out: output buffers are needed")
        sp = self._summ_buf(summaries, k, "summaries")
        if values is not None:
            vp = self._records(values, N.SUMMARY_DTYPE, "values", count) if count else None
            self._check(self._lib.l5dh_top_summaries(self._ctx, vp, count, by_i, order_i, int(min_count), gp, int(g), k,
                                                     ip, sp, np_), "l5dh_top_summaries")
            return
        qp = self._buf(q_values, (np.int64,), "q_values", k, writable=True)
        rp = self._summ_buf(series, count, "series")
        self._check(self._lib.l5dh_top(self._ctx, first, count, by_i, q, order_i, int(min_count), gp, int(g), k, ip, sp, qp,
                                       np_, rp, int(reset)), "l5dh_top")

    @staticmethod
    def _top_outputs(k, by_q: bool):
        """Host outputs (ids, n_out, summaries, q values or None) of a ranking of ``k``."""
        kk = max(1, min(int(k), N.TOP_LIMIT))  # (an illegal k is reported by top_into)
        return (np.zeros(kk, np.uint32), np.zeros(1, np.uint32), np.zeros(kk, dtype=N.SUMMARY_DTYPE),
                np.zeros(kk, np.int64) if by_q else None)

    def top(self, k: int, by="p99", order: str = "largest", min_count: int = 1, group=None, g: int = 0,
            first: int = 0, count: Optional[int] = None, reset: bool = False, with_series: bool = False):
        """(ids uint32 [n], summaries [n]) of the ``k`` series of [first, first+count) with
        the largest (``order="smallest"``: smallest) ``by`` -- a field name of
        SUMMARY_FIELDS, or a float q for the exact q-quantile, whose values then follow as
        int64 [n] -- in rank order, equal keys by ascending id; n = min(k, candidates).  The
        per-series summaries of the same state follow with ``with_series``; ``reset`` clears
        the range atomically with the ranking."""
        first, count = self._range(first, count)
        by_q = self._top_by(by)[0] == N.BY_QUANTILE
        ids, n_out, summ, qv = self._top_outputs(k, by_q)
        series = np.zeros(count, dtype=N.SUMMARY_DTYPE) if with_series else None
        self.top_into(k, by, ids, n_out, summ, qv, order=order, min_count=min_count, group=group, g=g, first=first,
                      count=count, reset=reset, series=series)
        n = int(n_out[0])
        return (ids[:n], summ[:n]) + ((qv[:n],) if by_q else ()) + ((series,) if with_series else ())

    def top_summaries(self, values, k: int, by="p99", order: str = "largest", min_count: int = 1, group=None,
                      g: int = 0):
        """(row indices uint32 [n], summaries [n]) of the ``k`` best rows of external
        summaries (numpy summary dtype or int64 [n*11]; a torch tensor on the engine's GPU is
        read in place), e.g. the group summaries of a rollup: "the worst routers"."""
        ids, n_out, summ, _ = self._top_outputs(k, False)
        self.top_into(k, by, ids, n_out, summ, order=order, min_count=min_count, group=group, g=g, values=values)
        n = int(n_out[0])
        return ids[:n], summ[:n]

    # -- Prometheus text on the device ------------------------------------------------
    def _names(self, names) -> "N.Names":
        """The l5dh_names of a prometheus.NameTable (numpy arrays, or torch tensors on the
        engine's GPU): every array checked as every other buffer is."""
        n = names.n
        return N.Names(self._buf(names.index, (np.uint32, np.int32), "names.index", n),
                       self._buf(names.key_off, (np.uint64, np.int64), "names.key_off", n + 1),
                       self._buf(names.key_bytes, (np.uint8,), "names.key_bytes"),
                       self._buf(names.lab_off, (np.uint64, np.int64), "names.lab_off", n + 1),
                       self._buf(names.lab_bytes, (np.uint8,), "names.lab_bytes"))

    def _render(self, call, where: str, out):
        """Runs call(out pointer, cap, byref(len)): into ``out`` (a uint8 buffer; returns
        the length), or into a host buffer of the right size (returns bytes).  The size of
        the last text is tried first, so a steady scrape takes one call, not a query and a
        call."""
        ln = ctypes.c_size_t(0)
        if out is QUERY:
            self._check(call(None, 0, ctypes.byref(ln)), where)
            return ln.value
        if out is not None:
            op = self._buf(out, (np.uint8,), "out", writable=True)
            self._check(call(op, _numel(out), ctypes.byref(ln)), where)
            return ln.value
        cap = self._render_cap.get(where, 0)
        while True:
            buf = np.empty(cap, np.uint8) if cap else None
            rc = call(None if buf is None else buf.ctypes.data, cap, ctypes.byref(ln))
            if rc == 0 and (buf is not None or ln.value == 0):
                self._render_cap[where] = ln.value
                return b"" if buf is None else buf[:ln.value].tobytes()
            if rc == 0 or (rc == -errno.ERANGE and ln.value > cap):
                cap = ln.value  # the size query's answer, or what the text outgrew
                continue
            self._check(rc, where)

    def render_summaries(self, names, values, out=None):
        """The summary blocks (``_count``, ``_sum``, ``_avg``, eight quantile lines) of
        the rows of ``names`` (prometheus.NameTable) from ``values``: summaries as the
        numpy summary dtype or int64 [nvalues*11], host or device; row j prints element
        names.index[j] (index None: j).  Byte for byte prometheus.write_metrics' lines.
        Returns bytes, or with ``out`` (a uint8 numpy array or torch tensor on the
        engine's GPU) writes there and returns the length; out=QUERY writes nothing and
        returns the length the text would have."""
        vp, nvalues = self._records(values, N.SUMMARY_DTYPE, "values"), _record_rows(values, N.SUMMARY_DTYPE)[0]
        nm, n = self._names(names), names.n
        return self._render(lambda op, cap, ln: self._lib.l5dh_render_summaries(
            self._ctx, ctypes.byref(nm), n, vp, nvalues, op, cap, ln), "l5dh_render_summaries", out)

    def render_le(self, names, le_rows, sums, le_labels, out=None):
        """The ``_hist`` blocks (K ``_hist_bucket`` lines, ``le="+Inf"``, ``_hist_sum``,
        ``_hist_count``) of the rows of ``names`` from le_rows uint64 (or int64)
        [nvalues][K+1], sums int64 [nvalues] (None: 0) and the K labels ``le_labels``
        (int64) -- what le_counts / le_cuts return.  Byte for byte
        prometheus.write_histogram_metrics' lines.  Returns as render_summaries does."""
        if not _is_torch(le_labels):
            le_labels = np.ascontiguousarray(np.asarray(le_labels, np.int64).reshape(-1))
        K = _numel(le_labels)
        lp = self._buf(le_labels, (np.int64,), "le_labels")
        nvalues = _numel(le_rows) // (K + 1)
        if nvalues * (K + 1) != _numel(le_rows):
            raise ValueError("le_rows must hold whole rows of K + 1 counts")
        rp = self._buf(le_rows, (np.uint64, np.int64), "le_rows")
        sp = self._buf(sums, (np.int64,), "sums", nvalues)
        nm, n = self._names(names), names.n
        return self._render(lambda op, cap, ln: self._lib.l5dh_render_le(
            self._ctx, ctypes.byref(nm), n, rp, sp, nvalues, lp, K, op, cap, ln), "l5dh_render_le", out)

    def render_quantiles(self, names, q_rows, q, out=None):
        """The configured quantiles' blocks (K lines ``key{..., quantile="<label>"} N``,
        the label Java's Double.toString of the quantile) of the rows of ``names`` from
        q_rows int64 [nvalues][K] and the K quantiles ``q`` (float64) -- what quantiles
        returns and took.  Byte for byte prometheus.write_quantile_metrics' lines.
        Returns as render_summaries does."""
        q = self._q(q)
        K = _numel(q)
        qp = self._buf(q, (np.float64,), "q")
        nvalues = _numel(q_rows) // K if K else 0  # (K = 0 is the library's to refuse)
        if K and nvalues * K != _numel(q_rows):
            raise ValueError("q_rows must hold whole rows of K values")
        rp = self._buf(q_rows, (np.int64,), "q_rows")
        nm, n = self._names(names), names.n
        return self._render(lambda op, cap, ln: self._lib.l5dh_render_quantiles(
            self._ctx, ctypes.byref(nm), n, rp, nvalues, qp, K, op, cap, ln), "l5dh_render_quantiles", out)

    # -- fleet merge (RCCL) ------------------------------------------------------
    @staticmethod
    def comm_unique_id() -> bytes:
        lib = N.load()
        buf = ctypes.create_string_buffer(N.UNIQUE_ID_BYTES)
        rc = lib.l5dh_comm_unique_id(buf)
        if rc != 0:
            raise N.L5dhError(rc, "l5dh_comm_unique_id")
        return buf.raw

    def comm_init_rank(self, uid: bytes, nranks: int, rank: int) -> None:
        if len(uid) != N.UNIQUE_ID_BYTES:
            raise ValueError(f"unique id must be {N.UNIQUE_ID_BYTES} bytes")
        self._check(self._lib.l5dh_comm_init_rank(self._ctx, ctypes.create_string_buffer(uid, len(uid)),
                                                  int(nranks), int(rank)), "l5dh_comm_init_rank")
        self.nranks, self.rank = int(nranks), int(rank)

    @staticmethod
    def _ctx_array(engines: Sequence["HistogramEngine"]):
        return (ctypes.c_void_p * len(engines))(*[e._ctx.value for e in engines])

    @staticmethod
    def _comm_init_group(engines: Sequence["HistogramEngine"], entry: str) -> None:
        rc = getattr(N.load(), entry)(HistogramEngine._ctx_array(engines), len(engines))
        if rc != 0:
            engines[0]._check(rc, entry)
        for i, e in enumerate(engines):
            e.nranks, e.rank = len(engines), i

    @staticmethod
    def comm_init_all(engines: Sequence["HistogramEngine"]) -> None:
        HistogramEngine._comm_init_group(engines, "l5dh_comm_init_all")

    @staticmethod
    def comm_init_loopback(engines: Sequence["HistogramEngine"]) -> None:
        """l5dh_comm_init_loopback: the engines (one device) as an n-rank group whose
        collectives are device copies -- the multi-rank merge path on one GPU (tests)."""
        HistogramEngine._comm_init_group(engines, "l5dh_comm_init_loopback")

    @staticmethod
    def merge_all(engines: Sequence["HistogramEngine"], mode: int = N.MERGE_REDUCE_SCATTER, with_counts: bool = False):
        """l5dh_merge_all over an l5dh_comm_init_all / loopback group: per rank
        (first, count, summaries[, counts, totals]) as numpy."""
        n = len(engines)
        rows = engines[0].merge_rows(mode)
        outs = [np.zeros(rows, dtype=N.SUMMARY_DTYPE) for _ in engines]
        cnts = [np.zeros((rows, N.NBUCKETS), np.int32) for _ in engines] if with_counts else None
        tots = [np.zeros(rows, np.int64) for _ in engines] if with_counts else None
        ptrs = lambda arrs: arrs and (ctypes.c_void_p * n)(*[a.ctypes.data for a in arrs])  # noqa: E731
        firsts, counts = (ctypes.c_uint32 * n)(), (ctypes.c_uint32 * n)()
        rc = N.load().l5dh_merge_all(HistogramEngine._ctx_array(engines), n, int(mode), ptrs(outs), ptrs(cnts),
                                     ptrs(tots), firsts, counts)
        if rc != 0:
            engines[0]._check(rc, "l5dh_merge_all")
        res = []
        for i in range(n):
            f, c = firsts[i], counts[i]
            item = (f, c, outs[i][:c])
            if with_counts:
                item += (cnts[i][:c], tots[i][:c])
            res.append(item)
        return res

    def comm_destroy(self) -> None:
        self._check(self._lib.l5dh_comm_destroy(self._ctx), "l5dh_comm_destroy")
        self.nranks, self.rank = 1, 0

    def merge_rows(self, mode: int = N.MERGE_REDUCE_SCATTER) -> int:
        """Rows each output of ``merge`` must hold."""
        per = -(-self.max_series // self.nranks)
        return per if mode == N.MERGE_REDUCE_SCATTER else self.max_series

    def merge(self, mode: int = N.MERGE_REDUCE_SCATTER, out=None, counts=None, totals=None):
        """Collective fleet merge (l5dh_merge): every rank's samples summed over RCCL,
        then this rank's rows summarized.  Returns (first, count[, summaries]) --
        summaries as numpy when ``out`` is None."""
        rows = self.merge_rows(mode)
        own = out is None
        if own:
            out = np.zeros(rows, dtype=N.SUMMARY_DTYPE)
        op = self._summ_buf(out, rows, "out")
        cp = self._buf(counts, (np.int32,), "counts", rows * N.NBUCKETS, writable=True)
        tp = self._buf(totals, (np.int64,), "totals", rows, writable=True)
        first, count = ctypes.c_uint32(0), ctypes.c_uint32(0)
        self._check(self._lib.l5dh_merge(self._ctx, int(mode), op, cp, tp, ctypes.byref(first), ctypes.byref(count)),
                    "l5dh_merge")
        return (first.value, count.value, out[:count.value]) if own else (first.value, count.value)

    def tile_totals(self) -> np.ndarray:
        """l5dh_tile_totals: records per 32-series tile of the last binned batch."""
        F = (self.max_series + 31) // 32
        out = np.zeros(F, np.uint64)
        self._check(self._lib.l5dh_tile_totals(self._ctx, out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), F),
                    "l5dh_tile_totals")
        return out

    def partition_redos(self):
        """l5dh_partition_redos: (level-1 redos, level-2 redos, level-2 counting first
        passes) since open."""
        a, b, k = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
        if not hasattr(self._lib, "l5dh_partition_redos"):  # (an older A/B build, L5DH_LIB)
            return 0, 0, 0
        self._check(self._lib.l5dh_partition_redos(self._ctx, ctypes.byref(a), ctypes.byref(b), ctypes.byref(k)),
                    "l5dh_partition_redos")
        return a.value, b.value, k.value

    def merge_bytes(self) -> dict:
        """l5dh_merge_bytes: dense / encoded / sent bytes of the last merge."""
        d, e, s = ctypes.c_uint64(0), ctypes.c_uint64(0), ctypes.c_uint64(0)
        self._check(self._lib.l5dh_merge_bytes(self._ctx, ctypes.byref(d), ctypes.byref(e), ctypes.byref(s)),
                    "l5dh_merge_bytes")
        return {"dense": d.value, "encoded": e.value, "sent": s.value}

    # -- plumbing -------------------------------------------------------------
    def sync(self):
        self._check(self._lib.l5dh_sync(self._ctx), "l5dh_sync")

    def set_stream(self, stream_handle: Optional[int]):
        """Run on an external hipStream_t handle (0: the legacy null stream, where
        torch's default stream work runs); None restores the context's own stream."""
        h = N.OWN_STREAM if stream_handle is None else int(stream_handle)
        self._check(self._lib.l5dh_set_stream(self._ctx, h), "l5dh_set_stream")
        self._stream = stream_handle

    def set_param(self, param: int, value: int):
        self._check(self._lib.l5dh_set_param(self._ctx, int(param), int(value)), "l5dh_set_param")

    def kernel_time(self, kernel_id: int, reset: bool = False):
        ms = ctypes.c_double(0)
        n = ctypes.c_int64(0)
        self._check(self._lib.l5dh_kernel_time(self._ctx, kernel_id, ctypes.byref(ms), ctypes.byref(n),
                                               int(reset)), "l5dh_kernel_time")
        return ms.value, n.value

    def kernel_times(self, reset: bool = False) -> dict:
        """The engine's own timed phases (the ids below K_WINDOW; window.Window.kernel_time
        reads the sliding window's)."""
        return {name: self.kernel_time(k, reset) for k, name in enumerate(N.KERNEL_NAMES[:N.K_WINDOW])}
