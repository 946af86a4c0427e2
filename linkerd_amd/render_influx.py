"""The InfluxDB line protocol body rendered on the device (l5dh_render_influx): the table
of a tree, its pure-Python replay, and the call over a HistogramEngine's argument rules.

An InfluxDB line is a measurement head followed by the fields of every metric directly
under one parent, sorted together by key, so the rows of the table are **fields** in the
order they are printed, beside a small table of **lines**.  Row j prints

    ( first row of its line ? head[l] host tail[l] : "," )  key  "="  value  ( last row of its line ? "\\n" : "" )

with l = line[j]; a row is first when j == 0 or line[j-1] != l, last when j == n-1 or
line[j+1] != l.  A line id without rows prints nothing, so take() drops the eleven rows of
a Stat without a snapshot and renumbers nothing.  render_host is that grammar in Python:
the table's executable specification.
"""
from __future__ import annotations

import ctypes
from typing import List

import numpy as np

from . import _native as N
from .engine import QUERY, _numel  # noqa: F401  (QUERY: for the callers)
from .javafmt import double_to_string, float_to_string, long_to_string
from .nametable import (NO_INDEX, counter_ids, escape_key, gather_texts, kind_of, nonempty, pack_texts, scalar_ordinals,  # noqa: F401
                        scalar_values, scrape_rows, series_index, uploader, utf16_key, walk)
from .render_json import value_args
from .telemetry import MetricsTree

ROOT_PREFIX = ("root",)
# a Stat's fields as InfluxDbTelemeter prints them: (key suffix, the field's index in the summary record)
STAT_FIELDS = (("_count", N.BY_COUNT), ("_sum", N.BY_SUM), ("_avg", N.BY_AVG), ("_min", N.BY_MIN), ("_max", N.BY_MAX),
               ("_p50", N.BY_P50), ("_p90", N.BY_P90), ("_p95", N.BY_P95), ("_p99", N.BY_P99), ("_p999", N.BY_P9990),
               ("_p9999", N.BY_P9999))
influx_values, _pack = scalar_values, pack_texts  # (the names this module's earlier callers know them by)


class InfluxTable:
    """What l5dh_render_influx needs of the names, none of which varies per scrape.  Per
    field row: ``line`` (uint32, non-decreasing, < nlines), ``kinds`` (uint8, _native.KIND_*),
    ``field`` (uint8: a stat row's field in the summary record, the BY_* numbering),
    ``index`` (uint32: the element of the row's kind's value array) and the whole field key
    as UTF-8 behind ``key_off`` / ``key_bytes``.  Per line: the text up to and including
    ``host=`` (``head_off`` / ``head_bytes``) and the text after the host value up to and
    including the space (``tail_off`` / ``tail_bytes``).  Host tables also keep ``metrics``,
    the metric behind each row, ``stats``, the tree's Stats, and ``stat_ord``, a stat row's
    Stat in that list."""

    def __init__(self, line, kinds, field, index, key_off, key_bytes, head_off, head_bytes, tail_off, tail_bytes,
                 metrics=None, stats=None, stat_ord=None):
        self.line, self.kinds, self.field, self.index = line, kinds, field, index
        self.key_off, self.key_bytes = key_off, key_bytes
        self.head_off, self.head_bytes, self.tail_off, self.tail_bytes = head_off, head_bytes, tail_off, tail_bytes
        self.metrics, self.stats, self.stat_ord = metrics, stats, stat_ord

    @property
    def n(self) -> int:
        return int(self.key_off.shape[0]) - 1

    @property
    def nlines(self) -> int:
        return int(self.head_off.shape[0]) - 1

    def with_index(self, index) -> "InfluxTable":
        """The same rows printing other elements of the value arrays."""
        t = InfluxTable(*self._arrays())
        t.index = index
        return t

    def _arrays(self):
        return (self.line, self.kinds, self.field, self.index, self.key_off, self.key_bytes, self.head_off,
                self.head_bytes, self.tail_off, self.tail_bytes, self.metrics, self.stats, self.stat_ord)

    def take(self, rows) -> "InfluxTable":
        """The table of the given field rows, in that order (a host table); the lines stay
        as they are."""
        rows = np.asarray(rows, np.int64)
        metrics = None if self.metrics is None else [self.metrics[int(r)] for r in rows]
        stat_ord = None if self.stat_ord is None else self.stat_ord[rows]
        return InfluxTable(self.line[rows], self.kinds[rows], self.field[rows], self.index[rows],
                           *gather_texts(self.key_off, self.key_bytes, rows), self.head_off, self.head_bytes,
                           self.tail_off, self.tail_bytes, metrics, self.stats, stat_ord)

    def to_device(self, device: int = 0) -> "InfluxTable":
        """The same table in device memory (torch tensors): uploaded once, reused by every
        scrape."""
        return InfluxTable(*map(uploader(device), self._arrays()[:10]), self.metrics, self.stats, self.stat_ord)


def influx_table(tree: MetricsTree) -> InfluxTable:
    """The table of ``tree``, walked exactly as influxdb.write_metrics walks it under the
    tags ``host=<host>``: lines numbered as they are emitted (post-order, deeper lines
    first), the same prefix rewrite, escape and ``root`` prefix, the same stable sorts by
    UTF-16 code units over a line's fields in child order and over its tags.  Every Stat has
    its eleven rows, snapshot or not; a stat row's ``index`` is the series id (NO_INDEX
    without one), a counter's or gauge's its ordinal among the table's rows of its kind -- or,
    for a counter that lives in a CounterEngine, its counter id."""
    line: List[int] = []
    kinds: List[int] = []
    field: List[int] = []
    keys: List[str] = []
    metrics: list = []
    stat_ord: List[int] = []
    stats: list = []
    ord_of = {}  # a Stat's place in ``stats``: the walk reaches it before the parent that prints it
    heads: List[str] = []
    tails: List[str] = []
    HOST = ("host", "")  # the request's tag: found again by identity after the sort
    suffixes = [sfx for sfx, _ in STAT_FIELDS]
    stat_kinds, stat_words = [N.KIND_STAT] * 11, [f for _, f in STAT_FIELDS]

    for prefix, tags, t, children in walk(tree, (), (HOST,), post=True):  # deeper lines first
        if t is not tree and kind_of(t.metric) == N.KIND_STAT:
            ord_of[t.metric] = len(stats)
            stats.append(t.metric)
        # the line's fields in child order, a column each (no object per field: a tree of 10^5 Stats has 10^6)
        ks, kd, fl, ms, so = [], [], [], [], []
        for name, child in children.items():
            m = child.metric
            kind = kind_of(m)
            if kind == N.KIND_STAT:
                ks += [name + sfx for sfx in suffixes]
                kd += stat_kinds
                fl += stat_words
                ms += [m] * 11
                so += [ord_of[m]] * 11
            elif kind is not None:
                ks.append(name)
                kd.append(kind)
                fl.append(0)
                ms.append(m)
                so.append(0)
        if not ks:
            continue
        # the tags split at the host entry itself (tag values are arbitrary text: no placeholder is searched for)
        tags = sorted(tags, key=lambda kv: utf16_key(kv[0]))
        at = next(i for i, kv in enumerate(tags) if kv is HOST)
        measurement = escape_key(":".join(prefix if prefix else ROOT_PREFIX))
        heads.append(measurement + "".join(f",{k}={v}" for k, v in tags[:at]) + ",host=")
        tails.append("".join(f",{k}={v}" for k, v in tags[at + 1:]) + " ")
        # the stable sort by key, as a permutation (ASCII keys: the code-point order is the UTF-16 order)
        ascii_keys = all(map(str.isascii, ks))
        order = sorted(range(len(ks)), key=ks.__getitem__ if ascii_keys else lambda i: utf16_key(ks[i]))
        line.extend([len(heads) - 1] * len(ks))
        for column, values in ((keys, ks), (kinds, kd), (field, fl), (metrics, ms), (stat_ord, so)):
            column.extend([values[i] for i in order])

    kinds_a = np.asarray(kinds, np.uint8)
    # a stat row's index is its Stat's series id; a counter's or a gauge's its ordinal among the rows of its kind
    ids = np.asarray(series_index(stats) + [NO_INDEX], np.int64)
    index = scalar_ordinals(ids[np.asarray(stat_ord, np.int64)] if kinds else np.zeros(0, np.int64), kinds_a)
    index = counter_ids(index, kinds_a, metrics)
    return InfluxTable(np.asarray(line, np.uint32), kinds_a, np.asarray(field, np.uint8), index.astype(np.uint32),
                       *pack_texts(keys), *pack_texts(heads), *pack_texts(tails), metrics, stats,
                       np.asarray(stat_ord, np.uint32))


def scrape_inputs(table: InfluxTable, summaries=None):
    """(table, summaries, counters, gauges) of one scrape of a host table, as render_influx
    takes them.  ``summaries``: the snapshot's records indexed by series id, host or device
    -- the rows of a Stat without a series id are dropped; None takes each Stat's
    snapshotted summary, its index its ordinal among the Stats that have one, and drops
    the rows of a Stat without one.  An empty value array is None."""
    counters, gauges = scalar_values(table)
    stat_of = np.where(table.kinds == N.KIND_STAT, table.stat_ord.astype(np.int64), -1)
    table, summaries = scrape_rows(table, table.stats, summaries, stat_of)
    return table, summaries, nonempty(counters), nonempty(gauges)


def _host_bytes(host) -> bytes:
    return host.encode("utf-8") if isinstance(host, str) else bytes(host)


def render_host(table: InfluxTable, host, summaries, counters, gauges) -> bytes:
    """The row grammar replayed in Python over the arrays of a host table, numbers by
    javafmt: what l5dh_render_influx writes.  ``summaries``: the numpy summary dtype."""
    host = _host_bytes(host)
    n, line = table.n, table.line
    key, head, tail = table.key_bytes.tobytes(), table.head_bytes.tobytes(), table.tail_bytes.tobytes()
    ko, ho, to = ([int(x) for x in off] for off in (table.key_off, table.head_off, table.tail_off))
    out: List[bytes] = []
    for j in range(n):
        l, kind, i = int(line[j]), int(table.kinds[j]), int(table.index[j])
        if j == 0 or int(line[j - 1]) != l:
            out += [head[ho[l]:ho[l + 1]], host, tail[to[l]:to[l + 1]]]
        else:
            out.append(b",")
        out += [key[ko[j]:ko[j + 1]], b"="]
        if kind == N.KIND_COUNTER:
            text = long_to_string(int(counters[i]))
        elif kind == N.KIND_GAUGE:
            text = float_to_string(float(gauges[i]))
        else:
            f = int(table.field[j])
            v = summaries[i][N.SUMMARY_FIELDS[f]]
            text = double_to_string(float(v)) if f == N.BY_AVG else long_to_string(int(v))
        out.append(text.encode("ascii"))
        if j == n - 1 or int(line[j + 1]) != l:
            out.append(b"\n")
    return b"".join(out)


def influx_names(engine, table: InfluxTable) -> "N.InfluxNames":
    """The l5dh_influx_names of a table (numpy arrays, or torch tensors on the engine's
    GPU): every array checked as every other buffer is."""
    n, nl = table.n, table.nlines
    return N.InfluxNames(engine._buf(table.line, (np.uint32, np.int32), "table.line", n),
                         engine._buf(table.kinds, (np.uint8,), "table.kinds", n),
                         engine._buf(table.field, (np.uint8,), "table.field", n),
                         engine._buf(table.index, (np.uint32, np.int32), "table.index", n),
                         engine._buf(table.key_off, (np.uint64, np.int64), "table.key_off", n + 1),
                         engine._buf(table.key_bytes, (np.uint8,), "table.key_bytes"),
                         engine._buf(table.head_off, (np.uint64, np.int64), "table.head_off", nl + 1),
                         engine._buf(table.head_bytes, (np.uint8,), "table.head_bytes"),
                         engine._buf(table.tail_off, (np.uint64, np.int64), "table.tail_off", nl + 1),
                         engine._buf(table.tail_bytes, (np.uint8,), "table.tail_bytes"))


def render_influx(engine, table: InfluxTable, host, summaries, counters, gauges, out=None):
    """The body of /admin/metrics/influxdb of the rows of ``table`` under the request's
    ``host`` (str, UTF-8 encoded, or bytes), byte for byte InfluxDbTelemeter.render's text:
    a counter row prints counters[index] (int64) as a Java long, a gauge row gauges[index]
    (float32) as Float.toString (never quoted), a stat row field ``field`` of
    summaries[index] (the numpy summary dtype or int64 [n*11]) -- whatever its count is.
    Each value array is host or device memory, or None when no row is of its kind.  Answers
    as render_json does: bytes, or with ``out`` the length written there, or with out=QUERY
    the length alone.  Reads no engine state."""
    values = value_args(engine, summaries, counters, gauges)
    hb = np.frombuffer(_host_bytes(host), np.uint8)
    nm, n, nl = influx_names(engine, table), table.n, table.nlines
    return engine._render(lambda op, cap, ln: engine._lib.l5dh_render_influx(
        engine._ctx, ctypes.byref(nm), n, nl, hb.ctypes.data if hb.size else None, _numel(hb), *values, op, cap, ln),
        "l5dh_render_influx", out)
