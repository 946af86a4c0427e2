"""What the exporters share: the labelled walk of a MetricsTree, the name tables the device
renderers read, and the selection of the rows one scrape shows.

The Prometheus and InfluxDB telemeters of the reference rewrite the prefix segments
rt/<router>, rt/service/<path>, rt/client/<id>, rt/client/service/<path>, rt/server/<srv>
into labels while they descend (PrometheusTelemeter.scala:37-135, InfluxDbTelemeter.scala:63-75).
``walk`` is that descent, once: every writer and every table builder is a loop over it.
"""
from __future__ import annotations

import errno
import re
from contextlib import nullcontext
from typing import Iterator, Sequence, Tuple

import numpy as np

from . import _native as N
from .telemetry import Metric, MetricsTree

Labels = Tuple[Tuple[str, str], ...]
NO_INDEX = 0xFFFFFFFF  # a table's index of a Stat without a series id (no device call takes such a row)

_KEY_DISALLOWED = re.compile(r"[^a-zA-Z0-9:]")
# the prefix before a segment that becomes a label -> the label's name
_REWRITES = {("rt",): "rt", ("rt", "service"): "service", ("rt", "client"): "client",
             ("rt", "client", "service"): "service", ("rt", "server"): "server"}
_KIND_OF = {Metric.Counter: N.KIND_COUNTER, Metric.Gauge: N.KIND_GAUGE, Metric.Stat: N.KIND_STAT}


def escape_key(key: str) -> str:
    return _KEY_DISALLOWED.sub("_", key)


def utf16_key(s: str) -> bytes:
    """The sort key of Java's String ordering (UTF-16 code units)."""
    return s.encode("utf-16-be", "surrogatepass")


def rewrite(prefix: Tuple[str, ...], labels: Labels):
    """The segment after a known prefix becomes a label, unless the label exists already."""
    name = _REWRITES.get(prefix[:-1])
    if name is None or any(k == name for k, _ in labels):
        return prefix, labels
    return prefix[:-1], labels + ((name, prefix[-1]),)


def walk(tree: MetricsTree, prefix0: Tuple[str, ...] = (), labels0: Labels = (), post: bool = False
         ) -> Iterator[Tuple[Tuple[str, ...], Labels, MetricsTree, dict]]:
    """(rewritten prefix, labels, node, the node's children) of every node, children in the
    reference's order: a node before its subtree, or with ``post`` after it (InfluxDB's
    lines, deeper first).  The children are the dict the walk itself descends into, so a
    caller that prints them asks the node no second time.  One generator over a stack of
    open nodes, not one per level: a scrape walks 10^5 nodes."""
    top = rewrite(prefix0, labels0) + (tree, tree.children)
    if not post:
        yield top
    open_nodes, rest = [top], [iter(top[3].items())]  # the nodes being descended into, their children not yet visited
    while open_nodes:
        for name, child in rest[-1]:
            below = rewrite(open_nodes[-1][0] + (name,), open_nodes[-1][1]) + (child, child.children)
            if not post:
                yield below
            open_nodes.append(below)
            rest.append(iter(below[3].items()))
            break
        else:
            rest.pop()
            if post:
                yield open_nodes[-1]
            open_nodes.pop()


def kind_of(metric):
    """_native.KIND_COUNTER / KIND_GAUGE / KIND_STAT, or None for a node without a metric."""
    return _KIND_OF.get(type(metric))


def counter_engine(metrics):
    """The counters.CounterEngine behind the device-backed counters among ``metrics`` (those
    of one tree share one), None when the counters are host values."""
    for m in metrics:
        if type(m) is Metric.Counter:
            return m._counters
    return None


def scalar_ordinals(index: np.ndarray, kinds: np.ndarray) -> np.ndarray:
    """``index`` with every counter and gauge row's entry set to its ordinal among the rows
    of its kind: the element of scalar_values' array it prints."""
    for kind in (N.KIND_COUNTER, N.KIND_GAUGE):
        rows = kinds == kind
        index[rows] = np.arange(int(rows.sum()))
    return index


def counter_ids(index: np.ndarray, kinds: np.ndarray, metrics) -> np.ndarray:
    """``index`` (scalar_ordinals') of the rows of ``metrics``: when the counters live in a
    CounterEngine, a counter row's entry becomes its counter id (NO_INDEX once pruned), the
    element of the engine's live array it prints; unchanged for host counters."""
    if counter_engine(metrics) is not None:
        rows = kinds == N.KIND_COUNTER
        index[rows] = [NO_INDEX if m.counter_id is None else m.counter_id
                       for m, is_counter in zip(metrics, rows) if is_counter]
    return index


def series_index(stats) -> list:
    """Per Stat its series id, NO_INDEX without one."""
    return [NO_INDEX if m.series_id is None else int(m.series_id) for m in stats]


def scalar_values(table):
    """(counters int64, gauges float32) of one scrape: the current values of the counter and
    gauge rows of a host table (NameTable with kinds, InfluxTable), each at the element its
    row's ``index`` names.  Counters that live in a CounterEngine are not read: the counters
    are then its live device array (CounterEngine.device_values, a torch tensor), which the
    rows index by counter id -- for a renderer on the CounterEngine's own engine."""
    out = []
    for kind, dtype in ((N.KIND_COUNTER, np.int64), (N.KIND_GAUGE, np.float32)):
        rows = np.flatnonzero(table.kinds == kind)
        ce = counter_engine(table.metrics[int(j)] for j in rows[:1]) if kind == N.KIND_COUNTER else None
        if ce is not None:
            out.append(ce.device_values())
            continue
        values = np.zeros(int(table.index[rows].max()) + 1 if rows.size else 0, dtype)
        values[table.index[rows]] = [table.metrics[int(j)].get() for j in rows]
        out.append(values)
    return tuple(out)


def nonempty(values):
    """A value array of scalar_values, or None when it holds nothing (the renderers' NULL)."""
    return values if (values.size if isinstance(values, np.ndarray) else values.numel()) else None


def bulk_counters(tree: MetricsTree):
    """The block in which a host writer prints ``tree``: with a CounterEngine behind the
    tree's counters, one bulk read of its values answers every counter's get() inside (no
    device read per counter); without one, nothing changes."""
    ce = getattr(tree, "_counters", None)
    return nullcontext() if ce is None else ce.bulk_reads()


# ---- table plumbing --------------------------------------------------------------------------
def pack_texts(texts: Sequence[str]):
    """(n + 1 uint64 offsets, the UTF-8 bytes behind them)."""
    enc = [t.encode("utf-8") for t in texts]
    off = np.zeros(len(enc) + 1, np.uint64)
    off[1:] = np.cumsum(np.asarray([len(b) for b in enc], np.uint64))
    return off, np.frombuffer(b"".join(enc), np.uint8).copy()


def gather_texts(off: np.ndarray, data: np.ndarray, rows: np.ndarray):
    """pack_texts' pair of the given rows (int64), in that order."""
    start = off[rows].astype(np.int64)
    length = off[rows + 1].astype(np.int64) - start
    new = np.zeros(rows.size + 1, np.uint64)
    new[1:] = np.cumsum(length.astype(np.uint64))
    src = np.repeat(start - new[:-1].astype(np.int64), length) + np.arange(int(new[-1]), dtype=np.int64)
    return new, data[src]


def uploader(device: int):
    """numpy array -> torch tensor on cuda:``device`` (None stays None)."""
    import torch
    dev = torch.device("cuda", int(device))

    def up(a):
        if a is None:
            return None
        a = np.ascontiguousarray(a)
        # (the same bits under torch's long-standing signed types)
        a = a.view({8: np.int64, 4: np.int32}.get(a.dtype.itemsize, np.uint8)) if a.dtype.kind == "u" else a
        return torch.from_numpy(a).to(dev)
    return up


class NameTable:
    """What the device renderer (HistogramEngine.render_summaries / render_le) needs of
    the names, none of which varies per scrape: per row the escaped metric key and the
    escaped text between the braces, as UTF-8 bytes behind n + 1 offsets, and ``index``,
    the element of the value arrays the row prints (None: the row's own number).
    ``metrics`` (host tables of a tree) are the rows' Stats.  ``kinds`` (None: every row a
    Stat) is a uint8 per row, _native.KIND_COUNTER / KIND_GAUGE / KIND_STAT, for the calls
    of linkerd_amd.render_json: ``index`` then counts within the row's kind, and
    ``metrics`` holds the rows' metrics of any kind."""

    def __init__(self, index, key_off, key_bytes, lab_off, lab_bytes, metrics=None, kinds=None):
        self.index, self.key_off, self.key_bytes = index, key_off, key_bytes
        self.lab_off, self.lab_bytes, self.metrics = lab_off, lab_bytes, metrics
        self.kinds = kinds

    @property
    def n(self) -> int:
        return int(self.key_off.shape[0]) - 1

    @staticmethod
    def build(keys: Sequence[str], inners: Sequence[str], index=None, metrics=None, kinds=None) -> "NameTable":
        if index is not None:
            index = np.ascontiguousarray(np.asarray(index, np.int64).astype(np.uint32))
        if kinds is not None:
            kinds = np.ascontiguousarray(np.asarray(kinds, np.uint8))
        return NameTable(index, *pack_texts(keys), *pack_texts(inners), metrics, kinds)

    def with_index(self, index) -> "NameTable":
        """The same rows printing other elements of the value arrays."""
        return NameTable(index, self.key_off, self.key_bytes, self.lab_off, self.lab_bytes, self.metrics, self.kinds)

    def take(self, rows) -> "NameTable":
        """The table of the given rows, in that order (a host table)."""
        rows = np.asarray(rows, np.int64)
        index = None if self.index is None else self.index[rows]
        metrics = None if self.metrics is None else [self.metrics[int(r)] for r in rows]
        kinds = None if self.kinds is None else self.kinds[rows]
        return NameTable(index, *gather_texts(self.key_off, self.key_bytes, rows),
                         *gather_texts(self.lab_off, self.lab_bytes, rows), metrics, kinds)

    def to_device(self, device: int = 0) -> "NameTable":
        """The same table in device memory (torch tensors): uploaded once, reused by
        every scrape."""
        up = uploader(device)
        return NameTable(up(self.index), up(self.key_off), up(self.key_bytes), up(self.lab_off), up(self.lab_bytes),
                         self.metrics, up(self.kinds))


# ---- one scrape ----------------------------------------------------------------------------------
def summary_records(summaries) -> np.ndarray:
    """HistogramSummary objects as the engine's summary records."""
    out = np.zeros(len(summaries), N.SUMMARY_DTYPE)
    for f in N.SUMMARY_FIELDS:
        out[f] = [getattr(s, f) for s in summaries]
    return out


def scrape_rows(table, stats, values, stat_of=None, need_snapshot: bool = False):
    """(the rows of a host ``table`` one scrape shows, the records they print).  ``stats``
    are the table's Stats and ``stat_of`` a row's Stat among them (None: row j prints Stat
    j), negative for a counter or gauge row, which always shows.  ``values`` indexed by
    series id (the snapshot's records, host or device): a stat row shows if its ``index``
    is an id -- with ``need_snapshot`` only if its Stat has a snapshot too -- and stays
    the id.  ``values`` None: a stat row shows if its Stat has a snapshot; the records are
    those Stats' snapshots in table order (None without any) and the row's ``index``
    becomes its Stat's ordinal among them."""
    if stat_of is None:
        stat_of = np.arange(table.n)
    scalar = stat_of < 0
    keep = scalar if values is None else scalar | (table.index != NO_INDEX)
    if values is None or need_snapshot:
        snaps = [m.snapshotted_summary for m in stats]
        has = np.asarray([s is not None for s in snaps] + [False], bool)  # (the last: where a scalar row's -1 points)
        keep = keep & has[stat_of] | scalar
        if values is None:
            keep = has[stat_of] | scalar
            ordinal = (np.cumsum(has) - 1).astype(np.uint32)
            table = table.with_index(np.where(scalar, table.index, ordinal[stat_of]))
            values = summary_records([s for s in snaps if s is not None]) if has.any() else None
    return (table if keep.all() else table.take(np.flatnonzero(keep))), values


def device_or_host(device_call, host_call):
    """The device renderer's bytes, or the host writer's when a value lies outside the device
    formatter's domain (the library answers ERANGE)."""
    try:
        return device_call()
    except N.L5dhError as e:
        if e.code != -errno.ERANGE:
            raise
        return host_call()
