"""Prometheus text export from GPU-produced summaries.

Restates PrometheusTelemeter.writeMetrics
(reference: telemetry/prometheus/src/main/scala/io/buoyant/telemetry/prometheus/
PrometheusTelemeter.scala:37-135): prefix segments rt/<router>, rt/service/<path>,
rt/client/<id>, rt/client/service/<path>, rt/server/<srv> are rewritten into labels;
counters print as Java Long, gauges as Java Float, stats print _count/_sum/_avg
(avg as Java Double) plus 8 quantile lines from `snapshotted_summary`, and nothing
before the first snapshot.  Child order follows the tree's map order (the
reference's immutable-Map hash order), so compare outputs as line multisets.
"""
from __future__ import annotations

import re
from typing import List, Sequence, Tuple

import numpy as np

from .javafmt import double_to_string, float_to_string, long_to_string
from .telemetry import Metric, MetricsTree

_METRIC_NAME_DISALLOWED = re.compile(r"[^a-zA-Z0-9:]")
_LABEL_KEY_DISALLOWED = re.compile(r"[^a-zA-Z0-9_]")
_LABEL_VAL_DISALLOWED = re.compile(r'(\\|"|\n)')

Labels = Tuple[Tuple[str, str], ...]


def escape_key(key: str) -> str:
    return _METRIC_NAME_DISALLOWED.sub("_", key)


def escape_label_key(key: str) -> str:
    return _LABEL_KEY_DISALLOWED.sub("_", key)


def escape_label_val(v: str) -> str:
    # replaceAllIn(key, """\\\\""") : each of \ " newline becomes two backslashes
    return _LABEL_VAL_DISALLOWED.sub(lambda m: "\\\\", v)


def format_labels(labels: Labels) -> str:
    if not labels:
        return ""
    return "{" + ", ".join(f'{escape_label_key(k)}="{escape_label_val(v)}"' for k, v in labels) + "}"


def _label_exists(labels: Labels, name: str) -> bool:
    return any(k == name for k, _ in labels)


def _rewrite(prefix: Tuple[str, ...], labels: Labels):
    if len(prefix) == 2 and prefix[0] == "rt" and not _label_exists(labels, "rt"):
        return ("rt",), labels + (("rt", prefix[1]),)
    if len(prefix) == 3 and prefix[:2] == ("rt", "service") and not _label_exists(labels, "service"):
        return ("rt", "service"), labels + (("service", prefix[2]),)
    if len(prefix) == 3 and prefix[:2] == ("rt", "client") and not _label_exists(labels, "client"):
        return ("rt", "client"), labels + (("client", prefix[2]),)
    if len(prefix) == 4 and prefix[:3] == ("rt", "client", "service") and not _label_exists(labels, "service"):
        return ("rt", "client", "service"), labels + (("service", prefix[3]),)
    if len(prefix) == 3 and prefix[:2] == ("rt", "server") and not _label_exists(labels, "server"):
        return ("rt", "server"), labels + (("server", prefix[2]),)
    return prefix, labels


QUANTILES = (("0", "min"), ("0.5", "p50"), ("0.9", "p90"), ("0.95", "p95"), ("0.99", "p99"),
             ("0.999", "p9990"), ("0.9999", "p9999"), ("1", "max"))


def write_metrics(tree: MetricsTree, out: List[str], prefix0: Tuple[str, ...] = (), labels0: Labels = ()) -> None:
    prefix1, labels1 = _rewrite(prefix0, labels0)
    key = escape_key(":".join(prefix1))
    m = tree.metric
    if isinstance(m, Metric.Counter):
        out.append(f"{key}{format_labels(labels1)} {long_to_string(m.get())}\n")
    elif isinstance(m, Metric.Gauge):
        out.append(f"{key}{format_labels(labels1)} {float_to_string(m.get())}\n")
    elif isinstance(m, Metric.Stat):
        s = m.snapshotted_summary
        if s is not None:
            lab = format_labels(labels1)
            out.append(f"{key}_count{lab} {long_to_string(s.count)}\n")
            out.append(f"{key}_sum{lab} {long_to_string(s.sum)}\n")
            out.append(f"{key}_avg{lab} {double_to_string(s.avg)}\n")
            for q, field in QUANTILES:
                out.append(f"{key}{format_labels(labels1 + (('quantile', q),))} {long_to_string(getattr(s, field))}\n")
    for name, child in tree.children.items():
        write_metrics(child, out, prefix1 + (name,), labels1)


def write_histogram_metrics(tree: MetricsTree, engine, out: List[str], prefix0: Tuple[str, ...] = (),
                            labels0: Labels = ()) -> None:
    """Prometheus histogram lines of every live Stat from the lifetime cumulative buckets
    of ``engine`` (a StatEngine after enable_le): ``{key}_hist_bucket{..., le="<le>"}`` per
    cut, then ``le="+Inf"``, ``{key}_hist_sum`` and ``{key}_hist_count``.  Counters that
    only grow, so the server can sum and divide them (sum by (le), histogram_quantile);
    the ``_hist`` infix keeps them apart from the summary's per-interval _count / _sum.
    Keys, labels and escaping are write_metrics'; each le is the exact snapped label."""
    prefix1, labels1 = _rewrite(prefix0, labels0)
    m = tree.metric
    if isinstance(m, Metric.Stat) and m.series_id is not None and engine.le_cuts is not None:
        key = escape_key(":".join(prefix1))
        row = engine.le_buckets[m.series_id]
        for le, n in zip(engine.le_labels, row[:-1]):
            lab = format_labels(labels1 + (("le", long_to_string(int(le))),))
            out.append(f"{key}_hist_bucket{lab} {long_to_string(int(n))}\n")
        out.append(f"{key}_hist_bucket{format_labels(labels1 + (('le', '+Inf'),))} {long_to_string(int(row[-1]))}\n")
        lab = format_labels(labels1)
        out.append(f"{key}_hist_sum{lab} {long_to_string(int(engine.le_sums[m.series_id]))}\n")
        out.append(f"{key}_hist_count{lab} {long_to_string(int(row[-1]))}\n")
    for name, child in tree.children.items():
        write_histogram_metrics(child, engine, out, prefix1 + (name,), labels1)


def write_quantile_metrics(tree: MetricsTree, engine, out: List[str], prefix0: Tuple[str, ...] = (),
                           labels0: Labels = ()) -> None:
    """The configured quantiles of ``engine`` (a StatEngine after enable_quantiles) as
    further lines of each Stat's summary: ``{key}{..., quantile="<label>"} <value>`` per
    quantile, the label Java's Double.toString of it (0.75, 0.995, 1.0E-4), the value the
    last snapshot_all_quantiles'.  A Stat prints them only if it holds a series id and has
    a snapshotted summary -- beside the summary block write_metrics prints, never without
    it.  Keys, labels and escaping are write_metrics'."""
    prefix1, labels1 = _rewrite(prefix0, labels0)
    m = tree.metric
    if (isinstance(m, Metric.Stat) and m.series_id is not None and m.snapshotted_summary is not None
            and engine.quantile_q is not None):
        key = escape_key(":".join(prefix1))
        for label, v in zip(engine.quantile_labels, engine.quantile_values[m.series_id]):
            out.append(f"{key}{format_labels(labels1 + (('quantile', label),))} {long_to_string(int(v))}\n")
    for name, child in tree.children.items():
        write_quantile_metrics(child, engine, out, prefix1 + (name,), labels1)


NO_INDEX = 0xFFFFFFFF  # NameTable.index of a Stat without a series id (no device call takes such a row)


def label_text(labels: Labels) -> str:
    """The text between the braces of format_labels(labels) ("" for no labels)."""
    return ", ".join(f'{escape_label_key(k)}="{escape_label_val(v)}"' for k, v in labels)


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
        def pack(texts):
            enc = [t.encode("utf-8") for t in texts]
            off = np.zeros(len(enc) + 1, np.uint64)
            off[1:] = np.cumsum(np.asarray([len(b) for b in enc], np.uint64))
            return off, np.frombuffer(b"".join(enc), np.uint8).copy()
        key_off, key_bytes = pack(keys)
        lab_off, lab_bytes = pack(inners)
        if index is not None:
            index = np.ascontiguousarray(np.asarray(index, np.int64).astype(np.uint32))
        if kinds is not None:
            kinds = np.ascontiguousarray(np.asarray(kinds, np.uint8))
        return NameTable(index, key_off, key_bytes, lab_off, lab_bytes, metrics, kinds)

    def take(self, rows) -> "NameTable":
        """The table of the given rows, in that order (a host table)."""
        rows = np.asarray(rows, np.int64)

        def gather(off, data):
            start = off[rows].astype(np.int64)
            length = off[rows + 1].astype(np.int64) - start
            new = np.zeros(rows.size + 1, np.uint64)
            new[1:] = np.cumsum(length.astype(np.uint64))
            src = np.repeat(start - new[:-1].astype(np.int64), length) + np.arange(int(new[-1]), dtype=np.int64)
            return new, data[src]
        key_off, key_bytes = gather(self.key_off, self.key_bytes)
        lab_off, lab_bytes = gather(self.lab_off, self.lab_bytes)
        index = None if self.index is None else self.index[rows]
        metrics = None if self.metrics is None else [self.metrics[int(r)] for r in rows]
        kinds = None if self.kinds is None else self.kinds[rows]
        return NameTable(index, key_off, key_bytes, lab_off, lab_bytes, metrics, kinds)

    def to_device(self, device: int = 0) -> "NameTable":
        """The same table in device memory (torch tensors): uploaded once, reused by
        every scrape."""
        import torch
        dev = torch.device("cuda", int(device))

        def up(a):
            if a is None:
                return None
            a = np.ascontiguousarray(a)
            # (the same bits under torch's long-standing signed types)
            a = a.view({8: np.int64, 4: np.int32}.get(a.dtype.itemsize, np.uint8)) if a.dtype.kind == "u" else a
            return torch.from_numpy(a).to(dev)
        return NameTable(up(self.index), up(self.key_off), up(self.key_bytes), up(self.lab_off), up(self.lab_bytes),
                         self.metrics, up(self.kinds))


def stat_name_table(tree: MetricsTree) -> NameTable:
    """The name table of the Stats of ``tree``, walked exactly as write_metrics walks it
    (the same prefix rewrite, escapes and child order): one row per Stat in DFS order,
    ``index`` its series id (NO_INDEX for a Stat without one)."""
    keys: List[str] = []
    inners: List[str] = []
    index: List[int] = []
    metrics: list = []

    def visit(t: MetricsTree, prefix0: Tuple[str, ...], labels0: Labels) -> None:
        prefix1, labels1 = _rewrite(prefix0, labels0)
        m = t.metric
        if isinstance(m, Metric.Stat):
            keys.append(escape_key(":".join(prefix1)))
            inners.append(label_text(labels1))
            index.append(NO_INDEX if m.series_id is None else int(m.series_id))
            metrics.append(m)
        for name, child in t.children.items():
            visit(child, prefix1 + (name,), labels1)

    visit(tree, (), ())
    return NameTable.build(keys, inners, index, metrics)


def rollup_name_table(plan) -> NameTable:
    """The name table of a rollup.RollupPlan's groups: row g prints group g (no index)."""
    return NameTable.build([key for key, _ in plan.groups], [label_text(labels) for _, labels in plan.groups])


def summary_records(summaries) -> np.ndarray:
    """HistogramSummary objects as the engine's summary records."""
    from ._native import SUMMARY_DTYPE, SUMMARY_FIELDS
    out = np.zeros(len(summaries), SUMMARY_DTYPE)
    for f in SUMMARY_FIELDS:
        out[f] = [getattr(s, f) for s in summaries]
    return out


def write_scalar_metrics(tree: MetricsTree, out: List[str], prefix0: Tuple[str, ...] = (), labels0: Labels = ()) -> None:
    """write_metrics' counter and gauge lines alone (the values the engine does not hold)."""
    prefix1, labels1 = _rewrite(prefix0, labels0)
    m = tree.metric
    if isinstance(m, Metric.Counter):
        out.append(f"{escape_key(':'.join(prefix1))}{format_labels(labels1)} {long_to_string(m.get())}\n")
    elif isinstance(m, Metric.Gauge):
        out.append(f"{escape_key(':'.join(prefix1))}{format_labels(labels1)} {float_to_string(m.get())}\n")
    for name, child in tree.children.items():
        write_scalar_metrics(child, out, prefix1 + (name,), labels1)


def scalar_name_table(tree: MetricsTree) -> NameTable:
    """The name table of the counters and gauges of ``tree``, walked exactly as
    write_scalar_metrics walks it: one row per counter or gauge in DFS order with its
    kind, ``index`` its ordinal among the rows of its kind (the order of scalar_values)."""
    from ._native import KIND_COUNTER, KIND_GAUGE
    keys: List[str] = []
    inners: List[str] = []
    index: List[int] = []
    kinds: List[int] = []
    metrics: list = []
    seen = [0, 0]

    def visit(t: MetricsTree, prefix0: Tuple[str, ...], labels0: Labels) -> None:
        prefix1, labels1 = _rewrite(prefix0, labels0)
        m = t.metric
        if isinstance(m, (Metric.Counter, Metric.Gauge)):
            kind = KIND_COUNTER if isinstance(m, Metric.Counter) else KIND_GAUGE
            keys.append(escape_key(":".join(prefix1)))
            inners.append(label_text(labels1))
            kinds.append(kind)
            index.append(seen[kind])
            seen[kind] += 1
            metrics.append(m)
        for name, child in t.children.items():
            visit(child, prefix1 + (name,), labels1)

    visit(tree, (), ())
    return NameTable.build(keys, inners, index, metrics, kinds)


def scalar_values(table: NameTable):
    """(counters int64, gauges float32) of one scrape: the current values of the counter
    and gauge rows of a host table, each in the order its rows' ``index`` counts."""
    from ._native import KIND_COUNTER, KIND_GAUGE
    counters = [m.get() for m, k in zip(table.metrics, table.kinds) if k == KIND_COUNTER]
    gauges = [m.get() for m, k in zip(table.metrics, table.kinds) if k == KIND_GAUGE]
    return np.asarray(counters, np.int64), np.asarray(gauges, np.float32)


class PrometheusTelemeter:
    """PrometheusTelemeter (PrometheusTelemeter.scala:17-35): /admin/metrics/prometheus."""

    path = "/admin/metrics/prometheus"

    def __init__(self, metrics: MetricsTree, rollups=None, histograms=None, quantiles=None):
        self.metrics = metrics
        # optional (RollupPlan, group summaries) pair of linkerd_amd.rollup, settable
        # later: its lines follow the tree's
        self.rollups = rollups
        # optional StatEngine with enable_le, settable later: the Stats' cumulative
        # `le` bucket lines (write_histogram_metrics) follow the tree's and the rollups'
        self.histograms = histograms
        # optional StatEngine with enable_quantiles, settable later: the Stats' configured
        # quantile lines (write_quantile_metrics) follow the `_hist` blocks
        self.quantiles = quantiles

    def render(self) -> str:
        out: List[str] = []
        write_metrics(self.metrics, out)
        if self.rollups is not None:
            from .rollup import write_rollup_metrics
            plan, summaries = self.rollups
            write_rollup_metrics(plan, summaries, out)
        if self.histograms is not None:
            write_histogram_metrics(self.metrics, self.histograms, out)
        if self.quantiles is not None:
            write_quantile_metrics(self.metrics, self.quantiles, out)
        return "".join(out)

    def render_bytes(self, engine, names: "NameTable" = None, summaries=None, scalars_on_device: bool = False) -> bytes:
        """The exposition as bytes, the Stats' text rendered on the device by ``engine``
        (a HistogramEngine): the counter and gauge lines (printed here: the engine does
        not hold them), the Stat blocks, the rollup blocks if ``rollups`` is set, the
        ``_hist`` blocks if ``histograms`` is set, the configured quantiles' blocks if
        ``quantiles`` is set.  As a line multiset this is render().
        ``names``: stat_name_table(self.metrics) kept by the caller (host memory, or
        to_device() for the device calls); built here when None.  ``summaries``: the
        snapshot's records indexed by series id, host or device (every Stat of the table
        then prints its record); None takes each Stat's snapshotted summary, and a Stat
        without one prints nothing.  ``scalars_on_device``: the counter and gauge lines
        are rendered on the device too (render_json.render_scalars over
        scalar_name_table(self.metrics)), the same bytes."""
        if scalars_on_device:
            from .render_json import render_scalars
            scalars = scalar_name_table(self.metrics)
            counters, gauges = scalar_values(scalars)
            parts = [render_scalars(engine, scalars, counters, gauges) if scalars.n else b""]
        else:
            out: List[str] = []
            write_scalar_metrics(self.metrics, out)
            parts = ["".join(out).encode("utf-8")]
        table = stat_name_table(self.metrics) if names is None else names
        host = table if table.metrics is not None and isinstance(table.key_off, np.ndarray) else None
        if summaries is not None:
            if table.n:
                parts.append(engine.render_summaries(table, summaries))
        else:
            if host is None:
                host = stat_name_table(self.metrics)
            snaps = [m.snapshotted_summary for m in host.metrics]
            rows = [j for j, s in enumerate(snaps) if s is not None]
            if rows:
                # the kept rows in table order with their records beside them: no index
                shown = host if len(rows) == host.n else host.take(rows)
                shown = NameTable(None, shown.key_off, shown.key_bytes, shown.lab_off, shown.lab_bytes, shown.metrics)
                parts.append(engine.render_summaries(shown, summary_records([snaps[j] for j in rows])))
        if self.rollups is not None:
            plan, group_summaries = self.rollups
            k = min(plan.ngroups, len(group_summaries))
            if k:
                groups = rollup_name_table(plan)
                groups = groups if k == groups.n else groups.take(range(k))
                parts.append(engine.render_summaries(groups, summary_records(list(group_summaries)[:k])))
        h = self.histograms
        if h is not None and h.le_cuts is not None and table.n:
            # write_histogram_metrics prints every Stat that holds a series id
            live = table
            if table.metrics is not None and any(m.series_id is None for m in table.metrics):
                if host is None:
                    host = stat_name_table(self.metrics)
                live = host.take([j for j, m in enumerate(host.metrics) if m.series_id is not None])
            if live.n:
                parts.append(engine.render_le(live, h.le_buckets, h.le_sums, h.le_labels))
        qe = self.quantiles
        if qe is not None and qe.quantile_q is not None and table.n:
            # write_quantile_metrics prints every Stat with a series id and a snapshotted summary
            if host is None:
                host = stat_name_table(self.metrics)
            rows = [j for j, m in enumerate(host.metrics)
                    if m.series_id is not None and m.snapshotted_summary is not None]
            if rows:
                shown = host if len(rows) == host.n else host.take(rows)
                parts.append(engine.render_quantiles(shown, qe.quantile_values, qe.quantile_q))
        return b"".join(parts)


def line_multiset(text: str) -> dict:
    from collections import Counter
    return Counter(l for l in text.split("\n") if l)
