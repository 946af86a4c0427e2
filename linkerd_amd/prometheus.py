"""Prometheus text export from GPU-produced summaries.

Restates PrometheusTelemeter.writeMetrics
(reference: telemetry/prometheus/src/main/scala/io/buoyant/telemetry/prometheus/
PrometheusTelemeter.scala:37-135): prefix segments rt/<router>, rt/service/<path>,
rt/client/<id>, rt/client/service/<path>, rt/server/<srv> are rewritten into labels
(nametable.walk); counters print as Java Long, gauges as Java Float, stats print
_count/_sum/_avg (avg as Java Double) plus 8 quantile lines from `snapshotted_summary`,
and nothing before the first snapshot.  Child order follows the tree's map order (the
reference's immutable-Map hash order), so compare outputs as line multisets.
"""
from __future__ import annotations

import re
from collections import Counter
from typing import List, Tuple

import numpy as np

from . import _native as N
from .javafmt import double_to_string, float_to_string, long_to_string
from .nametable import (NO_INDEX, Labels, NameTable, bulk_counters, counter_ids, escape_key, kind_of,  # noqa: F401
                        scalar_ordinals, scalar_values, scrape_rows, series_index, summary_records, walk)
from .render_json import render_scalars
from .telemetry import MetricsTree

_LABEL_KEY_DISALLOWED = re.compile(r"[^a-zA-Z0-9_]")
_LABEL_VAL_DISALLOWED = re.compile(r'(\\|"|\n)')


def escape_label_key(key: str) -> str:
    return _LABEL_KEY_DISALLOWED.sub("_", key)


def escape_label_val(v: str) -> str:
    # replaceAllIn(key, """\\\\""") : each of \ " newline becomes two backslashes
    return _LABEL_VAL_DISALLOWED.sub(lambda m: "\\\\", v)


def label_text(labels: Labels) -> str:
    """The text between the braces of format_labels(labels) ("" for no labels)."""
    return ", ".join(f'{escape_label_key(k)}="{escape_label_val(v)}"' for k, v in labels)


def format_labels(labels: Labels) -> str:
    return "{" + label_text(labels) + "}" if labels else ""


QUANTILES = (("0", "min"), ("0.5", "p50"), ("0.9", "p90"), ("0.95", "p95"), ("0.99", "p99"),
             ("0.999", "p9990"), ("0.9999", "p9999"), ("1", "max"))


def write_summary(key: str, labels: Labels, s, out: List[str]) -> None:
    """The eleven lines of one HistogramSummary: _count, _sum, _avg, eight quantiles."""
    lab = format_labels(labels)
    out.append(f"{key}_count{lab} {long_to_string(s.count)}\n")
    out.append(f"{key}_sum{lab} {long_to_string(s.sum)}\n")
    out.append(f"{key}_avg{lab} {double_to_string(s.avg)}\n")
    for q, field in QUANTILES:
        out.append(f"{key}{format_labels(labels + (('quantile', q),))} {long_to_string(getattr(s, field))}\n")


# The lines of one walked node (prefix, labels, node, its children); the write_* functions loop over the walk.
def _metric_lines(prefix, labels, t, _, out: List[str], stats: bool = True) -> None:
    m = t.metric
    kind = kind_of(m)
    if kind == N.KIND_COUNTER:
        out.append(f"{escape_key(':'.join(prefix))}{format_labels(labels)} {long_to_string(m.get())}\n")
    elif kind == N.KIND_GAUGE:
        out.append(f"{escape_key(':'.join(prefix))}{format_labels(labels)} {float_to_string(m.get())}\n")
    elif kind == N.KIND_STAT and stats and m.snapshotted_summary is not None:
        write_summary(escape_key(":".join(prefix)), labels, m.snapshotted_summary, out)


def _histogram_lines(prefix, labels, t, _, engine, out: List[str]) -> None:
    m = t.metric
    if kind_of(m) == N.KIND_STAT and m.series_id is not None and engine.le_cuts is not None:
        key = escape_key(":".join(prefix))
        row = engine.le_buckets[m.series_id]
        for le, n in zip(engine.le_labels, row[:-1]):
            lab = format_labels(labels + (("le", long_to_string(int(le))),))
            out.append(f"{key}_hist_bucket{lab} {long_to_string(int(n))}\n")
        out.append(f"{key}_hist_bucket{format_labels(labels + (('le', '+Inf'),))} {long_to_string(int(row[-1]))}\n")
        lab = format_labels(labels)
        out.append(f"{key}_hist_sum{lab} {long_to_string(int(engine.le_sums[m.series_id]))}\n")
        out.append(f"{key}_hist_count{lab} {long_to_string(int(row[-1]))}\n")


def _quantile_lines(prefix, labels, t, _, engine, out: List[str]) -> None:
    m = t.metric
    if (kind_of(m) == N.KIND_STAT and m.series_id is not None and m.snapshotted_summary is not None
            and engine.quantile_q is not None):
        key = escape_key(":".join(prefix))
        for label, v in zip(engine.quantile_labels, engine.quantile_values[m.series_id]):
            out.append(f"{key}{format_labels(labels + (('quantile', label),))} {long_to_string(int(v))}\n")


def write_metrics(tree: MetricsTree, out: List[str], prefix0: Tuple[str, ...] = (), labels0: Labels = ()) -> None:
    for node in walk(tree, prefix0, labels0):
        _metric_lines(*node, out)


def write_scalar_metrics(tree: MetricsTree, out: List[str], prefix0: Tuple[str, ...] = (), labels0: Labels = ()) -> None:
    """write_metrics' counter and gauge lines alone (the values the engine does not hold)."""
    for node in walk(tree, prefix0, labels0):
        _metric_lines(*node, out, stats=False)


def write_histogram_metrics(tree: MetricsTree, engine, out: List[str], prefix0: Tuple[str, ...] = (),
                            labels0: Labels = ()) -> None:
    """Prometheus histogram lines of every live Stat from the lifetime cumulative buckets
    of ``engine`` (a StatEngine after enable_le): ``{key}_hist_bucket{..., le="<le>"}`` per
    cut, then ``le="+Inf"``, ``{key}_hist_sum`` and ``{key}_hist_count``.  Counters that
    only grow, so the server can sum and divide them (sum by (le), histogram_quantile);
    the ``_hist`` infix keeps them apart from the summary's per-interval _count / _sum.
    Keys, labels and escaping are write_metrics'; each le is the exact snapped label."""
    for node in walk(tree, prefix0, labels0):
        _histogram_lines(*node, engine, out)


def write_quantile_metrics(tree: MetricsTree, engine, out: List[str], prefix0: Tuple[str, ...] = (),
                           labels0: Labels = ()) -> None:
    """The configured quantiles of ``engine`` (a StatEngine after enable_quantiles) as
    further lines of each Stat's summary: ``{key}{..., quantile="<label>"} <value>`` per
    quantile, the label Java's Double.toString of it (0.75, 0.995, 1.0E-4), the value the
    last snapshot_all_quantiles'.  A Stat prints them only if it holds a series id and has
    a snapshotted summary -- beside the summary block write_metrics prints, never without
    it.  Keys, labels and escaping are write_metrics'."""
    for node in walk(tree, prefix0, labels0):
        _quantile_lines(*node, engine, out)


def write_rollup_metrics(plan, summaries, out: List[str]) -> None:
    """Per group of a rollup.RollupPlan the eleven lines a Stat gets from write_metrics,
    with the group's remaining labels."""
    for (key, labels), s in zip(plan.groups, summaries):
        write_summary(key, labels, s, out)


def _name_rows(tree: MetricsTree, kinds):
    """(keys, label texts, metrics) of the nodes of ``tree`` whose metric is of one of
    ``kinds``, walked exactly as write_metrics walks it: a row each, in DFS order."""
    keys, inners, metrics = [], [], []  # (a column each, no object per row: a tree has 10^5 of them)
    for prefix, labels, t, _ in walk(tree):
        if kind_of(t.metric) in kinds:
            keys.append(escape_key(":".join(prefix)))
            inners.append(label_text(labels))
            metrics.append(t.metric)
    return keys, inners, metrics


def stat_name_table(tree: MetricsTree) -> NameTable:
    """The name table of the Stats of ``tree``: one row per Stat in write_metrics' order,
    ``index`` its series id (NO_INDEX for a Stat without one)."""
    keys, inners, metrics = _name_rows(tree, (N.KIND_STAT,))
    return NameTable.build(keys, inners, series_index(metrics), metrics)


def scalar_name_table(tree: MetricsTree) -> NameTable:
    """The name table of the counters and gauges of ``tree``: one row per counter or gauge
    in write_scalar_metrics' order with its kind, ``index`` its ordinal among the rows of
    its kind (the order of scalar_values) -- or, for a counter that lives in a CounterEngine,
    its counter id."""
    keys, inners, metrics = _name_rows(tree, (N.KIND_COUNTER, N.KIND_GAUGE))
    kinds = np.asarray([kind_of(m) for m in metrics], np.uint8)
    return NameTable.build(keys, inners, counter_ids(scalar_ordinals(np.zeros(kinds.size, np.int64), kinds), kinds, metrics),
                           metrics, kinds)


def rollup_name_table(plan) -> NameTable:
    """The name table of a rollup.RollupPlan's groups: row g prints group g (no index)."""
    return NameTable.build([key for key, _ in plan.groups], [label_text(labels) for _, labels in plan.groups])


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
        nodes = list(walk(self.metrics))  # one walk: every block describes the same Stats
        with bulk_counters(self.metrics):
            for node in nodes:
                _metric_lines(*node, out)
        if self.rollups is not None:
            write_rollup_metrics(*self.rollups, out)
        if self.histograms is not None:
            for node in nodes:
                _histogram_lines(*node, self.histograms, out)
        if self.quantiles is not None:
            for node in nodes:
                _quantile_lines(*node, self.quantiles, out)
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
            scalars = scalar_name_table(self.metrics)
            parts = [render_scalars(engine, scalars, *scalar_values(scalars)) if scalars.n else b""]
        else:
            out: List[str] = []
            with bulk_counters(self.metrics):
                write_scalar_metrics(self.metrics, out)
            parts = ["".join(out).encode("utf-8")]
        table = stat_name_table(self.metrics) if names is None else names
        host = table if table.metrics is not None and isinstance(table.key_off, np.ndarray) else None

        def shown(values, **how):
            """The rows of the host table (built when ``names`` is not one) a block shows."""
            nonlocal host
            if host is None:
                host = stat_name_table(self.metrics)
            return scrape_rows(host, host.metrics, values, **how)
        if summaries is not None:
            if table.n:
                parts.append(engine.render_summaries(table, summaries))
        else:
            rows, records = shown(None)
            if rows.n:
                # the kept rows in table order with their records beside them: no index
                parts.append(engine.render_summaries(rows.with_index(None), records))
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
                live = shown(h.le_buckets)[0]
            if live.n:
                parts.append(engine.render_le(live, h.le_buckets, h.le_sums, h.le_labels))
        qe = self.quantiles
        if qe is not None and qe.quantile_q is not None and table.n:
            # write_quantile_metrics prints every Stat with a series id and a snapshotted summary
            rows = shown(qe.quantile_values, need_snapshot=True)[0]
            if rows.n:
                parts.append(engine.render_quantiles(rows, qe.quantile_values, qe.quantile_q))
        return b"".join(parts)


def line_multiset(text: str) -> dict:
    return Counter(l for l in text.split("\n") if l)
