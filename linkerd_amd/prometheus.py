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


class PrometheusTelemeter:
    """PrometheusTelemeter (PrometheusTelemeter.scala:17-35): /admin/metrics/prometheus."""

    path = "/admin/metrics/prometheus"

    def __init__(self, metrics: MetricsTree, rollups=None, histograms=None):
        self.metrics = metrics
        # optional (RollupPlan, group summaries) pair of linkerd_amd.rollup, settable
        # later: its lines follow the tree's
        self.rollups = rollups
        # optional StatEngine with enable_le, settable later: the Stats' cumulative
        # `le` bucket lines (write_histogram_metrics) follow the tree's and the rollups'
        self.histograms = histograms

    def render(self) -> str:
        out: List[str] = []
        write_metrics(self.metrics, out)
        if self.rollups is not None:
            from .rollup import write_rollup_metrics
            plan, summaries = self.rollups
            write_rollup_metrics(plan, summaries, out)
        if self.histograms is not None:
            write_histogram_metrics(self.metrics, self.histograms, out)
        return "".join(out)


def line_multiset(text: str) -> dict:
    from collections import Counter
    return Counter(l for l in text.split("\n") if l)
