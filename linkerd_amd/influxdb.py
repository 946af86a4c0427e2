"""InfluxDB LINE protocol export from GPU-produced summaries.

Restates InfluxDbTelemeter.writeMetrics
(reference: telemetry/influxdb/src/main/scala/io/buoyant/telemetry/influxdb/
InfluxDbTelemeter.scala:17-130): the prefix segments rt/<router>,
rt/service/<path>, rt/client/<id>, rt/client/service/<path>, rt/server/<srv>
become tags (:63-75); the metrics directly under one parent are written as the
fields of one measurement, after the lines of their own subtrees (:78-108);
counters print as Java Long, gauges as Java Float, and a snapshotted Stat as
<name>_count/_sum/_avg/_min/_max/_p50/_p90/_p95/_p99/_p999/_p9999 (avg as Java
Double); tags and fields are sorted by key (:46-50); top-level metrics go under
the measurement "root" (:36, :111-118); the measurement name is escaped with
[^a-zA-Z0-9:] -> _ (:42-43).  Tag and field values are not escaped (as in the
reference).
"""
from __future__ import annotations

from operator import attrgetter
from typing import List, Sequence, Tuple

from . import _native as N
from .javafmt import double_to_string, float_to_string, long_to_string
from .nametable import bulk_counters, device_or_host, escape_key, kind_of, utf16_key, walk  # noqa: F401
from .render_influx import ROOT_PREFIX, STAT_FIELDS, influx_table, render_influx, scrape_inputs
from .telemetry import MetricsTree

Tags = Tuple[Tuple[str, str], ...]
# a Stat's fields: their values of a summary, and per field (key suffix, formatter)
_stat_values = attrgetter(*(N.SUMMARY_FIELDS[f] for _, f in STAT_FIELDS))
_STAT_TEXTS = [(sfx, double_to_string if f == N.BY_AVG else long_to_string) for sfx, f in STAT_FIELDS]


def format_labels(labels: Sequence[Tuple[str, str]]) -> str:
    return ",".join(f"{k}={v}" for k, v in sorted(labels, key=lambda kv: utf16_key(kv[0])))  # stable sortBy(_._1)


def _fields(name: str, m) -> List[Tuple[str, str]]:
    kind = kind_of(m)
    if kind == N.KIND_COUNTER:
        return [(name, long_to_string(m.get()))]
    if kind == N.KIND_GAUGE:
        return [(name, float_to_string(m.get()))]
    s = m.snapshotted_summary if kind == N.KIND_STAT else None
    return [] if s is None else [(name + sfx, text(v)) for (sfx, text), v in zip(_STAT_TEXTS, _stat_values(s))]


def write_metrics(tree: MetricsTree, out: List[str], prefix0: Tuple[str, ...] = (), tags0: Tags = ()) -> None:
    for prefix, tags, _, children in walk(tree, prefix0, tags0, post=True):  # deeper lines first
        fields = [f for name, child in children.items() for f in _fields(name, child.metric)]
        if fields:
            line = escape_key(":".join(prefix if prefix else ROOT_PREFIX))
            if tags:
                line += "," + format_labels(tags)
            out.append(line + " " + format_labels(fields) + "\n")


class InfluxDbTelemeter:
    """InfluxDbTelemeter (:17-40): /admin/metrics/influxdb."""

    path = "/admin/metrics/influxdb"

    def __init__(self, metrics: MetricsTree):
        self.metrics = metrics

    def render(self, host: str = "none") -> str:
        """The handler body; `host` is the request's Host header ("none" if absent)."""
        out: List[str] = []
        with bulk_counters(self.metrics):
            write_metrics(self.metrics, out, (), (("host", host),))
        return "".join(out)

    def render_bytes(self, engine, host: str = "none", table=None, summaries=None) -> bytes:
        """render(host) as UTF-8 bytes, rendered on the device by ``engine`` (a
        HistogramEngine) -- the same bytes.  ``table``: render_influx.influx_table(self.metrics)
        kept by the caller (a host table); built here when None.  ``summaries``: the
        snapshot's records indexed by series id, host or device -- every Stat with a series
        id then prints its record; None takes each Stat's snapshotted summary, and a Stat
        without one prints nothing.  A body with an avg outside the device formatter's
        domain is the host writer's text."""
        inputs = scrape_inputs(influx_table(self.metrics) if table is None else table, summaries)
        return device_or_host(lambda: render_influx(engine, inputs[0], host, *inputs[1:]),
                              lambda: self.render(host).encode("utf-8"))
