"""/admin/metrics/top.json: which Stats are the worst, answered on the GPU.

The exporters print every Stat; an operator looking for the twenty clients with the
highest p99 does not want every Stat.  The engine holds the open interval's rows in
device memory, so the selection runs there (HistogramEngine.top: an exact, deterministic
top-k over one summary field or any quantile) and k names with their summaries come
back (telemetry.top_stats).

This endpoint is the project's own: the reference has no such query.  It borrows the
conventions of AdminMetricsExportTelemeter (reference: telemetry/admin-metrics-export/
src/main/scala/io/buoyant/telemetry/admin/AdminMetricsExportTelemeter.scala:31-54): the
``q`` parameter names a subtree, split as there, and an unknown one answers 404 with the
same body; numbers are printed as every exporter here prints them (Java long / double
texts, non-finite doubles quoted, jackson string escapes).

Parameters
  by         a summary field (count, min, max, sum, p50, p90, p95, p99, p9990, p9999, avg;
             default p99), or ``q<double>`` -- q0.995 -- for the exact quantile
  k          1 .. 1024 (default 20)
  order      largest (default) or smallest
  min_count  Stats with fewer samples in the open interval do not rank (default 1)
  q          only the Stats under this subtree rank
A bad parameter answers 400 with {"error": "..."}.

The body is a JSON array in rank order (equal keys by ascending series id).  Each element
is an object: "name" (the Stat's a/b/c key from the root of the tree), then count, max, min,
p50, p90, p95, p99, p9990, p9999, sum, avg -- the order of metrics.json -- and, when ranking
by ``q<double>``, that quantile's value as "quantile".  The summaries are those of the open
interval (nothing is reset), not the last snapshot's.
"""
from __future__ import annotations

import math
from typing import List, Optional, Tuple
from urllib.parse import parse_qs, urlsplit

from . import _native as N
from .admin_metrics import STAT_FIELDS, _Gen, _java_split_slash, _json_float, json_string
from .javafmt import double_to_string, long_to_string
from .telemetry import MetricsTree, StatEngine, top_stats

K_DEFAULT = 20


class BadParameter(ValueError):
    pass


def parse_by(text: str):
    """A ``by`` parameter: a field name as it is, ``q<double>`` as the float in [0, 1]."""
    if text in N.SUMMARY_FIELDS:
        return text
    if text.startswith("q") and len(text) > 1:
        try:
            q = float(text[1:])
        except ValueError:
            q = math.nan
        if 0.0 <= q <= 1.0:  # (NaN fails both)
            return q
        raise BadParameter(f"by: {text} is not a quantile in [0, 1]")
    raise BadParameter(f"by: {text} is neither a summary field nor q<double>")


def _int_param(params, name: str, default: int, lo: int, hi: Optional[int]) -> int:
    v = params.get(name)
    if not v:
        return default
    try:
        x = int(v[0], 10)
    except ValueError:
        raise BadParameter(f"{name}: {v[0]} is not an integer") from None
    if x < lo or (hi is not None and x > hi):
        raise BadParameter(f"{name}: {x} is outside [{lo}, {hi}]" if hi is not None else f"{name}: {x} is below {lo}")
    return x


def parse_params(uri: str):
    """(by, k, order, min_count, q) of a request URI; BadParameter names the first bad one."""
    params = parse_qs(urlsplit(uri).query, keep_blank_values=True)
    by = parse_by(params["by"][0]) if "by" in params else "p99"
    k = _int_param(params, "k", K_DEFAULT, 1, N.TOP_LIMIT)
    order = params["order"][0] if "order" in params else "largest"
    if order not in ("largest", "smallest"):
        raise BadParameter(f"order: {order} is not largest or smallest")
    min_count = _int_param(params, "min_count", 1, 0, None)
    q = params["q"][0] if "q" in params else None
    return by, k, order, min_count, q


def write_top_json(items) -> str:
    """The body: one object per (path, HistogramSummary[, q value]) of ``items``, in order."""
    parts: List[str] = []
    for item in items:
        path, s = item[0], item[1]
        jg = _Gen(False)
        jg.start_object()
        jg.number_field("name", json_string("/".join(path)))
        jg.number_field("count", long_to_string(s.count))
        for f in STAT_FIELDS:
            jg.number_field(f, long_to_string(getattr(s, f)))
        jg.number_field("avg", _json_float(s.avg, double_to_string))
        if len(item) > 2:
            jg.number_field("quantile", long_to_string(item[2]))
        jg.end_object()
        parts.append(jg.text())
    return "[" + ",".join(parts) + "]"


class TopStatsHandler:
    """/admin/metrics/top.json over a MetricsTree and its StatEngine."""

    path = "/admin/metrics/top.json"

    def __init__(self, metrics: MetricsTree, engine: Optional[StatEngine] = None):
        self.metrics = metrics
        self.engine = engine if engine is not None else metrics._engine

    def handle(self, uri: str) -> Tuple[int, str, str]:
        """(status, media type, body) for a request URI such as
        /admin/metrics/top.json?by=q0.995&k=10&q=rt/http."""
        try:
            by, k, order, min_count, q = parse_params(uri)
        except BadParameter as e:
            return 400, "application/json", '{"error": %s}' % json_string(str(e))
        scope = ()
        if q is not None:
            scope = tuple(_java_split_slash(q))
            if self.metrics.try_resolve(scope) is None:
                return 404, "application/json", '{"error": "No such subtree: %s"}' % q
        items = top_stats(self.metrics, self.engine, k, by=by, order=order, min_count=min_count, scope=scope)
        return 200, "application/json", write_top_json(items)
