"""A whole scrape rendered on the device: the flat compact /admin/metrics.json document
(l5dh_render_json) and the counter and gauge lines of the Prometheus exposition
(l5dh_render_scalars), over a HistogramEngine's argument rules.

The tables are nametable.NameTable with ``kinds`` (uint8 per row: _native.KIND_COUNTER,
KIND_GAUGE, KIND_STAT); a row's ``index`` counts within its kind's value array.  Both calls
answer as HistogramEngine.render_summaries does: bytes, or with ``out`` the length written
there, or with out=QUERY the length alone.  They read no engine state.
"""
from __future__ import annotations

import ctypes

import numpy as np

from . import _native as N
from .engine import QUERY, _numel, _record_rows  # noqa: F401  (QUERY: for the callers)


def _kinds(engine, names):
    if names.kinds is None:
        raise ValueError("names: a table with kinds is needed (admin_metrics.flat_name_table, "
                         "prometheus.scalar_name_table)")
    return engine._buf(names.kinds, (np.uint8,), "names.kinds", names.n)


def value_args(engine, summaries, counters, gauges):
    """The six C arguments of a scrape's values: pointer and count of the summary records,
    the counters (int64) and the gauges (float32), each optional (NULL, 0)."""
    def values(x, dtype, name):
        return (None, 0) if x is None else (engine._buf(x, (dtype,), name), _numel(x))
    sp, ns = None, 0
    if summaries is not None:
        sp, ns = engine._records(summaries, N.SUMMARY_DTYPE, "summaries"), _record_rows(summaries, N.SUMMARY_DTYPE)[0]
    return (sp, ns) + values(counters, np.int64, "counters") + values(gauges, np.float32, "gauges")


def render_json(engine, names, summaries, counters, gauges, out=None):
    """The document ``{"<key>":<number>,...}`` of the rows of ``names``, byte for byte
    admin_metrics.write_flat_json's compact text: a counter row prints counters[index]
    (int64) as a Java long, a gauge row gauges[index] (float32) as Float.toString (quoted
    when not finite), a stat row summaries[index] (the numpy summary dtype or int64
    [n*11]) as ``.count`` and, when count > 0, the nine longs and ``.avg``.  Each value
    array is host or device memory, or None when no row is of its kind.  The table's label
    text is not read.  ``{}`` for a table without rows."""
    values = value_args(engine, summaries, counters, gauges)
    nm, n, kp = engine._names(names), names.n, _kinds(engine, names)
    return engine._render(lambda op, cap, ln: engine._lib.l5dh_render_json(
        engine._ctx, ctypes.byref(nm), kp, n, *values, op, cap, ln), "l5dh_render_json", out)


def render_scalars(engine, names, counters, gauges, out=None):
    """One line ``key[{inner}] <value>`` per row of ``names``, byte for byte
    prometheus.write_scalar_metrics' lines: a counter as a Java long, a gauge as
    Float.toString (never quoted).  A stat row is an error."""
    values = value_args(engine, None, counters, gauges)[2:]
    nm, n, kp = engine._names(names), names.n, _kinds(engine, names)
    return engine._render(lambda op, cap, ln: engine._lib.l5dh_render_scalars(
        engine._ctx, ctypes.byref(nm), kp, n, *values, op, cap, ln), "l5dh_render_scalars", out)
