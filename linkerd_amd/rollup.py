"""Label rollups of latency histograms: labels -> groups -> Prometheus lines.

The exporters print one summary per series (``rt:client:request_latency_ms{rt="http",
client="a", quantile="0.99"}``), and quantiles of different series cannot be
combined.  The engine keeps every series' raw bucket counts, and the histogram of a
union of series is the element-wise integer sum of their rows, so the summary of a
group -- say one router's latency over all its clients -- is exact: what one
Metric.Stat would report had it received every member's samples
(HistogramEngine.rollup).  This module names the groups: it walks a MetricsTree with
the prefix rewrite of the Prometheus exporter and groups the Stats whose labels
differ only in the ``without`` keys.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Dict, List, Sequence, Tuple

import numpy as np

from ._native import KIND_STAT, NO_GROUP
from .nametable import Labels, escape_key, kind_of, walk
from .prometheus import write_rollup_metrics  # noqa: F401  (the groups' lines: a Prometheus writer)
from .telemetry import HistogramSummary, MetricsTree, StatEngine, live_stats

GroupId = Tuple[str, Labels]


@dataclass
class RollupPlan:
    group_of: np.ndarray      # uint32 [capacity]: the group of each series id, or NO_GROUP
    groups: List[GroupId]     # group g = (metric key, remaining labels)

    @property
    def ngroups(self) -> int:
        return len(self.groups)


def plan_rollup(tree: MetricsTree, without: Sequence[str], capacity: int) -> RollupPlan:
    """Group the live Stats of ``tree`` by (metric key, labels minus the ``without``
    keys, order kept).  A Stat with none of those labels stays ungrouped (its group
    would only duplicate it), as does a pruned one (no series id)."""
    drop = frozenset(without)
    group_of = np.full(int(capacity), NO_GROUP, dtype=np.uint32)
    index: Dict[GroupId, int] = {}
    groups: List[GroupId] = []
    for prefix, labels, t, _ in walk(tree):
        sid = t.metric.series_id if kind_of(t.metric) == KIND_STAT else None
        if sid is not None and any(k in drop for k, _ in labels):
            gid = (escape_key(":".join(prefix)), tuple((k, v) for k, v in labels if k not in drop))
            g = index.get(gid)
            if g is None:
                g = index[gid] = len(groups)
                groups.append(gid)
            group_of[sid] = g
    return RollupPlan(group_of, groups)


def snapshot_histograms_rollup(tree: MetricsTree, engine: StatEngine, plan: RollupPlan) -> List[HistogramSummary]:
    """telemetry.snapshot_histograms plus the plan's rollups, from one engine call:
    every Stat's snapshottedSummary and reset time are set as there, and the group
    summaries -- of exactly the samples the per-series summaries saw -- are returned."""
    now = time.time()
    series, grouped = engine.snapshot_all_rollup(plan.group_of, max(1, plan.ngroups), reset=True)
    for _, m in live_stats(tree):
        m._set_snapshot(HistogramSummary.from_record(series[m.series_id]), now)
    return [HistogramSummary.from_record(grouped[g]) for g in range(plan.ngroups)]
