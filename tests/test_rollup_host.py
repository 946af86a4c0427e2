"""Label rollups on the host: labels -> groups (plan_rollup), the Prometheus lines of
the groups, the telemeter's optional rollups, StatEngine.snapshot_all_rollup over an
oracle-backed stand-in engine, and the map checks HistogramEngine applies before the
C-ABI.  The truth of a rollup everywhere: the members' oracle bucket counts and totals
summed per group (np.add.at) and summarized by the oracle.
"""
import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd.engine import HistogramEngine
from linkerd_amd.prometheus import PrometheusTelemeter, write_metrics
from linkerd_amd.rollup import RollupPlan, plan_rollup, snapshot_histograms_rollup, write_rollup_metrics
from linkerd_amd.telemetry import HistogramSummary, MetricsTree, MetricsTreeStatsReceiver, StatEngine

from .test_host_engine import OracleEngine


def rollup_truth(O, counts, totals, group, G):
    """(summaries, counts int64 [G][1798], totals int64 [G]) of the groups."""
    group = np.asarray(group, np.uint32)
    m = group != N.NO_GROUP
    gc = np.zeros((G, N.NBUCKETS), np.int64)
    gt = np.zeros(G, np.int64)
    np.add.at(gc, group[m], np.asarray(counts)[m])
    np.add.at(gt, group[m], np.asarray(totals)[m])
    return O.summarize_counts(gc.astype(np.int32), gt), gc, gt


class RollupOracleEngine(OracleEngine):
    """OracleEngine plus HistogramEngine.rollup (full signature), counting engine calls."""

    def __init__(self, S, oracle):
        super().__init__(S, oracle)
        self.calls = []

    def snapshot(self, *a, **kw):
        self.calls.append("snapshot")
        return super().snapshot(*a, **kw)

    def rollup(self, group, ngroups, first=0, count=None, reset=False, with_counts=False, with_series=False):
        self.calls.append("rollup")
        with self.lock:
            count = self.max_series - first if count is None else count
            assert len(group) == count
            sl = slice(first, first + count)
            counts, totals = self.h.h["counts"][sl].copy(), self.h.h["total"][sl].copy()
            out, gc, gt = rollup_truth(self.O, counts, totals, group, ngroups)
            series = self.O.summarize_counts(counts, totals)
            if reset:
                self.h.h[sl] = 0
        res = (out,) + ((gc.astype(np.int32), gt) if with_counts else ()) + ((series,) if with_series else ())
        return res if len(res) > 1 else out


def _tree(eng=None):
    tree = MetricsTree(eng)
    return tree, MetricsTreeStatsReceiver(tree)


def test_plan_rollup_groups_clients_of_a_router(oracle):
    eng = StatEngine(engine=OracleEngine(16, oracle), batch=4)
    tree, stats = _tree(eng)
    a = stats.scope("rt", "http", "client", "a").stat("request_latency_ms")
    b = stats.scope("rt", "http", "client", "b").stat("request_latency_ms")
    h2 = stats.scope("rt", "h2", "client", "a").stat("request_latency_ms")
    conn = stats.scope("rt", "http", "client", "a").stat("connect_latency_ms")
    srv = stats.scope("rt", "http", "server", "x").stat("request_latency_ms")
    stats.scope("rt", "http", "client", "a").counter("requests")  # not a Stat: ignored
    plan = plan_rollup(tree, without=("client",), capacity=16)
    assert plan.group_of.dtype == np.uint32 and plan.group_of.shape == (16,)
    assert sorted(plan.groups) == sorted([
        ("rt:client:request_latency_ms", (("rt", "http"),)),
        ("rt:client:request_latency_ms", (("rt", "h2"),)),
        ("rt:client:connect_latency_ms", (("rt", "http"),)),
    ])
    g = {gid: i for i, gid in enumerate(plan.groups)}
    assert plan.group_of[a.series_id] == plan.group_of[b.series_id] == g[("rt:client:request_latency_ms", (("rt", "http"),))]
    assert plan.group_of[h2.series_id] == g[("rt:client:request_latency_ms", (("rt", "h2"),))]
    assert plan.group_of[conn.series_id] == g[("rt:client:connect_latency_ms", (("rt", "http"),))]
    assert plan.group_of[srv.series_id] == N.NO_GROUP  # no `client` label: would only duplicate itself
    used = {s.series_id for s in (a, b, h2, conn, srv)}
    assert all(plan.group_of[i] == N.NO_GROUP for i in range(16) if i not in used)


def test_plan_rollup_without_two_labels(oracle):
    eng = StatEngine(engine=OracleEngine(16, oracle), batch=4)
    tree, stats = _tree(eng)
    ss = [stats.scope("rt", r, "client", c).stat("request_latency_ms") for r in ("http", "h2") for c in ("a", "b")]
    srv = stats.scope("rt", "http", "server", "x").stat("request_latency_ms")
    plan = plan_rollup(tree, without=("client", "rt"), capacity=16)
    # all four client Stats in one label-free group; the server Stat loses `rt` and keeps `server`
    assert sorted(plan.groups) == sorted([("rt:client:request_latency_ms", ()),
                                          ("rt:server:request_latency_ms", (("server", "x"),))])
    assert len({int(plan.group_of[s.series_id]) for s in ss}) == 1
    assert plan.groups[plan.group_of[ss[0].series_id]] == ("rt:client:request_latency_ms", ())
    assert plan.groups[plan.group_of[srv.series_id]] == ("rt:server:request_latency_ms", (("server", "x"),))


def test_plan_rollup_skips_pruned_stats_and_follows_reissued_ids(oracle, monkeypatch):
    monkeypatch.setattr(N, "limits", oracle.limits)
    eng = StatEngine(engine=OracleEngine(4, oracle), batch=4)
    tree, stats = _tree(eng)
    a = stats.scope("rt", "http", "client", "a").stat("request_latency_ms")
    b = stats.scope("rt", "http", "client", "b").stat("request_latency_ms")
    old_b = b.series_id
    stats.prune("rt", "http", "client", "b")
    assert b.series_id is None
    plan = plan_rollup(tree, without=("client",), capacity=4)
    assert plan.groups == [("rt:client:request_latency_ms", (("rt", "http"),))]
    assert plan.group_of[a.series_id] == 0 and plan.group_of[old_b] == N.NO_GROUP
    # the id is handed out again, to a Stat of another router: it follows its new owner
    c = stats.scope("rt", "h2", "client", "c").stat("request_latency_ms")
    assert c.series_id == old_b
    plan = plan_rollup(tree, without=("client",), capacity=4)
    assert plan.groups[plan.group_of[c.series_id]] == ("rt:client:request_latency_ms", (("rt", "h2"),))
    assert plan.groups[plan.group_of[a.series_id]] == ("rt:client:request_latency_ms", (("rt", "http"),))


def test_write_rollup_metrics_format():
    plan = RollupPlan(np.zeros(0, np.uint32), [("rt:client:request_latency_ms", (("rt", "http"),)),
                                               ("rt:client:connect_latency_ms", ())])
    summaries = [HistogramSummary(3, 1, 113, 120, 6, 113, 113, 113, 113, 113, 40.0),
                 HistogramSummary(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0)]  # an empty group
    out = []
    write_rollup_metrics(plan, summaries, out)
    assert out == [
        'rt:client:request_latency_ms_count{rt="http"} 3\n',
        'rt:client:request_latency_ms_sum{rt="http"} 120\n',
        'rt:client:request_latency_ms_avg{rt="http"} 40.0\n',
        'rt:client:request_latency_ms{rt="http", quantile="0"} 1\n',
        'rt:client:request_latency_ms{rt="http", quantile="0.5"} 6\n',
        'rt:client:request_latency_ms{rt="http", quantile="0.9"} 113\n',
        'rt:client:request_latency_ms{rt="http", quantile="0.95"} 113\n',
        'rt:client:request_latency_ms{rt="http", quantile="0.99"} 113\n',
        'rt:client:request_latency_ms{rt="http", quantile="0.999"} 113\n',
        'rt:client:request_latency_ms{rt="http", quantile="0.9999"} 113\n',
        'rt:client:request_latency_ms{rt="http", quantile="1"} 113\n',
        'rt:client:connect_latency_ms_count 0\n',
        'rt:client:connect_latency_ms_sum 0\n',
        'rt:client:connect_latency_ms_avg 0.0\n',
        'rt:client:connect_latency_ms{quantile="0"} 0\n',
        'rt:client:connect_latency_ms{quantile="0.5"} 0\n',
        'rt:client:connect_latency_ms{quantile="0.9"} 0\n',
        'rt:client:connect_latency_ms{quantile="0.95"} 0\n',
        'rt:client:connect_latency_ms{quantile="0.99"} 0\n',
        'rt:client:connect_latency_ms{quantile="0.999"} 0\n',
        'rt:client:connect_latency_ms{quantile="0.9999"} 0\n',
        'rt:client:connect_latency_ms{quantile="1"} 0\n',
    ]


def _fed_tree(oracle, S=16):
    eng = StatEngine(engine=RollupOracleEngine(S, oracle), batch=8)
    tree, stats = _tree(eng)
    rng = np.random.default_rng(5)
    fed = {}
    for r in ("http", "h2"):
        for c in ("a", "b", "c"):
            s = stats.scope("rt", r, "client", c).stat("request_latency_ms")
            vals = np.exp(3.0 + rng.standard_normal(40)).astype(np.float32)
            for v in vals:
                s.add(float(v))
            fed.setdefault(r, []).extend(vals.tolist())
    stats.scope("rt", "http", "client", "a").counter("requests").incr(7)
    return eng, tree, fed


def test_telemeter_without_rollups_is_unchanged_and_appends_with(oracle):
    eng, tree, fed = _fed_tree(oracle)
    plan = plan_rollup(tree, without=("client",), capacity=eng.capacity)
    summaries = snapshot_histograms_rollup(tree, eng, plan)
    plain = []
    write_metrics(tree, plain)
    assert PrometheusTelemeter(tree).render() == "".join(plain)  # byte-identical to today's
    tel = PrometheusTelemeter(tree, rollups=(plan, summaries))
    extra = []
    write_rollup_metrics(plan, summaries, extra)
    assert len(extra) == 22
    assert tel.render() == "".join(plain) + "".join(extra)
    tel.rollups = None  # settable later
    assert tel.render() == "".join(plain)


def test_snapshot_all_rollup_is_one_engine_call_and_matches_one_stat_per_group(oracle):
    eng, tree, fed = _fed_tree(oracle)
    plan = plan_rollup(tree, without=("client",), capacity=eng.capacity)
    eng.engine.calls.clear()
    series, groups = eng.snapshot_all_rollup(plan.group_of, plan.ngroups, reset=True)
    assert eng.engine.calls == ["rollup"]  # the flush ingests; ONE snapshotting call
    assert len(series) == eng.capacity and len(groups) == plan.ngroups == 2
    for g, (key, labels) in enumerate(plan.groups):
        one = oracle.PyStat()  # ONE Stat fed the union of the router's samples
        for v in fed[dict(labels)["rt"]]:
            one.add(v)
        want = one.summary()
        for f in N.SUMMARY_FIELDS:
            assert groups[g][f] == want[f], (key, labels, f)
    assert int(series["count"].sum()) == 240 and int(groups["count"].sum()) == 240
    # reset=True cleared the state: a second call sees nothing
    series, groups = eng.snapshot_all_rollup(plan.group_of, plan.ngroups, reset=True)
    assert not series["count"].any() and not groups["count"].any()


def test_snapshot_histograms_rollup_sets_every_stat_like_snapshot_histograms(oracle):
    from linkerd_amd.telemetry import snapshot_histograms
    eng, tree, _ = _fed_tree(oracle)
    eng2, tree2, _ = _fed_tree(oracle)
    plan = plan_rollup(tree, without=("client",), capacity=eng.capacity)
    snapshot_histograms_rollup(tree, eng, plan)
    snapshot_histograms(tree2, eng2)
    a, b = [], []
    write_metrics(tree, a)
    write_metrics(tree2, b)
    assert sorted(a) == sorted(b) and len(a) == 6 * 11 + 1


def _bare_engine(S=100, device=0):
    e = HistogramEngine.__new__(HistogramEngine)  # no context: only the host-side checks run
    e.max_series, e.device, e._stream, e._events = S, device, None, []
    return e


def test_rollup_map_checks_run_before_the_c_call():
    e = _bare_engine()
    g, G = e._group_map(np.array([0, -1, 2] + [1] * 97, np.int64), 3, 100)
    assert g.dtype == np.uint32 and G == 3 and g[1] == N.NO_GROUP and g[2] == 2
    g, _ = e._group_map(np.full(100, -1, np.int32), 1, 100)
    assert (g == N.NO_GROUP).all()
    ok = np.zeros(100, np.uint32)
    for bad in (0, -1, N.MAX_SERIES + 1):
        with pytest.raises(ValueError, match="ngroups"):
            e.rollup(ok, bad)
    with pytest.raises(ValueError, match="entries for 100 series"):
        e.rollup(np.zeros(99, np.uint32), 4)
    with pytest.raises(ValueError, match="entries for 10 series"):
        e.rollup(ok, 4, first=5, count=10)
    with pytest.raises(ValueError, match="dtype"):
        e.rollup(np.zeros(100, np.float32), 4)
    with pytest.raises(ValueError, match="dtype"):
        e.rollup(np.zeros(100, np.uint16), 4)
    with pytest.raises(ValueError, match="-1"):
        e.rollup(np.full(100, -2, np.int64), 4)
    with pytest.raises(ValueError, match="-1"):
        e.rollup(np.full(100, 2 ** 32, np.int64), 4)
    with pytest.raises(ValueError, match="outside"):
        e.rollup(ok, 4, first=90, count=20)
    with pytest.raises(ValueError, match="whole rows"):
        e.rollup_dense(np.zeros(1799, np.int32), None, np.zeros(1, np.uint32), 1)
    with pytest.raises(ValueError, match="entries for 2 series"):
        e.rollup_dense(np.zeros((2, 1798), np.int32), None, np.zeros(3, np.uint32), 1)
    import torch
    with pytest.raises(ValueError, match="dtype"):
        e.rollup(torch.zeros(100, dtype=torch.int64), 4)


def test_native_mirrors_rollup_constants():
    import re
    h = open(N.HEADER_PATH).read()
    assert int(re.search(r"L5DH_PARAM_ROLLUP_ITEM = (\d+)", h).group(1)) == N.PARAM_ROLLUP_ITEM == 14
    assert int(re.search(r"#define L5DH_NO_GROUP (0x[0-9A-Fa-f]+)u", h).group(1), 16) == N.NO_GROUP
    assert {"l5dh_rollup", "l5dh_rollup_dense"} <= set(N.SIGNATURES) & set(N.header_symbols())
