"""The three device scrapes over a tree whose counters live in a CounterEngine: the counters
are printed from the engine's live array (no value is fetched per counter), byte for byte the
host writers' text, which pins Java's Long.toString.
"""
import numpy as np
import pytest

from linkerd_amd import _native as N

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
VALUES = [0, -1, (1 << 53) + 1, I64_MAX, I64_MIN, 7, -(1 << 31), 10 ** 18, 12345678901, -42]


def fill(tree, ce=None):
    """About 40 nodes: Stats, counters and gauges under the prefixes the exporters rewrite
    into labels (rt/<router>, rt/<r>/service, rt/<r>/client, rt/<r>/client/<c>/service,
    rt/<r>/server).  Returns the counters in creation order."""
    counters = []
    k = 0
    for r in ("http", "h2"):
        base = ["rt", r]
        for scope in (["service", "svc/a"], ["client", "$/inet/10.0.0.1/80"], ["client", "c2", "service", "svc/b"],
                      ["server", "0.0.0.0/4140"], []):
            node = tree.resolve(base + scope)
            for name in ("requests", "success"):
                counters.append(node.resolve([name]).mk_counter())
            node.resolve(["request_latency_ms"]).mk_stat()
            k += 1
            node.resolve(["load"]).register_gauge(lambda k=k: 0.5 * k)
    counters.append(tree.resolve(["jvm", "gc", "count"]).mk_counter())
    tree.resolve(["jvm", "uptime"]).register_gauge(lambda: 1234.5)
    return counters


def set_values(counters, ce=None):
    """Every counter reaches its value of VALUES (cyclic) through incr alone, or, where an
    Int cannot carry it, through a write of the device value plus increments."""
    for j, m in enumerate(counters):
        v = VALUES[j % len(VALUES)]
        if -(1 << 31) <= v < (1 << 31):
            m.incr(v - 3 if v >= 0 else v + 3)
            m.incr(3 if v >= 0 else -3)
        elif ce is not None:
            ce.write(m.counter_id, np.array([v - 2 if v > 0 else v + 2], np.int64))
            m.incr(2 if v > 0 else -2)
        else:
            m._value = v  # (a host counter: any Python integer)


def snapshot(se, tree):
    from linkerd_amd.telemetry import live_stats, snapshot_histograms
    rng = np.random.default_rng(1)
    for j, (_, stat) in enumerate(live_stats(tree)):
        for v in rng.integers(1, 5000, 3 + j):
            stat.add(float(v))
    snapshot_histograms(tree, se)


@pytest.fixture(scope="module")
def scene(gpu_available):
    from linkerd_amd.counters import CounterEngine
    from linkerd_amd.telemetry import MetricsTree, StatEngine
    se = StatEngine(capacity=64)
    ce = CounterEngine(se, 100, batch=64)
    tree = MetricsTree(se, ce)
    counters = fill(tree, ce)
    set_values(counters, ce)
    snapshot(se, tree)
    yield se, ce, tree, counters
    se.engine.close()


def scrapes(tree, engine):
    """(device bytes, host bytes) of the three exporters."""
    from linkerd_amd.admin_metrics import AdminMetricsExportTelemeter
    from linkerd_amd.influxdb import InfluxDbTelemeter
    from linkerd_amd.prometheus import PrometheusTelemeter
    admin, prom, influx = AdminMetricsExportTelemeter(tree), PrometheusTelemeter(tree), InfluxDbTelemeter(tree)
    return {
        "admin": (admin.handle_bytes("/admin/metrics.json", engine)[2], admin.handle("/admin/metrics.json")[2].encode()),
        # (render_bytes prints the scalar lines first: render()'s lines, in blocks)
        "prometheus": (prom.render_bytes(engine, scalars_on_device=True), prom.render_bytes(engine)),
        "influx": (influx.render_bytes(engine, "h:1"), influx.render("h:1").encode()),
    }


def test_counter_rows_index_by_counter_id(scene):
    from linkerd_amd.admin_metrics import flat_name_table
    from linkerd_amd.nametable import scalar_values
    from linkerd_amd.prometheus import scalar_name_table
    from linkerd_amd.render_influx import influx_table
    se, ce, tree, counters = scene
    for table in (flat_name_table(tree), scalar_name_table(tree), influx_table(tree)):
        rows = np.flatnonzero(table.kinds == N.KIND_COUNTER)
        assert rows.size == len(counters)
        assert [int(table.index[j]) for j in rows] == [table.metrics[int(j)].counter_id for j in rows]
        got, gauges = scalar_values(table)
        assert got.is_cuda and got.data_ptr() == ce.device_values().data_ptr() and got.numel() == ce.capacity
        assert isinstance(gauges, np.ndarray)


def test_values_are_exact(scene):
    se, ce, tree, counters = scene
    assert [m.get() for m in counters] == [VALUES[j % len(VALUES)] for j in range(len(counters))]
    assert {0, -1, (1 << 53) + 1, I64_MAX, I64_MIN} <= {m.get() for m in counters}


def test_device_scrapes_equal_the_host_writers(scene):
    se, ce, tree, counters = scene
    for name, (device, host) in scrapes(tree, se.engine).items():
        assert device == host, name
    from linkerd_amd.prometheus import PrometheusTelemeter, line_multiset
    text = scrapes(tree, se.engine)["prometheus"][0].decode()
    assert line_multiset(text) == line_multiset(PrometheusTelemeter(tree).render())
    assert "9223372036854775807" in text and "-9223372036854775808" in text and "9007199254740993" in text
    assert 'rt:client:requests{rt="http", client="$/inet/10.0.0.1/80"} ' in text
    assert 'rt:service:requests{rt="h2", service="svc/a"} ' in text
    assert 'rt:server:success{rt="h2", server="0.0.0.0/4140"} ' in text


def test_host_writers_take_one_bulk_read(scene, monkeypatch):
    from linkerd_amd.admin_metrics import AdminMetricsExportTelemeter
    from linkerd_amd.influxdb import InfluxDbTelemeter
    from linkerd_amd.prometheus import PrometheusTelemeter
    se, ce, tree, counters = scene
    reads = []
    read = type(ce)._read
    monkeypatch.setattr(type(ce), "_read", lambda self, first, count: (reads.append((first, count)),
                                                                        read(self, first, count))[1])
    monkeypatch.setattr(type(ce), "get", lambda self, cid: pytest.fail("a device read of one counter"))
    admin = AdminMetricsExportTelemeter(tree)
    for render in (PrometheusTelemeter(tree).render, lambda: admin.handle("/admin/metrics.json"),
                   lambda: admin.handle("/admin/metrics.json?tree=1"), lambda: admin.handle("/admin/metrics.json?pretty=1"),
                   InfluxDbTelemeter(tree).render):
        del reads[:]
        assert render()
        assert reads == [(0, ce.capacity)]  # one copy of the whole space


def test_device_scrapes_read_no_counter(scene, monkeypatch):
    """No .get() and no read of the space: the renderers print the live array."""
    se, ce, tree, counters = scene
    monkeypatch.setattr(type(counters[0]), "get", lambda self: pytest.fail("Counter.get during a device scrape")
                        if self._counters is not None else self._value)
    monkeypatch.setattr(type(ce), "values", lambda self: pytest.fail("a bulk read during a device scrape"))
    from linkerd_amd.admin_metrics import AdminMetricsExportTelemeter
    from linkerd_amd.influxdb import InfluxDbTelemeter
    from linkerd_amd.prometheus import PrometheusTelemeter
    assert AdminMetricsExportTelemeter(tree).handle_bytes("/admin/metrics.json", se.engine)[0] == 200
    assert PrometheusTelemeter(tree).render_bytes(se.engine, scalars_on_device=True)
    assert InfluxDbTelemeter(tree).render_bytes(se.engine)


def test_a_pruned_id_starts_at_zero_under_its_new_counter(scene):
    se, ce, tree, counters = scene
    old = tree.resolve(["rt", "h2", "server", "0.0.0.0/4140", "requests"]).metric
    cid, last = old.counter_id, old.get()
    assert last != 0
    tree.resolve(["rt", "h2", "server", "0.0.0.0/4140", "requests"]).prune()
    assert old.counter_id is None and old.get() == last
    old.incr(1000)  # (pruned: staged nowhere)
    new = tree.resolve(["rt", "h2", "server", "fresh", "requests"]).mk_counter()
    assert new.counter_id == cid and new.get() == 0
    new.incr(5)
    new.incr(-7)
    assert new.get() == -2
    for name, (device, host) in scrapes(tree, se.engine).items():
        assert device == host, name
    assert b'rt:server:requests{rt="h2", server="fresh"} -2\n' in scrapes(tree, se.engine)["prometheus"][0]


def test_a_tree_without_a_counter_engine_renders_as_before(gpu_available):
    from linkerd_amd.nametable import scalar_values
    from linkerd_amd.prometheus import scalar_name_table
    from linkerd_amd.telemetry import MetricsTree, StatEngine
    se = StatEngine(capacity=64)
    try:
        tree = MetricsTree(se)
        counters = fill(tree)
        set_values(counters)
        snapshot(se, tree)
        table = scalar_name_table(tree)
        rows = table.kinds == N.KIND_COUNTER
        np.testing.assert_array_equal(table.index[rows], np.arange(int(rows.sum())))  # ordinals
        got, _ = scalar_values(table)
        assert isinstance(got, np.ndarray)  # the host values, one .get() per counter, in table order
        assert got.tolist() == [table.metrics[int(j)].get() for j in np.flatnonzero(rows)]
        assert sorted(got.tolist()) == sorted(m.get() for m in counters)
        for name, (device, host) in scrapes(tree, se.engine).items():
            assert device == host, name
        assert b"9223372036854775807" in scrapes(tree, se.engine)["admin"][0]
    finally:
        se.engine.close()
