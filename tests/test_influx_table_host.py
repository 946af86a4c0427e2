"""The InfluxDB table on the CPU: render_host over influx_table(tree) -- the row grammar
l5dh_render_influx implements, replayed in Python -- against InfluxDbTelemeter.render,
byte for byte, for every tree of tests/influx_cases.py and three host values.
"""
import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd.influxdb import InfluxDbTelemeter
from linkerd_amd.render_influx import influx_table, influx_values, render_host, scrape_inputs

from . import influx_cases as C


def replay(tree, host):
    table, summaries, counters, gauges = scrape_inputs(influx_table(tree))
    return render_host(table, host, summaries, counters, gauges)


@pytest.mark.parametrize("name", sorted(C.NAMED))
@pytest.mark.parametrize("host", C.HOSTS)
def test_named_trees(name, host):
    tree = C.NAMED[name]()
    assert replay(tree, host) == InfluxDbTelemeter(tree).render(host).encode("utf-8")


def test_the_cases_are_what_they_claim():
    assert replay(C.counter_tree(), "none") == b"foo:bar,host=none bas=2\n"
    assert replay(C.gauge_tree(), "none") == b"foo:bar,host=none bas=2.0\n"
    assert replay(C.stat_tree(), "h:80") == (b"foo:bar,host=h:80 bas_avg=1.5,bas_count=2,bas_max=2,bas_min=1,bas_p50=1,"
                                             b"bas_p90=2,bas_p95=2,bas_p99=2,bas_p999=2,bas_p9999=2,bas_sum=3\n")
    assert replay(C.root_tree(), "").startswith(b"root,host= abc=1,def_avg=3.0,")
    rewrites = replay(C.rewrite_tree(), "none").decode("utf-8")
    for line in ("rt,host=none,rt=incoming ", "rt:service,host=none,rt=incoming,service=/svc/foo ",
                 "rt:client,client=/#/bar,host=none,rt=incoming ",
                 "rt:client:service,client=/#/bar,host=none,rt=incoming,service=/svc/foo ",
                 "rt:server,host=none,rt=incoming,server=127.0.0.1/4141 ", "rt:service:service:t,host=none,rt=r,service=s "):
        assert "\n" + line + "requests=1\n" in "\n" + rewrites, line
    # a Stat's fields interleave with its siblings; the duplicate key keeps child order (the Stat's 2, then 7)
    assert replay(C.interleaved_tree(), "none").decode() == C.INTERLEAVED
    # UTF-16 code units, not UTF-8 bytes
    assert C.TILDE.encode("utf-8") < C.SMILE.encode("utf-8")
    assert replay(C.utf16_tree(), "none").decode("utf-8") == f"u,host=none {C.SMILE}=2,{C.TILDE}=1\n"
    # a Stat without a snapshot: its rows are gone, and a parent with nothing else has no line
    table = influx_table(C.unsnapshotted_tree())
    assert table.n == 23 and table.nlines == 2
    assert scrape_inputs(table)[0].n == 1
    assert replay(C.unsnapshotted_tree(), "none") == b"p,host=none c=3\n"
    assert replay(C.empty_tree(), "none") == b""
    assert influx_table(C.empty_tree()).n == 0 and influx_table(C.empty_tree()).nlines == 0


def test_table_arrays():
    table = influx_table(C.interleaved_tree())
    assert (table.n, table.nlines) == (13, 1)
    assert table.line.dtype == np.uint32 and table.kinds.dtype == np.uint8 and table.field.dtype == np.uint8
    assert table.index.dtype == np.uint32 and table.key_off.dtype == np.uint64 and table.key_off.shape == (14,)
    assert table.head_bytes.tobytes() == b"x,host=" and table.tail_bytes.tobytes() == b" "
    keys = [table.key_bytes[int(a):int(b)].tobytes().decode() for a, b in zip(table.key_off[:-1], table.key_off[1:])]
    assert keys[:4] == ["a_avg", "a_count", "a_count", "a_max"]
    assert list(table.kinds[:4]) == [N.KIND_STAT, N.KIND_STAT, N.KIND_COUNTER, N.KIND_STAT]
    assert list(table.field[:2]) == [N.BY_AVG, N.BY_COUNT] and table.field[keys.index("a_p999")] == N.BY_P9990
    counters, gauges = influx_values(table)
    assert list(counters) == [7, 5] and gauges.size == 0 and gauges.dtype == np.float32
    assert list(table.index[table.kinds == N.KIND_COUNTER]) == [0, 1]
    client = influx_table(C.rewrite_tree())
    heads = [client.head_bytes[int(a):int(b)].tobytes() for a, b in zip(client.head_off[:-1], client.head_off[1:])]
    tails = [client.tail_bytes[int(a):int(b)].tobytes() for a, b in zip(client.tail_off[:-1], client.tail_off[1:])]
    assert (b"rt:client,client=/#/bar,host=", b",rt=incoming ") in list(zip(heads, tails))
    assert (np.diff(client.line.astype(np.int64)) >= 0).all() and int(client.line.max()) < client.nlines


def test_random_trees():
    seen = 0
    for seed in range(C.N_RANDOM):
        tree = C.random_tree(seed)
        tel = InfluxDbTelemeter(tree)
        for host in C.HOSTS:
            assert replay(tree, host) == tel.render(host).encode("utf-8"), seed
        seen += 1
    assert seen == C.N_RANDOM == 300


def test_random_trees_cover_the_grammar():
    bodies = [InfluxDbTelemeter(C.random_tree(seed)).render("none") for seed in range(C.N_RANDOM)]
    text = "".join(bodies)
    assert sum(1 for b in bodies if b) > 290 and "a_count=" in text and C.SMILE in text and "root,host=none " in text
    assert ",rt=" in text and ",service=" in text and "client=" in text and "=NaN" in text and "=-0.0" in text


def test_take_drops_stats_without_renumbering():
    """Every other Stat loses its snapshot: the taken table prints the writer's text."""
    for seed in (3, 17, 42, 99):
        tree = C.random_tree(seed)
        table = influx_table(tree)
        full = scrape_inputs(table)
        dropped = table.stats[::2]
        for m in dropped:
            m._set_snapshot(None)
        want = InfluxDbTelemeter(tree).render("h").encode("utf-8")
        # (by hand: the full table's rows minus those Stats', the values as they were)
        gone = {id(m) for m in dropped}
        rows = [j for j, m in enumerate(full[0].metrics) if id(m) not in gone]
        assert render_host(full[0].take(rows), "h", *full[1:]) == want
        assert full[0].take(rows).nlines == table.nlines
        assert replay(tree, "h") == want


def test_the_call_is_declared():
    assert "l5dh_render_influx" in N.SIGNATURES and "l5dh_render_influx" in N.header_symbols()
