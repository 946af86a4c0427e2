"""The InfluxDB body of the device renderer (l5dh_render_influx) against the Python writer,
byte for byte: InfluxDbTelemeter.render of a tree, and render_influx.render_host -- the
table's grammar replayed in Python -- where the table or the values are crafted.
"""
import ctypes
import errno

import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd.influxdb import InfluxDbTelemeter
from linkerd_amd.prometheus import summary_records
from linkerd_amd.render_influx import (QUERY, InfluxTable, pack_texts, influx_names, influx_table, render_host, render_influx,
                                       scrape_inputs)
from linkerd_amd.telemetry import (HistogramSummary, MetricsTree, MetricsTreeStatsReceiver, StatEngine,
                                   snapshot_histograms)

from . import influx_cases as IC
from . import render_cases as C
from .test_exporters_host import ONE_TWO
from .test_gpu_render_json import GUARD, _dev, last_error, render_guarded

pytestmark = pytest.mark.gpu

CHUNK, STAGE = 64, 4096  # rows of a write-pass chunk, bytes of a chunk built in LDS (l5dh_influx.hip)


@pytest.fixture(scope="module")
def eng(gpu_available):
    from linkerd_amd.engine import HistogramEngine
    with HistogramEngine(32) as e:
        yield e


def dev_values(summaries, counters, gauges):
    return (None if summaries is None else _dev(summaries.view(np.int64)), None if counters is None else _dev(counters),
            None if gauges is None else _dev(gauges))


def check(eng, table, host, values, want, skew=5):
    """Host table and values into a host buffer; the size query; the device table and
    values into a guarded device buffer of exactly len(want) bytes."""
    got = render_influx(eng, table, host, *values)
    assert len(got) == len(want)
    assert got == want
    assert render_influx(eng, table, host, *values, out=QUERY) == len(want)
    if want:
        dtab, dv = table.to_device(), dev_values(*values)
        assert render_guarded(lambda out: render_influx(eng, dtab, host, *dv, out=out), len(want), skew) == want


def check_tree(eng, tree, host="none", skew=5):
    table, *values = scrape_inputs(influx_table(tree))
    check(eng, table, host, values, InfluxDbTelemeter(tree).render(host).encode("utf-8"), skew)
    return table


# ---- row counts around the chunk -----------------------------------------------------------
def rows_tree(n):
    """A tree whose table has n field rows: Stats (eleven rows), counters and gauges spread
    over client scopes, so lines of several lengths begin and end inside the chunks."""
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    left, i = n, 0
    while left:
        sc = stats.scope("rt", f"r{i % 3}", "client", f"$inet$10.0.0.{i % 4}$80")
        if left >= 11 and i % 3 == 0:
            sc.stat(f"latency{i}")._set_snapshot(IC.SUMMARIES[i % len(IC.SUMMARIES)])
            left -= 11
        elif i % 2:
            sc.counter(f"requests{i}").incr(10 ** (i % 19) - i)
            left -= 1
        else:
            sc.add_gauge(f"load{i}", f=lambda v=IC.GAUGES[i % len(IC.GAUGES)]: v)
            left -= 1
        i += 1
    return tree


@pytest.mark.parametrize("n", [1, 11, 63, 64, 65, 128, 129, 257])
def test_row_counts_around_the_chunk(eng, n):
    table = check_tree(eng, rows_tree(n), "h:80", skew=n % 16)
    assert table.n == n


def counters_tree(sizes):
    """One scope per entry of sizes, with that many counters."""
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    for s, size in enumerate(sizes):
        for i in range(size):
            stats.scope(f"scope{s:03d}").counter(f"c{i:03d}").incr(s * 1000 + i)
    return tree


def test_lines_and_chunks(eng):
    # one line of 200 counters: the line spans four chunks
    table = check_tree(eng, counters_tree([200]))
    assert (table.n, table.nlines) == (200, 1)
    # one-field lines: 64 line starts in one chunk
    table = check_tree(eng, counters_tree([1] * 70))
    assert (table.n, table.nlines) == (70, 70)
    # a line that ends exactly at row 63 and another exactly at row 64
    # (crafted: a tree's child order is the reference's hash order, not the order of registration)
    table = crafted([f"m{l},host=" for l in range(3)], [f",rt=r{l} " for l in range(3)],
                    counter_rows([f"c{j}" for j in range(70)], [0] * CHUNK + [1] + [2] * 5))
    counters = np.arange(70, dtype=np.int64) - 35
    assert list(np.flatnonzero(np.diff(table.line.astype(np.int64))) + 1) == [CHUNK, CHUNK + 1]
    check(eng, table, "none", (None, counters, None), render_host(table, "none", None, counters, None))


def test_output_at_every_skew(eng):
    tree = rows_tree(65)
    table, *values = scrape_inputs(influx_table(tree))
    want = InfluxDbTelemeter(tree).render("none").encode("utf-8")
    dtab, dv = table.to_device(), dev_values(*values)
    for skew in range(16):
        assert render_guarded(lambda out: render_influx(eng, dtab, "none", *dv, out=out), len(want), skew) == want


# ---- the long pieces -------------------------------------------------------------------------
def crafted(heads, tails, rows):
    """A table from its texts: rows of (line, kind, field, index, key)."""
    key_off, key_bytes = pack_texts([r[4] for r in rows])
    head_off, head_bytes = pack_texts(heads)
    tail_off, tail_bytes = pack_texts(tails)
    col = lambda i, dt: np.asarray([r[i] for r in rows], np.int64).astype(dt)  # noqa: E731
    return InfluxTable(col(0, np.uint32), col(1, np.uint8), col(2, np.uint8), col(3, np.uint32), key_off, key_bytes,
                       head_off, head_bytes, tail_off, tail_bytes)


def counter_rows(keys, lines=None):
    return [(0 if lines is None else lines[j], N.KIND_COUNTER, 0, j, k) for j, k in enumerate(keys)]


@pytest.mark.parametrize("at", [CHUNK, CHUNK - 1])
def test_long_field_key(eng, at):
    """A 5 000-byte key as the first row of a chunk and as lane 63: its chunk is built
    straight in the output, the other one in LDS."""
    keys = [f"k{j:02d}" for j in range(80)]
    keys[at] = "K" * 5000
    table = crafted(["m,host="], [",rt=r "], counter_rows(keys))
    counters = np.arange(80, dtype=np.int64) * 977
    for skew in (0, 9):
        check(eng, table, "none", (None, counters, None), render_host(table, "none", None, counters, None), skew)


def test_long_head_tail_and_host(eng):
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    for i in range(40):  # a 5 000-byte router name (the tail) and client id (the head), short ones around them
        stats.scope("rt", "R" * 5000 if i == 7 else f"r{i}", "client", "C" * 5000 if i == 20 else f"c{i}").counter(
            "requests").incr(i)
        stats.scope("rt", "R" * 5000 if i == 7 else f"r{i}", "client", "C" * 5000 if i == 20 else f"c{i}").add_gauge(
            "load", f=lambda i=i: i / 4)
    table = influx_table(tree)
    assert table.n >= 70 and np.diff(table.head_off.astype(np.int64)).max() > 5000
    assert np.diff(table.tail_off.astype(np.int64)).max() > 5000
    for host, skew in (("none", 0), ("none", 13), ("H" * 300, 3), ("H" * 300, 8), ("", 1), ("", 15)):
        check_tree(eng, tree, host, skew)


@pytest.mark.parametrize("total", [STAGE - 1, STAGE, STAGE + 1])
def test_chunk_around_the_stage_size(eng, total):
    """The first chunk's bytes just under, at and just over the stage, from key lengths."""
    keys = [("k%02d" % j) * (1 + j % 30) for j in range(70)]  # 3 to 90 bytes: both kinds of key copy
    counters = np.arange(70, dtype=np.int64)
    first = lambda t: len(render_host(t.take(np.arange(CHUNK)), "none", None, counters, None)) - 1  # noqa: E731 (no newline)
    base = first(crafted(["m,host="], [" "], counter_rows(keys)))
    keys[10] = "x" * (len(keys[10]) + total - base)
    table = crafted(["m,host="], [" "], counter_rows(keys))
    assert first(table) == total
    for skew in (0, 7):
        check(eng, table, "none", (None, counters, None), render_host(table, "none", None, counters, None), skew)


# ---- values -------------------------------------------------------------------------------------
def test_values(eng):
    gauges = np.array([float("nan"), float("inf"), -float("inf"), -0.0, 3.4028235e38, 1e-45, 2.0 ** 70, 0.1, 123456.79],
                      np.float32)
    counters = np.array([-2 ** 63, 2 ** 63 - 1, 0, -1, 10 ** 18], np.int64)
    avgs = [x for x in C.KNOWN + C.EDGES if C.in_domain(x)]
    summ = np.zeros(len(avgs) + 1, N.SUMMARY_DTYPE)
    edges = np.array(C.INT64_EDGES, np.int64)
    for f, name in enumerate(N.SUMMARY_FIELDS[:-1]):
        summ[name] = edges[(np.arange(summ.size) * 5 + 7 * f) % edges.size]
    summ["avg"][:-1] = avgs
    summ[-1] = summary_records([HistogramSummary(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0)])[0]  # count == 0: eleven fields
    rows, line = [], 0
    for i in range(summ.size):
        rows += [(line, N.KIND_STAT, f, i, f"s{i}{sfx}") for f, sfx in enumerate(("_count", "_min", "_max", "_sum", "_p50",
                                                                                  "_p90", "_p95", "_p99", "_p999", "_p9999",
                                                                                  "_avg"))]
        line += i % 2
    rows += [(line, N.KIND_GAUGE, 0, i, f"g{i}") for i in range(gauges.size)]
    rows += [(line + 1, N.KIND_COUNTER, 0, i, f"c{i}") for i in range(counters.size)]
    table = crafted([f"m{l},host=" for l in range(line + 2)], [" "] * (line + 2), rows)
    want = render_host(table, "none", summ, counters, gauges)
    text = want.decode()
    for piece in ("=NaN", "=Infinity", "=-Infinity", "=-0.0", "=3.4028235E38", "=1.4E-45", "=1.1805916E21",
                  "c0=-9223372036854775808", "c1=9223372036854775807", "_avg=2.82879384806159008E17",
                  f"s{summ.size - 1}_count=0,", f"s{summ.size - 1}_avg=0.0"):
        assert piece in text, piece
    check(eng, table, "none", (summ, counters, gauges), want)
    # an index with repeats, and a permutation
    rng = np.random.default_rng(5)
    stat = table.kinds == N.KIND_STAT
    for index in (np.where(stat, rng.integers(0, summ.size, table.n), table.index),
                  np.where(stat, rng.permutation(summ.size)[table.index % summ.size], table.index)):
        t2 = table.with_index(index.astype(np.uint32))
        check(eng, t2, "h", (summ, counters, gauges), render_host(t2, "h", summ, counters, gauges), skew=11)


# ---- the contract ---------------------------------------------------------------------------------
def _raw(eng, table, host, summ, counters, gauges, out, cap, n=None, nlines=None, host_len=None):
    nm, ln = influx_names(eng, table), ctypes.c_size_t(12345)
    arr = lambda a: (None, 0) if a is None else (a.ctypes.data, a.size)  # noqa: E731
    hb = np.frombuffer(host, np.uint8) if host else None
    rc = eng._lib.l5dh_render_influx(eng._ctx, ctypes.byref(nm), table.n if n is None else n,
                                     table.nlines if nlines is None else nlines, *arr(hb)[:1],
                                     len(host) if host_len is None else host_len, *arr(summ), *arr(counters), *arr(gauges),
                                     None if out is None else out.data_ptr(), cap, ctypes.byref(ln))
    return rc, ln.value


def contract_case():
    tree = rows_tree(65)
    table, *values = scrape_inputs(influx_table(tree))
    return table, values, InfluxDbTelemeter(tree).render("none").encode("utf-8")


def test_contract_sizes(eng):
    import torch
    table, values, want = contract_case()
    assert _raw(eng, table, b"none", *values, None, 0) == (0, len(want))  # the size query
    assert render_influx(eng, table, b"none", *values, out=QUERY) == len(want)
    buf = torch.full((len(want) + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    assert _raw(eng, table, b"none", *values, buf, len(want) - 1) == (-errno.ERANGE, len(want))
    assert last_error(eng) == f"render_influx: the text takes {len(want)} bytes, cap is {len(want) - 1}"
    assert (buf.cpu().numpy() == GUARD).all()  # nothing was written
    assert _raw(eng, table, b"none", *values, buf, len(want)) == (0, len(want))
    assert buf.cpu().numpy()[:len(want)].tobytes() == want and (buf.cpu().numpy()[len(want):] == GUARD).all()
    # n == 0
    assert _raw(eng, table, b"none", *values, buf, 64, n=0) == (0, 0)
    empty = influx_table(MetricsTree())
    assert render_influx(eng, empty, "none", None, None, None) == b""
    assert render_influx(eng, empty, "none", None, None, None, out=QUERY) == 0
    # nlines larger than any used id: more heads and tails than lines with rows
    more = InfluxTable(table.line, table.kinds, table.field, table.index, table.key_off, table.key_bytes,
                       *pack_texts([table.head_bytes[int(a):int(b)].tobytes().decode() for a, b in
                               zip(table.head_off[:-1], table.head_off[1:])] + ["unused,host="] * 3),
                       *pack_texts([table.tail_bytes[int(a):int(b)].tobytes().decode() for a, b in
                               zip(table.tail_off[:-1], table.tail_off[1:])] + [" "] * 3))
    assert more.nlines == table.nlines + 3
    assert render_influx(eng, more, "none", *values) == want
    # the host's checks
    ln = ctypes.c_size_t(0)
    assert eng._lib.l5dh_render_influx(eng._ctx, None, 65, 1, None, 0, None, 0, None, 0, None, 0, None, 0,
                                       ctypes.byref(ln)) == -errno.EINVAL
    nm = influx_names(eng, table)
    nm.field = None
    assert eng._lib.l5dh_render_influx(eng._ctx, ctypes.byref(nm), 65, table.nlines, None, 0, None, 0, None, 0, None, 0,
                                       None, 0, ctypes.byref(ln)) == -errno.EINVAL
    assert _raw(eng, table, b"", *values, None, 0, host_len=4)[0] == -errno.EINVAL  # a null host with a length
    long_host = b"h" * 65536
    assert _raw(eng, table, long_host, *values, None, 0)[0] == -errno.EINVAL
    assert _raw(eng, table, long_host[:65535], *values, None, 0) == (0, len(want) + table_lines(want) * (65535 - 4))
    s, c, g = values
    assert eng._lib.l5dh_render_influx(eng._ctx, ctypes.byref(influx_names(eng, table)), 65, table.nlines, None, 0,
                                       s.ctypes.data, s.size, None, 3, g.ctypes.data, g.size, None, 0,
                                       ctypes.byref(ln)) == -errno.EINVAL  # a count without its array


def table_lines(body: bytes) -> int:
    return body.count(b"\n")


def test_device_findings(eng):
    table, (summ, counters, gauges), want = contract_case()

    def finding(code, row, message, t=None, s=summ, c=counters, g=gauges):
        with pytest.raises(N.L5dhError, match=f"row {row}( |$)") as ei:
            render_influx(eng, table if t is None else t, "none", s, c, g)
        assert ei.value.code == code
        assert last_error(eng) == "render_influx: " + message.format(row=row)
        assert render_influx(eng, table, "none", summ, counters, gauges) == want  # a valid call afterwards succeeds

    def changed(**arrays):
        t = InfluxTable(*table._arrays())
        for k, v in arrays.items():
            setattr(t, k, v)
        return t

    stat_rows = np.flatnonzero(table.kinds == N.KIND_STAT)
    gauge_rows = np.flatnonzero(table.kinds == N.KIND_GAUGE)
    kinds = table.kinds.copy()
    kinds[[37, 50]] = 7
    finding(-errno.EINVAL, 37, "the kind of row {row} is none of the three", changed(kinds=kinds))
    field = table.field.copy()
    field[stat_rows[[4, 9]]] = 11
    finding(-errno.EINVAL, stat_rows[4], "field of row {row} is above 10", changed(field=field))
    # an index at its kind's count: one gauge fewer than the rows name
    top = int(table.index[gauge_rows].max())
    finding(-errno.EINVAL, min(r for r in gauge_rows if table.index[r] >= top),
            "index of row {row} is not < the count of its kind", g=gauges[:top])
    finding(-errno.EINVAL, stat_rows[0], "index of row {row} is not < the count of its kind", s=None)  # a kind without values
    line = table.line.copy()
    line[30] = line[29] + 1
    assert line[31] < line[30]
    finding(-errno.EINVAL, 31, "line of row {row} is not < nlines, or descends", changed(line=line))  # descending
    line = table.line.copy()
    line[40:] = np.maximum(line[40:], table.nlines)
    finding(-errno.EINVAL, 40, "line of row {row} is not < nlines, or descends", changed(line=line))  # >= nlines
    off = table.key_off.copy()
    off[51] = off[50] - 1
    finding(-errno.EINVAL, 50, "key_off descends at row {row}", changed(key_off=off))
    l = int(table.line[45])
    off = table.head_off.copy()
    off[l + 1] = off[l] - 1
    finding(-errno.EINVAL, int(np.flatnonzero(table.line == l)[0]),
            "head_off or tail_off descends at the line of row {row}", changed(head_off=off))
    far = summ.copy()
    avg_rows = stat_rows[table.field[stat_rows] == N.BY_AVG]
    far["avg"][table.index[avg_rows[1]]] = 2.0 ** 70
    finding(-errno.ERANGE, min(r for r in avg_rows if table.index[r] == table.index[avg_rows[1]]),
            "avg of row {row} is outside +-[2^-64, 2^64), 0, NaN, Infinity", s=far)
    assert _raw(eng, table, b"h" * 65536, summ, counters, gauges, None, 0)[0] == -errno.EINVAL


# ---- end to end -------------------------------------------------------------------------------------
def test_render_bytes_end_to_end(gpu_available):
    """The small StatEngine tree of test_gpu_render_json's end-to-end test, one snapshot."""
    rng = np.random.default_rng(6)
    se = StatEngine(capacity=64, batch=1 << 12)
    tree = MetricsTree(se)
    stats = MetricsTreeStatsReceiver(tree)
    made = []
    for i in range(12):
        sc = stats.scope("rt", ("incoming", "outgoing")[i % 2], "client", f"$inet$10.0.0.{i}$8080")
        made.append(sc.stat("request_latency_ms"))
        sc.counter("requests").incr(1000 * i + 1)
        sc.add_gauge("connections", f=lambda i=i: i * 1.25 if i != 5 else float("nan"))
    idle = stats.scope("rt", "incoming").stat("idle")  # no samples: count == 0
    for st in made:
        for v in np.exp(3.0 + 2.0 * rng.standard_normal(50)).astype(np.float32):
            st.add(float(v))
    assert snapshot_histograms(tree, se) == 13
    late = stats.scope("rt", "incoming").stat("late")  # registered since: no snapshotted summary
    assert idle.snapshotted_summary.count == 0 and late.snapshotted_summary is None
    tel, eng = InfluxDbTelemeter(tree), se.engine
    body = tel.render("none")
    assert tel.render_bytes(eng) == body.encode("utf-8")
    assert "idle_count=0," in body and "late_" not in body and "connections=NaN" in body and "request_latency_ms_avg=" in body
    assert tel.render_bytes(eng, "example.org:4140") == tel.render("example.org:4140").encode("utf-8")
    # the table kept by the caller, the records (by series id) left on the device: `late` has a
    # series id, so it prints its (empty) record
    table = influx_table(tree)
    recs = np.zeros(se.capacity, N.SUMMARY_DTYPE)
    for m in table.stats:
        if m.snapshotted_summary is not None:
            recs[m.series_id] = summary_records([m.snapshotted_summary])[0]
    got = tel.render_bytes(eng, "none", table=table, summaries=_dev(recs.view(np.int64)))
    late._set_snapshot(HistogramSummary.from_record(recs[late.series_id]))
    assert got == tel.render("none").encode("utf-8") and b"late_count=0," in got
    # an avg outside the device formatter's domain: the body is the host writer's
    made[0]._set_snapshot(HistogramSummary(2, 1, 2, 3, 1, 2, 2, 2, 2, 2, 2.0 ** 70))
    assert tel.render_bytes(eng) == tel.render().encode("utf-8") and b"_avg=1.1805916207174113E21" in tel.render_bytes(eng)
    se.engine.close()


def test_random_trees_on_the_device(eng):
    seen = 0
    for seed in range(IC.N_RANDOM):
        tree = IC.random_tree(seed)
        table, *values = scrape_inputs(influx_table(tree))
        assert render_influx(eng, table, "h:80", *values) == InfluxDbTelemeter(tree).render("h:80").encode("utf-8"), seed
        seen += 1
    assert seen == 300


def test_one_two_is_the_reference_line(eng):
    tree = MetricsTree()
    MetricsTreeStatsReceiver(tree).scope("foo", "bar").stat("bas")._set_snapshot(ONE_TWO)
    assert InfluxDbTelemeter(tree).render_bytes(eng) == (
        b"foo:bar,host=none bas_avg=1.5,bas_count=2,bas_max=2,bas_min=1,bas_p50=1,bas_p90=2,bas_p95=2,bas_p99=2,"
        b"bas_p999=2,bas_p9999=2,bas_sum=3\n")
