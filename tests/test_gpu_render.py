"""The device renderer (l5dh_render_summaries, l5dh_render_le) against the Python
exporters, byte for byte: the engine is used for its context only, names and values are
crafted.  The expected bytes are "".join(lines).encode() with the lines of write_metrics
on a Stat-only tree, of write_rollup_metrics, and of write_histogram_metrics over a stub
engine -- exact equality in table order.
"""
import ctypes
import errno
import types

import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd.prometheus import (NameTable, PrometheusTelemeter, line_multiset, rollup_name_table, stat_name_table,
                                    summary_records, write_histogram_metrics, write_metrics)
from linkerd_amd.rollup import RollupPlan, plan_rollup, write_rollup_metrics
from linkerd_amd.telemetry import (HistogramSummary, MetricsTree, MetricsTreeStatsReceiver, StatEngine,
                                   snapshot_histograms_le)

from . import render_cases as C

pytestmark = pytest.mark.gpu

BOUNDS16 = (1, 2, 5, 10, 25, 50, 100, 250, 500, 1000, 2500, 5000, 10000, 30000, 60000, float("inf"))
GUARD = 0xA5


@pytest.fixture(scope="module")
def eng(gpu_available):
    from linkerd_amd.engine import HistogramEngine
    with HistogramEngine(32) as e:
        yield e


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ---- crafted names and values ---------------------------------------------------------
def stat_tree(n):
    """A Stat-only tree of n Stats: keys of 1 to 40 bytes without labels (an empty inner
    text, every alignment of the output cursor), a key of 300 bytes, a label text of 5 000
    bytes, multi-byte UTF-8 in a label, then labelled Stats of C5's shape."""
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    for j in range(n):
        if j < 40:
            stats.stat(("abcdefghij" * 4)[:j + 1])
        elif j == 40:
            stats.stat("K" * 300)
        elif j == 41:
            stats.scope("rt", "r", "client", "c" * 5000).stat("lat")
        elif j == 42:
            stats.scope("rt", "http", "client", 'é√日本"\\\n').stat("request_latency_ms")
        else:
            stats.scope("rt", f"router{j % 7}", "client", f"$inet$10.0.{j // 256}.{j % 256}$8080").stat(
                "request_latency_ms")
    return tree


@pytest.fixture(scope="module")
def avgs():
    """The avg set of the CPU test: every fixed case inside the domain, 2 000 quotients."""
    return np.array([x for x in C.fixed_doubles() if C.in_domain(x)] + list(C.quotients()[:2000]), np.float64)


def crafted_summaries(nvalues, avgs):
    """Every integer edge value in every one of the ten integer fields (a negative sum
    among them), the avgs cycled."""
    v = np.zeros(nvalues, N.SUMMARY_DTYPE)
    edges = np.array(C.INT64_EDGES, np.int64)
    i = np.arange(nvalues)
    for f, name in enumerate(N.SUMMARY_FIELDS[:-1]):
        v[name] = edges[(i + 7 * f) % edges.size]
    v["avg"] = avgs[i % avgs.size]
    return v


def summary_case(n, index_kind, avgs, seed=1):
    """(table, values, expected bytes): the expected text from write_metrics on the tree
    whose Stats hold the records the table's index points at."""
    tree = stat_tree(n)
    table = stat_name_table(tree)
    assert table.n == n
    nvalues = n + 5
    values = crafted_summaries(nvalues, avgs)
    if index_kind == "none":
        index = None
    else:  # a permutation with repeats
        index = np.random.default_rng(seed).integers(0, nvalues, n).astype(np.uint32)
        index[:2] = index[-1:]
    table = NameTable(index, table.key_off, table.key_bytes, table.lab_off, table.lab_bytes, table.metrics)
    for j, m in enumerate(table.metrics):
        m._set_snapshot(HistogramSummary.from_record(values[j if index is None else int(index[j])]))
    lines = []
    write_metrics(tree, lines)
    assert len(lines) == 11 * n
    return table, values, "".join(lines).encode()


def render_guarded(call, want_len, skew):
    """Runs call(out) into a device buffer of exactly want_len bytes at byte offset skew
    of a guarded allocation; returns the bytes after checking the guards."""
    import torch
    buf = torch.full((want_len + 128,), GUARD, dtype=torch.uint8, device="cuda:0")
    out = buf[64 + skew:64 + skew + want_len]
    assert call(out) == want_len
    host = buf.cpu().numpy()
    assert (host[:64 + skew] == GUARD).all() and (host[64 + skew + want_len:] == GUARD).all()
    return host[64 + skew:64 + skew + want_len].tobytes()


@pytest.mark.parametrize("n,index_kind", [(0, "none"), (1, "none"), (63, "perm"), (64, "none"), (65, "perm"),
                                          (257, "perm"), (4097, "none")])
def test_summary_blocks_equal_write_metrics(eng, avgs, n, index_kind):
    table, values, want = summary_case(n, index_kind, avgs)
    got = eng.render_summaries(table, values)  # host inputs, host output
    assert len(got) == len(want)
    assert got == want
    if n == 0:
        return
    # device inputs, a device output of exactly len bytes between guards, at an odd address
    dtab, dvals = table.to_device(), _dev(values.view(np.int64))
    got_dev = render_guarded(lambda out: eng.render_summaries(dtab, dvals, out=out), len(want), skew=n % 16)
    assert got_dev == want


def test_summaries_cover_every_edge_and_avg(eng, avgs):
    """The 4097-row case prints every record: each edge in each field, each avg."""
    v = crafted_summaries(4097 + 5, avgs)
    for name in N.SUMMARY_FIELDS[:-1]:
        assert set(C.INT64_EDGES) <= set(v[name][:4097].tolist())
    assert avgs.size <= 4097 and (v["sum"][:4097] < 0).any()
    assert np.isnan(avgs).any() and np.isinf(avgs).any() and (avgs == 2.82879384806159e17).any()


def test_rollup_blocks_equal_write_rollup_metrics(eng, avgs):
    groups = [("rt:client:request_latency_ms", (("rt", f"r{g}"),)) for g in range(70)]
    groups += [("lat_ms", ()), ("k" * 300, (("service", "/svc/é"), ("rt", "x" * 5000)))]
    plan = RollupPlan(np.zeros(1, np.uint32), groups)
    values = crafted_summaries(len(groups), avgs[::-1].copy())
    lines = []
    write_rollup_metrics(plan, [HistogramSummary.from_record(r) for r in values], lines)
    want = "".join(lines).encode()
    table = rollup_name_table(plan)
    assert table.index is None and table.n == 72
    assert eng.render_summaries(table, values) == want
    assert render_guarded(lambda out: eng.render_summaries(table.to_device(), _dev(values.view(np.int64)), out=out),
                          len(want), skew=5) == want


def le_case(n, K, with_sums, seed=2):
    tree = stat_tree(n)
    table = stat_name_table(tree)
    nvalues = n + 3
    rng = np.random.default_rng(seed)
    index = rng.permutation(nvalues)[:n].astype(np.uint32)
    edges = np.array(C.UINT64_EDGES, np.uint64)  # 0, 2^63 and 2^64 - 1 among them
    le_rows = np.ascontiguousarray(edges[(np.arange(nvalues * (K + 1)) * 5 + 1) % edges.size].reshape(nvalues, K + 1))
    sums = np.array(C.INT64_EDGES, np.int64)[np.arange(nvalues) % len(C.INT64_EDGES)] if with_sums else None
    labels = {1: np.array([250], np.int64), 16: np.array([1, 2, 5, 10, 25, 50, 100, 250, 497, 997, 2499, 4987, 9981,
                                                         29896, 59971, 2147483646], np.int64)}.get(K)
    if labels is None:
        labels = np.arange(K, dtype=np.int64) * 33554431 + 1
    assert labels.size == K
    table = NameTable(index, table.key_off, table.key_bytes, table.lab_off, table.lab_bytes, table.metrics)
    for j, m in enumerate(table.metrics):
        m.series_id = int(index[j])
    stub = types.SimpleNamespace(le_cuts=labels, le_labels=labels, le_buckets=le_rows,
                                 le_sums=np.zeros(nvalues, np.int64) if sums is None else sums)
    lines = []
    write_histogram_metrics(tree, stub, lines)
    assert len(lines) == (K + 3) * n
    return table, le_rows, sums, labels, "".join(lines).encode()


@pytest.mark.parametrize("n,K,with_sums", [(65, 1, True), (257, 16, True), (65, 64, False), (1, 16, False)])
def test_hist_blocks_equal_write_histogram_metrics(eng, n, K, with_sums):
    table, le_rows, sums, labels, want = le_case(n, K, with_sums)
    assert {0, 2 ** 63, 2 ** 64 - 1} <= set(le_rows.ravel().tolist())
    got = eng.render_le(table, le_rows, sums, labels)
    assert len(got) == len(want)
    assert got == want
    dtab, drows = table.to_device(), _dev(le_rows.view(np.int64))
    dsums, dlabels = (None if sums is None else _dev(sums)), _dev(labels)
    got_dev = render_guarded(lambda out: eng.render_le(dtab, drows, dsums, dlabels, out=out), len(want), skew=K % 16)
    assert got_dev == want


# ---- the contract -----------------------------------------------------------------------
def _raw_summaries(eng, table, values, out, cap):
    nm, ln = eng._names(table), ctypes.c_size_t(12345)
    op = None if out is None else out.data_ptr()
    rc = eng._lib.l5dh_render_summaries(eng._ctx, ctypes.byref(nm), table.n, values.ctypes.data, values.size, op, cap,
                                        ctypes.byref(ln))
    return rc, ln.value


def last_error(eng):
    """The whole text l5dh_last_error holds for the engine's context."""
    return eng._lib.l5dh_last_error(eng._ctx).decode()


def cap_message(eng, call, want_len):
    """call(out) into a host buffer one byte short: -ERANGE, and the message names both sizes."""
    with pytest.raises(N.L5dhError) as ei:
        call(np.empty(want_len - 1, np.uint8))
    assert ei.value.code == -errno.ERANGE
    assert last_error(eng) == f"render: the text takes {want_len} bytes, cap is {want_len - 1}"


def test_contract_sizes_and_device_findings(eng, avgs):
    import torch
    n = 70
    table, values, want = summary_case(n, "perm", avgs)
    assert _raw_summaries(eng, table, values, None, 0) == (0, len(want))  # the size query
    buf = torch.full((len(want) + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    assert _raw_summaries(eng, table, values, buf, len(want) - 1) == (-errno.ERANGE, len(want))
    assert last_error(eng) == f"render: the text takes {len(want)} bytes, cap is {len(want) - 1}"
    le_table, le_rows, le_sums, le_labels, le_want = le_case(65, 1, True)
    cap_message(eng, lambda out: eng.render_le(le_table, le_rows, le_sums, le_labels, out=out), len(le_want))
    assert (buf.cpu().numpy() == GUARD).all()  # nothing was written
    empty = NameTable(None, np.zeros(1, np.uint64), np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint8))
    assert _raw_summaries(eng, empty, values, buf, 64) == (0, 0) and (buf.cpu().numpy() == GUARD).all()
    nm, ln = eng._names(table), ctypes.c_size_t(0)
    lib = eng._lib
    assert lib.l5dh_render_summaries(eng._ctx, None, n, values.ctypes.data, values.size, None, 0, ctypes.byref(ln)) == -errno.EINVAL
    assert lib.l5dh_render_summaries(eng._ctx, ctypes.byref(nm), n, values.ctypes.data, 0, None, 0, ctypes.byref(ln)) == -errno.EINVAL
    no_off = N.Names(nm.index, None, nm.key_bytes, nm.lab_off, nm.lab_bytes)
    assert lib.l5dh_render_summaries(eng._ctx, ctypes.byref(no_off), n, values.ctypes.data, values.size, None, 0,
                                     ctypes.byref(ln)) == -errno.EINVAL
    for K in (0, 65):
        assert lib.l5dh_render_le(eng._ctx, ctypes.byref(nm), n, values.ctypes.data, None, values.size, values.ctypes.data,
                                  K, None, 0, ctypes.byref(ln)) == -errno.EINVAL
    # a bad index
    bad = table.index.copy()
    bad[37] = values.size
    with pytest.raises(N.L5dhError, match="row 37") as ei:
        eng.render_summaries(NameTable(bad, table.key_off, table.key_bytes, table.lab_off, table.lab_bytes), values)
    assert ei.value.code == -errno.EINVAL
    assert last_error(eng) == "render: index of row 37 is not < nvalues"
    # an offset that descends
    off = table.lab_off.copy()
    off[51] = off[50] - 1
    with pytest.raises(N.L5dhError, match="row 50") as ei:
        eng.render_summaries(NameTable(table.index, table.key_off, table.key_bytes, off, table.lab_bytes), values)
    assert ei.value.code == -errno.EINVAL
    assert last_error(eng) == "render: key_off or lab_off descends at row 50"
    # an avg outside the domain: -ERANGE, and l5dh_last_error names the row
    far = values.copy()
    far["avg"][int(table.index[12])] = 2.0 ** 70
    first = min(j for j in range(n) if table.index[j] == table.index[12])
    with pytest.raises(N.L5dhError, match=f"row {first} ") as ei:
        eng.render_summaries(table, far)
    assert ei.value.code == -errno.ERANGE
    assert last_error(eng) == f"render: avg or gauge of row {first} is outside +-[2^-64, 2^64), 0, NaN, Infinity"
    assert eng.render_summaries(table, values) == want  # a valid call afterwards succeeds


# ---- end to end ---------------------------------------------------------------------------
def test_render_bytes_is_render_as_a_line_multiset(gpu_available):
    """A C5-shaped tree at 1/100 size: 1 000 Stats x 100 samples, 1 000 counters, 100
    gauges, one rollup plan, the 16 default `le` bounds."""
    rng = np.random.default_rng(5)
    se = StatEngine(capacity=1024, batch=1 << 14)
    se.enable_le(BOUNDS16)
    tree = MetricsTree(se)
    stats = MetricsTreeStatsReceiver(tree)
    made = []
    for i in range(1000):
        sc = stats.scope("rt", f"router{i % 10}", "client", f"$inet$10.0.{i // 250}.{i % 250}$8080")
        made.append(sc.stat("request_latency_ms"))
        sc.counter("requests").incr(i + 1)
    for g in range(100):
        stats.scope("jvm", f"pool{g}").add_gauge("used", f=lambda g=g: float(g) * 1.5)
    vals = np.exp(3.0 + 2.0 * rng.standard_normal((1000, 100))).astype(np.float32)
    for st, row in zip(made, vals):
        for v in row:
            st.add(float(v))
    plan = plan_rollup(tree, ("client",), se.capacity)
    assert plan.ngroups == 10
    _, grouped = se.snapshot_all_rollup(plan.group_of, plan.ngroups, reset=False)  # a look: the interval stays
    group_summaries = [HistogramSummary.from_record(r) for r in grouped]
    assert snapshot_histograms_le(tree, se) == 1000
    tel = PrometheusTelemeter(tree, rollups=(plan, group_summaries), histograms=se)
    text = tel.render()
    got = tel.render_bytes(se.engine)
    assert line_multiset(got.decode("utf-8")) == line_multiset(text)
    assert len(got) == len(text.encode("utf-8")) and text.count("\n") == 1000 + 100 + 11 * 1000 + 11 * 10 + 19 * 1000
    assert sum(s.count for s in group_summaries) == 100_000
    # the same bytes with the table kept on the device and the records (by series id) left there
    names = stat_name_table(tree)
    recs = np.zeros(se.capacity, N.SUMMARY_DTYPE)
    recs[names.index] = summary_records([m.snapshotted_summary for m in names.metrics])
    assert tel.render_bytes(se.engine, names=names.to_device(), summaries=_dev(recs.view(np.int64))) == got
    # a Stat registered since the snapshot: a `_hist` block (it holds a series id), no summary block
    stats.scope("rt", "router0", "client", "late").stat("request_latency_ms")
    late = tel.render_bytes(se.engine)
    assert line_multiset(late.decode("utf-8")) == line_multiset(tel.render()) and len(late) > len(got)
    se.engine.close()
