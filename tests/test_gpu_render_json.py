"""The JSON and the scalar block of the device renderer (l5dh_render_json,
l5dh_render_scalars) against the Python exporters, byte for byte: the expected bytes are
admin_metrics.write_flat_json's compact document and prometheus.write_scalar_metrics'
lines of a tree whose metrics hold the values the table's index points at.
"""
import ctypes
import errno

import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd.admin_metrics import AdminMetricsExportTelemeter, flat_name_table, scalar_values, write_flat_json
from linkerd_amd.prometheus import (NO_INDEX, NameTable, PrometheusTelemeter, scalar_name_table, summary_records,
                                    write_scalar_metrics)
from linkerd_amd.render_json import QUERY, render_json, render_scalars
from linkerd_amd.telemetry import (HistogramSummary, MetricsTree, MetricsTreeStatsReceiver, StatEngine,
                                   snapshot_histograms)

from . import render_cases as C
from .test_fmt_host import WIDE

pytestmark = pytest.mark.gpu

GUARD = 0xA5
SIZES = (1, 63, 64, 65, 257)
GAUGE_EDGES = np.array([float("nan"), float("inf"), -float("inf"), -0.0, 0.0, 1.48832833e12, 1e7, 9999999.0, 0.001,
                        9.999e-4, 2.0 ** 24 - 1, 2.0 ** 24 + 2, 4008938.8, 2.0 ** -64, 2.0 ** 63, 3.4028235e38, 1e-45,
                        1.17549435e-38, -1.5, 0.1, 1 / 3, 123456.79, -2.0 ** 70, 6e-39], np.float32)
WEIRD = 'we"ird\\na\nme\x01/é√日本'


@pytest.fixture(scope="module")
def eng(gpu_available):
    from linkerd_amd.engine import HistogramEngine
    with HistogramEngine(32) as e:
        yield e


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


# ---- crafted names and values ---------------------------------------------------------
def crafted_values(nvalues):
    """(summaries, counters, gauges): test_fmt_host's WIDE, every int64 edge in every
    integer field (so counts of 0 and below: `.count` alone), the avg set of the double
    formatter with non-finite avgs under a positive count, the int64 edges as counters,
    the float edges and seeded random floats as gauges."""
    avgs = np.array([x for x in C.fixed_doubles() if C.in_domain(x)][::3] + list(C.quotients()[:40]), np.float64)
    edges = np.array(C.INT64_EDGES, np.int64)
    i = np.arange(nvalues)
    summ = np.zeros(nvalues, N.SUMMARY_DTYPE)
    for f, name in enumerate(N.SUMMARY_FIELDS[:-1]):
        summ[name] = edges[(i * 5 + 7 * f) % edges.size]
    summ["avg"] = avgs[i % avgs.size]
    summ["count"][::2] = 1 + i[::2]  # every other record prints all eleven entries
    summ["count"][1::4] = 0
    summ["count"][3::8] = -7
    for k, x in enumerate((float("nan"), float("inf"), -float("inf"))):
        summ["avg"][2 + 2 * k::16] = x  # (even records: a positive count)
    summ[::16] = summary_records([WIDE])[0]
    counters = edges[(i * 3 + 1) % edges.size].copy()
    bits = np.random.default_rng(31).integers(0, 1 << 32, nvalues, dtype=np.uint64).astype(np.uint32)
    gauges = np.where(i % 4 != 3, GAUGE_EDGES[(i - i // 4) % GAUGE_EDGES.size], bits.view(np.float32)).astype(np.float32)
    return summ, counters, gauges


def mixed_tree(n):
    """n metrics of mixed kinds under keys of 1 to 40 bytes (every alignment of the
    output cursor), nested scopes, a name that needs every JSON escape, and at row 9 a key
    of 5 000 bytes (a row built straight in the output)."""
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    for j in range(n):
        kind = (j + j // 7) % 3
        if j == 9:
            name = ("L" * 5000,)
        elif j == 11:
            name = (WEIRD, "x")
        elif j < 40:
            name = (("abcdefghij" * 4)[:j + 1],)
        else:
            name = ("rt", f"router{j % 7}", f"m{j}")
        if kind == N.KIND_COUNTER:
            stats.counter(*name)
        elif kind == N.KIND_GAUGE:
            stats.add_gauge(*name, f=lambda: 0.0)
        else:
            stats.stat(*name)
    return tree


def with_index(table, index):
    return NameTable(index, table.key_off, table.key_bytes, table.lab_off, table.lab_bytes, table.metrics, table.kinds)


def point_metrics_at(table, index, summ, counters, gauges):
    """Every metric of the table takes the value its row prints."""
    for j, m in enumerate(table.metrics):
        i = j if index is None else int(index[j])
        if table.kinds[j] == N.KIND_COUNTER:
            m.incr(int(counters[i]) - m.get())
        elif table.kinds[j] == N.KIND_GAUGE:
            m._f = lambda v=float(gauges[i]): v
        else:
            m._set_snapshot(HistogramSummary.from_record(summ[i]))


def make_index(kind, n, nvalues, seed=3):
    rng = np.random.default_rng(seed)
    if kind == "none":
        return None
    if kind == "perm":
        return rng.permutation(nvalues)[:n].astype(np.uint32)
    index = rng.integers(0, nvalues, n).astype(np.uint32)  # repeats
    index[:2] = index[-1:]
    return index


def json_case(n, index_kind):
    tree = mixed_tree(n)
    table = flat_name_table(tree)
    assert table.n == n and table.kinds.dtype == np.uint8
    nvalues = n + 5
    values = crafted_values(nvalues)
    index = make_index(index_kind, n, nvalues)
    table = with_index(table, index)
    point_metrics_at(table, index, *values)
    return table, values, write_flat_json(tree).encode("utf-8")


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


@pytest.mark.parametrize("n,index_kind", [(1, "none"), (63, "perm"), (64, "none"), (65, "repeats"), (257, "perm"),
                                          (257, "none"), (64, "repeats")])
def test_json_equals_write_flat_json(eng, n, index_kind):
    table, (summ, counters, gauges), want = json_case(n, index_kind)
    got = render_json(eng, table, summ, counters, gauges)  # host table and values, host output
    assert len(got) == len(want)
    assert got == want
    assert render_json(eng, table, summ, counters, gauges, out=QUERY) == len(want)
    # device table and values, a device output of exactly len bytes between guards, at an odd address
    dtab, dv = table.to_device(), (_dev(summ.view(np.int64)), _dev(counters), _dev(gauges))
    assert render_guarded(lambda out: render_json(eng, dtab, *dv, out=out), len(want), skew=n % 16) == want


def test_json_case_covers_the_edges():
    table, (summ, counters, gauges), want = json_case(257, "perm")
    text = want.decode("utf-8")
    for kind in (N.KIND_COUNTER, N.KIND_GAUGE, N.KIND_STAT):
        assert (table.kinds == kind).sum() > 80
    assert int(table.key_off[10] - table.key_off[9]) == 5000 or (np.diff(table.key_off.astype(np.int64)) == 5000).any()
    assert '.avg":"NaN"' in text and '.avg":"Infinity"' in text and '.avg":"-Infinity"' in text
    assert '":"NaN"' in text and '.avg":2.82879384806159008E17' in text and '.sum":-9223372036854775808' in text
    assert text.count(".count") > text.count(".max") > 20  # Stats with count <= 0 print `.count` alone
    assert '\\"ird\\\\na\\nme\\u0001/é√日本/x' in text and "1.48832833E12" in text and "3.4028235E38" in text
    printed = summ[table.index[table.kinds == N.KIND_STAT]]
    assert (printed["count"] == 0).any() and (printed["count"] < 0).any()


def test_json_documents(eng):
    empty = NameTable.build([], [], [], [], [])
    assert render_json(eng, empty, None, None, None) == b"{}"
    assert render_json(eng, empty, None, None, None, out=QUERY) == 2
    assert render_guarded(lambda out: render_json(eng, empty, None, None, None, out=out), 2, skew=3) == b"{}"
    one = NameTable.build(["a"], [""], [0], None, [N.KIND_COUNTER])
    assert render_json(eng, one, None, np.array([1], np.int64), None) == b'{"a":1}'
    assert render_json(eng, with_index(one, None), None, np.array([-5], np.int64), None) == b'{"a":-5}'
    gauge = NameTable(None, one.key_off, one.key_bytes, None, None, None, np.array([N.KIND_GAUGE], np.uint8))
    assert render_json(eng, gauge, None, None, np.array([np.nan], np.float32)) == b'{"a":"NaN"}'  # (lab_off: null)
    # a table whose only Stat was never snapshotted: the host drops the row, n = 0
    tree = MetricsTree()
    MetricsTreeStatsReceiver(tree).stat("never")
    tel = AdminMetricsExportTelemeter(tree)
    assert tel.handle_bytes("/admin/metrics.json", eng) == (200, "application/json", b"{}")
    assert tel.handle("/admin/metrics.json")[2] == "{}"


# ---- the contract -----------------------------------------------------------------------
def _raw_json(eng, table, summ, counters, gauges, out, cap, kinds=None):
    nm, ln = eng._names(table), ctypes.c_size_t(12345)
    kinds = table.kinds if kinds is None else kinds
    rc = eng._lib.l5dh_render_json(eng._ctx, ctypes.byref(nm), kinds.ctypes.data, table.n, summ.ctypes.data, summ.size,
                                   counters.ctypes.data, counters.size, gauges.ctypes.data, gauges.size,
                                   None if out is None else out.data_ptr(), cap, ctypes.byref(ln))
    return rc, ln.value


def test_json_contract_sizes(eng):
    import torch
    table, values, want = json_case(65, "perm")
    assert _raw_json(eng, table, *values, None, 0) == (0, len(want))  # the size query
    buf = torch.full((len(want) + 64,), GUARD, dtype=torch.uint8, device="cuda:0")
    assert _raw_json(eng, table, *values, buf, len(want) - 1) == (-errno.ERANGE, len(want))
    assert last_error(eng) == f"render: the text takes {len(want)} bytes, cap is {len(want) - 1}"
    assert (buf.cpu().numpy() == GUARD).all()  # nothing was written
    assert _raw_json(eng, table, *values, buf, len(want)) == (0, len(want))
    assert buf.cpu().numpy()[:len(want)].tobytes() == want and (buf.cpu().numpy()[len(want):] == GUARD).all()
    ln = ctypes.c_size_t(0)
    nm = eng._names(table)
    s, c, g = values
    lib = eng._lib
    assert lib.l5dh_render_json(eng._ctx, None, table.kinds.ctypes.data, 65, s.ctypes.data, s.size, c.ctypes.data, c.size,
                                g.ctypes.data, g.size, None, 0, ctypes.byref(ln)) == -errno.EINVAL
    assert lib.l5dh_render_json(eng._ctx, ctypes.byref(nm), None, 65, s.ctypes.data, s.size, c.ctypes.data, c.size,
                                g.ctypes.data, g.size, None, 0, ctypes.byref(ln)) == -errno.EINVAL
    assert lib.l5dh_render_json(eng._ctx, ctypes.byref(nm), table.kinds.ctypes.data, 65, s.ctypes.data, s.size, None, 3,
                                g.ctypes.data, g.size, None, 0, ctypes.byref(ln)) == -errno.EINVAL
    nolab = N.Names(nm.index, nm.key_off, nm.key_bytes, None, None)
    assert lib.l5dh_render_scalars(eng._ctx, ctypes.byref(nolab), table.kinds.ctypes.data, 65, c.ctypes.data, c.size,
                                   g.ctypes.data, g.size, None, 0, ctypes.byref(ln)) == -errno.EINVAL


def test_json_output_at_every_skew(eng):
    """The rows start at out + 1: the aligned-store head and tail at each of 16 skews, with
    no byte outside [0, len) written."""
    table, (summ, counters, gauges), want = json_case(65, "repeats")
    dtab, dv = table.to_device(), (_dev(summ.view(np.int64)), _dev(counters), _dev(gauges))
    for skew in range(16):
        assert render_guarded(lambda out: render_json(eng, dtab, *dv, out=out), len(want), skew=skew) == want


def last_error(eng):
    """The whole text l5dh_last_error holds for the engine's context."""
    return eng._lib.l5dh_last_error(eng._ctx).decode()


def test_device_findings(eng):
    table, (summ, counters, gauges), want = json_case(70, "perm")
    stat_rows = np.flatnonzero(table.kinds == N.KIND_STAT)
    # a kind that is none
    kinds = table.kinds.copy()
    kinds[[37, 50]] = 7
    bad = NameTable(table.index, table.key_off, table.key_bytes, table.lab_off, table.lab_bytes, None, kinds)
    with pytest.raises(N.L5dhError, match="row 37 ") as ei:
        render_json(eng, bad, summ, counters, gauges)
    assert ei.value.code == -errno.EINVAL
    assert last_error(eng) == "render: the kind of row 37 is not one the call prints"
    # a stat row in render_scalars
    with pytest.raises(N.L5dhError, match=f"row {stat_rows[0]} ") as ei:
        render_scalars(eng, table, counters, gauges)
    assert ei.value.code == -errno.EINVAL
    assert last_error(eng) == f"render: the kind of row {stat_rows[0]} is not one the call prints"
    # an index at its own kind's count: the gauges are fewer than the other arrays
    j = int(np.flatnonzero(table.kinds == N.KIND_GAUGE)[3])
    few = gauges[:int(table.index[j])]
    rows = [r for r in np.flatnonzero(table.kinds == N.KIND_GAUGE) if table.index[r] >= few.size]
    with pytest.raises(N.L5dhError, match=f"row {min(rows)} ") as ei:
        render_json(eng, table, summ, counters, few)
    assert ei.value.code == -errno.EINVAL
    assert last_error(eng) == f"render: index of row {min(rows)} is not < nvalues"
    assert (table.index[table.kinds != N.KIND_GAUGE] >= few.size).any()  # (legal for the other kinds)
    # a kind without values: each of its rows is out of range
    with pytest.raises(N.L5dhError, match=f"row {stat_rows[0]} ") as ei:
        render_json(eng, table, None, counters, gauges)
    assert ei.value.code == -errno.EINVAL
    assert last_error(eng) == f"render: index of row {stat_rows[0]} is not < nvalues"
    # offsets that descend
    off = table.key_off.copy()
    off[51] = off[50] - 1
    with pytest.raises(N.L5dhError, match="row 50") as ei:
        render_json(eng, NameTable(table.index, off, table.key_bytes, None, None, None, table.kinds), summ, counters, gauges)
    assert ei.value.code == -errno.EINVAL
    assert last_error(eng) == "render: key_off or lab_off descends at row 50"
    # an avg outside the double formatter's domain under a positive count: -ERANGE, the row named
    far = summ.copy()
    k = int(table.index[stat_rows[5]])
    far["avg"][k], far["count"][k] = 2.0 ** 70, 3
    first = min(int(r) for r in stat_rows if table.index[r] == k)
    with pytest.raises(N.L5dhError, match=f"row {first} ") as ei:
        render_json(eng, table, far, counters, gauges)
    assert ei.value.code == -errno.ERANGE
    assert last_error(eng) == f"render: avg or gauge of row {first} is outside +-[2^-64, 2^64), 0, NaN, Infinity"
    # the cap too small message of the scalar call
    one = NameTable.build(["a"], [""], [0], None, [N.KIND_COUNTER])
    with pytest.raises(N.L5dhError) as ei:
        render_scalars(eng, one, np.array([-5], np.int64), None, out=np.empty(4, np.uint8))  # `a -5\n`
    assert ei.value.code == -errno.ERANGE
    assert last_error(eng) == "render: the text takes 5 bytes, cap is 4"
    far["count"][k] = 0  # not printed: not formatted
    assert len(render_json(eng, table, far, counters, gauges)) > 0
    # (l5dh_format_float covers every float -- FLT_MAX, the least subnormal and 2^70 are
    # among the gauges above -- so no gauge is outside the domain)
    assert render_json(eng, table, summ, counters, gauges) == want  # a valid call afterwards succeeds


# ---- scalars --------------------------------------------------------------------------------
def scalar_tree(n):
    """n counters and gauges, with and without label text (every _rewrite case of the
    Prometheus walk among them), a 5 000-byte label and a weird label value."""
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    scopes = [(), ("rt", "incoming"), ("rt", "incoming", "client", "/#/bar"), ("rt", "incoming", "server", "127.0.0.1/4141"),
              ("jvm-mem.current", "used$x"), ("rt", 'we\\ird"na\nme/é√'), ("rt", "in", "service", "/svc/foo")]
    for j in range(n):
        sc = stats.scope(*scopes[j % len(scopes)]) if j != 9 else stats.scope("rt", "r", "client", "c" * 5000)
        if (j + j // 5) % 2:
            sc.counter(f"c{j}")
        else:
            sc.add_gauge(f"g{j}", f=lambda: 0.0)
    return tree


@pytest.mark.parametrize("n", SIZES)
def test_scalars_equal_write_scalar_metrics(eng, n):
    tree = scalar_tree(n)
    table = scalar_name_table(tree)
    assert table.n == n
    nvalues = n + 5
    _, counters, gauges = crafted_values(nvalues)
    index = make_index("repeats" if n % 2 else "perm", n, nvalues, seed=n)
    table = with_index(table, index)
    point_metrics_at(table, index, None, counters, gauges)
    lines = []
    write_scalar_metrics(tree, lines)
    want = "".join(lines).encode("utf-8")
    assert len(lines) == n
    got = render_scalars(eng, table, counters, gauges)
    assert len(got) == len(want)
    assert got == want
    if n == 257:
        text = want.decode("utf-8")
        assert " NaN\n" in text and " Infinity\n" in text and " -0.0\n" in text and '"' + "c" * 5000 + '"' in text
        assert "\nc0 " in "\n" + text or "\ng0 " in "\n" + text  # a row without label text
    dtab = table.to_device()
    assert render_guarded(lambda out: render_scalars(eng, dtab, _dev(counters), _dev(gauges), out=out), len(want),
                          skew=(n + 7) % 16) == want


def test_scalars_of_no_rows(eng):
    empty = NameTable.build([], [], [], [], [])
    assert render_scalars(eng, empty, None, None) == b"" and render_scalars(eng, empty, None, None, out=QUERY) == 0


# ---- end to end -------------------------------------------------------------------------------
def test_handle_bytes_and_scalars_on_device_end_to_end(gpu_available):
    """A small StatEngine tree, one snapshot: the device answers equal the host's."""
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
    stats.scope("jvm", WEIRD).add_gauge("heap", f=lambda: 1.48832833e12)
    idle = stats.scope("rt", "incoming").stat("idle")  # no samples: count == 0
    for st in made:
        for v in np.exp(3.0 + 2.0 * rng.standard_normal(50)).astype(np.float32):
            st.add(float(v))
    assert snapshot_histograms(tree, se) == 13
    late = stats.scope("rt", "incoming").stat("late")  # registered since: no snapshotted summary
    assert idle.snapshotted_summary.count == 0 and late.snapshotted_summary is None
    tel = AdminMetricsExportTelemeter(tree, engine=se)
    eng = se.engine
    for uri in ("/admin/metrics.json", "/admin/metrics.json?q=rt/incoming", "/admin/metrics.json?pretty=1",
                "/admin/metrics.json?tree=1", "/admin/metrics.json?q=rt/nowhere", "/admin/metrics.json?q=rt/incoming&pretty=0"):
        status, media, body = tel.handle(uri)
        assert tel.handle_bytes(uri, eng) == (status, media, body.encode("utf-8")), uri
    flat = tel.handle("/admin/metrics.json")[2]
    assert '"rt/incoming/idle.count":0' in flat and "/late" not in flat and '.avg":' in flat and '":"NaN"' in flat
    assert tel.handle("/admin/metrics.json?q=rt/nowhere")[0] == 404
    # the table kept by the caller, the records (by series id) left on the device: `late` has
    # a series id, so it prints its (empty) record
    names = flat_name_table(tree)
    recs = np.zeros(se.capacity, N.SUMMARY_DTYPE)
    for m in names.metrics:
        if isinstance(m, type(idle)) and m.snapshotted_summary is not None:
            recs[m.series_id] = summary_records([m.snapshotted_summary])[0]
    body = tel.handle_bytes("/admin/metrics.json", eng, names=names, summaries=_dev(recs.view(np.int64)))[2]
    late._set_snapshot(HistogramSummary.from_record(recs[late.series_id]))
    assert body == tel.handle("/admin/metrics.json")[2].encode("utf-8") and b'"rt/incoming/late.count":0' in body
    # an avg outside the device formatter's domain: that request is the host writer's
    made[0]._set_snapshot(HistogramSummary(2, 1, 2, 3, 1, 2, 2, 2, 2, 2, 2.0 ** 70))
    assert tel.handle_bytes("/admin/metrics.json", eng)[2] == tel.handle("/admin/metrics.json")[2].encode("utf-8")
    made[0]._set_snapshot(HistogramSummary(2, 1, 2, 3, 1, 2, 2, 2, 2, 2, 1.5))
    ptel = PrometheusTelemeter(tree)
    assert ptel.render_bytes(eng, scalars_on_device=True) == ptel.render_bytes(eng)
    counters, gauges = scalar_values(scalar_name_table(tree))
    assert counters.size == 12 and gauges.size == 13
    se.engine.close()
