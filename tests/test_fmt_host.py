"""The host side of the device renderer, on CPU: the library's number texts
(l5dh_format_double / _long / _ulong, the functions the kernels compile too) against
linkerd_amd.javafmt, and the name tables of prometheus.py, pinned by composing
write_metrics' lines from a table in pure Python.
"""
import ctypes
import errno
import os
import shutil
import subprocess

import pytest

from linkerd_amd import _native as N
from linkerd_amd.javafmt import double_to_string
from linkerd_amd.prometheus import (NO_INDEX, QUANTILES, PrometheusTelemeter, rollup_name_table, stat_name_table,
                                    write_histogram_metrics, write_metrics)
from linkerd_amd.rollup import plan_rollup, write_rollup_metrics
from linkerd_amd.telemetry import HistogramSummary, MetricsTree, MetricsTreeStatsReceiver, snapshot_histograms_le

from . import render_cases as C
from .test_le_exporters_host import _tree as le_tree

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ONE_TWO = HistogramSummary(2, 1, 2, 3, 1, 2, 2, 2, 2, 2, 1.5)
WIDE = HistogramSummary(3, -7, 2 ** 63 - 1, -2 ** 63, 0, 10, 99, 100, 10 ** 18, -10 ** 18, 2.82879384806159e17)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(N.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libl5dhist.so not built and no hipcc to build it")
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "linkerd_amd", "csrc")], check=True)
    return N.load()


def fmt_double(lib, x):
    """(status, text) of l5dh_format_double; the buffer is exactly L5DH_DOUBLE_CHARS."""
    buf, n = ctypes.create_string_buffer(N.DOUBLE_CHARS), ctypes.c_size_t(99)
    rc = lib.l5dh_format_double(float(x), buf, ctypes.byref(n))
    return rc, buf.raw[:n.value].decode()


def check_doubles(lib, xs):
    refused = 0
    for x in xs:
        rc, text = fmt_double(lib, x)
        if C.in_domain(x):
            assert rc == 0, f"{x!r} is inside the domain and was refused ({rc})"
            assert text == double_to_string(x), repr(x)
        else:  # only what the test built outside [2^-64, 2^64) may be refused -- and must be
            assert rc == -errno.ERANGE and text == "", repr(x)
            refused += 1
    return refused


def test_format_double_fixed_cases(lib):
    xs = C.fixed_doubles()
    assert len(xs) > 142 + 128 + 39
    refused = check_doubles(lib, xs)
    outside = [x for x in xs if not C.in_domain(x)]
    assert refused == len(outside) and {2.0 ** 64, 1e23, 5e-324, 2.0 ** 70} <= set(outside)
    assert fmt_double(lib, 2.82879384806159e17) == (0, "2.82879384806159008E17")  # the exact-long path
    assert fmt_double(lib, -2.82879384806159e17) == (0, "-2.82879384806159008E17")
    assert fmt_double(lib, 2.0 ** -64) == (0, "5.421010862427522E-20")
    assert fmt_double(lib, 2.0 ** 63) == (0, "9.223372036854776E18")


def test_format_double_random_quotients(lib):
    """50 000 sum / count quotients: none may be refused, each equals javafmt."""
    xs = C.quotients()
    assert len(xs) == 50_000 and all(C.in_domain(x) for x in xs)
    assert check_doubles(lib, xs) == 0


def test_format_double_rejects_null_arguments(lib):
    n = ctypes.c_size_t(0)
    assert lib.l5dh_format_double(1.0, None, ctypes.byref(n)) == -errno.EINVAL
    assert lib.l5dh_format_double(1.0, ctypes.create_string_buffer(N.DOUBLE_CHARS), None) == -errno.EINVAL


def test_format_long_and_ulong_edges(lib):
    buf, n = ctypes.create_string_buffer(N.LONG_CHARS), ctypes.c_size_t(0)
    assert {0, 9, -9, 10, -10, 10 ** 18, -10 ** 18, 10 ** 18 - 1, 2 ** 63 - 1, -2 ** 63} <= set(C.INT64_EDGES)
    for v in C.INT64_EDGES:
        assert lib.l5dh_format_long(v, buf, ctypes.byref(n)) == 0
        assert buf.raw[:n.value].decode() == str(v)
    assert {0, 10 ** 19, 10 ** 19 - 1, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1} <= set(C.UINT64_EDGES)
    for v in C.UINT64_EDGES:
        assert lib.l5dh_format_ulong(v, buf, ctypes.byref(n)) == 0
        assert buf.raw[:n.value].decode() == str(v)


# ---- name tables ---------------------------------------------------------------------
def row_texts(table, j):
    key = bytes(table.key_bytes[int(table.key_off[j]):int(table.key_off[j + 1])]).decode("utf-8")
    inner = bytes(table.lab_bytes[int(table.lab_off[j]):int(table.lab_off[j + 1])]).decode("utf-8")
    return key, inner


def labels(inner, extra=None):
    """What the device composes from the inner text and an extra label."""
    if extra is None:
        return "{" + inner + "}" if inner else ""
    return "{" + (inner + ", " if inner else "") + extra + "}"


def summary_block(table, j, s):
    key, inner = row_texts(table, j)
    lab = labels(inner)
    out = [f"{key}_count{lab} {s.count}\n", f"{key}_sum{lab} {s.sum}\n", f"{key}_avg{lab} {double_to_string(s.avg)}\n"]
    return out + [key + labels(inner, 'quantile="' + q + '"') + f" {getattr(s, f)}\n" for q, f in QUANTILES]


def hist_block(table, j, le_labels, row, total):
    key, inner = row_texts(table, j)
    out = [key + "_hist_bucket" + labels(inner, 'le="' + str(int(le)) + '"') + f" {int(n)}\n"
           for le, n in zip(le_labels, row[:-1])]
    out.append(key + "_hist_bucket" + labels(inner, 'le="+Inf"') + f" {int(row[-1])}\n")
    return out + [f"{key}_hist_sum{labels(inner)} {int(total)}\n", f"{key}_hist_count{labels(inner)} {int(row[-1])}\n"]


def exporters_tree():
    """An engine-less tree as tests/test_exporters_host.py builds them (summaries set the
    way the snapshot driver sets them), covering every _rewrite case, a label value with
    a backslash, a quote, a newline and a non-ASCII character, and keys needing escape."""
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    scopes = [("rt", "incoming", "service", "/svc/foo"), ("rt", "incoming", "client", "/#/bar"),
              ("rt", "incoming", "client", "/#/bar", "service", "/svc/foo"), ("rt", "incoming", "server", "127.0.0.1/4141"),
              ("rt", "incoming"), ("rt", 'we\\ird"na\nme/é√'), ("foo", "bar"), ("jvm-mem.current", "used$x"), ()]
    made = []
    for i, scope in enumerate(scopes):
        st = stats.scope(*scope).stat("request latency-ms" if i % 2 else "request_latency_ms")
        st._set_snapshot(WIDE if i % 3 == 0 else ONE_TWO)
        made.append(st)
    stats.scope("rt", "incoming").counter("requests").incr(3)  # not a Stat: no row
    stats.scope("foo").stat("never_snapshotted")
    return tree, made


def test_stat_name_table_reproduces_write_metrics():
    tree, made = exporters_tree()
    table = stat_name_table(tree)
    assert table.n == len(made) + 1 and len(table.metrics) == table.n
    assert table.index.tolist() == [NO_INDEX] * table.n  # no engine: no series ids
    assert table.key_off[0] == 0 and table.lab_off[0] == 0
    assert table.key_off[-1] == table.key_bytes.size and table.lab_off[-1] == table.lab_bytes.size
    lines = []
    for j, m in enumerate(table.metrics):
        if m.snapshotted_summary is not None:
            lines += summary_block(table, j, m.snapshotted_summary)
    want = []
    write_metrics(tree, want)
    want = [l for l in want if not l.startswith("rt:requests")]  # the counter's line
    assert lines == want and len(lines) == 11 * len(made)  # exact, in the walk's order
    text = "".join(lines)
    assert 'rt="we\\\\ird\\\\na\\\\me/é√"' in text and "jvm_mem_current:used_x:request_latency_ms_count " in text
    assert 'rt:client:service:request_latency_ms{rt="incoming", client="/#/bar", service="/svc/foo", quantile="0.5"}' in text
    assert "request_latency_ms_sum -9223372036854775808\n" in text  # the root Stat: no labels, no braces
    # a subset in another order keeps each row's bytes
    part = table.take([3, 0])
    assert row_texts(part, 0) == row_texts(table, 3) and row_texts(part, 1) == row_texts(table, 0)
    assert part.metrics == [table.metrics[3], table.metrics[0]]


def test_stat_and_rollup_name_tables_of_an_engine_tree(oracle):
    """The tree of tests/test_le_exporters_host.py: series ids as index, the histogram
    block and the rollup block composed from their tables."""
    eng, tree, stats = le_tree(oracle)
    a = stats.scope("rt", "http", "client", 'a"b').stat("request_latency_ms")
    b = stats.scope("rt", "http", "client", "b").stat("request_latency_ms")
    plain = stats.stat("lat-ms")
    for v in (0.5, 1.0, 3.0, 250.0, 251.0, 497.0, 498.0, 3e9):
        a.add(v)
    b.add(100.0)
    assert snapshot_histograms_le(tree, eng) == 3
    table = stat_name_table(tree)
    assert sorted(table.index.tolist()) == sorted(m.series_id for m in (a, b, plain))
    assert [m.series_id for m in table.metrics] == table.index.tolist()
    lines, hist = [], []
    for j, m in enumerate(table.metrics):
        lines += summary_block(table, j, m.snapshotted_summary)
        hist += hist_block(table, j, eng.le_labels, eng.le_buckets[m.series_id], eng.le_sums[m.series_id])
    want, want_hist = [], []
    write_metrics(tree, want)
    write_histogram_metrics(tree, eng, want_hist)
    assert lines == want and hist == want_hist and len(hist) == 3 * (len(eng.le_labels) + 3)
    plan = plan_rollup(tree, ("client",), eng.capacity)
    groups = rollup_name_table(plan)
    assert groups.n == plan.ngroups == 1 and groups.index is None
    got, want = summary_block(groups, 0, ONE_TWO), []
    write_rollup_metrics(plan, [ONE_TWO], want)
    assert got == want and got[0] == 'rt:client:request_latency_ms_count{rt="http"} 2\n'
    assert PrometheusTelemeter(tree).render() == "".join(lines)  # render() itself is untouched
