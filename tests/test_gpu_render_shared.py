"""What the device renderers share: rows around the write pass's LDS stage in every block of
l5dh_render.hip, one context taking every renderer in turn, and a render call beside the
sparse export and the window push (the three users of the count / scan / total step).

The expected bytes are the Python exporters' throughout; the export and the window are
checked as tests/test_gpu_import.py and tests/test_gpu_window.py check them.
"""
import errno
import types

import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd.admin_metrics import AdminMetricsExportTelemeter, flat_name_table, scalar_values, write_flat_json
from linkerd_amd.influxdb import InfluxDbTelemeter
from linkerd_amd.javafmt import double_to_string
from linkerd_amd.prometheus import (PrometheusTelemeter, line_multiset, scalar_name_table, stat_name_table, summary_records,
                                    write_metrics, write_quantile_metrics, write_scalar_metrics)
from linkerd_amd.render_influx import influx_table, render_influx
from linkerd_amd.render_json import render_json, render_scalars
from linkerd_amd.telemetry import HistogramSummary, MetricsTree, MetricsTreeStatsReceiver

from . import render_cases as C
from .influx_cases import rewrite_tree
from .test_gpu_import import _csr
from .test_gpu_render import le_case, summary_case
from .test_gpu_render_influx import contract_case as influx_case
from .test_gpu_render_json import (_dev, crafted_values, json_case, make_index, point_metrics_at, render_guarded,
                                   scalar_tree, with_index)
from .test_gpu_window import Truth, _batch, _check, _window

pytestmark = pytest.mark.gpu

STAGE = 4096  # bytes of a row built in LDS (l5dh_render.hip)
AROUND = [STAGE - 1, STAGE, STAGE + 1]
SKEWS = (0, 1, 15)
RECORD = HistogramSummary(2, 1, 2, 3, 1, 2, 2, 2, 2, 2, 1.5)


@pytest.fixture(scope="module")
def eng(gpu_available):
    from linkerd_amd.engine import HistogramEngine
    with HistogramEngine(32) as e:
        yield e


@pytest.fixture(scope="module")
def avgs():
    return np.array([x for x in C.fixed_doubles() if C.in_domain(x)], np.float64)


def last_error(eng):
    """The whole text l5dh_last_error holds for the engine's context."""
    return eng._lib.l5dh_last_error(eng._ctx).decode()


def scalar_case(n):
    """(table, (counters, gauges), expected bytes): write_scalar_metrics' lines of
    test_gpu_render_json's scalar_tree(n), its metrics holding the values the index points at."""
    tree = scalar_tree(n)
    nvalues = n + 5
    _, counters, gauges = crafted_values(nvalues)
    index = make_index("repeats", n, nvalues, seed=n)
    table = with_index(scalar_name_table(tree), index)
    point_metrics_at(table, index, None, counters, gauges)
    lines = []
    write_scalar_metrics(tree, lines)
    assert len(lines) == n
    return table, (counters, gauges), "".join(lines).encode("utf-8")


# ---- rows around the stage size -------------------------------------------------------------
def keys_of(lengths):
    """Distinct keys of the given byte lengths (letters: no escape changes them)."""
    return ["abcdefghij"[i] * n for i, n in enumerate(lengths)]


def at_every_skew(call, want):
    for skew in SKEWS:
        assert render_guarded(call, len(want), skew) == want, skew


def test_scalar_rows_around_the_stage(eng):
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    for key in keys_of([n - 3 for n in AROUND]):  # `key 7\n`
        stats.counter(key).incr(7)
    lines = []
    write_scalar_metrics(tree, lines)
    assert sorted(len(l) for l in lines) == AROUND
    want = "".join(lines).encode()
    table = scalar_name_table(tree)
    counters, gauges = scalar_values(table)
    assert render_scalars(eng, table, counters, None) == want
    dtab, dc = table.to_device(), _dev(counters)
    at_every_skew(lambda out: render_scalars(eng, dtab, dc, None, out=out), want)


def test_json_rows_around_the_stage(eng):
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    for key in keys_of([n - 5 for n in AROUND]):  # `"key":7,`
        stats.counter(key).incr(7)
    want = write_flat_json(tree).encode()
    assert sorted(len(e) + 1 for e in want[1:-1].split(b",")) == AROUND
    table = flat_name_table(tree)
    counters, _ = scalar_values(table)
    assert render_json(eng, table, None, counters, None) == want
    dtab, dc = table.to_device(), _dev(counters)
    at_every_skew(lambda out: render_json(eng, dtab, None, dc, None, out=out), want)


def test_quantile_rows_around_the_stage(eng):
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    fixed = len('{quantile="0.5"} 7\n')
    for i, key in enumerate(keys_of([n - fixed for n in AROUND])):
        m = stats.stat(key)
        m.series_id = i
        m._set_snapshot(RECORD)
    q = np.array([0.5])
    q_rows = np.full((3, 1), 7, np.int64)
    stub = types.SimpleNamespace(quantile_q=q, quantile_labels=[double_to_string(0.5)], quantile_values=q_rows)
    lines = []
    write_quantile_metrics(tree, stub, lines)
    assert sorted(len(l) for l in lines) == AROUND
    want = "".join(lines).encode()
    table = stat_name_table(tree)
    assert eng.render_quantiles(table, q_rows, q) == want
    dtab, drows, dq = table.to_device(), _dev(q_rows), _dev(q)
    at_every_skew(lambda out: eng.render_quantiles(dtab, drows, dq, out=out), want)


def summary_tree(key_lengths):
    tree = MetricsTree()
    stats = MetricsTreeStatsReceiver(tree)
    for i, key in enumerate(keys_of(key_lengths)):
        m = stats.stat(key)
        m.series_id = i
        m._set_snapshot(RECORD)
    lines = []
    write_metrics(tree, lines)
    assert len(lines) == 11 * len(key_lengths)
    return tree, lines


def test_summary_rows_around_the_stage(eng):
    """Eleven lines repeat the key, so a block's length moves in steps of 11: four
    consecutive key lengths put a block into [4086, 4096] and the next into [4097, 4107]."""
    fixed = sum(len(l) for l in summary_tree([1])[1]) - 11  # a block's bytes beside its keys
    k = (STAGE - fixed) // 11  # the longest key whose block still fits the stage
    tree, lines = summary_tree([k - 1, k, k + 1, k + 2])
    blocks = sorted(sum(len(l) for l in lines[i:i + 11]) for i in range(0, len(lines), 11))
    assert blocks == [fixed + 11 * n for n in (k - 1, k, k + 1, k + 2)]
    assert STAGE - 10 <= blocks[1] <= STAGE and STAGE + 1 <= blocks[2] <= STAGE + 11
    want = "".join(lines).encode()
    table = stat_name_table(tree)
    values = np.zeros(4, N.SUMMARY_DTYPE)
    for j, m in enumerate(table.metrics):
        values[int(table.index[j])] = summary_records([m.snapshotted_summary])[0]
    assert eng.render_summaries(table, values) == want
    dtab, dv = table.to_device(), _dev(values.view(np.int64))
    at_every_skew(lambda out: eng.render_summaries(dtab, dv, out=out), want)


# ---- one context, every renderer in turn ----------------------------------------------------
def test_one_context_all_renderers_in_turn(eng, avgs):
    itab, ivalues, iwant = influx_case()
    jtab, jvalues, jwant = json_case(65, "perm")
    stab, svalues, swant = summary_case(65, "perm", avgs)
    ctab, (ccounters, cgauges), cwant = scalar_case(65)
    ltab, le_rows, sums, labels, lwant = le_case(65, 1, True)
    assert itab.n == jtab.n == stab.n == ctab.n == ltab.n == 65
    assert render_influx(eng, itab, "none", *ivalues) == iwant
    assert render_json(eng, jtab, *jvalues) == jwant
    assert eng.render_summaries(stab, svalues) == swant
    assert render_scalars(eng, ctab, ccounters, cgauges) == cwant
    assert eng.render_le(ltab, le_rows, sums, labels) == lwant
    assert render_influx(eng, itab, "none", *ivalues) == iwant
    # a finding in one format, then a good call of another
    kinds = jtab.kinds.copy()
    kinds[[37, 50]] = 7
    bad = type(jtab)(jtab.index, jtab.key_off, jtab.key_bytes, jtab.lab_off, jtab.lab_bytes, None, kinds)
    with pytest.raises(N.L5dhError, match="row 37 ") as ei:
        render_json(eng, bad, *jvalues)
    assert ei.value.code == -errno.EINVAL
    assert last_error(eng) == "render: the kind of row 37 is not one the call prints"
    assert render_influx(eng, itab, "none", *ivalues) == iwant
    bad_kinds = itab.kinds.copy()
    bad_kinds[12] = 9
    ibad = type(itab)(*itab._arrays())
    ibad.kinds = bad_kinds
    with pytest.raises(N.L5dhError, match="row 12 ") as ei:
        render_influx(eng, ibad, "none", *ivalues)
    assert ei.value.code == -errno.EINVAL
    assert last_error(eng) == "render_influx: the kind of row 12 is none of the three"
    assert eng.render_summaries(stab, svalues) == swant
    assert render_json(eng, jtab, *jvalues) == jwant


# ---- every scrape entry point against its host writer, on one small tree ------------------------
def test_scrape_entry_points_print_the_host_writers_text(eng):
    """The rewrite cases beside three Stats -- one whole, one without a snapshot, one without
    a series id: the smallest tree at which a wrong ``index`` or a wrongly kept row shows.
    Every entry point, table built here and kept, records the Stats' own and given by id."""
    tree = rewrite_tree()
    stats = MetricsTreeStatsReceiver(tree)
    stats.scope("jvm").add_gauge("heap", f=lambda: 1.5)
    whole = stats.scope("rt", "incoming", "client", "/#/bar").stat("latency_ms")
    never = stats.scope("foo").stat("never")
    pruned = stats.stat("pruned")
    whole.series_id, never.series_id = 3, 1
    whole._set_snapshot(RECORD)
    pruned._set_snapshot(HistogramSummary(5, 1, 9, 20, 2, 3, 4, 5, 6, 7, 4.0))
    prom, admin, influx = PrometheusTelemeter(tree), AdminMetricsExportTelemeter(tree), InfluxDbTelemeter(tree)
    uri = "/admin/metrics.json"

    def check(summaries, stat_rows):
        names = stat_name_table(tree)
        for kept in (None, names, names.to_device()):
            for on_device in (False, True):
                got = prom.render_bytes(eng, kept, summaries, scalars_on_device=on_device).decode("utf-8")
                assert line_multiset(got) == line_multiset(prom.render()) and got.count("_count") == stat_rows
        for kept in (None, flat_name_table(tree)):
            status, media, body = admin.handle(uri)
            assert admin.handle_bytes(uri, eng, kept, summaries) == (status, media, body.encode("utf-8"))
            assert body.count(".count") == stat_rows
        for kept in (None, influx_table(tree)):
            assert influx.render_bytes(eng, "h:80", kept, summaries) == influx.render("h:80").encode("utf-8")
        assert influx.render("h:80").count("_count=") == stat_rows

    check(None, 2)  # the Stats' own snapshots: `never` prints nothing, `pruned` prints without an id
    # the snapshot's records by series id: every Stat with an id prints its record, so the host
    # writers are given the same state -- `never` its record, `pruned` (no id: no record) none
    recs = np.zeros(8, N.SUMMARY_DTYPE)
    recs[[3, 1]] = summary_records([RECORD, HistogramSummary(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0)])
    never._set_snapshot(HistogramSummary.from_record(recs[1]))
    pruned._set_snapshot(None)
    for kept in (None, flat_name_table(tree)):
        status, media, body = admin.handle(uri)
        assert admin.handle_bytes(uri, eng, kept, recs) == (status, media, body.encode("utf-8"))
    for kept in (None, influx_table(tree)):
        assert influx.render_bytes(eng, "h:80", kept, _dev(recs.view(np.int64))) == influx.render("h:80").encode("utf-8")
    # (the Prometheus table takes no row without an id when the records go by id: the Stat is gone)
    stats.prune("pruned")
    check(recs, 2)


# ---- the sparse export and the window push beside a render call --------------------------------
def test_export_and_window_push_beside_a_render_call(oracle, gpu_available):
    from linkerd_amd.engine import HistogramEngine
    S = 32
    jtab, jvalues, jwant = json_case(65, "perm")
    with HistogramEngine(S) as e:
        win, truth = _window(e, 2), Truth(oracle, S)
        series, vals = _batch(21, S, 4000)
        e.ingest(series, vals)
        ref = truth.interval(series, vals)
        assert render_json(e, jtab, *jvalues) == jwant
        # the sparse export: the CSR of the dense rows
        dense_c, dense_t = e.export_state()
        assert dense_c.tobytes() == ref.counts().tobytes() and dense_t.tobytes() == ref.totals().tobytes()
        want_ro, want_en, _ = _csr(dense_c)
        row_off, entries, totals = e.export_sparse()
        assert e.export_sparse_size() == want_en.size == int(want_ro[-1]) > 0
        assert row_off.tobytes() == want_ro.tobytes() and entries.tobytes() == want_en.tobytes()
        assert totals.tobytes() == dense_t.tobytes()
        # the window push: the interval's summaries, and the window reads as the oracle's rows
        got = win.push(with_series=True)
        assert got.tobytes() == ref.snapshot(reset=False).tobytes()
        assert win.info()["filled"] == 1 and win.info()["pushes"] == 1
        _check(win, truth, 1, "after the push")
        assert win.summaries(1).tobytes() == truth.one_oracle(1).tobytes()
        assert render_json(e, jtab, *jvalues) == jwant
