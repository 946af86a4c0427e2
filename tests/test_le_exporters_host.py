"""Cumulative `le` buckets above the engine, on the host: StatEngine.enable_le /
snapshot_all_le / release, telemetry.snapshot_histograms_le, the Prometheus histogram
lines and the telemeter's optional histograms, over an oracle-backed stand-in engine.
The truth of the buckets everywhere: np.cumsum of the oracle's bucket counts (uint64)
at columns cuts - 1, with the row sum for +Inf.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd.engine import HistogramEngine
from linkerd_amd.prometheus import PrometheusTelemeter, write_histogram_metrics, write_metrics
from linkerd_amd.telemetry import (MetricsTree, MetricsTreeStatsReceiver, StatEngine, snapshot_histograms,
                                   snapshot_histograms_le)

from .test_host_engine import OracleEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def le_truth(counts, cuts):
    """uint64 [rows][K+1]: the counts at the cuts, then the row count."""
    cum = np.cumsum(np.asarray(counts).astype(np.uint64), axis=1)
    return np.concatenate([cum[:, np.asarray(cuts, np.int64) - 1], cum[:, -1:]], axis=1)


class LeOracleEngine(OracleEngine):
    """OracleEngine plus HistogramEngine.le_cuts / le_counts (full signature), counting
    engine calls."""

    le_cuts = staticmethod(HistogramEngine.le_cuts)  # (host code of the library: no GPU)

    def __init__(self, S, oracle):
        super().__init__(S, oracle)
        self.calls = []

    def snapshot(self, *a, **kw):
        self.calls.append("snapshot")
        return super().snapshot(*a, **kw)

    def le_counts(self, cuts, first=0, count=None, reset=False, with_series=False, accumulate_into=None):
        self.calls.append("le_counts")
        with self.lock:
            count = self.max_series - first if count is None else count
            sl = slice(first, first + count)
            counts, totals = self.h.h["counts"][sl].copy(), self.h.h["total"][sl].copy()
            le, sums = le_truth(counts, cuts), totals.astype(np.int64)
            series = self.O.summarize_counts(counts, totals)
            if reset:
                self.h.h[sl] = 0
        if accumulate_into is not None:
            acc_le, acc_sums = accumulate_into
            acc_le += le
            acc_sums += sums
            le, sums = acc_le, acc_sums
        return (le, sums, series) if with_series else (le, sums)


@pytest.fixture(scope="module", autouse=True)
def lib():
    if not os.path.exists(N.LIB_PATH):
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libl5dhist.so not built and no hipcc to build it")
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "linkerd_amd", "csrc")], check=True)
    return N.load()


BOUNDS = (1, 250, 500)  # cuts 2, 193, 262; labels 1, 250, 497


def _tree(oracle, S=8, bounds=BOUNDS):
    eng = StatEngine(engine=LeOracleEngine(S, oracle), batch=4)
    eng.enable_le(bounds)
    tree = MetricsTree(eng)
    return eng, tree, MetricsTreeStatsReceiver(tree)


def test_enable_le_dedupes_snapped_bounds(oracle):
    eng, _, _ = _tree(oracle, bounds=(1000, 997, 250, 250.9, 1, float("inf")))
    assert eng.le_cuts.tolist() == [2, 193, 332, 1797]
    assert eng.le_labels.tolist() == [1, 250, 997, int(oracle.limits()[1796]) - 1]
    assert eng.le_buckets.shape == (8, 5) and eng.le_buckets.dtype == np.uint64
    assert eng.le_sums.shape == (8,) and eng.le_sums.dtype == np.int64
    with pytest.raises(RuntimeError, match="enable_le"):
        StatEngine(engine=LeOracleEngine(4, oracle)).snapshot_all_le()


def test_two_resetting_intervals_accumulate_and_never_decrease(oracle):
    eng, tree, stats = _tree(oracle)
    a = stats.scope("rt", "http", "client", "a").stat("request_latency_ms")
    b = stats.scope("rt", "http", "client", "b").stat("request_latency_ms")
    rng = np.random.default_rng(3)
    ref = oracle.OracleHistograms(8)  # never reset: the lifetime truth
    total_count, prev = 0, eng.le_buckets.copy()
    for interval in range(3):
        for st in (a, b):
            vals = np.exp(4.0 + 2.0 * rng.standard_normal(50)).astype(np.float32)
            for v in vals:
                st.add(float(v))
            assert ref.ingest(np.full(50, st.series_id, np.uint32), vals) == 0
        eng.engine.calls.clear()
        assert snapshot_histograms_le(tree, eng) == 2
        assert eng.engine.calls == ["le_counts"]  # ONE snapshotting engine call
        total_count += a.snapshotted_summary.count + b.snapshotted_summary.count
        assert a.snapshotted_summary.count == b.snapshotted_summary.count == 50  # per interval: it was reset
        assert (eng.le_buckets >= prev).all()
        prev = eng.le_buckets.copy()
        np.testing.assert_array_equal(eng.le_buckets, le_truth(ref.counts(), eng.le_cuts))
        np.testing.assert_array_equal(eng.le_sums, ref.totals())
        assert (np.diff(eng.le_buckets.astype(np.int64), axis=1) >= 0).all()  # cumulative along le
    assert int(eng.le_buckets[:, -1].sum()) == total_count == 300
    out = []
    write_histogram_metrics(tree, eng, out)
    counts = [int(l.rsplit(" ", 1)[1]) for l in out if "_hist_count" in l]
    infs = [int(l.rsplit(" ", 1)[1]) for l in out if 'le="+Inf"' in l]
    assert counts == infs and sum(counts) == total_count
    # a look without reset adds nothing
    look = eng.snapshot_all_le(reset=False)
    assert not look["count"].any()
    np.testing.assert_array_equal(eng.le_buckets, prev)


def test_release_zeroes_the_lifetime_row_before_the_id_is_reused(oracle, monkeypatch):
    monkeypatch.setattr(N, "limits", oracle.limits)
    eng, tree, stats = _tree(oracle, S=2)
    a = stats.scope("rt", "http", "client", "a").stat("request_latency_ms")
    keep = stats.stat("kept")
    for v in (1.0, 2.0, 300.0):
        a.add(v)
    keep.add(7.0)
    snapshot_histograms_le(tree, eng)
    sid = a.series_id
    assert eng.le_buckets[sid].tolist() == [1, 2, 3, 3] and eng.le_sums[sid] == 303
    a.add(5.0)  # staged, never snapshotted: it goes with the Stat
    stats.prune("rt", "http", "client", "a")
    assert not eng.le_buckets[sid].any() and eng.le_sums[sid] == 0
    assert eng.le_buckets[keep.series_id].tolist() == [0, 1, 1, 1]
    b = stats.scope("rt", "http", "client", "b").stat("request_latency_ms")
    assert b.series_id == sid
    b.add(400.0)
    snapshot_histograms_le(tree, eng)
    assert eng.le_buckets[sid].tolist() == [0, 0, 1, 1] and eng.le_sums[sid] == 400
    assert eng.le_buckets[keep.series_id].tolist() == [0, 1, 1, 1]  # an empty interval adds nothing


def test_exact_lines_of_a_three_stat_tree(oracle):
    eng, tree, stats = _tree(oracle)
    a = stats.scope("rt", "http", "client", 'a"b').stat("request_latency_ms")
    srv = stats.scope("rt", "http", "server", "x").stat("request_latency_ms")
    plain = stats.stat("lat-ms")
    stats.scope("rt", "http").counter("requests").incr(3)  # not a Stat: no histogram lines
    for v in (0.5, 1.0, 3.0, 250.0, 251.0, 497.0, 498.0, 3e9):
        a.add(v)
    srv.add(100.0)
    assert snapshot_histograms_le(tree, eng) == 3
    for v in (2.0, 600.0):  # a second interval: lifetime counters grow
        srv.add(v)
    assert snapshot_histograms_le(tree, eng) == 3
    out = []
    write_histogram_metrics(tree, eng, out)
    la = 'rt="http", client="a\\\\b"'
    ls = 'rt="http", server="x"'
    want = [
        f'rt:client:request_latency_ms_hist_bucket{{{la}, le="1"}} 2\n',
        f'rt:client:request_latency_ms_hist_bucket{{{la}, le="250"}} 4\n',
        f'rt:client:request_latency_ms_hist_bucket{{{la}, le="497"}} 6\n',
        f'rt:client:request_latency_ms_hist_bucket{{{la}, le="+Inf"}} 8\n',
        f'rt:client:request_latency_ms_hist_sum{{{la}}} {0 + 1 + 3 + 250 + 251 + 497 + 498 + 2147483647}\n',
        f'rt:client:request_latency_ms_hist_count{{{la}}} 8\n',
        f'rt:server:request_latency_ms_hist_bucket{{{ls}, le="1"}} 0\n',
        f'rt:server:request_latency_ms_hist_bucket{{{ls}, le="250"}} 2\n',
        f'rt:server:request_latency_ms_hist_bucket{{{ls}, le="497"}} 2\n',
        f'rt:server:request_latency_ms_hist_bucket{{{ls}, le="+Inf"}} 3\n',
        f'rt:server:request_latency_ms_hist_sum{{{ls}}} 702\n',
        f'rt:server:request_latency_ms_hist_count{{{ls}}} 3\n',
        'lat_ms_hist_bucket{le="1"} 0\n',
        'lat_ms_hist_bucket{le="250"} 0\n',
        'lat_ms_hist_bucket{le="497"} 0\n',
        'lat_ms_hist_bucket{le="+Inf"} 0\n',
        'lat_ms_hist_sum 0\n',
        'lat_ms_hist_count 0\n',
    ]
    assert sorted(out) == sorted(want)  # (child order is the tree's map order)
    for k in range(0, 18, 6):  # each Stat's six lines stand together, in order
        i = out.index(want[k])
        assert out[i:i + 6] == want[k:k + 6]
    # the summary lines keep the interval's numbers: the second interval of srv
    summ = []
    write_metrics(tree, summ)
    assert f'rt:server:request_latency_ms_count{{{ls}}} 2\n' in summ
    assert f'rt:server:request_latency_ms_sum{{{ls}}} 602\n' in summ


def test_telemeter_without_histograms_is_unchanged_and_appends_with(oracle):
    eng, tree, stats = _tree(oracle)
    twin_eng = StatEngine(engine=LeOracleEngine(8, oracle), batch=4)
    twin_tree = MetricsTree(twin_eng)
    twin_stats = MetricsTreeStatsReceiver(twin_tree)
    for st_ in (stats, twin_stats):
        s = st_.scope("rt", "http", "client", "a").stat("request_latency_ms")
        for v in (1.0, 20.0, 300.0):
            s.add(v)
        st_.scope("rt", "http").counter("requests").incr(2)
    snapshot_histograms_le(tree, eng)
    snapshot_histograms(twin_tree, twin_eng)  # today's driver, no buckets
    plain = []
    write_metrics(tree, plain)
    today = PrometheusTelemeter(twin_tree).render()
    assert PrometheusTelemeter(tree).render() == "".join(plain) == today  # byte-identical to today's
    extra = []
    write_histogram_metrics(tree, eng, extra)
    assert len(extra) == 6
    tel = PrometheusTelemeter(tree, histograms=eng)
    assert tel.render() == "".join(plain) + "".join(extra)
    tel.histograms = None  # settable later
    assert tel.render() == "".join(plain)
