"""Configurable quantiles above the engine, on the host: StatEngine.enable_quantiles /
snapshot_all_quantiles / release / grow / checkpoint / restore,
telemetry.snapshot_histograms_quantiles, the Prometheus quantile lines and the telemeter's
optional quantiles, over an oracle-backed stand-in engine whose quantiles are
l5do_percentile's.  The values are checked against oracle.PyStat.percentile.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd.prometheus import PrometheusTelemeter, write_histogram_metrics, write_metrics, write_quantile_metrics
from linkerd_amd.telemetry import (MetricsTree, MetricsTreeStatsReceiver, StatEngine, snapshot_histograms,
                                   snapshot_histograms_quantiles)

from .test_le_exporters_host import LeOracleEngine

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QS = (0.75, 0.25, 0.995)  # stored ascending: 0.25, 0.75, 0.995


class QuantOracleEngine(LeOracleEngine):
    """LeOracleEngine (an OracleEngine) plus HistogramEngine.quantiles (full signature) and
    what grow / checkpoint / restore call: the constructor's (capacity, device),
    export_sparse, import_sparse, close."""

    ORACLE = None  # the oracle module (set by the fixture below)

    def __init__(self, S, device=0):
        super().__init__(S, self.ORACLE)
        self.device, self.closed = device, False

    def quantiles(self, q, first=0, count=None, reset=False, with_series=False):
        self.calls.append("quantiles")
        f = self.O.lib().l5do_percentile
        f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_void_p, ctypes.c_double]
        with self.lock:
            count = self.max_series - first if count is None else count
            sl = slice(first, first + count)
            h = self.h.h[sl].copy()
            out = np.array([[f(h.ctypes.data + i * h.dtype.itemsize, float(x)) for x in q] for i in range(count)],
                           np.int64).reshape(count, len(q))
            series = self.O.summarize_counts(h["counts"], h["total"])
            if reset:
                self.h.h[sl] = 0
        return (out, series) if with_series else out

    def export_sparse(self, first=0, count=None, reset=False):
        with self.lock:
            count = self.max_series - first if count is None else count
            sl = slice(first, first + count)
            counts, totals = self.h.h["counts"][sl].copy(), self.h.h["total"][sl].copy()
            if reset:
                self.h.h[sl] = 0
        r, b = np.nonzero(counts)
        entries = np.zeros(r.size, N.BUCKET_ENTRY_DTYPE)
        entries["bucket"], entries["count"] = b, counts[r, b]
        row_off = np.zeros(count + 1, np.uint64)
        row_off[1:] = np.cumsum(np.bincount(r, minlength=count))
        return row_off, entries, totals

    def import_sparse(self, row_off, entries, totals, first=0):
        with self.lock:
            for i in range(len(row_off) - 1):
                e = entries[int(row_off[i]):int(row_off[i + 1])]
                rec = self.h.h[first + i]
                rec["counts"][e["bucket"]] += e["count"].astype(np.int32)
                self.h.h["num"][first + i] += int(e["count"].sum())
                self.h.h["total"][first + i] += totals[i]

    def close(self):
        self.closed = True


@pytest.fixture(scope="module", autouse=True)
def lib(oracle):
    QuantOracleEngine.ORACLE = oracle
    if not os.path.exists(N.LIB_PATH):  # (enable_le snaps its bounds with the library's host code)
        if shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"):
            pytest.skip("libl5dhist.so not built and no hipcc to build it")
        subprocess.run(["make", "-s", "-C", os.path.join(REPO, "linkerd_amd", "csrc")], check=True)
    return N.load()


def _tree(S=8, qs=QS, le=None):
    eng = StatEngine(engine=QuantOracleEngine(S), batch=4)
    if le is not None:
        eng.enable_le(le)
    if qs is not None:
        eng.enable_quantiles(qs)
    tree = MetricsTree(eng)
    return eng, tree, MetricsTreeStatsReceiver(tree)


def _py(oracle, values, qs):
    ref = oracle.PyStat()
    for v in values:
        ref.add(float(v))
    return [ref.percentile(float(q)) for q in qs]


def test_enable_quantiles_validation():
    eng, _, _ = _tree()
    assert eng.quantile_q.dtype == np.float64 and eng.quantile_q.tolist() == [0.25, 0.75, 0.995]
    assert eng.quantile_labels == ["0.25", "0.75", "0.995"]
    assert eng.quantile_values.shape == (8, 3) and eng.quantile_values.dtype == np.int64 and not eng.quantile_values.any()
    bad = [[], list(np.arange(1, 66) / 100.0), [0.25, 0.75, 0.25], [0.25, float("nan")], [-0.0001], [1.0001],
           [0.25, float("inf")]]
    bad += [[0.25, q] for q in (0, 0.5, 0.9, 0.95, 0.99, 0.999, 0.9999, 1)]  # the summary block's own
    for qs in bad:
        with pytest.raises(ValueError, match="enable_quantiles"):
            eng.enable_quantiles(qs)
    assert eng.quantile_q.tolist() == [0.25, 0.75, 0.995]  # a refused call changes nothing
    eng.enable_quantiles(np.arange(1, 65) / 100.0 + 0.001)  # 64 are fine
    assert eng.quantile_values.shape == (8, 64)
    eng.enable_quantiles([1e-4])
    assert eng.quantile_labels == ["1.0E-4"] and eng.quantile_values.shape == (8, 1)
    with pytest.raises(RuntimeError, match="enable_quantiles"):
        _tree(qs=None)[0].snapshot_all_quantiles()


def test_snapshot_all_quantiles_values_and_overwrite(oracle):
    eng, tree, stats = _tree()
    a = stats.scope("rt", "http", "client", "a").stat("request_latency_ms")
    b = stats.stat("other")
    for v in range(1, 101):
        a.add(float(v))
    skewed = [1.0, 2.0, 2.0, 300.0, 5000.0, 3e9, 0.2]
    for v in skewed:
        b.add(v)
    eng.engine.calls.clear()
    assert snapshot_histograms_quantiles(tree, eng) == 2
    assert eng.engine.calls == ["quantiles"]  # ONE engine call: the values, the summaries, the reset
    assert eng.quantile_values[a.series_id].tolist() == [25, 75, 100] == _py(oracle, range(1, 101), eng.quantile_q)
    assert eng.quantile_values[b.series_id].tolist() == _py(oracle, skewed, eng.quantile_q)
    assert a.snapshotted_summary.count == 100 and a.snapshotted_summary.p50 == 50 and b.snapshotted_summary.count == 7
    assert not eng.quantile_values[2:].any()
    # the next interval overwrites: quantiles do not accumulate
    a.add(9.0)
    look = eng.snapshot_all_quantiles(reset=False)  # only looks
    assert look["count"][a.series_id] == 1 and eng.quantile_values[a.series_id].tolist() == [0, 9, 9]
    assert snapshot_histograms_quantiles(tree, eng) == 2
    assert eng.quantile_values[a.series_id].tolist() == [0, 9, 9] == _py(oracle, [9.0], eng.quantile_q)
    assert not eng.quantile_values[b.series_id].any() and b.snapshotted_summary.count == 0
    assert snapshot_histograms_quantiles(tree, eng) == 2
    assert not eng.quantile_values.any()


def test_exact_lines_of_a_three_stat_tree():
    eng, tree, stats = _tree(qs=(0.75, 1e-4))
    a = stats.scope("rt", "http", "client", 'a"b').stat("request_latency_ms")
    gone = stats.scope("rt", "http", "client", "gone").stat("request_latency_ms")
    plain = stats.stat("lat-ms")
    stats.scope("rt", "http").counter("requests").incr(3)  # not a Stat: no quantile lines
    for v in range(1, 101):
        a.add(float(v))
    gone.add(5.0)
    plain.add(40.0)
    assert snapshot_histograms_quantiles(tree, eng) == 3
    stats.prune("rt", "http", "client", "gone")  # pruned: prints nothing
    late = stats.stat("late")  # not yet snapshotted: prints nothing
    late.add(1.0)
    out = []
    write_quantile_metrics(tree, eng, out)
    la = 'rt="http", client="a\\\\b"'
    want = [
        f'rt:client:request_latency_ms{{{la}, quantile="1.0E-4"}} 0\n',
        f'rt:client:request_latency_ms{{{la}, quantile="0.75"}} 75\n',
        'lat_ms{quantile="1.0E-4"} 0\n',
        'lat_ms{quantile="0.75"} 40\n',
    ]
    assert sorted(out) == sorted(want)  # (child order is the tree's map order)
    for k in (0, 2):  # each Stat's lines stand together, in the order of quantile_q
        i = out.index(want[k])
        assert out[i:i + 2] == want[k:k + 2]
    assert snapshot_histograms_quantiles(tree, eng) == 3  # a, lat-ms, late
    out = []
    write_quantile_metrics(tree, eng, out)
    assert 'late{quantile="0.75"} 1\n' in out and len(out) == 6
    off = []
    write_quantile_metrics(tree, _tree(qs=None)[0], off)  # an engine without enable_quantiles
    assert off == []


def test_with_le_one_quantiles_and_one_le_counts_call_per_interval(oracle):
    eng, tree, stats = _tree(le=(1, 250, 500))
    a = stats.scope("rt", "http", "client", "a").stat("request_latency_ms")
    total = 0
    for interval in range(2):
        vals = [1.0, 3.0, 250.0, 251.0, 600.0][:3 + 2 * interval]
        for v in vals:
            a.add(v)
        total += len(vals)
        eng.engine.calls.clear()
        assert snapshot_histograms_quantiles(tree, eng) == 1
        assert eng.engine.calls == ["quantiles", "le_counts"]  # and no plain snapshot
        assert eng.quantile_values[a.series_id].tolist() == _py(oracle, vals, eng.quantile_q)  # the interval's
        assert a.snapshotted_summary.count == len(vals)
        assert int(eng.le_buckets[a.series_id][-1]) == total  # the lifetime's
    assert eng.le_buckets[a.series_id].tolist() == [2, 6, 7, 8] and eng.le_sums[a.series_id] == 254 + 1105
    a.add(2.0)
    eng.engine.calls.clear()
    before = eng.le_buckets.copy()
    assert eng.snapshot_all_quantiles(reset=False)["count"][a.series_id] == 1  # a look
    assert eng.engine.calls == ["quantiles"] and (eng.le_buckets == before).all()
    assert eng.quantile_values[a.series_id].tolist() == [0, 2, 2]


def test_release_grow_checkpoint_restore():
    eng, tree, stats = _tree(S=2)
    a = stats.scope("rt", "http", "client", "a").stat("request_latency_ms")
    keep = stats.stat("kept")
    for v in (10.0, 20.0, 30.0, 40.0):
        a.add(v)
    keep.add(7.0)
    snapshot_histograms_quantiles(tree, eng)
    sid = a.series_id
    assert eng.quantile_values[sid].tolist() == [10, 30, 40] and eng.quantile_values[keep.series_id].tolist() == [0, 7, 7]
    stats.prune("rt", "http", "client", "a")  # release zeroes the id's row
    assert not eng.quantile_values[sid].any() and eng.quantile_values[keep.series_id].tolist() == [0, 7, 7]
    b = stats.scope("rt", "http", "client", "b").stat("request_latency_ms")
    assert b.series_id == sid
    b.add(50.0)  # stays in the open interval through grow and the checkpoint
    old = eng.engine
    eng.grow(5)
    assert old.closed and eng.capacity == 5 and eng.quantile_values.shape == (5, 3)
    assert eng.quantile_values[keep.series_id].tolist() == [0, 7, 7] and not eng.quantile_values[2:].any()
    ckpt = eng.checkpoint()
    assert all(isinstance(v, np.ndarray) for v in ckpt.values())
    assert ckpt["quantile_q"].tolist() == [0.25, 0.75, 0.995] and ckpt["quantile_values"].shape == (2, 3)
    fresh = StatEngine(engine=QuantOracleEngine(4), batch=4)
    fresh.restore(ckpt)
    assert fresh.quantile_q.tolist() == [0.25, 0.75, 0.995] and fresh.quantile_labels == ["0.25", "0.75", "0.995"]
    assert fresh.quantile_values.shape == (4, 3)
    assert fresh.quantile_values[:2].tobytes() == eng.quantile_values[:2].tobytes() and not fresh.quantile_values[2:].any()
    summ = fresh.snapshot_all_quantiles()
    assert summ["count"][sid] == 1 and fresh.quantile_values[sid].tolist() == [0, 50, 50]
    # a checkpoint written before the feature existed, and one of an engine with it off
    legacy = {k: v for k, v in ckpt.items() if not k.startswith("quantile_")}
    for ck in (legacy, _tree(qs=None)[0].checkpoint()):
        plain = StatEngine(engine=QuantOracleEngine(4), batch=4)
        plain.restore(ck)
        assert plain.quantile_q is None and plain.quantile_values is None
    off = _tree(qs=None)[0].checkpoint()
    assert off["quantile_q"].size == 0 and off["quantile_q"].dtype == np.float64 and off["quantile_values"].size == 0


def test_telemeter_without_quantiles_is_unchanged_and_appends_with():
    eng, tree, stats = _tree(le=(1, 250, 500))
    twin = StatEngine(engine=QuantOracleEngine(8), batch=4)
    twin_tree = MetricsTree(twin)
    twin_stats = MetricsTreeStatsReceiver(twin_tree)
    for st_ in (stats, twin_stats):
        s = st_.scope("rt", "http", "client", "a").stat("request_latency_ms")
        for v in (1.0, 20.0, 300.0):
            s.add(v)
        st_.scope("rt", "http").counter("requests").incr(2)
    snapshot_histograms_quantiles(tree, eng)
    snapshot_histograms(twin_tree, twin)  # the plain driver
    plain, hist, extra = [], [], []
    write_metrics(tree, plain)
    write_histogram_metrics(tree, eng, hist)
    write_quantile_metrics(tree, eng, extra)
    assert PrometheusTelemeter(tree).render() == "".join(plain) == PrometheusTelemeter(twin_tree).render()
    assert PrometheusTelemeter(tree, None, eng).render() == "".join(plain + hist)  # positional arguments as before
    assert len(extra) == 3
    tel = PrometheusTelemeter(tree, histograms=eng, quantiles=eng)
    assert tel.render() == "".join(plain + hist + extra)  # after the `_hist` blocks
    tel.quantiles = None  # settable later
    assert tel.render() == "".join(plain + hist)
    # no line of the exposition appears twice: the configured quantiles are none of the summary's
    lines = PrometheusTelemeter(tree, quantiles=eng).render().splitlines()
    assert len({l.rsplit(" ", 1)[0] for l in lines}) == len(lines)
