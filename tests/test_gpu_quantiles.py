"""GPU configurable quantiles (l5dh_quantiles, l5dh_quantiles_dense, l5dh_render_quantiles)
against the CPU oracle.

The truth everywhere: l5do_percentile (oracle/hist_oracle.c, upstream
BucketedHistogram.percentile) per row and quantile, num the 64-bit row sum; the rows come
from the oracle's ingest or from the crafted rows of tests/summary_rows.py.  Values and
summaries are compared as bytes; the renderer against write_quantile_metrics' f-strings.
"""
import ctypes
import errno
import threading
import types

import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd.javafmt import double_to_string
from linkerd_amd.prometheus import (NameTable, PrometheusTelemeter, line_multiset, stat_name_table,
                                    write_quantile_metrics)
from linkerd_amd.telemetry import (HistogramSummary, MetricsTree, MetricsTreeStatsReceiver, StatEngine,
                                   snapshot_histograms_quantiles)

from tests import render_cases as C
from tests import summary_rows as SR
from tests.test_gpu_render import GUARD, render_guarded, stat_tree

pytestmark = pytest.mark.gpu

NB = N.NBUCKETS
FIXED = (("p50", 0.5), ("p90", 0.9), ("p95", 0.95), ("p99", 0.99), ("p9990", 0.999), ("p9999", 0.9999))


# ---- the truth ---------------------------------------------------------------------------
def _percentile(oracle):
    f = oracle.lib().l5do_percentile
    f.restype, f.argtypes = ctypes.c_int64, [ctypes.c_void_p, ctypes.c_double]
    return f


def oracle_hists(oracle, counts):
    """The rows as l5do_hist records: num the 64-bit row sum."""
    counts = np.asarray(counts, np.int32).reshape(-1, NB)
    h = np.zeros(counts.shape[0], oracle.HIST_DTYPE)
    h["counts"] = counts
    h["num"] = counts.astype(np.int64).sum(axis=1)
    return h


def truth(oracle, hists, qs):
    """int64 [rows][K]: l5do_percentile(row, q) for every row and q."""
    f, base, step = _percentile(oracle), hists.ctypes.data, hists.dtype.itemsize
    qs = [float(q) for q in qs]
    out = np.empty((hists.shape[0], len(qs)), np.int64)
    for r in range(hists.shape[0]):
        p = base + r * step
        out[r] = [f(p, q) for q in qs]
    return out


def _engine(S, stage=None):
    from linkerd_amd.engine import HistogramEngine
    e = HistogramEngine(S)
    if stage is not None:
        e.set_param(N.PARAM_STAGE_SAMPLES, stage)
    return e


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _raw(x):
    return (x if isinstance(x, np.ndarray) else x.cpu().numpy()).tobytes()


# ---- dense rows: every answer position -----------------------------------------------------
# The 29 sets of 64 that together hold (b + 1) / 1798 for every bucket b (the last overlaps)
POSITION_SETS = [np.arange(s, s + 64, dtype=np.float64) / 1798.0 for s in [min(s, 1798 - 63) for s in range(1, 1799, 64)]]
HALF = 0.5
OTHER_SETS = [
    np.array([0.5]),                                                   # K = 1
    np.array([0.0, 1.0]),
    np.array([0.99, 0.25, 0.5, 0.25, 1.0, 0.0, 0.75, 0.99, 0.25]),     # unsorted, duplicates
    np.array([1e-12, 1.0 - 2.0 ** -53, np.nextafter(HALF, 0.0), np.nextafter(HALF, 1.0), 0.25, 0.75, 0.995]),
    np.array([q for _, q in FIXED] + [1.0]),                           # the summary's own six, and max
]
SETS = POSITION_SETS + OTHER_SETS
ROW_ONES, ROW_INTMAX = 1797, 1798 + 2000 + 2  # dense_rows(): the last staircase row, every bucket at 2^31 - 1


@pytest.fixture(scope="module")
def dense(oracle, gpu_available):
    rows, _ = SR.dense_rows()
    assert (rows[ROW_ONES] == 1).all() and (rows[ROW_INTMAX] == SR.INT_MAX).all()
    hists = oracle_hists(oracle, rows)
    assert int(hists["num"].max()) == 1798 * SR.INT_MAX > 2 ** 32 and not rows[-1].any()
    with _engine(32) as e:
        summ = e.summarize_dense(rows, np.zeros(rows.shape[0], np.int64))
        yield types.SimpleNamespace(e=e, rows=rows, hists=hists, summ=summ, covered={ROW_ONES: set(), ROW_INTMAX: set()})


def test_position_sets_hold_every_bucket():
    assert len(POSITION_SETS) == 29 and all(s.size == 64 for s in POSITION_SETS)
    assert set(np.concatenate(POSITION_SETS).tolist()) == {(b + 1) / 1798.0 for b in range(1798)}


@pytest.mark.parametrize("k", range(len(SETS)))
def test_dense_every_answer_position(oracle, dense, k):
    qs = SETS[k]
    want = truth(oracle, dense.hists, qs)
    if k < len(POSITION_SETS):
        # on the all-ones row and on the all-(2^31 - 1) row, q = (b + 1) / 1798 answers bucket b
        mids = [int(oracle.lib().l5do_midpoint(b)) for b in range(NB)]
        b0 = int(round(qs[0] * 1798)) - 1
        for r in (ROW_ONES, ROW_INTMAX):
            assert want[r].tolist() == mids[b0:b0 + 64], (k, r)
            dense.covered[r] |= set(range(b0, b0 + 64))
    got = dense.e.quantiles_dense(dense.rows, qs)
    assert got.dtype == np.int64 and got.shape == want.shape
    if got.tobytes() != want.tobytes():
        r, c = np.argwhere(got != want)[0]
        raise AssertionError(f"set {k}: row {r} q = {qs[c]!r} (num {dense.hists['num'][r]}): got {got[r, c]} "
                             f"want {want[r, c]}")
    # the invariants, on the GPU's output
    some = dense.hists["num"] > 0
    for c, q in enumerate(qs):
        for name, fq in FIXED:
            if q == fq:
                assert got[:, c].tobytes() == dense.summ[name].tobytes(), (k, name)
        if q == 1.0:
            assert (got[some, c] == dense.summ["max"][some]).all() and not got[~some, c].any()
        if q == 0.0:
            assert not got[:, c].any()
    if k == len(POSITION_SETS) - 1:  # (the sets run in order: every bucket was an answer by now)
        assert dense.covered[ROW_ONES] == dense.covered[ROW_INTMAX] == set(range(NB))


def test_dense_device_buffers(oracle, dense):
    rows, hists = dense.rows[1790:1830], dense.hists[1790:1830]
    qs = OTHER_SETS[3]
    out = _dev(np.full((rows.shape[0], qs.size), -1, np.int64))
    dense.e.quantiles_into(_dev(qs), out, dense=_dev(rows))
    assert _raw(out) == truth(oracle, hists, qs).tobytes()


def test_invalid_arguments_write_nothing(dense):
    rows = dense.rows[:37]
    bad_sets = [np.zeros(0), np.full(65, 0.5), np.array([0.5, -0.0001]), np.array([1.0001, 0.5]),
                np.array([0.25, float("nan"), 0.75])]
    for qs in bad_sets:
        pattern = np.full((37, max(qs.size, 1)), 0x5A5A5A5A5A5A5A5A, np.int64)
        for q_kind in ("host", "device"):
            for o_kind in ("host", "device"):
                q = qs if q_kind == "host" else _dev(qs)
                out = pattern.copy() if o_kind == "host" else _dev(pattern)
                with pytest.raises(N.L5dhError) as ei:
                    dense.e.quantiles_into(q, out, dense=rows)
                assert ei.value.code == -errno.EINVAL, (qs, q_kind, o_kind)
                assert _raw(out) == pattern.tobytes(), (qs, q_kind, o_kind)
    lib, q = N.load(), np.array([0.5])
    out = np.full(37, 7, np.int64)
    assert lib.l5dh_quantiles_dense(dense.e._ctx, rows.ctypes.data, 37, None, 1, out.ctypes.data) == -errno.EINVAL
    assert lib.l5dh_quantiles_dense(dense.e._ctx, rows.ctypes.data, 37, q.ctypes.data, 1, None) == -errno.EINVAL
    assert lib.l5dh_quantiles_dense(dense.e._ctx, rows.ctypes.data, 0, q.ctypes.data, 1, None) == 0  # nothing to do
    assert (out == 7).all()


# ---- live state ------------------------------------------------------------------------------
S, QUIET = 257, range(96, 128)  # 9 tiles, the last of one series; tile 3 receives no sample
FIRST, COUNT = 5, 200  # starts and ends inside a tile
QS = np.array([0.25, 0.5, 0.75, 0.9, 0.995, 0.9999, 1.0, 0.0, 1e-4, 0.25])


def _batch(seed, n, space=S, quiet=QUIET):
    rng = np.random.default_rng(seed)
    live = np.array([s for s in range(space) if s not in quiet], np.uint32)
    series = live[rng.integers(0, live.size, size=n)]
    vals = np.exp(3.0 + 1.5 * rng.standard_normal(n)).astype(np.float32)
    vals[:6] = np.array([0, 113, 3030, 1e9, 3e9, -5], dtype=np.float32)
    series[:6] = np.array([space - 1, 6, 31, 32, 204, 33]) % space
    return series, vals


def _live_case(oracle, space, quiet):
    batches = [_batch(11, 30_000, space, quiet), _batch(12, 20_000, space, quiet), _batch(13, 3_000, space, quiet)]
    ref = oracle.OracleHistograms(space)
    for s, v in batches:
        assert ref.ingest(s, v) == 0
    counts, totals = ref.counts(), ref.totals()
    assert counts[:, 0].any() and counts[:, 1797].any()
    return dict(batches=batches, counts=counts, totals=totals, hists=oracle_hists(oracle, counts),
                summ=oracle.summarize_counts(counts, totals))


@pytest.fixture(scope="module")
def case(oracle, gpu_available):
    c = _live_case(oracle, S, QUIET)
    assert not c["counts"][list(QUIET)].any()
    return c


def _fed(case, space):
    """A dirty state (the first batch, folded by a look), a pending segment (the second) and
    samples still in the staging ring (the third)."""
    e = _engine(space, 0)
    e.ingest(*case["batches"][0])
    e.snapshot(reset=False)
    e.ingest(*case["batches"][1])
    e.set_param(N.PARAM_STAGE_SAMPLES, 1 << 16)
    e.ingest(*case["batches"][2])
    return e


def test_live_several_tiles(oracle, case):
    sl = slice(FIRST, FIRST + COUNT)
    want = truth(oracle, case["hists"][sl], QS)
    with _fed(case, S) as e:
        got = e.quantiles(QS, first=FIRST, count=COUNT)  # reset = False
        assert got.tobytes() == want.tobytes()
        assert not got[QUIET.start - FIRST:QUIET.stop - FIRST].any()
        assert e.snapshot(reset=False, with_counts=True)[1].tobytes() == case["counts"].tobytes()  # nothing was touched
        # a bad range or a bad q with reset = 1: -EINVAL from the library, nothing written, nothing reset
        lib, buf = N.load(), np.zeros((S, QS.size), np.int64)
        assert lib.l5dh_quantiles(e._ctx, S - 1, 2, QS.ctypes.data, QS.size, buf.ctypes.data, None, 1) == -errno.EINVAL
        bad = QS.copy()
        bad[3] = 1.5
        assert lib.l5dh_quantiles(e._ctx, 0, S, bad.ctypes.data, QS.size, buf.ctypes.data, None, 1) == -errno.EINVAL
        assert lib.l5dh_quantiles(e._ctx, 0, S, QS.ctypes.data, QS.size, None, None, 1) == -errno.EINVAL
        assert lib.l5dh_quantiles(e._ctx, 0, 0, QS.ctypes.data, QS.size, None, None, 1) == 0  # count == 0
        assert not buf.any()
        assert e.snapshot(reset=False, with_counts=True)[1].tobytes() == case["counts"].tobytes()
        # with the series' summaries and the reset of the same range
        got, series = e.quantiles(QS, first=FIRST, count=COUNT, reset=True, with_series=True)
        assert got.tobytes() == want.tobytes()
        assert series.tobytes() == case["summ"][sl].tobytes()
        after, counts = e.snapshot(reset=False, with_counts=True)
        expect, tot = case["counts"].copy(), case["totals"].copy()
        expect[sl], tot[sl] = 0, 0
        assert counts.tobytes() == expect.tobytes()  # the series outside the range are untouched
        assert after.tobytes() == oracle.summarize_counts(expect, tot).tobytes()
        assert not e.quantiles(QS, first=FIRST, count=COUNT).any()
        assert e.quantiles(QS).tobytes() == truth(oracle, oracle_hists(oracle, expect), QS).tobytes()


def test_live_one_tile_space(oracle, gpu_available):
    S1 = 8  # one tile: every batch is folded at ingest
    c = _live_case(oracle, S1, ())
    with _fed(c, S1) as e:
        got, series = e.quantiles(QS, with_series=True, reset=True)
        assert got.tobytes() == truth(oracle, c["hists"], QS).tobytes()
        assert series.tobytes() == c["summ"].tobytes()
        assert not e.quantiles(QS).any() and not e.snapshot(reset=False)["count"].any()


def test_live_device_outputs_on_a_torch_stream(oracle, case):
    import torch
    sl = slice(FIRST, FIRST + COUNT)
    stream = torch.cuda.Stream()
    with _fed(case, S) as e, torch.cuda.stream(stream):
        e.set_stream(stream.cuda_stream)
        out = torch.full((COUNT, QS.size), -1, dtype=torch.int64, device="cuda:0")
        series = torch.zeros((COUNT, 11), dtype=torch.int64, device="cuda:0")
        e.quantiles_into(_dev(QS), out, series, first=FIRST, count=COUNT, reset=True)
        stream.synchronize()
        assert _raw(out) == truth(oracle, case["hists"][sl], QS).tobytes()
        assert _raw(series) == case["summ"][sl].tobytes()
        assert not e.quantiles(QS, first=FIRST, count=COUNT).any()
        e.set_stream(None)


def test_rollup_linearity(oracle, case):
    G = 3
    group = (np.arange(S) % G).astype(np.uint32)
    group[::9] = N.NO_GROUP
    with _fed(case, S) as e:
        _, g_counts, _ = e.rollup(group, G, with_counts=True)
        got = e.quantiles_dense(g_counts, QS)
    summed = np.zeros((G, NB), np.int64)
    m = group != N.NO_GROUP
    np.add.at(summed, group[m], case["counts"][m].astype(np.int64))
    assert summed.max() <= SR.INT_MAX
    assert got.tobytes() == truth(oracle, oracle_hists(oracle, summed.astype(np.int32)), QS).tobytes()


# ---- the renderer ------------------------------------------------------------------------------
Q64 = np.concatenate([[0.75, 0.995, 1e-4, 0.25, 1e-3, 2.0 ** -64, 1.0 - 2.0 ** -53, 0.1], np.arange(1, 57) / 57.0])


def quantile_case(n, qs, seed=3):
    """(table, q_rows, expected bytes): the text of write_quantile_metrics over a stub engine
    whose rows hold 0, +-1, INT64_MIN, INT64_MAX and the other integer edges."""
    tree = stat_tree(n)
    table = stat_name_table(tree)
    nvalues, K = n + 3, len(qs)
    index = np.random.default_rng(seed).permutation(nvalues)[:n].astype(np.uint32)
    edges = np.array(sorted(set(C.INT64_EDGES) | {1, -1}), np.int64)
    q_rows = np.ascontiguousarray(edges[(np.arange(nvalues * K) * 5 + 1) % edges.size].reshape(nvalues, K))
    table = NameTable(index, table.key_off, table.key_bytes, table.lab_off, table.lab_bytes, table.metrics)
    for j, m in enumerate(table.metrics):
        m.series_id = int(index[j])
        m._set_snapshot(HistogramSummary(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0))
    stub = types.SimpleNamespace(quantile_q=np.asarray(qs), quantile_labels=[double_to_string(float(q)) for q in qs],
                                 quantile_values=q_rows)
    lines = []
    write_quantile_metrics(tree, stub, lines)
    assert len(lines) == K * n
    return table, q_rows, "".join(lines).encode()


@pytest.mark.parametrize("n,qs", [(65, [0.75]), (257, [0.25, 0.75, 0.995, 1e-4]), (65, Q64), (1, Q64)])
def test_quantile_blocks_equal_write_quantile_metrics(dense, n, qs):
    eng = dense.e
    qs = np.asarray(qs, np.float64)
    table, q_rows, want = quantile_case(n, qs)
    if n * qs.size > 1000:  # (every edge value is printed)
        assert {0, 1, -1, -2 ** 63, 2 ** 63 - 1} <= set(q_rows[table.index].ravel().tolist())
    if n > 41:
        assert b'\nabcde{quantile="' in want  # an empty inner text
        assert max(len(l) for l in want.split(b"\n")) > 4096  # a row longer than 4096 bytes
    if qs.size == 4:
        assert b'quantile="1.0E-4"} ' in want and b'quantile="0.995"} ' in want
    got = eng.render_quantiles(table, q_rows, qs)  # host inputs, host output
    assert len(got) == len(want)
    assert got == want
    # device inputs, a device output of exactly len bytes between guards, at an odd address
    dtab, drows, dq = table.to_device(), _dev(q_rows), _dev(qs)
    got_dev = render_guarded(lambda out: eng.render_quantiles(dtab, drows, dq, out=out), len(want), skew=1 + qs.size % 15)
    assert got_dev == want


def test_render_contract(dense):
    import torch
    from linkerd_amd.engine import QUERY
    eng, qs = dense.e, np.array([0.25, 0.75, 0.995])
    table, q_rows, want = quantile_case(70, qs)
    assert eng.render_quantiles(table, q_rows, qs, out=QUERY) == len(want)  # the size query
    nm, ln = eng._names(table), ctypes.c_size_t(12345)
    buf = torch.full((len(want) + 64,), GUARD, dtype=torch.uint8, device="cuda:0")

    def raw(q, nq, out, cap, names=nm, rows=q_rows):
        rc = eng._lib.l5dh_render_quantiles(eng._ctx, ctypes.byref(names) if names is not None else None, table.n,
                                            rows.ctypes.data, rows.shape[0], None if q is None else q.ctypes.data, nq,
                                            out, cap, ctypes.byref(ln))
        return rc, ln.value
    assert raw(qs, 3, buf.data_ptr(), len(want) - 1) == (-errno.ERANGE, len(want))
    assert eng._lib.l5dh_last_error(eng._ctx).decode() == (
        f"render: the text takes {len(want)} bytes, cap is {len(want) - 1}")
    assert (buf.cpu().numpy() == GUARD).all()  # nothing was written
    assert raw(qs, 3, buf.data_ptr(), len(want)) == (0, len(want))
    assert buf[:len(want)].cpu().numpy().tobytes() == want
    for q, nq in ((qs, 0), (np.full(65, 0.5), 65), (np.array([0.5, 1.5, 0.1]), 3), (np.array([float("nan")] * 3), 3),
                  (None, 3)):
        assert raw(q, nq, None, 0) == (-errno.EINVAL, 0)
    assert raw(np.array([0.5, 1e-30, 0.1]), 3, None, 0) == (-errno.ERANGE, 0)  # no Double.toString on the device side
    assert raw(qs, 3, None, 0, names=None) == (-errno.EINVAL, 0)
    bad = table.index.copy()
    bad[37] = q_rows.shape[0]
    with pytest.raises(N.L5dhError, match="row 37") as ei:
        eng.render_quantiles(NameTable(bad, table.key_off, table.key_bytes, table.lab_off, table.lab_bytes), q_rows, qs)
    assert ei.value.code == -errno.EINVAL
    assert eng.render_quantiles(table, q_rows, qs) == want  # a valid call afterwards succeeds


# ---- end to end ----------------------------------------------------------------------------------
def test_end_to_end_tree_to_prometheus(oracle, gpu_available):
    se = StatEngine(capacity=64, device=0, batch=128)
    se.enable_le([1, 250, 500, float("inf")])
    se.enable_quantiles([0.75, 0.25, 0.995, 1e-4])
    tree = MetricsTree(se)
    stats = MetricsTreeStatsReceiver(tree)
    a = stats.scope("rt", "http", "client", "a").stat("request_latency_ms")
    b = stats.scope("rt", "http", "server", "b").stat("request_latency_ms")
    stats.stat("idle")
    stats.counter("requests").incr(3)

    def feed(stat, lo):
        for v in range(lo, lo + 1000):
            stat.add(float(v))
    threads = [threading.Thread(target=feed, args=(a, 1)), threading.Thread(target=feed, args=(b, 5001))]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert snapshot_histograms_quantiles(tree, se) == 3
    late = stats.stat("late")  # registered since the snapshot: no quantile lines, no summary block
    assert late.snapshotted_summary is None
    for st, lo in ((a, 1), (b, 5001)):
        ref = oracle.PyStat()
        for v in range(lo, lo + 1000):
            ref.add(float(v))
        assert se.quantile_values[st.series_id].tolist() == [ref.percentile(float(q)) for q in se.quantile_q]
        assert st.snapshotted_summary.count == 1000
        assert int(se.le_buckets[st.series_id][-1]) == 1000  # the same interval fed the `le` counters
    assert se.quantile_labels == ["1.0E-4", "0.25", "0.75", "0.995"]
    tel = PrometheusTelemeter(tree, histograms=se, quantiles=se)
    text = tel.render()
    lines = line_multiset(text)
    lab = 'rt="http", client="a"'
    assert lines[f'rt:client:request_latency_ms{{{lab}, quantile="0.25"}} {se.quantile_values[a.series_id][1]}'] == 1
    assert lines['idle{quantile="1.0E-4"} 0'] == 1 and not any(l.startswith("late{quantile") for l in lines)
    got = tel.render_bytes(se.engine)
    assert line_multiset(got.decode("utf-8")) == lines and len(got) == len(text.encode("utf-8"))
    assert text.count('quantile="0.995"') == 3
    # the next interval overwrites: quantiles do not accumulate, the `le` counters do
    a.add(7.0)
    assert snapshot_histograms_quantiles(tree, se) == 4
    ref = oracle.PyStat()
    ref.add(7.0)
    assert se.quantile_values[a.series_id].tolist() == [ref.percentile(float(q)) for q in se.quantile_q] == [0, 0, 7, 7]
    assert not se.quantile_values[b.series_id].any()
    assert int(se.le_buckets[a.series_id][-1]) == 1001
    tel2 = PrometheusTelemeter(tree, histograms=se, quantiles=se)
    assert line_multiset(tel2.render_bytes(se.engine).decode("utf-8")) == line_multiset(tel2.render())
    se.engine.close()
