"""GPU cumulative `le` buckets (l5dh_le, l5dh_le_dense) against the CPU oracle.

The truth everywhere: np.cumsum of the bucket counts (uint64) at columns cuts - 1, with
the row sum for +Inf; counts and totals come from the oracle or from the crafted rows of
tests/summary_rows.py.  Buckets, sums and summaries are compared as bytes.
"""
import itertools

import numpy as np
import pytest

from linkerd_amd import _native as N

from tests import summary_rows as SR

pytestmark = pytest.mark.gpu

NB = N.NBUCKETS


def le_truth(counts, cuts):
    cum = np.cumsum(np.asarray(counts).astype(np.uint64), axis=1)
    return np.ascontiguousarray(np.concatenate([cum[:, np.asarray(cuts, np.int64) - 1], cum[:, -1:]], axis=1))


def _engine(S, stage=None):
    from linkerd_amd.engine import HistogramEngine
    e = HistogramEngine(S)
    if stage is not None:
        e.set_param(N.PARAM_STAGE_SAMPLES, stage)
    return e


def _dev(a):
    import torch
    return torch.from_numpy(a).to("cuda:0")


def _raw(x):
    return (x if isinstance(x, np.ndarray) else x.cpu().numpy()).tobytes()


# ---- dense rows --------------------------------------------------------------------
def _crafted_rows():
    """37 rows (the last workgroup of four waves holds one): 29 staircases over the lane
    and group edges, every bucket at 2^31 - 1 (group sums and prefixes past 2^32), one-hot
    rows at the first / last bins of lanes 0, 1 and 63 and of lane 63's extra groups, and
    the empty row."""
    stairs = SR.staircase_rows()[np.array(SR.FOLD_ROWS[:28] + (1798,)) - 1]
    hot = np.zeros((6, NB), np.int32)
    hot[np.arange(6), [0, 27, 28, 1791, 1792, 1797]] = [1, 2, 3, 4, SR.INT_MAX, 6]
    rows = np.ascontiguousarray(np.concatenate([stairs, np.full((1, NB), SR.INT_MAX, np.int32), hot,
                                                np.zeros((1, NB), np.int32)]))
    assert rows.shape == (37, NB)
    totals = np.resize(np.array(SR.SPECIAL_TOTALS, np.int64), 37)
    return rows, totals


@pytest.fixture(scope="module")
def dense(gpu_available):
    rows, totals = _crafted_rows()
    with _engine(32) as e:
        yield e, rows, totals


def test_dense_every_cut_position(dense):
    e, rows, totals = dense
    cum = np.cumsum(rows.astype(np.uint64), axis=1)
    assert int(cum[29, -1]) == 1798 * SR.INT_MAX > 2 ** 32
    starts = [min(s, 1797 - 63) for s in range(1, 1798, 64)]
    assert len(starts) == 29
    sets = [np.arange(s, s + 64, dtype=np.uint32) for s in starts]
    assert set(np.concatenate(sets).tolist()) == set(range(1, 1798))  # all 1797 cuts
    sets += [np.array([1], np.uint32), np.array([1797], np.uint32), np.array([900], np.uint32),  # K = 1
             np.arange(28, 1793, 28, dtype=np.uint32),          # K = 64: every lane's first bin
             np.array([2, 3, 6, 11, 26, 51, 101, 193, 262, 332, 743, 1797], np.uint32)]
    assert len(sets[-2]) == 64
    for cuts in sets:
        le, sums = e.le_counts_dense(rows, totals, cuts)
        assert le.dtype == np.uint64 and le.shape == (37, len(cuts) + 1)
        want = le_truth(rows, cuts)
        if le.tobytes() != want.tobytes():
            r, k = np.argwhere(le != want)[0]
            raise AssertionError(f"cuts {cuts[0]}..{cuts[-1]}: row {r} column {k} (cut "
                                 f"{cuts[k] if k < len(cuts) else '+Inf'}): got {le[r, k]} want {want[r, k]}")
        assert sums.tobytes() == totals.tobytes()
    # no totals: sums of zero, the same buckets
    le, sums = e.le_counts_dense(rows, None, sets[0])
    assert le.tobytes() == le_truth(rows, sets[0]).tobytes() and not sums.any()


def test_dense_invalid_arguments_write_nothing(dense):
    e, rows, totals = dense
    bad_sets = [np.zeros(0, np.uint32), np.arange(1, 66, dtype=np.uint32),      # ncuts 0 and 65
                np.array([0, 5], np.uint32), np.array([5, 1798], np.uint32),    # cuts 0 and 1798
                np.array([5, 5], np.uint32), np.array([9, 4], np.uint32)]       # equal, descending
    for cuts in bad_sets:
        le = np.full((37, len(cuts) + 1), 0xABABABABABABABAB, np.uint64)
        sums = np.full(37, -77, np.int64)
        for kind in ("host", "device"):
            o_le, o_sums = (le.copy(), sums.copy()) if kind == "host" else (_dev(le.view(np.int64)), _dev(sums))
            with pytest.raises(N.L5dhError) as ei:
                e.le_counts_into(cuts, o_le, o_sums, dense=(rows, totals))
            assert ei.value.code == -22, (cuts, kind)
            assert _raw(o_le) == le.tobytes() and _raw(o_sums) == sums.tobytes(), (cuts, kind)
    # device cuts are checked on the host all the same
    with pytest.raises(N.L5dhError) as ei:
        e.le_counts_into(_dev(np.array([9, 4], np.uint32)), np.zeros((37, 3), np.uint64), dense=(rows, totals))
    assert ei.value.code == -22


# ---- live state ----------------------------------------------------------------------
S, QUIET = 257, range(96, 128)  # 9 tiles, the last of one series; tile 3 receives no sample
CUTS = np.array([1, 2, 3, 6, 11, 26, 28, 29, 51, 101, 193, 262, 332, 743, 1792, 1797], np.uint32)
FIRST, COUNT = 5, 200  # starts and ends inside a tile


def _batch(seed, n):
    rng = np.random.default_rng(seed)
    live = np.array([s for s in range(S) if s not in QUIET], np.uint32)
    series = live[rng.integers(0, live.size, size=n)]
    vals = np.exp(3.0 + 1.5 * rng.standard_normal(n)).astype(np.float32)
    vals[:8] = np.array([0, 1, 2, 113, 3030, 1e9, 3e9, -5], dtype=np.float32)  # smoke()'s edge values
    series[:8] = [256, 6, 31, 32, 204, 150, 200, 33]
    return series, vals


@pytest.fixture(scope="module")
def case(oracle):
    """Two batches (50 k samples), the oracle's state after each and after both."""
    batches = [_batch(1, 30_000), _batch(2, 20_000)]
    refs = []
    for bs in ([batches[0]], [batches[1]], batches):
        ref = oracle.OracleHistograms(S)
        for s, v in bs:
            assert ref.ingest(s, v) == 0
        refs.append((ref.counts().copy(), ref.totals().copy()))
    counts, totals = refs[2]
    assert not counts[list(QUIET)].any() and counts[:, 0].any() and counts[:, 1797].any()
    return dict(batches=batches, each=refs[:2], counts=counts, totals=totals,
                summ=oracle.summarize_counts(counts, totals))


def _fed(case, stage=None):
    e = _engine(S, stage)
    for s, v in case["batches"]:
        e.ingest(s, v)
    return e


@pytest.mark.parametrize("stage", [None, 0])  # the samples still staged / two pending segments
def test_live_several_tiles(oracle, case, stage):
    sl = slice(FIRST, FIRST + COUNT)
    want = le_truth(case["counts"][sl], CUTS)
    with _fed(case, stage) as e:
        le, sums = e.le_counts(CUTS, first=FIRST, count=COUNT)  # reset=False
        assert le.tobytes() == want.tobytes() and sums.tobytes() == case["totals"][sl].tobytes()
        assert not le[QUIET.start - FIRST:QUIET.stop - FIRST].any()
        summ, counts = e.snapshot(reset=False, with_counts=True)  # nothing was touched
        assert counts.tobytes() == case["counts"].tobytes() and summ.tobytes() == case["summ"].tobytes()
        # a bad range or bad cuts with reset = 1: -EINVAL from the library, nothing reset
        lib, buf = N.load(), np.zeros((S, len(CUTS) + 1), np.uint64)
        assert lib.l5dh_le(e._ctx, S - 1, 2, CUTS.ctypes.data, len(CUTS), buf.ctypes.data, None, 0, None, 1) == -22
        desc = CUTS[::-1].copy()
        assert lib.l5dh_le(e._ctx, 0, S, desc.ctypes.data, len(CUTS), buf.ctypes.data, None, 0, None, 1) == -22
        assert not buf.any()
        assert e.snapshot(reset=False, with_counts=True)[1].tobytes() == case["counts"].tobytes()
        # with the series' summaries and the reset of the same range
        le, sums, series = e.le_counts(CUTS, first=FIRST, count=COUNT, reset=True, with_series=True)
        assert le.tobytes() == want.tobytes() and sums.tobytes() == case["totals"][sl].tobytes()
        assert series.tobytes() == case["summ"][sl].tobytes()
        after, counts = e.snapshot(reset=False, with_counts=True)
        expect, tot = case["counts"].copy(), case["totals"].copy()
        expect[sl], tot[sl] = 0, 0
        assert counts.tobytes() == expect.tobytes()
        assert after.tobytes() == oracle.summarize_counts(expect, tot).tobytes()
        le, sums = e.le_counts(CUTS, first=FIRST, count=COUNT)
        assert not le.any() and not sums.any()


def test_live_one_tile_space_includes_sumfix(oracle):
    S1 = 20  # one tile: every batch is folded at ingest, escaped samples' sums stay in sumfix
    rng = np.random.default_rng(5)
    series = rng.integers(0, S1, size=4000, dtype=np.uint32)
    vals = np.exp(3.0 + 2.0 * rng.standard_normal(4000)).astype(np.float32)
    vals[:40] = np.resize(np.array([1e9, 3e9, -5, 2.5e6, 2 ** 21, 2 ** 21 - 2048, 4e6, 1e7], np.float32), 40)
    ref = oracle.OracleHistograms(S1)
    assert ref.ingest(series, vals) == 0
    counts, totals = ref.counts().copy(), ref.totals().copy()
    with _engine(S1) as e:
        e.ingest(series, vals)
        le, sums, summ = e.le_counts(CUTS, with_series=True, reset=True)
        assert le.tobytes() == le_truth(counts, CUTS).tobytes()
        assert sums.tobytes() == totals.tobytes()
        assert summ.tobytes() == oracle.summarize_counts(counts, totals).tobytes()
        assert not e.snapshot(reset=False)["count"].any()


def test_accumulate_two_intervals(case):
    (c0, t0), (c1, t1) = case["each"]
    want = le_truth(c0, CUTS) + le_truth(c1, CUTS)
    want_sums = t0 + t1
    garbage = np.full((S, len(CUTS) + 1), 0xDEADBEEFDEADBEEF, np.uint64)
    for kind in ("host", "device"):
        put = (lambda a: a.copy()) if kind == "host" else _dev
        le, sums = put(garbage.view(np.int64)), put(np.full(S, 12345, np.int64))
        with _engine(S, 0) as e:
            for j, (s, v) in enumerate(case["batches"]):
                e.ingest(s, v)
                # the first interval overwrites the garbage, the second adds to it
                e.le_counts_into(CUTS, le, sums, reset=True, accumulate=j > 0)
                if j == 0:
                    assert _raw(le) == le_truth(c0, CUTS).tobytes() and _raw(sums) == t0.tobytes(), kind
        assert _raw(le) == want.tobytes() and _raw(sums) == want_sums.tobytes(), kind
    # the numpy face: accumulate_into returns the same arrays
    with _engine(S, 0) as e:
        acc = (np.zeros((S, len(CUTS) + 1), np.uint64), np.zeros(S, np.int64))
        for s, v in case["batches"]:
            e.ingest(s, v)
            got = e.le_counts(CUTS, reset=True, accumulate_into=acc)
            assert got[0] is acc[0] and got[1] is acc[1]
        assert acc[0].tobytes() == want.tobytes() and acc[1].tobytes() == want_sums.tobytes()
        # sums wrap like a Java long
        wrap = (np.zeros((1, 2), np.uint64), np.array([2 ** 63 - 1], np.int64))
        rows = np.zeros((1, NB), np.int32)
        rows[0, 3] = 1
        e.le_counts_into(np.array([4], np.uint32), wrap[0], wrap[1], accumulate=True,
                         dense=(rows, np.array([2], np.int64)))
        assert wrap[0].tolist() == [[1, 1]] and wrap[1][0] == -(2 ** 63) + 1


def test_pointer_kinds_give_the_same_bytes(case):
    """Host and device variants of cuts, le_out and sums_out, live and dense."""
    want = le_truth(case["counts"], CUTS).tobytes()
    with _fed(case) as e:
        for dc, dl, ds, src in itertools.product((False, True), (False, True), (False, True), ("live", "dense")):
            cuts = _dev(CUTS) if dc else CUTS
            le = np.zeros((S, len(CUTS) + 1), np.uint64)
            le = _dev(le.view(np.int64)) if dl else le
            sums = _dev(np.zeros(S, np.int64)) if ds else np.zeros(S, np.int64)
            if src == "live":
                e.le_counts_into(cuts, le, sums)
            else:
                e.le_counts_into(cuts, le, sums, dense=(_dev(case["counts"]) if dl else case["counts"], case["totals"]))
            assert _raw(le) == want and _raw(sums) == case["totals"].tobytes(), (dc, dl, ds, src)
        # a host view 4 bytes off 8-byte alignment goes through the staging buffer
        backing = np.zeros(S * (len(CUTS) + 1) * 2 + 2, np.uint32)
        view = backing[1:-1].view(np.uint64) if backing.ctypes.data % 8 == 0 else backing[:-2].view(np.uint64)
        assert view.ctypes.data % 8 == 4
        e.le_counts_into(CUTS, view)
        assert view.tobytes() == want


def test_rollup_linearity(case):
    G = 5
    group = (np.arange(S) % G).astype(np.uint32)
    group[::9] = N.NO_GROUP
    with _fed(case) as e:
        _, g_counts, g_totals = e.rollup(group, G, with_counts=True)
        le, sums = e.le_counts(CUTS)
        got = e.le_counts_dense(g_counts, g_totals, CUTS)
    m = group != N.NO_GROUP
    want, want_sums = np.zeros((G, len(CUTS) + 1), np.uint64), np.zeros(G, np.int64)
    np.add.at(want, group[m], le[m])
    np.add.at(want_sums, group[m], sums[m])
    assert got[0].tobytes() == want.tobytes() and got[1].tobytes() == want_sums.tobytes()


def test_end_to_end_tree_to_prometheus(oracle):
    from linkerd_amd.prometheus import PrometheusTelemeter, line_multiset
    from linkerd_amd.telemetry import MetricsTree, MetricsTreeStatsReceiver, StatEngine, snapshot_histograms_le
    eng = StatEngine(capacity=64, device=0, batch=128)
    eng.enable_le([1, 250, 500, float("inf")])
    tree = MetricsTree(eng)
    stats = MetricsTreeStatsReceiver(tree)
    a = stats.scope("rt", "http", "client", "a").stat("request_latency_ms")
    for interval in ((0.5, 1.0, 3.0, 250.0), (251.0, 497.0, 498.0, 3e9)):
        for v in interval:
            a.add(v)
        assert snapshot_histograms_le(tree, eng) == 1
    lines = line_multiset(PrometheusTelemeter(tree, histograms=eng).render())
    lab = 'rt="http", client="a"'
    top = int(oracle.limits()[1796]) - 1
    for le, n in (("1", 2), ("250", 4), ("497", 6), (str(top), 7), ("+Inf", 8)):
        assert lines[f'rt:client:request_latency_ms_hist_bucket{{{lab}, le="{le}"}} {n}'] == 1, le
    assert lines[f'rt:client:request_latency_ms_hist_count{{{lab}}} 8'] == 1
    assert lines[f'rt:client:request_latency_ms_hist_sum{{{lab}}} {1500 + 2147483647}'] == 1
    assert lines[f'rt:client:request_latency_ms_count{{{lab}}} 4'] == 1  # the summary: the last interval
    eng.engine.close()
