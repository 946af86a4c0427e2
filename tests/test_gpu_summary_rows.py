"""The summary stage (wave_summary) pinned at each of its call sites with the crafted
rows of tests/summary_rows.py: staircases that put every percentile target on its own
bucket, runs over every lane and group boundary, counts up to 2^31 - 1 per bucket (4-bin
group sums past 2^32, row counts past 2^41) and totals that round in avg's (double).

All 11 summary fields, the dense counts and the totals are compared bytewise with the
CPU oracle (oracle.summarize_counts); tests/test_summary_rows.py shows on the CPU that
the rows expose what they claim.

Not reachable here: a state row (u32 buckets) whose group sums pass 2^32 takes 2^32
ingested samples.  The state-row sites (k_hot_finish, k_rows, the dirty emit_series) build
their group sums with the same WideSums code as the external-row sites tested below.
"""
import numpy as np
import pytest

from linkerd_amd import _native as N
from tests import summary_rows as R

pytestmark = pytest.mark.gpu

NB = R.NB
ITEMS = pytest.mark.parametrize("item", [None, 1], ids=["item_default", "item_1"])


def _assert_summaries_equal(got, want, label=""):
    for f in N.SUMMARY_FIELDS:
        g, w = got[f], want[f]
        if f == "avg":
            bad = ~((g == w) | (np.isnan(g) & np.isnan(w)))
        else:
            bad = g != w
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError(f"{label} field {f}: {int(bad.sum())} mismatches; first row {i}: "
                                 f"got {g[i]!r} want {w[i]!r}\n got={got[i]}\nwant={want[i]}")
    assert got.tobytes() == want.tobytes(), label


def _engine(S, params=None, stage=0):
    from linkerd_amd.engine import HistogramEngine
    e = HistogramEngine(S)
    if stage is not None:
        e.set_param(N.PARAM_STAGE_SAMPLES, stage)
    for k, v in (params or {}).items():
        e.set_param(k, v)
    return e


# ---------------------------------------------------------------- dense entry points

@pytest.fixture(scope="module")
def dense(oracle):
    rows, totals = R.dense_rows()
    want = oracle.summarize_counts(rows, totals, threads=8)
    for a in (rows, totals, want):
        a.setflags(write=False)
    return rows, totals, want


def test_summarize_dense_numpy_and_device(dense):
    import torch
    rows, totals, want = dense
    with _engine(64) as e:
        _assert_summaries_equal(e.summarize_dense(rows, totals), want, "summarize_dense numpy")
        dev = torch.device("cuda", e.device)
        d_rows, d_totals = torch.from_numpy(rows.copy()).to(dev), torch.from_numpy(totals.copy()).to(dev)
        out = torch.full((rows.shape[0] * 11,), -1, dtype=torch.int64, device=dev)
        e.summarize_dense(d_rows, d_totals, out=out)
        torch.cuda.synchronize()
        _assert_summaries_equal(out.cpu().numpy().view(N.SUMMARY_DTYPE), want, "summarize_dense device")


@ITEMS
def test_rollup_dense_singleton_groups_are_the_rows(dense, item):
    """group[i] = i: each group is its one row, finished by its only k_ru_accum item."""
    rows, totals, want = dense
    n = rows.shape[0]
    with _engine(64, {N.PARAM_ROLLUP_ITEM: item} if item else None) as e:
        summ, counts, tot = e.rollup_dense(rows, totals, np.arange(n, dtype=np.uint32), n, with_counts=True)
        np.testing.assert_array_equal(counts, rows)
        np.testing.assert_array_equal(tot, totals)
        _assert_summaries_equal(summ, want, f"rollup_dense singletons item={item}")


@ITEMS
@pytest.mark.parametrize("size", [2, 3])
def test_rollup_dense_groups_of_staircase_rows(oracle, item, size):
    """Groups of 2 and 3 consecutive staircase rows against the summed rows (with one
    member per item they are summed by k_ru_finish); the last group's members add up to
    2^31 - 2 (pairs) and 2^31 - 1 (triples) in EVERY bucket: group sums of 2^33 - 4."""
    rows = np.concatenate([R.staircase_rows(), np.full((2, NB), 2 ** 30, np.int32)])
    rows[-1] -= 2
    contrib = R.BUCKET_VALUES.astype(np.int64)
    contrib[-1] = R.INT_MAX
    totals = np.concatenate([np.cumsum(contrib), [2 ** 53 + 1, -7]])
    group = (np.arange(rows.shape[0]) // size).astype(np.uint32)
    G = int(group[-1]) + 1
    gc = np.zeros((G, NB), np.int64)
    gt = np.zeros(G, np.int64)
    np.add.at(gc, group, rows)
    np.add.at(gt, group, totals)
    assert gc.max() == 2 ** 31 - 4 + size and (gc[-1] == gc.max()).all()
    want = oracle.summarize_counts(gc.astype(np.int32), gt)
    with _engine(64, {N.PARAM_ROLLUP_ITEM: item} if item else None) as e:
        summ, counts, tot = e.rollup_dense(rows, totals, group, G, with_counts=True)
        np.testing.assert_array_equal(counts, gc)
        np.testing.assert_array_equal(tot, gt)
        _assert_summaries_equal(summ, want, f"rollup_dense groups of {size} item={item}")


# ---------------------------------------------------------------- live paths

@pytest.fixture(scope="module")
def live(oracle):
    """S = 1798: series n - 1 receives BUCKET_VALUES[:n] (1 617 301 samples, shuffled);
    the oracle's truth for one ingest of the batch and for two."""
    series, values = R.staircase_series()
    o = oracle.OracleHistograms(NB)
    assert o.ingest(series, values, threads=8) == 0
    counts, totals = o.counts(), o.totals()
    np.testing.assert_array_equal(counts, R.staircase_rows())
    want = o.snapshot(reset=False)
    want2 = oracle.summarize_counts(2 * counts, 2 * totals, threads=8)
    for a in (series, values, counts, totals, want, want2):
        a.setflags(write=False)
    return dict(series=series, values=values, counts=counts, totals=totals, want=want, want2=want2)


def _snap(e, live, reset, with_counts, times, label):
    """A whole-range snapshot checked against the batch ingested `times` times."""
    want = live["want"] if times == 1 else live["want2"]
    if with_counts:
        got, counts = e.snapshot(reset=reset, with_counts=True)
        np.testing.assert_array_equal(counts, times * live["counts"], err_msg=label)
    else:
        got = e.snapshot(reset=reset)
    _assert_summaries_equal(got, want, label)


BIG = {N.PARAM_COLD_LIMIT: 500}  # every tile of the staircase (>= 528 records) takes the big-tile path
SITES = {
    # default parameters: cold half-tiles, the 32-bit linear path (reset, dense rows)
    "cold_linear": (None, [(True, True)]),
    # emit_series: clean with kept state, then the same batch again over the dirty rows
    "emit_keep_dirty": (None, [(False, True), (True, True)]),
    "emit_keep_keep": (None, [(False, True), (False, True)]),
    # the branches without a dense row
    "no_counts_reset": (None, [(True, False)]),
    "no_counts_dirty": (None, [(False, False), (True, False)]),
    # big tiles whose halves are one item each write their rows themselves (TF_SOLO);
    # halves above the item size the engine derives from the load go through k_hot_finish
    "solo": ({**BIG, N.PARAM_HOT_CHUNK: 1 << 20}, [(True, True)]),
    # the smallest chunk: several items per half, k_hot_finish over the output rows ...
    "hot_finish_out": ({**BIG, N.PARAM_HOT_CHUNK: 1024}, [(True, True)]),
    # ... and over the state rows, clean and then dirty
    "hot_finish_state": ({**BIG, N.PARAM_HOT_CHUNK: 1024}, [(False, True), (True, True)]),
    "hot_finish_state_no_counts": ({**BIG, N.PARAM_HOT_CHUNK: 1024}, [(False, False), (False, False)]),
}


@pytest.mark.parametrize("site", list(SITES))
def test_live_snapshot_sites(live, site):
    params, snaps = SITES[site]
    with _engine(NB, params) as e:
        for times, (reset, with_counts) in enumerate(snaps, 1):
            e.ingest(live["series"], live["values"])
            _snap(e, live, reset, with_counts, times, f"{site} snapshot {times}")
        after = e.snapshot(reset=False)
        if snaps[-1][0]:
            assert not after["count"].any() and not after["sum"].any()
        else:
            _assert_summaries_equal(after, live["want"] if len(snaps) == 1 else live["want2"], f"{site} after")


@pytest.mark.parametrize("params", [None, {**BIG, N.PARAM_HOT_CHUNK: 1024}], ids=["cold", "big"])
def test_range_snapshot_of_state_rows(live, params):
    """k_rows over state rows: series 1000..1100 (inside tiles at both ends)."""
    a, n = 1000, 101
    with _engine(NB, params) as e:
        e.ingest(live["series"], live["values"])
        got, counts = e.snapshot(first=a, count=n, reset=False, with_counts=True)
        np.testing.assert_array_equal(counts, live["counts"][a:a + n])
        _assert_summaries_equal(got, live["want"][a:a + n], "range")
        _assert_summaries_equal(e.snapshot(first=a, count=n, reset=True), live["want"][a:a + n], "range, no counts")
        rest = e.snapshot(reset=False)
        assert not rest["count"][a:a + n].any()
        _assert_summaries_equal(rest[:a], live["want"][:a], "below the range")
        _assert_summaries_equal(rest[a + n:], live["want"][a + n:], "above the range")


@pytest.mark.parametrize("variant", [0, 1], ids=["fold1", "fold1_u16"])
def test_one_tile_fold_then_rows(oracle, variant):
    """S = 32: k_fold1 folds the batch into the state rows, k_rows summarizes them."""
    series, values = R.staircase_series(R.FOLD_ROWS)
    o = oracle.OracleHistograms(32)
    assert o.ingest(series, values) == 0
    counts = o.counts()
    for i, n in enumerate(R.FOLD_ROWS):
        assert (counts[i, :n] == 1).all() and not counts[i, n:].any()
    want = o.snapshot(reset=False)
    with _engine(32, {N.PARAM_VARIANT: variant}) as e:
        e.ingest(series, values)
        got, c = e.snapshot(reset=False, with_counts=True)
        np.testing.assert_array_equal(c, counts)
        _assert_summaries_equal(got, want, "fold")
        e.ingest(series, values)
        got, c = e.snapshot(reset=True, with_counts=True)
        np.testing.assert_array_equal(c, 2 * counts)
        _assert_summaries_equal(got, oracle.summarize_counts(2 * counts, 2 * o.totals()), "fold twice")


@ITEMS
@pytest.mark.parametrize("size", [1, 2], ids=["singletons", "pairs"])
def test_live_rollup(oracle, live, item, size):
    group = (np.arange(NB) // size).astype(np.uint32)
    G = int(group[-1]) + 1
    gc = np.zeros((G, NB), np.int64)
    gt = np.zeros(G, np.int64)
    np.add.at(gc, group, live["counts"])
    np.add.at(gt, group, live["totals"])
    want = oracle.summarize_counts(gc.astype(np.int32), gt, threads=8)
    with _engine(NB, {N.PARAM_ROLLUP_ITEM: item} if item else None) as e:
        e.ingest(live["series"], live["values"])
        summ, counts, tot, series = e.rollup(group, G, with_counts=True, with_series=True)
        np.testing.assert_array_equal(counts, gc)
        np.testing.assert_array_equal(tot, gt)
        _assert_summaries_equal(summ, want, f"live rollup size={size} item={item}")
        _assert_summaries_equal(series, live["want"], "series of the rollup")


@pytest.mark.parametrize("mode", [N.MERGE_REDUCE_SCATTER, N.MERGE_ALL_REDUCE], ids=["reduce_scatter", "all_reduce"])
@pytest.mark.parametrize("W", [2, 3])
def test_loopback_merge_decodes_the_staircase(live, W, mode):
    """Sample i on rank i mod W: every merged row is a staircase row again (k_mdecode
    for the reduce-scatter's slices, the dense rows' summary for the all-reduce)."""
    from linkerd_amd.engine import HistogramEngine
    engines = [_engine(NB, stage=None) for _ in range(W)]
    try:
        HistogramEngine.comm_init_loopback(engines)
        for r, e in enumerate(engines):
            e.ingest(live["series"][r::W], live["values"][r::W])
        per = -(-NB // W)
        for r, (first, count, summ, cnt, tot) in enumerate(HistogramEngine.merge_all(engines, mode, with_counts=True)):
            if mode == N.MERGE_REDUCE_SCATTER:
                assert (first, count) == (min(r * per, NB), max(0, min(per, NB - r * per)))
            else:
                assert (first, count) == (0, NB)
            sl = slice(first, first + count)
            np.testing.assert_array_equal(cnt, live["counts"][sl])
            np.testing.assert_array_equal(tot, live["totals"][sl])
            _assert_summaries_equal(summ, live["want"][sl], f"merge W={W} rank {r}")
    finally:
        for e in engines:
            e.close()
