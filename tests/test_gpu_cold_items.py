"""Every emission form of the cold accumulate kernels, reached on purpose.

The dense snapshot kernel and the fleet merge's sparse export kernel emit a cold
half-tile item in four forms: dense linear (a clean, whole, even-aligned half of a
resetting snapshot with counts), dense rows (every other dense case: a ragged half,
no counts, kept state, dirty rows, a fold), sparse clean (first-touch lists, or the
whole bin row past ENC_LIST = 256 touches) and sparse dirty.  The other GPU tests meet
them through Zipf workloads of 10^5..10^6 samples; here the shape is the smallest that
still takes each one, and the preconditions that make it so are asserted from the CPU
oracle's counts, not hoped for.

S = 72 is three tiles (not the one-tile fold); tile 2 holds 8 series, so its half 0
is ragged and its half 1 lies wholly past S.  Series WIDE has one sample at each of
1..474, the smallest such range with more than 256 non-empty buckets (257); every
other series stays far below 256.  The staging ring is off, so one ingest is one
segment.  Every comparison is byte for byte with the oracle.
"""
import numpy as np
import pytest

from linkerd_amd import _native as N

pytestmark = pytest.mark.gpu

S, TILE = 72, 32
WIDE, WIDE_TOP = 5, 474
EMPTY = 70
ENC_LIST = 256
COLD_LIMIT = 65535
FIRST, COUNT = 16, 40


def _oracle(oracle, parts):
    o = oracle.OracleHistograms(S)
    for s, v in parts:
        assert o.ingest(s, v) == 0
    return dict(counts=o.counts(), totals=o.totals(), summ=o.snapshot(reset=False))


def _cold_preconditions(counts, what):
    per_tile = np.add.reduceat(counts.sum(axis=1, dtype=np.int64), np.arange(0, S, TILE))
    assert per_tile.size == 3 and (per_tile > 0).all() and (per_tile < COLD_LIMIT).all(), f"{what}: every tile cold"
    nonempty = (counts > 0).sum(axis=1)
    assert nonempty[WIDE] > ENC_LIST, f"{what}: the wide row has {nonempty[WIDE]} non-empty buckets"
    assert (np.delete(nonempty, WIDE) <= ENC_LIST).all(), f"{what}: only the wide row passes the list"


@pytest.fixture(scope="module")
def case(oracle):
    """The batch, its two-segment and two-rank splits and the oracle's results, computed once."""
    rng = np.random.default_rng(17)
    narrow_ids = np.array([s for s in range(S) if s not in (WIDE, EMPTY)], dtype=np.uint32)
    series = np.repeat(narrow_ids, 40)
    vals = np.exp(3.0 + rng.standard_normal(series.size)).astype(np.float32)
    # escapes, zero and a negative value in every tile half that has series (smoke()'s edge values)
    edge_s = np.array([71, 0, 31, 32, 63, 64, 69, 33], dtype=np.uint32)
    edge_v = np.array([0, 1, 2, 113, 3030, 1e9, 3e9, -5], dtype=np.float32)
    series, vals = np.concatenate([series, edge_s]), np.concatenate([vals, edge_v])
    wide = (np.full(WIDE_TOP, WIDE, np.uint32), np.arange(1, WIDE_TOP + 1, dtype=np.float32))

    def shuffled(s, v):
        p = rng.permutation(s.size)
        return s[p], v[p]

    batch = shuffled(np.concatenate([series, wide[0]]), np.concatenate([vals, wide[1]]))
    assert 2000 < batch[0].size < 5000
    # the fleet: the narrow samples dealt to two ranks, the wide series whole on rank 0
    ranks = [shuffled(np.concatenate([series[0::2], wide[0]]), np.concatenate([vals[0::2], wide[1]])),
             (series[1::2], vals[1::2])]
    once = _oracle(oracle, [batch])
    twice = _oracle(oracle, [batch, batch])
    _cold_preconditions(once["counts"], "the batch")
    _cold_preconditions(_oracle(oracle, [ranks[0]])["counts"], "rank 0")
    assert once["counts"][EMPTY].sum() == 0 and once["counts"][64:].sum() > 0
    fleet = _oracle(oracle, ranks)
    assert fleet["counts"].tobytes() == once["counts"].tobytes() and fleet["totals"].tobytes() == once["totals"].tobytes()
    return dict(batch=batch, ranks=ranks, once=once, twice=twice)


def _engine():
    from linkerd_amd.engine import HistogramEngine
    e = HistogramEngine(S)
    e.set_param(N.PARAM_STAGE_SAMPLES, 0)  # one ingest, one segment
    e.set_param(N.PARAM_MAX_SEGMENTS, 2)
    return e


def _ingest(e, part, nseg):
    s, v = part
    h = s.size // 2
    for sl in ([slice(None)] if nseg == 1 else [slice(0, h), slice(h, None)]):
        e.ingest(s[sl], v[sl])


def _same(got, want, what, rows=slice(None)):
    for k, g in got.items():
        if g is not None:
            assert g.tobytes() == want[k][rows].tobytes(), f"{what}: {k} differ from the oracle"


NSEG = pytest.mark.parametrize("nseg", [1, 2], ids=["one_segment", "two_segments"])


@NSEG
def test_reset_with_counts(case, nseg):
    """Dense linear form (tiles 0 and 1); tile 2's ragged half through the row form."""
    with _engine() as e:
        _ingest(e, case["batch"], nseg)
        summ, counts = e.snapshot(reset=True, with_counts=True)
        _same(dict(summ=summ, counts=counts), case["once"], "reset, counts")
        after, counts = e.snapshot(reset=True, with_counts=True)
        assert not counts.any() and not after["count"].any() and not after["sum"].any()


@NSEG
def test_reset_without_counts(case, nseg):
    with _engine() as e:
        _ingest(e, case["batch"], nseg)
        _same(dict(summ=e.snapshot(reset=True)), case["once"], "reset, no counts")
        _ingest(e, case["batch"], nseg)  # the LDS rows were cleared: the same again
        summ, counts = e.snapshot(reset=True, with_counts=True)
        _same(dict(summ=summ, counts=counts), case["once"], "reset, second interval")


@NSEG
def test_kept_state_then_dirty_rows(case, nseg):
    with _engine() as e:
        _ingest(e, case["batch"], nseg)
        summ, counts = e.snapshot(reset=False, with_counts=True)
        _same(dict(summ=summ, counts=counts), case["once"], "kept state")
        _ingest(e, case["batch"], nseg)
        summ, counts = e.snapshot(reset=True, with_counts=True)
        _same(dict(summ=summ, counts=counts), case["twice"], "dirty rows")
        assert not e.snapshot(reset=True)["count"].any()


@NSEG
def test_range_snapshot_after_pending_segment(case, nseg):
    """The pending segments are folded into the state rows (no emission), then read."""
    with _engine() as e:
        _ingest(e, case["batch"], nseg)
        summ, counts = e.snapshot(first=FIRST, count=COUNT, reset=False, with_counts=True)
        _same(dict(summ=summ, counts=counts), case["once"], "range", slice(FIRST, FIRST + COUNT))
        summ, counts = e.snapshot(reset=True, with_counts=True)
        _same(dict(summ=summ, counts=counts), case["once"], "whole range after the fold")


@NSEG
def test_export_state_whole_range(case, nseg):
    with _engine() as e:
        _ingest(e, case["batch"], nseg)
        counts, totals = e.export_state(reset=True)
        _same(dict(counts=counts, totals=totals), case["once"], "export")
        assert not e.snapshot(reset=False)["count"].any()


@pytest.mark.parametrize("mode", [N.MERGE_REDUCE_SCATTER, N.MERGE_ALL_REDUCE], ids=["reduce_scatter", "all_reduce"])
def test_two_rank_loopback_merge(case, mode):
    """Interval 0, clean: the list form, the whole-row form (WIDE on rank 0) and, with
    rank 0's two segments, half 1's base summed over segments.  Interval 1: half of each
    rank's samples folded first, so every tile is dirty under new records."""
    from linkerd_amd.engine import HistogramEngine
    engines = [_engine() for _ in range(2)]
    try:
        HistogramEngine.comm_init_loopback(engines)
        for interval in range(2):
            for r, e in enumerate(engines):
                s, v = case["ranks"][r]
                if interval == 1:
                    h = s.size // 2
                    e.ingest(s[:h], v[:h])
                    e.snapshot(reset=False)
                    e.ingest(s[h:], v[h:])
                else:
                    _ingest(e, (s, v), 2 if r == 0 else 1)
            res = HistogramEngine.merge_all(engines, mode, with_counts=True)
            per = -(-S // 2)
            for r, (first, count, summ, cnt, tot) in enumerate(res):
                assert (first, count) == ((r * per, per) if mode == N.MERGE_REDUCE_SCATTER else (0, S))
                _same(dict(summ=summ, counts=cnt, totals=tot), case["once"], f"interval {interval} rank {r}",
                      slice(first, first + count))
            for e in engines:
                assert not e.snapshot(reset=False)["count"].any()
    finally:
        for e in engines:
            e.close()
