"""Level 1's direct value sums (k_rbin1w): u32 LDS sums under a record-count guard, and
the u64 sums of variant bit 3, bit-exact against the CPU oracle.

A u32 sum takes payloads below 2^17 only (a larger one goes to sumfix with a global
atomic), and the thread that owns a direct half-bin flushes the bin's sums once it
has seen more than 16384 records since the last flush -- so a sum stays below
2 * 16384 * (2^17 - 1) < 2^32.  The cases put one series' samples where a missing or
late flush wraps: whole 16K-slot sub-chunks of one series at the largest u32-path
value, and the values around both thresholds (2^17, V_ESC).
"""
import numpy as np
import pytest

from linkerd_amd import _native as N

pytestmark = pytest.mark.gpu

V_ESC = (1 << 21) - 2048
SUMS = pytest.mark.parametrize("variant", [0, 8], ids=["u32", "u64"])


def _assert_equal(eng, o, reset, label):
    got, counts = eng.snapshot(reset=reset, with_counts=True)
    np.testing.assert_array_equal(counts, o.counts(), err_msg=label)
    want = o.snapshot(reset=reset)
    for f in N.SUMMARY_FIELDS:
        g, w = got[f], want[f]
        same = (g == w) | (np.isnan(g) & np.isnan(w)) if f == "avg" else g == w
        assert same.all(), f"{label} field {f}: series {int(np.flatnonzero(~same)[0])}: " \
                           f"got {g[~same][0]!r} want {w[~same][0]!r}"


def _engine(S, variant, params=()):
    from linkerd_amd.engine import HistogramEngine
    e = HistogramEngine(S)
    e.set_param(N.PARAM_STAGE_SAMPLES, 0)  # every ingest binned at once
    e.set_param(N.PARAM_VARIANT, variant)
    for k, v in params:
        e.set_param(k, v)
    return e


@SUMS
@pytest.mark.parametrize("order", ["runs", "shuffled"])
def test_u32_guard_one_hot_series(oracle, variant, order):
    """One direct series: 2^20 samples of 131071 and 2^16 of 131072 in one batch of two
    slabs, over a thin uniform background.  Its exact sum, 1.46e11, is 34 x 2^32, and
    each slab's share 17 x 2^32; "runs" leaves the hot samples contiguous, so whole
    sub-chunks go to one half-bin at 16384 x 131071 per sub-chunk (the guard's bound
    exactly); sum and avg are compared bitwise."""
    rng = np.random.default_rng(41)
    S, hot = 4096, 47 * 32 + 21  # a series of a tile's upper half
    nb = 1 << 17
    series = np.concatenate([np.full((1 << 20) + (1 << 16), hot, np.uint32),
                             rng.integers(0, S, size=nb, dtype=np.uint32)])
    vals = np.concatenate([np.full(1 << 20, 131071.0, np.float32), np.full(1 << 16, 131072.0, np.float32),
                           np.exp(3.0 + rng.standard_normal(nb)).astype(np.float32)])
    if order == "shuffled":
        p = rng.permutation(series.size)
        series, vals = series[p], vals[p]
    o = oracle.OracleHistograms(S)
    o.ingest(series, vals)
    assert int(o.snapshot(reset=False)["sum"][hot]) > 30 << 32
    with _engine(S, variant, [(N.PARAM_MAX_SLABS, 2)]) as eng:
        eng.ingest(series, vals)
        _assert_equal(eng, o, True, f"hot {order}")


def _skewed(rng, S, n, tile):
    """Three series of one tile hold ~60 % of the samples, the rest are uniform; the
    values include every class level 1 tells apart."""
    hot = tile * 32 + np.array([1, 16, 31], np.uint32)
    series = rng.integers(0, S, size=n, dtype=np.uint32)
    m = rng.random(n) < 0.6
    series[m] = hot[rng.integers(0, 3, size=int(m.sum()))]
    vals = np.exp(4.0 + 1.5 * rng.standard_normal(n)).astype(np.float32)
    edge = np.array([0.0, -0.0, -7.5, np.nan, np.inf, 131071.0, 131071.5, 131072.0, V_ESC - 1, V_ESC - 0.5, V_ESC,
                     2.0 ** 31], np.float32)
    pos = rng.choice(n, size=n // 8, replace=False)
    vals[pos] = edge[rng.integers(0, edge.size, size=pos.size)]
    return series, vals


@SUMS
@pytest.mark.parametrize("regime", ["default", "redo", "nodirect"])
def test_skewed_batch_threshold_values(oracle, variant, regime):
    """S = 4096, N = 2^21, four slabs; with regions at 40 % of the plan level 1 is redone
    (the redo pass adds nothing to any sum: nothing is counted twice); with no direct
    tiles every value in [2^17, V_ESC) stays in its record for level 2."""
    rng = np.random.default_rng(43)
    S, n = 4096, 1 << 21
    series, vals = _skewed(rng, S, n, tile=77)
    params = [(N.PARAM_MAX_SLABS, 4)] + {"default": [], "redo": [(N.PARAM_REGION_PCT, 40)],
                                         "nodirect": [(N.PARAM_DIRECT_MAX, 0)]}[regime]
    o = oracle.OracleHistograms(S)
    with _engine(S, variant, params) as eng:
        r0 = eng.partition_redos()[0]
        eng.ingest(series, vals)
        o.ingest(series, vals)
        _assert_equal(eng, o, True, f"skewed {regime}")
        if regime == "redo":
            assert eng.partition_redos()[0] > r0


@SUMS
def test_two_segments_moving_hot_tile(oracle, variant):
    """Two ingests (two segments) with the hot tile different in each, a non-resetting
    snapshot, a third ingest and a resetting snapshot."""
    rng = np.random.default_rng(47)
    S, n = 4096, 1 << 19
    o = oracle.OracleHistograms(S)
    with _engine(S, variant, [(N.PARAM_MAX_SLABS, 3), (N.PARAM_MAX_SEGMENTS, 2)]) as eng:
        for tile in (5, 99):
            b = _skewed(rng, S, n, tile)
            eng.ingest(*b)
            o.ingest(*b)
        _assert_equal(eng, o, False, "two segments")
        b = _skewed(rng, S, n, 127)
        eng.ingest(*b)
        o.ingest(*b)
        _assert_equal(eng, o, True, "third ingest")
        np.testing.assert_array_equal(eng.tile_totals(), np.bincount(b[0] >> 5, minlength=S // 32).astype(np.uint64))
