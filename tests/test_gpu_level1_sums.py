"""Level 1's direct value sums (k_rbin1w): u32 LDS sums under a record-count guard,
bit-exact against the CPU oracle; and the far ends of the kernel's LDS arrays.

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


def _u32(*cases):
    """Case ids with the sums' width, which these cases pin, after the case's own name."""
    return [f"{c}-u32" for c in cases]


def _assert_equal(eng, o, reset, label):
    got, counts = eng.snapshot(reset=reset, with_counts=True)
    np.testing.assert_array_equal(counts, o.counts(), err_msg=label)
    want = o.snapshot(reset=reset)
    for f in N.SUMMARY_FIELDS:
        g, w = got[f], want[f]
        same = (g == w) | (np.isnan(g) & np.isnan(w)) if f == "avg" else g == w
        assert same.all(), f"{label} field {f}: series {int(np.flatnonzero(~same)[0])}: " \
                           f"got {g[~same][0]!r} want {w[~same][0]!r}"


def _engine(S, params=()):
    from linkerd_amd.engine import HistogramEngine
    e = HistogramEngine(S)
    e.set_param(N.PARAM_STAGE_SAMPLES, 0)  # every ingest binned at once
    for k, v in params:
        e.set_param(k, v)
    return e


@pytest.mark.parametrize("order", ["runs", "shuffled"], ids=_u32("runs", "shuffled"))
def test_u32_guard_one_hot_series(oracle, order):
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
    with _engine(S, [(N.PARAM_MAX_SLABS, 2)]) as eng:
        eng.ingest(series, vals)
        _assert_equal(eng, o, True, f"hot {order}")


def _skewed(rng, S, n, tile):
    """Three series of one tile hold ~60 % of the samples, the rest are uniform; the
    values include every class level 1 tells apart."""
    hot = tile * 32 + np.array([1, 16, 31], np.uint32)
    series = rng.integers(0, S, size=n, dtype=np.uint32)
    m = rng.random(n) < 0.6
    series[m] = hot[rng.integers(0, 3, size=int(m.sum()))]
    return series, _values(rng, n)


def _values(rng, n):
    """Lognormal values, an eighth of them replaced by the edges of level 1's value classes."""
    vals = np.exp(4.0 + 1.5 * rng.standard_normal(n)).astype(np.float32)
    edge = np.array([0.0, -0.0, -7.5, np.nan, np.inf, 131071.0, 131071.5, 131072.0, V_ESC - 1, V_ESC - 0.5, V_ESC,
                     2.0 ** 31], np.float32)
    pos = rng.choice(n, size=n // 8, replace=False)
    vals[pos] = edge[rng.integers(0, edge.size, size=pos.size)]
    return vals


@pytest.mark.parametrize("regime", ["default", "redo", "nodirect"], ids=_u32("default", "redo", "nodirect"))
def test_skewed_batch_threshold_values(oracle, regime):
    """S = 4096, N = 2^21, four slabs; with regions at 40 % of the plan level 1 is redone
    (the redo pass adds nothing to any sum: nothing is counted twice); with no direct
    tiles every value in [2^17, V_ESC) stays in its record for level 2."""
    rng = np.random.default_rng(43)
    S, n = 4096, 1 << 21
    series, vals = _skewed(rng, S, n, tile=77)
    params = [(N.PARAM_MAX_SLABS, 4)] + {"default": [], "redo": [(N.PARAM_REGION_PCT, 40)],
                                         "nodirect": [(N.PARAM_DIRECT_MAX, 0)]}[regime]
    o = oracle.OracleHistograms(S)
    with _engine(S, params) as eng:
        r0 = eng.partition_redos()[0]
        eng.ingest(series, vals)
        o.ingest(series, vals)
        _assert_equal(eng, o, True, f"skewed {regime}")
        if regime == "redo":
            assert eng.partition_redos()[0] > r0


def test_two_segments_moving_hot_tile(oracle):
    """Two ingests (two segments) with the hot tile different in each, a non-resetting
    snapshot, a third ingest and a resetting snapshot."""
    rng = np.random.default_rng(47)
    S, n = 4096, 1 << 19
    o = oracle.OracleHistograms(S)
    with _engine(S, [(N.PARAM_MAX_SLABS, 3), (N.PARAM_MAX_SEGMENTS, 2)]) as eng:
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


def _rows_equal(got, want, label):
    for f in N.SUMMARY_FIELDS:
        g, w = got[f], want[f]
        same = (g == w) | (np.isnan(g) & np.isnan(w)) if f == "avg" else g == w
        assert same.all(), f"{label} field {f}: row {int(np.flatnonzero(~same)[0])}: " \
                           f"got {g[~same][0]!r} want {w[~same][0]!r}"


@pytest.mark.parametrize("S,dmax", [(1 << 20, 251), (505 * 2048, 255)], ids=["FS512", "FS505"])
def test_layout_far_ends(oracle, S, dmax):
    """The largest plans level 1 can get: every direct tile the bin space has room for (dmax =
    (1024 - 9 - FS) / 2 with FS = F / 64 super-tile bins), among them tiles 0, 31, 32 and the
    last of the space.  FS512: F = 32768, 251 direct tiles, trash bin 1014 -- the last word and
    bit of the direct bitmap, the last super-tile.  FS505: F = 32320, 255 direct tiles, trash
    bin 1015 -- the largest bin index there is, and all 255 x 32 direct sums.

    The number of direct tiles is not observable from Python; it follows from k_rplan1's rule.
    A batch below 2^18 samples is sampled whole, so the plan is exact: with every hot tile's
    count in one power-of-two range, the direct tiles are the tiles of at least n // 8192
    records -- which the test asserts of its input to be exactly the dmax hot tiles."""
    rng = np.random.default_rng(53)
    F, nbg = S // 32, 1 << 16
    assert S % 2048 == 0 and dmax == (1024 - 9 - F // 64) // 2
    fixed = np.array([0, 31, 32, F - 1])
    rest = np.setdiff1d(np.arange(F), fixed)
    hot = np.sort(np.concatenate([fixed, rng.choice(rest, size=dmax - fixed.size, replace=False)]))
    series = np.concatenate([(hot[:, None] * 32 + np.arange(640)[None, :] % 32).ravel(),
                             rng.integers(0, S, size=nbg)]).astype(np.uint32)
    n = series.size
    assert n < 1 << 18
    vals = _values(rng, n)
    p = rng.permutation(n)
    series, vals = series[p], vals[p]
    per_tile = np.bincount(series >> 5, minlength=F)
    thr_min = n // 8192
    assert (per_tile >= thr_min).sum() == dmax and (per_tile[hot] >= thr_min).all()
    assert per_tile[hot].min() >= 512 and per_tile[hot].max() < 1024  # one power-of-two range
    cold = np.ones(F, bool)
    cold[hot] = False
    assert per_tile[cold].max() < thr_min

    # the oracle over the touched series only
    touched = np.unique(series)
    o = oracle.OracleHistograms(touched.size)
    cs = np.searchsorted(touched, series).astype(np.uint32)
    with _engine(S, [(N.PARAM_MAX_SLABS, 4)]) as eng:
        eng.ingest(series, vals)
        o.ingest(cs, vals)
        np.testing.assert_array_equal(eng.tile_totals(), per_tile.astype(np.uint64))
        got = eng.snapshot(reset=True)
        _rows_equal(got[touched], o.snapshot(reset=True), "full range")
        untouched = np.ones(S, bool)
        untouched[touched] = False
        assert not got["count"][untouched].any()

        eng.ingest(series, vals)
        o.ingest(cs, vals)
        want = o.snapshot(reset=False)
        bg_only = int(np.flatnonzero(cold & (per_tile > 0))[0])
        for tile in dict.fromkeys([int(hot[0]), int(hot[-1]), F - 1, bg_only]):
            rows, counts = eng.snapshot(first=tile * 32, count=32, reset=False, with_counts=True)
            ids = np.arange(tile * 32, tile * 32 + 32)
            at = np.searchsorted(touched, ids)
            hit = touched[np.minimum(at, touched.size - 1)] == ids
            assert hit.any()
            np.testing.assert_array_equal(counts[hit], o.h["counts"][at[hit]], err_msg=f"tile {tile}")
            assert not counts[~hit].any() and not rows["count"][~hit].any()
            _rows_equal(rows[hit], want[at[hit]], f"tile {tile}")
