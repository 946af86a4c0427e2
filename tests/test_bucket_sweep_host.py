"""Properties of the bucket-edge sweep (tests/bucket_sweep.py) that the GPU cases rely on,
and its expected answer stated twice: by the C oracle and by plain numpy
(bincount(searchsorted(limits, trunc(v), "right"))).  No GPU."""
import numpy as np

from tests import bucket_sweep as BS


def test_limits_are_the_oracles(oracle):
    np.testing.assert_array_equal(BS.limits(), oracle.limits())


def test_sets_are_what_they_say():
    sw = BS.sweep()
    assert sw.dense.size == BS.DENSE_END + 1 and sw.dense[-1] == 2.0 ** 21 + 2048
    np.testing.assert_array_equal(sw.dense.astype(np.int64), np.arange(sw.dense.size))  # all exact
    assert sw.near.size > 5 * 1790 and (sw.near < 2.0 ** 31).all()
    L = BS.limits()
    lo = L[L < (1 << 23)]
    np.testing.assert_array_equal(BS.java_f2l(sw.half), lo - 1)  # truncation, not rounding
    assert (sw.half.astype(np.float64) == lo - 0.5).all()
    bits = sw.all.view(np.uint32)
    assert np.unique(bits).size == bits.size
    for x in (-0.0, -2.0 ** 31 - 256, 2.0 ** 32 + 2.0 ** 9, 2.0 ** 63, -2.0 ** 64, 3e38, 2.0 ** -149, 2137204091.0):
        assert np.float32(x).view(np.uint32) in bits, x
    assert np.isnan(sw.wild).any() and np.isinf(sw.wild).sum() == 2


def test_every_bucket_touched_every_limit_tight():
    sw = BS.sweep()
    L = BS.limits()
    b = BS.expected_bucket(sw.core)
    assert np.unique(b).size == BS.NLIMITS + 1, "a bucket no value of the sweep maps to"
    # both float32 values next to each limit: the greatest below it and the least at or above it
    f = L.astype(np.float32)
    at_or_above = np.where(f.astype(np.float64) >= L, f, np.nextafter(f, np.float32(np.inf)))
    below = np.nextafter(at_or_above, np.float32(-np.inf))
    assert (at_or_above.astype(np.float64) >= L).all() and (below.astype(np.float64) < L).all()
    have = set(sw.core.view(np.uint32).tolist())
    assert all(int(x) in have for x in at_or_above.view(np.uint32)), "a limit not approached from above"
    assert all(int(x) in have for x in below.view(np.uint32)), "a limit not approached from below"
    # and they do fall on the two sides
    i = np.arange(L.size)
    np.testing.assert_array_equal(BS.expected_bucket(at_or_above), i + 1)
    np.testing.assert_array_equal(BS.expected_bucket(below), i)


def test_value_classes_of_level1():
    """Level 1 tells three classes apart: payloads below 2^17 (u32 LDS sums on a direct tile),
    [2^17, V_ESC) (the slow route's sumfix on a direct tile, the record's payload elsewhere),
    and V_ESC up (escaped)."""
    sw = BS.sweep()
    t = BS.java_f2l(sw.core)
    assert (t >= 0).all()
    small = int((t < BS.DSUM_PMAX).sum())
    mid = int(((t >= BS.DSUM_PMAX) & (t < BS.V_ESC)).sum())
    esc = int((t >= BS.V_ESC).sum())
    print(f"sweep: {sw.core.size} distinct values; {small} below 2^17, {mid} in [2^17, V_ESC), {esc} at or above V_ESC")
    assert small > 0 and mid > 0 and esc > 0 and small + mid + esc == sw.core.size
    L = BS.limits()
    assert small > (L < BS.DSUM_PMAX).sum() and mid > ((L >= BS.DSUM_PMAX) & (L < BS.V_ESC)).sum()
    assert esc > (L >= BS.V_ESC).sum()


def test_subsets():
    sw = BS.sweep()
    t = BS.java_f2l(sw.in_range)
    assert ((t >= 0) & (t < BS.V_ESC)).all() and not np.isnan(sw.in_range).any() and not np.signbit(sw.in_range).any()
    assert (sw.in_range < np.float32(BS.V_ESC)).all()  # level 1's own test: none takes the slow route
    assert sw.in_range.size + sw.escaped.size == sw.all.size
    # every escaped value but -0.0 is outside [0, V_ESC) as level 1 sees it (f >= 0 && f < V_ESC fails)
    e = sw.escaped
    fast = (e >= 0) & (e < np.float32(BS.V_ESC))
    assert fast.sum() == 1 and np.signbit(e[fast]).all() and (e[fast] == 0).all()
    # mixed: every value of the whole set, and no 64 consecutive samples without an escaped one
    assert set(sw.mixed.view(np.uint32).tolist()) == set(sw.all.view(np.uint32).tolist())
    gaps = np.diff(np.flatnonzero(np.concatenate([[True], sw.mixed_is_escaped, [True]])))
    assert BS.ESC_STRIDE <= 64 and gaps.max() <= BS.ESC_STRIDE
    # ... nor without an escaped record (the few slow-route values that truncate to 0 leave none)
    gaps = np.diff(np.flatnonzero(np.concatenate([[True], sw.mixed_escapes_record, [True]])))
    assert gaps.max() < 64, int(gaps.max())
    np.testing.assert_array_equal(sw.mixed[~sw.mixed_is_escaped], sw.in_range)


def test_oracle_counts_equal_plain_searchsorted(oracle):
    """The C oracle over the sweep against numpy: for the in-range part literally
    bincount(searchsorted(L, trunc(v), "right")) with trunc in int64; for the whole set the
    same with Long.toInt's wrap and the overflow bucket (bucket_sweep.expected_bucket)."""
    sw = BS.sweep()
    L = BS.limits()
    o = oracle.OracleHistograms(1)
    o.ingest(np.zeros(sw.in_range.size, np.uint32), sw.in_range)
    trunc = sw.in_range.astype(np.int64)
    want = np.bincount(np.searchsorted(L, trunc, "right"), minlength=BS.NLIMITS + 1)
    np.testing.assert_array_equal(o.counts()[0], want)
    assert int(o.totals()[0]) == int(trunc.sum())

    for name in ("mixed", "escaped"):
        v = sw.subset(name)
        o = oracle.OracleHistograms(1)
        o.ingest(np.zeros(v.size, np.uint32), v)
        np.testing.assert_array_equal(o.counts()[0], np.bincount(BS.expected_bucket(v), minlength=BS.NLIMITS + 1),
                                      err_msg=name)
        total = int(BS.expected_contribution(v).astype(np.uint64).sum(dtype=np.uint64))  # wraps as a long does
        assert int(o.totals()[0]) % (1 << 64) == total, name


def test_plan_sample_restatement():
    """plan_sample_tiles on a batch below 2^18 samples is the exact tile load (sampled whole)."""
    rng = np.random.default_rng(1)
    s = rng.integers(0, 1000, size=5000).astype(np.uint32)
    np.testing.assert_array_equal(BS.plan_sample_tiles(s, 1000), np.bincount(s >> 5, minlength=32))
