"""The crafted summary rows (tests/summary_rows.py) checked on the CPU: the fixture
builds what it claims and exposes every percentile target, every bin position within
a lane and the .5 ties of Math.round -- so the GPU tests that feed it to the kernels
can fail for a slip of one anywhere in the summary."""
import numpy as np

from oracle import oracle as O
from tests import summary_rows as R


def test_bucket_values_land_in_their_buckets_and_reproduce_the_staircase():
    L = O.limits()
    v = R.BUCKET_VALUES
    assert v.dtype == np.float32 and v.shape == (R.NB,) and v[0] == 0.0 and v[-1] == np.float32(3e9)
    for b in (1, 2, 113, 114, 900, 1796):
        assert O.lib().l5do_bucket_of(int(v[b])) == b and L[b - 1] <= int(v[b]) < L[b]
    # all 1798 into one series: one sample per bucket
    one = O.OracleHistograms(1)
    assert one.ingest(np.zeros(R.NB, np.uint32), v) == 0
    assert (one.counts()[0] == 1).all()
    # series by series: the staircase rows exactly, totals with 3e9 clipped to Int.MaxValue
    series, values = R.staircase_series()
    assert series.size == R.NB * (R.NB + 1) // 2
    o = O.OracleHistograms(R.NB)
    assert o.ingest(series, values, threads=8) == 0
    np.testing.assert_array_equal(o.counts(), R.staircase_rows())
    contrib = v.astype(np.int64)
    contrib[-1] = R.INT_MAX
    np.testing.assert_array_equal(o.totals(), np.cumsum(contrib))


def test_staircase_percentiles_are_the_targets_bucket():
    """Row n: every p-field is mid[py_round(p * n) - 1] -- the target, nothing else,
    decides the answer -- and min / max are the first and the last bucket."""
    rows = R.staircase_rows()
    got = O.summarize_counts(rows, np.zeros(R.NB, np.int64))
    mid = np.array([O.py_mid(b) for b in range(R.NB)], np.int64)
    assert (np.diff(mid) > 0).all()  # adjacent buckets report distinct values
    want = np.array([[t for t, _ in R.py_targets(n)] for n in range(1, R.NB + 1)], np.int64)
    for j, f in enumerate(("p50", "p90", "p95", "p99", "p9990", "p9999")):
        t = want[:, j]
        assert (t >= 0).all() and (t <= np.arange(1, R.NB + 1)).all()
        np.testing.assert_array_equal(got[f], np.where(t == 0, 0, mid[np.maximum(t - 1, 0)]), err_msg=f)
    np.testing.assert_array_equal(got["count"], np.arange(1, R.NB + 1))
    np.testing.assert_array_equal(got["min"], 0)
    np.testing.assert_array_equal(got["max"], mid)


def test_staircase_targets_cover_ties_and_every_bin_position():
    ties = np.zeros(6, int)
    pos = [set() for _ in range(6)]
    lanes = [set() for _ in range(6)]
    extra = set()  # lane 63's bins past its 28: 1792..1797
    for n in range(1, R.NB + 1):
        for j, (t, tie) in enumerate(R.py_targets(n)):
            ties[j] += bool(tie)
            if t >= 1:
                b = t - 1
                pos[j].add(min(b, 1791) % 28)
                lanes[j].add(min(b // 28, 63))
                if b >= 1792:
                    extra.add(b)
    # every percentile meets a .5 tie of Math.round -- but p9999, for which none exists at
    # n <= 1798 (0.9999 n = m + 1/2 needs 5000 | n): summary_rows.tie_rows() covers it
    assert (ties[:5] > 0).all() and ties[5] == 0, ties
    mid = np.array([O.py_mid(b) for b in range(R.NB)], np.int64)
    tr = R.tie_rows()
    got = O.summarize_counts(tr, np.zeros(tr.shape[0], np.int64))
    for i, (num, last) in enumerate((n, b) for n in R.TIE_NUMS for b in R.TIE_LAST):
        x = 0.9999 * float(num)
        assert x - np.floor(x) == 0.5 and got["count"][i] == num
        b = int(np.floor(x)) + 1 - (num - last)  # sample k > num - last sits alone in bucket k - (num - last)
        assert 1 <= b <= last and got["p9999"][i] == mid[b] != mid[b - 1]  # half up: the next sample's bucket
    # the issue's examples are among them
    for p, n in ((0.5, 7), (0.9, 5), (0.95, 10), (0.99, 50)):
        x = p * float(n)
        assert x - np.floor(x) == 0.5 and O.py_round(x) == int(np.floor(x)) + 1
    for j in range(6):
        assert pos[j] == set(range(28)), (j, sorted(pos[j]))  # every bin of a lane, per percentile
    assert lanes[0] >= set(range(32)) and lanes[5] == set(range(64))
    assert extra == set(range(1792, 1798))


def test_dense_rows_are_legal_and_hold_the_named_cases():
    rows, totals = R.dense_rows()
    assert rows.dtype == np.int32 and rows.flags["C_CONTIGUOUS"] and totals.shape == (rows.shape[0],)
    assert rows.min() == 0 and rows.max() == R.INT_MAX
    num = rows.astype(np.int64).sum(axis=1)
    assert num.max() == 1798 * R.INT_MAX == 3_861_175_597_306 and (num == 0).any()
    g4 = rows.astype(np.int64)[:, :1796].reshape(-1, 449, 4).sum(axis=2)
    assert (g4 >= 2 ** 32).any(axis=1).sum() > 100  # group sums that do not fit 32 bits
    assert set(R.SPECIAL_TOTALS) == set(totals.tolist())
    # the issue's example row and what the oracle says about it
    ex = np.zeros(R.NB, np.int32)
    ex[4:8], ex[100] = 2 ** 30, 1
    assert (rows == ex).all(axis=1).any()
    s = O.summarize_counts(ex[None], np.zeros(1, np.int64))[0]
    assert (s["count"], s["min"], s["max"], s["p50"], s["p90"], s["p9999"]) == (4294967297, 4, 100, 6, 7, 7)
    # every run start and end position within a lane's 28 bins, and within a 4-bin group
    nz = rows != 0
    first, last = nz.argmax(axis=1), R.NB - 1 - nz[:, ::-1].argmax(axis=1)
    ok = nz.any(axis=1)
    assert set((first[ok] % 28).tolist()) == set(range(28)) == set((np.minimum(last[ok], 1791) % 28).tolist())
