"""Crafted bucket-count rows that pin the summary stage (wave_summary and its callers).

Random samples put most percentile targets deep inside a fat bucket, where an
off-by-one in Math.round(p * num), the owner lane, the 4-bin group or the bin moves
nothing.  The rows here leave no such slack:

* staircase row n (n = 1..1798) holds one sample in each of buckets 0..n-1, so the
  target round(p * n) of every percentile lands in bucket target - 1 and a slip of one
  changes the reported midpoint (adjacent buckets have distinct midpoints);
* offset and scaled staircases (count k in buckets o..o+n-1) move the run over every
  lane and group boundary and carry the counts past 2^16, 2^21 (the merge encoding's
  escape), 2^32 per 4-bin group and 2^32 per row;
* explicit rows: every bucket at 2^29, 2^30 and 2^31 - 1; four adjacent buckets of one
  group at 2^30 and at 2^31 - 1 (a group sum of 2^32 and of 2^33 - 4) at every group of
  lanes 0, 31 and 63; buckets 0 and 1797 alone; every single bucket; the empty row.

Counts stay in [0, 2^31 - 1] (an int32 row, upstream's Int counts).  Everything is built
on the CPU; the oracle is the only reference.
"""
import numpy as np

from oracle import oracle as O

NB = O.NBUCKETS
INT_MAX = O.INT_MAX
INT64_MIN, INT64_MAX = -(2 ** 63), 2 ** 63 - 1
K_VALUES = (1, 2, 3, 65535, 65536, 2 ** 21 - 1, 2 ** 21, 2 ** 29, 2 ** 30, 2 ** 31 - 1)
# avg = (double)total / (double)num: 2^53 + 1 is the first total that (double) rounds
SPECIAL_TOTALS = (12345, 0, -5, INT64_MIN, INT64_MAX, 2 ** 53 + 1, -(2 ** 53) - 1, 1)
# rows of the one-tile (S = 32) engine: both ends, the .5 ties of the issue's examples
# (p50 of odd n, 0.9 * 5, 0.95 * 10, 0.99 * 50), lane 0 / 1 and lane 63's extra groups
FOLD_ROWS = (1, 2, 3, 4, 5, 7, 10, 27, 28, 29, 31, 32, 33, 50, 56, 57, 100, 150, 899, 900, 1000, 1500,
             1763, 1764, 1765, 1791, 1792, 1793, 1795, 1796, 1797, 1798)
assert len(FOLD_ROWS) == 32


def _bucket_values() -> np.ndarray:
    L = O.limits().astype(np.int64)
    v = np.zeros(NB, np.float32)
    v[NB - 1] = 3e9
    lo, hi = L[:-1], L[1:]  # bucket b in 1..1796 = [L[b-1], L[b])
    v[1:NB - 1] = np.where(hi - lo == 1, lo, (lo + hi) // 2).astype(np.float32)
    return v


# One float32 per bucket that the oracle places in exactly that bucket (bucket 0: 0.0,
# bucket 1797: 3e9, else the bucket's midpoint -- or its only value).
BUCKET_VALUES = _bucket_values()


def staircase_rows() -> np.ndarray:
    """[1798][1798] int32: row n - 1 holds one sample in each of buckets 0..n-1."""
    return np.tri(NB, NB, 0, dtype=np.int32)


def staircase_series(rows=None):
    """(series, values) that build the staircase rows by ingest: series i receives
    BUCKET_VALUES[:rows[i]] (rows: 1..1798 by default), shuffled with a fixed seed."""
    rows = np.arange(1, NB + 1) if rows is None else np.asarray(rows)
    series = np.repeat(np.arange(rows.size, dtype=np.uint32), rows)
    values = np.concatenate([BUCKET_VALUES[:n] for n in rows])
    perm = np.random.default_rng(1798).permutation(series.size)
    return series[perm], values[perm]


def py_targets(n: int):
    """Math.round(p * n) per percentile, from oracle.py's pure-Python restatement, and
    whether p * n (the double product) sits exactly on a .5 tie."""
    out = []
    for p in O.PERCENTILES:
        x = p * float(n)
        out.append((O.py_round(x), x - np.floor(x) == 0.5))
    return out


def group_rows(k: int) -> np.ndarray:
    """Four adjacent buckets of one 4-bin group at k each (group 8 of lane 63: its two
    bins), one sample in bucket 100: every group of lanes 0, 31 and 63 (lane 63: 0..8)."""
    b0s = [28 * lane + 4 * q for lane in (0, 31) for q in range(7)] + [28 * 63 + 4 * q for q in range(9)]
    rows = np.zeros((len(b0s), NB), np.int32)
    for i, b0 in enumerate(b0s):
        rows[i, b0:min(b0 + 4, NB)] = k
        rows[i, 100] += 1
    return rows


# 0.9999 * n meets no .5 tie for n <= 1798 (9999 n = 5000 (2 m + 1) needs 5000 | n), so
# the staircase cannot show p9999 one: rows of TIE_NUMS samples do (0.9999 * 5000 = 4999.5
# exactly, also as a double product).  The run's last buckets hold one sample each, so
# rounding half up and half down report different buckets; the run ends on bin 1797, on
# a lane's first bin, on a lane's last bin and on bin 3.
TIE_NUMS = (5000, 15000)
TIE_LAST = (1797, 28 * 17, 28 * 40 + 27, 3)


def tie_rows() -> np.ndarray:
    rows = np.zeros((len(TIE_NUMS) * len(TIE_LAST), NB), np.int32)
    i = 0
    for num in TIE_NUMS:
        for last in TIE_LAST:
            rows[i, :last + 1] = 1
            rows[i, 0] = num - last
            i += 1
    return rows


def dense_rows():
    """Every row of the dense entry points' test: (rows [R][1798] int32, totals [R]
    int64).  The totals cycle through SPECIAL_TOTALS."""
    rng = np.random.default_rng(20241019)
    parts = [staircase_rows()]
    # ~2000 triples (n, o, k): half short runs (n <= 64: around lane and group edges),
    # half of any length; the offset uniform over what fits
    T = 2000
    n = np.where(rng.random(T) < 0.5, rng.integers(1, 65, T), rng.integers(1, NB + 1, T))
    o = (rng.random(T) * (NB - n + 1)).astype(np.int64)
    k = rng.choice(np.array(K_VALUES, np.int64), T)
    tri = np.zeros((T, NB), np.int32)
    col = np.arange(NB)
    tri[(col >= o[:, None]) & (col < (o + n)[:, None])] = 1
    parts.append(tri * k[:, None].astype(np.int32))
    # all buckets at 2^29, 2^30, 2^31 - 1 (num up to 1798 (2^31 - 1) = 3 861 175 597 306)
    parts.append(np.array([[2 ** 29] * NB, [2 ** 30] * NB, [INT_MAX] * NB], np.int32))
    # a 4-bin group whose sum is 2^32 (the issue's example) and 2^33 - 4
    parts += [group_rows(2 ** 30), group_rows(INT_MAX)]
    ends = np.zeros((len(K_VALUES) + 2, NB), np.int32)  # buckets 0 and 1797 alone
    for i, kk in enumerate(K_VALUES):
        ends[i, 0], ends[i, NB - 1] = kk, K_VALUES[-1 - i]
    ends[-2, 0], ends[-2, NB - 1] = 1, 1
    ends[-1, 0], ends[-1, NB - 1] = INT_MAX, INT_MAX
    parts.append(ends)
    parts.append(tie_rows())
    parts.append(np.eye(NB, dtype=np.int32))      # the 1798 single-bucket rows
    parts.append(np.zeros((1, NB), np.int32))     # the empty row
    rows = np.ascontiguousarray(np.concatenate(parts))
    assert rows.min() >= 0
    totals = np.resize(np.array(SPECIAL_TOTALS, np.int64), rows.shape[0])
    return rows, totals
