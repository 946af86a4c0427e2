"""The bucket-edge sweep: one float32 value set that touches every bucket and pins every
limit from both sides, and a plain numpy statement of what each value must do.  Pure
numpy, importable without a GPU; tests/test_bucket_sweep_host.py asserts the set's
properties, tests/test_gpu_bucket_sweep.py drives it through each device decoder.

  dense  every integer 0 .. 2^21 + 2048 (exact in float32): every key of lut2 / lut3 and
         the escape threshold V_ESC = 2^21 - 2048
  near   float32(L[i]) and two float32 neighbours on each side, for every limit, below 2^31
  half   L[i] - 0.5 for every limit below 2^23: truncation sends it to L[i] - 1
  wild   test_gpu_parity's EDGE_VALUES and the far ends of Java's float -> long -> int
"""
import functools

import numpy as np

from oracle.oracle import INT_MAX, NLIMITS, py_make_limits
from tests.test_gpu_parity import EDGE_VALUES

V_ESC = (1 << 21) - 2048
DENSE_END = (1 << 21) + 2048  # inclusive
DSUM_PMAX = 1 << 17           # level 1's u32 sums take payloads below this
ITEM2 = 6144                  # level-1 records per level-2 item
ESC_STRIDE = 19               # mixed: a slow-route sample at every 19th position (odd: they visit every series)

WILD_EXTRA = np.array([
    -0.0, -0.5, -1.0, -2.0 ** 31, -2.0 ** 31 - 256,
    2.0 ** 31, 2.0 ** 32, 2.0 ** 32 + 2.0 ** 9, 2.0 ** 62, 2.0 ** 63, 2.0 ** 64, -2.0 ** 63, -2.0 ** 64,
    3e38, -3e38, np.nan, np.inf, -np.inf, 2.0 ** -149,
], dtype=np.float32)


@functools.lru_cache(maxsize=None)
def limits() -> np.ndarray:
    """makeLimitsFor(0.005) (oracle.py_make_limits, pure Python): 1797 ascending int32."""
    L = np.array(py_make_limits(0.005), dtype=np.int64)
    assert L.size == NLIMITS and (np.diff(L) > 0).all() and L[-1] < INT_MAX
    L.setflags(write=False)
    return L


def java_f2l(v: np.ndarray) -> np.ndarray:
    """Java's (long) of a float (JLS 5.1.3): NaN -> 0, saturating, else toward zero."""
    v = np.asarray(v, np.float32)
    out = np.zeros(v.shape, np.int64)
    hi = v >= np.float32(2.0 ** 63)
    lo = v <= np.float32(-2.0 ** 63)
    mid = ~(hi | lo | np.isnan(v))
    out[mid] = np.trunc(v[mid].astype(np.float64)).astype(np.int64)  # |v| < 2^63: exact in float64 and int64
    out[hi] = np.iinfo(np.int64).max
    out[lo] = np.iinfo(np.int64).min
    return out


def expected_bucket(v: np.ndarray) -> np.ndarray:
    """BucketedHistogram.add(value.toLong): the overflow bucket from Int.MaxValue up, else
    the insertion point of Long.toInt (the low 32 bits, signed) among the limits."""
    t = java_f2l(v)
    key = (t & 0xFFFFFFFF).astype(np.uint32).view(np.int32).astype(np.int64)
    return np.where(t >= INT_MAX, NLIMITS, np.searchsorted(limits(), key, side="right")).astype(np.int64)


def expected_contribution(v: np.ndarray) -> np.ndarray:
    """What a sample adds to its series' total: the long value, Int.MaxValue in the overflow bucket."""
    return np.minimum(java_f2l(v), INT_MAX)


def _distinct(v: np.ndarray) -> np.ndarray:
    """Distinct float32 bit patterns (NaN and -0.0 kept apart from the numbers), in first-seen order."""
    v = np.ascontiguousarray(v, np.float32)
    _, first = np.unique(v.view(np.uint32), return_index=True)
    return v[np.sort(first)]


class Sweep:
    """The value set and its sub-sets (float32 arrays, read-only, a fixed order)."""

    def __init__(self):
        L = limits()
        self.dense = np.arange(0, DENSE_END + 1, dtype=np.int64).astype(np.float32)
        f0 = L.astype(np.float32)
        d1 = np.nextafter(f0, np.float32(-np.inf))
        u1 = np.nextafter(f0, np.float32(np.inf))
        near = np.stack([np.nextafter(d1, np.float32(-np.inf)), d1, f0, u1, np.nextafter(u1, np.float32(np.inf))], 1)
        near = near.ravel()
        self.near = near[near < np.float32(2.0 ** 31)]
        self.half = (L[L < (1 << 23)].astype(np.float64) - 0.5).astype(np.float32)
        self.wild = _distinct(np.concatenate([EDGE_VALUES, WILD_EXTRA]))
        # dense u near u half, distinct; the near / half values follow the dense run
        self.core = _distinct(np.concatenate([self.dense, self.near, self.half]))
        self.all = _distinct(np.concatenate([self.core, self.wild]))
        t = java_f2l(self.all)
        inr = (t >= 0) & (t < V_ESC) & ~np.isnan(self.all) & ~np.signbit(self.all)
        self.in_range = self.all[inr]
        self.escaped = self.all[~inr]  # wild and >= V_ESC: level 1's slow route
        # mixed: the in-range values in order with the escaped ones, cycled, at every ESC_STRIDE-th position
        R = self.in_range.size
        m = np.arange(R + R // (ESC_STRIDE - 1) + 2) % ESC_STRIDE == 0
        m = m[:int(np.flatnonzero(~m)[R - 1]) + 1]  # ends with the last in-range value
        assert int((~m).sum()) == R and int(m.sum()) >= self.escaped.size
        mixed = np.empty(m.size, np.float32)
        mixed[m] = self.escaped[np.arange(int(m.sum())) % self.escaped.size]
        mixed[~m] = self.in_range
        self.mixed = mixed
        self.mixed_is_escaped = m
        # -0.0 and -0.5 leave the slow route with payload 0: no escaped record
        tm = java_f2l(mixed)
        self.mixed_escapes_record = m & ~((tm >= 0) & (tm < V_ESC))
        for a in (self.dense, self.near, self.half, self.wild, self.core, self.all, self.in_range, self.escaped,
                  self.mixed, self.mixed_is_escaped, self.mixed_escapes_record):
            a.setflags(write=False)

    def subset(self, name: str) -> np.ndarray:
        return {"in_range": self.in_range, "mixed": self.mixed, "escaped": self.escaped}[name]


@functools.lru_cache(maxsize=None)
def sweep() -> Sweep:
    return Sweep()


def tile_series(n: int, tile: int) -> np.ndarray:
    """Sample k on series tile * 32 + (k mod 32): every series of the tile gets a comb of keys."""
    return (tile * 32 + np.arange(n, dtype=np.int64) % 32).astype(np.uint32)


def spread_series(n: int, S: int) -> np.ndarray:
    return (np.arange(n, dtype=np.int64) % S).astype(np.uint32)


def with_background(series, vals, S, tile, nbg, seed):
    """nbg lognormal samples on the series outside `tile`, at random positions of the batch (evenly
    spaced ones can fall in step with the plan's evenly spaced draws)."""
    rng = np.random.default_rng(seed)
    bs = rng.integers(0, S - 32, size=nbg)
    bs = (bs + 32 * (bs >= tile * 32)).astype(np.uint32)
    bv = np.exp(4.0 + 1.5 * rng.standard_normal(nbg)).astype(np.float32)
    at = np.sort(rng.integers(0, series.size, size=nbg))
    return np.insert(series, at, bs), np.insert(vals, at, bv)


def plan_sample_tiles(series: np.ndarray, S: int) -> np.ndarray:
    """k_rsample and k_rplan1's estimate per 32-series tile, restated: m = min(n, 2^18) evenly spaced
    draws (draw k reads sample k n / m), each tile's draws scaled by n / m in double and truncated."""
    n = series.size
    m = min(n, 1 << 18)
    at = np.arange(m, dtype=np.uint64) * np.uint64(n) // np.uint64(m)
    drawn = series[at.astype(np.int64)]
    est = np.bincount(drawn[drawn < S] >> 5, minlength=(S + 31) // 32).astype(np.float64)
    return np.minimum(est * (float(n) / float(m)), 4294967295.0).astype(np.uint64)
