"""linkerd_amd/synth.py against its recipe, restated without it (no GPU).

The recipe (synth.py's header) in other arithmetic: Python integers for
mix64 / rand, np.longdouble (a 64-bit mantissa) for log, sqrt, cos and exp -- 2 pi stays
the recipe's double -- and plain Python floats for the Zipf CDF (the same sequential sum of
1/r in IEEE double, so the same bits; the draw is one double compare).  Series must be
equal; values must be equal once rounded to float32: a float64 libm result differs from the
64-bit-mantissa one by at most a few double ulps, which reaches the float32 rounding only
where the exact value lies within ~1e-15 of a rounding boundary -- measured: 0 values of
2 x 10^6 per config, so the 2^18 samples here are compared for equality.
"""
import bisect
import itertools
import math
import os

import numpy as np
import pytest

from linkerd_amd import synth

N_CHECK = 1 << 18
MASK = (1 << 64) - 1
GOLD = 0x9E3779B97F4A7C15
A, B = 2654435761, 40503
LD = np.longdouble
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

needs_extended = pytest.mark.skipif(np.finfo(np.longdouble).nmant < 63,
                                    reason="np.longdouble has fewer than 63 mantissa bits here: no wider reference")


def _mix64(z):
    z ^= z >> 30
    z = z * 0xBF58476D1CE4E5B9 & MASK
    z ^= z >> 27
    z = z * 0x94D049BB133111EB & MASK
    return z ^ (z >> 31)


def _rand(seed, stream, i):
    return _mix64((((((seed << 48) ^ (stream << 40) ^ i) & MASK) + 1) * GOLD) & MASK)


def _uniform(seed, stream, idx) -> np.ndarray:
    """(rand >> 11) * 2^-53 per index, as longdouble (every such value is exact in a double)."""
    return np.array([_rand(seed, stream, int(i)) >> 11 for i in idx], dtype=np.uint64).astype(LD) * LD(2.0 ** -53)


def _normal(seed, stream, idx) -> np.ndarray:
    u1 = _uniform(seed, stream, [2 * int(i) for i in idx]) + LD(2.0 ** -53)  # (0, 1]
    u2 = _uniform(seed, stream, [2 * int(i) + 1 for i in idx])
    return np.sqrt(LD(-2.0) * np.log(u1)) * np.cos(LD(2.0 * math.pi) * u2)


def _lognormal_f32(mu, sigma, z) -> np.ndarray:
    v = np.exp(mu + LD(sigma) * z)
    return np.minimum(np.maximum(v, LD(0.0)), LD(1e9)).astype(np.float32)


def _mu(seed, series) -> np.ndarray:
    """ln U[1, 1000] per series id (stream 1), one draw per distinct id."""
    ids, inv = np.unique(np.asarray(series, np.uint64), return_inverse=True)
    return np.log(LD(1.0) + LD(999.0) * _uniform(seed, 1, ids))[inv]


def _same_f32(got, want, label):
    assert got.dtype == np.float32 and want.dtype == np.float32
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), f"{label}: {int(diff.sum())} of {diff.size} values differ; first at {int(np.flatnonzero(diff)[0])}"


@needs_extended
@pytest.mark.parametrize("seed", [1, 17])
def test_c1_is_the_recipe(seed):
    s, v = synth.c1(n=N_CHECK, seed=seed)
    assert s.dtype == np.uint32 and not s.any()
    want = _lognormal_f32(LD(math.log(20.0)), 1.0, _normal(seed, 2, range(N_CHECK)))
    _same_f32(v, want, f"c1 seed {seed}")


@needs_extended
@pytest.mark.parametrize("series_base", [0, 4096])
def test_c2_is_the_recipe(series_base):
    S, K, seed = 2000, 1000, 2
    s, v = synth.c2(S=S, K=K, seed=seed, series_base=series_base)
    assert s.size == S * K
    np.testing.assert_array_equal(np.bincount(s, minlength=S), np.full(S, K))  # every series exactly K samples
    j = [(i * A + B) % (S * K) for i in range(N_CHECK)]
    series = np.array([x // K for x in j], dtype=np.uint32)
    np.testing.assert_array_equal(s[:N_CHECK], series)  # local ids whatever the base
    want = _lognormal_f32(_mu(seed, series.astype(np.uint64) + series_base), 0.8, _normal(seed, 2, j))
    _same_f32(v[:N_CHECK], want, f"c2 base {series_base}")


def _zipf_cdf(S):
    c = list(itertools.accumulate(1.0 / r for r in range(1, S + 1)))
    return [x / c[-1] for x in c]


def _c3_reference(S, seed, base_index, cdf, series_base):
    idx = range(base_index, base_index + N_CHECK)
    u = [(_rand(seed, 3, i) >> 11) * 2.0 ** -53 for i in idx]  # exact in a double
    series = np.array([min(bisect.bisect_right(cdf, x), S - 1) for x in u], dtype=np.uint32)
    ids = (series.astype(np.uint64) + series_base) & 0xFFFFFFFF
    return series, _lognormal_f32(_mu(seed, ids), 0.8, _normal(seed, 2, idx))


@needs_extended
@pytest.mark.parametrize("base_index", [0, (1 << 33) + 5])
def test_c3_is_the_recipe(base_index):
    S, seed = 1 << 20, 3
    cdf = _zipf_cdf(S)
    np.testing.assert_array_equal(synth.zipf_cdf(S), np.array(cdf))
    s, v = synth.c3(S=S, N=N_CHECK, seed=seed, base_index=base_index)
    want_s, want_v = _c3_reference(S, seed, base_index, cdf, 0)
    np.testing.assert_array_equal(s, want_s)
    _same_f32(v, want_v, f"c3 base_index {base_index}")


@needs_extended
def test_c3_shard_arguments():
    """A shard as bench.gen_batch draws it: a restricted CDF over `count` series from `first`,
    local ids, series_base = first seeding mu; and series_base's u32 wrap."""
    S, first, count, seed = 5000, 1234, 777, 4
    cdf = _zipf_cdf(S)
    lo = cdf[first - 1]
    sub = [(x - lo) / (cdf[first + count - 1] - lo) for x in cdf[first:first + count]]
    sub[-1] = 1.0
    s, v = synth.c3(S=count, N=N_CHECK, seed=seed, base_index=99, cdf=np.array(sub), series_base=first)
    want_s, want_v = _c3_reference(count, seed, 99, sub, first)
    np.testing.assert_array_equal(s, want_s)
    assert s.max() == count - 1
    _same_f32(v, want_v, "c3 shard")
    n = 1 << 12
    s2, v2 = synth.c3(S=count, N=n, seed=seed, cdf=np.array(sub), series_base=(1 << 32) - 5)
    np.testing.assert_array_equal(s2, synth.c3(S=count, N=n, seed=seed, cdf=np.array(sub))[0])  # ids stay local
    wrapped = (s2.astype(np.uint64) + (1 << 32) - 5) & 0xFFFFFFFF
    want = synth.lognormal_f32(synth.series_mu(seed, wrapped), 0.8, synth.normal(seed, 2, np.arange(n, dtype=np.uint64)))
    _same_f32(v2, want, "series_base wrap")


@pytest.mark.parametrize("name,call", [("c1_100k", lambda: synth.c1(n=100_000)),
                                       ("c2_200x500", lambda: synth.c2(S=200, K=500)),
                                       ("c3_zipf1000", lambda: synth.c3(S=1000, N=50_000))])
def test_defaults_keep_the_golden_bytes(name, call):
    """The optional arguments (cdf, series_base) left out: the committed vectors' bytes."""
    g = np.load(os.path.join(GOLDEN, f"golden_{name}.npz"))
    s, v = call()
    assert s.dtype == np.uint32 and v.dtype == np.float32
    assert s.tobytes() == np.ascontiguousarray(g["series"], np.uint32).tobytes()
    assert v.tobytes() == np.ascontiguousarray(g["values"], np.float32).tobytes()
