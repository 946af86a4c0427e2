"""Inputs shared by tests/test_fmt_host.py (the host formatter) and
tests/test_gpu_render.py (the device renderer): the doubles, the integer edges and the
seeded quotients, each built once."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the known answers of tests/test_javafmt.py (the ones outside the domain are told apart below)
KNOWN = (1.0, 1.5, 3030.0, 1e7, 1e-4, 0.001, 281.7352941176471, 0.0, -0.0, 9999999.0, 12345678.0, float("nan"),
         float("inf"), -float("inf"), 5e-324, 1.7976931348623157e308, 2.82879384806159e17, 1e23)
EDGES = (2.0 ** -64, 2.0 ** 64, float(np.nextafter(2.0 ** 64, 0.0)), 1.0 / 2 ** 63, 5e-4, 0.001, 9999999.0, 1e7,
         2.82879384806159e17, 1e23, float(np.nextafter(2.0 ** -64, 0.0)), 2.0 ** 70, 1e-20, 4.9e-324)


def in_domain(x: float) -> bool:
    """What l5dh_format_double takes: +-0.0, NaN, +-Infinity, finite 2^-64 <= |x| < 2^64."""
    return x != x or x in (float("inf"), -float("inf")) or x == 0.0 or 2.0 ** -64 <= abs(x) < 2.0 ** 64


@functools.lru_cache(maxsize=None)
def fixed_doubles():
    """Every fixed case, in and out of the domain."""
    avgs = [float(t["text"]) for t in json.load(open(os.path.join(GOLDEN, "p5_number_texts.json")))["texts"]
            if t["key"] == "stat.avg"]
    assert len(avgs) == 142
    pos = list(avgs) + list(KNOWN) + list(EDGES)
    pos += [2.0 ** k for k in range(-64, 64)]  # every power of two inside the domain
    pos += [float(f"1e{k}") for k in range(-19, 20)]  # every power of ten inside it
    neg = [-x for x in pos[::3] if x == x]
    return tuple(pos + neg)


@functools.lru_cache(maxsize=None)
def quotients(n: int = 50_000, seed: int = 20):
    """sum / count as the summary stage divides them: sum of 1 to 62 random bits, count
    of 1 to 40 random bits."""
    rng = np.random.default_rng(seed)
    sb, cb = rng.integers(1, 63, n), rng.integers(1, 41, n)
    sums = [max(1, int(rng.integers(0, 1 << int(b), dtype=np.uint64))) for b in sb]
    counts = [max(1, int(rng.integers(0, 1 << int(b), dtype=np.uint64))) for b in cb]
    return tuple(s / c for s, c in zip(sums, counts))


_P10 = [10 ** k for k in range(20)]
INT64_EDGES = tuple(sorted(set(
    [0, 9, -9, 10, -10, 2 ** 63 - 1, -2 ** 63] + [s * v for k in range(1, 19) for v in (_P10[k] - 1, _P10[k])
                                                  for s in (1, -1)])))
UINT64_EDGES = tuple(sorted(set([0, 9, 10, 2 ** 63 - 1, 2 ** 63, 2 ** 64 - 1] +
                                [v for k in range(1, 20) for v in (_P10[k] - 1, _P10[k])])))
