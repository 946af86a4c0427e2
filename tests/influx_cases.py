"""Trees for the InfluxDB table and its device renderer (tests/test_influx_table_host.py,
tests/test_gpu_render_influx.py): the reference's own cases as tests/test_exporters_host.py
restates them, the tag rewrites, interleaved and duplicate field keys, names whose UTF-16
order differs from their UTF-8 order, Stats without a snapshot, and seeded random trees.
"""
import numpy as np

from linkerd_amd.telemetry import HistogramSummary, MetricsTree, MetricsTreeStatsReceiver

from .test_exporters_host import ONE, ONE_TWO, TWO_FOUR

HOSTS = ("none", "h:80", "")
TILDE, SMILE = "～", "\U0001F600"  # UTF-8: ef bd 9e < f0 9f 98 80; UTF-16: ff5e > d83d de00
REWRITES = (("rt", "incoming"), ("rt", "incoming", "service", "/svc/foo"), ("rt", "incoming", "client", "/#/bar"),
            ("rt", "incoming", "client", "/#/bar", "service", "/svc/foo"), ("rt", "incoming", "server", "127.0.0.1/4141"))
TAGGED_TWICE = ("rt", "r", "service", "s", "service", "t")  # the prefix already carries the tag


def _new():
    tree = MetricsTree()
    return tree, MetricsTreeStatsReceiver(tree)


def counter_tree():
    tree, stats = _new()
    stats.scope("foo", "bar").counter("bas").incr(2)
    return tree


def gauge_tree():
    tree, stats = _new()
    stats.scope("foo", "bar").add_gauge("bas", f=lambda: 2.0)
    return tree


def stat_tree():
    tree, stats = _new()
    stats.scope("foo", "bar").stat("bas")._set_snapshot(ONE_TWO)
    return tree


def root_tree():
    tree, stats = _new()
    stats.counter("abc").incr()
    stats.add_gauge("ghi", f=lambda: 4.0)
    stats.stat("def")._set_snapshot(TWO_FOUR)
    return tree


def rewrite_tree():
    tree, stats = _new()
    for scope in REWRITES + (TAGGED_TWICE,):
        stats.scope(*scope).counter("requests").incr()
    return tree


def interleaved_tree():
    """Stat `a` beside counters `a_count` and `a_p`: the Stat's fields sort among them."""
    tree, stats = _new()
    sc = stats.scope("x")
    sc.stat("a")._set_snapshot(ONE_TWO)
    sc.counter("a_count").incr(7)
    sc.counter("a_p").incr(5)
    return tree


INTERLEAVED = ("x,host=none a_avg=1.5,a_count=2,a_count=7,a_max=2,a_min=1,a_p=5,a_p50=1,a_p90=2,a_p95=2,a_p99=2,"
               "a_p999=2,a_p9999=2,a_sum=3\n")


def utf16_tree():
    tree, stats = _new()
    stats.scope("u").counter(TILDE).incr(1)
    stats.scope("u").counter(SMILE).incr(2)
    return tree


def unsnapshotted_tree():
    """A Stat without a snapshot beside a counter, and a parent whose only child is one."""
    tree, stats = _new()
    stats.scope("p").stat("never")
    stats.scope("p").counter("c").incr(3)
    stats.scope("q").stat("alone")
    return tree


def empty_tree():
    return MetricsTree()


NAMED = {"counter": counter_tree, "gauge": gauge_tree, "stat": stat_tree, "root": root_tree, "rewrite": rewrite_tree,
         "interleaved": interleaved_tree, "utf16": utf16_tree, "unsnapshotted": unsnapshotted_tree, "empty": empty_tree}

ALPHABET = ("a", "a_count", "a_p", "a_p99", "b", "requests", TILDE, SMILE, "é", "we ird=,x", "rt", "client", "service",
            "server", "r", "/svc/foo", "Z", "0")
GAUGES = (0.0, -0.0, 1.5, float("nan"), float("inf"), -float("inf"), 1.48832833e12, 1e-45, 3.4028235e38, 0.001)
SUMMARIES = (ONE, ONE_TWO, TWO_FOUR, HistogramSummary(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0.0),
             HistogramSummary(3, -(2 ** 63), 2 ** 63 - 1, 10, 1, 2, 3, 4, 5, 6, 10 / 3),
             HistogramSummary(7, 1, 9, 2 ** 62, 2, 3, 4, 5, 6, 7, 2.82879384806159e17))
N_RANDOM = 300


def random_tree(seed: int) -> MetricsTree:
    """At most 40 metrics at depths 0..5 over ALPHABET: a path may be a metric and a scope
    at once, a fifth of the Stats have no snapshot."""
    rng = np.random.default_rng(1000 + seed)
    tree, stats = _new()
    made = {}
    for _ in range(int(rng.integers(1, 41))):
        path = tuple(ALPHABET[i] for i in rng.integers(0, len(ALPHABET), int(rng.integers(1, 7))))
        if path in made:
            continue
        kind = made[path] = int(rng.integers(0, 3))
        sc = stats.scope(*path[:-1])
        if kind == 0:
            sc.counter(path[-1]).incr(int(rng.integers(-2 ** 40, 2 ** 40)))
        elif kind == 1:
            sc.add_gauge(path[-1], f=lambda v=GAUGES[int(rng.integers(0, len(GAUGES)))]: v)
        else:
            st = sc.stat(path[-1])
            if rng.integers(0, 5):
                st._set_snapshot(SUMMARIES[int(rng.integers(0, len(SUMMARIES)))])
    return tree
