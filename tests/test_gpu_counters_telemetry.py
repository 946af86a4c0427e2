"""Device-backed Metric.Counter through the telemetry layer: concurrent incr from several
threads, StatEngine.grow taking the counters along, checkpoint and restore.
"""
import threading

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

THREADS, CALLS, COUNTERS = 4, 50_000, 100


def test_threads_incr_through_the_stats_receiver(gpu_available):
    from linkerd_amd.counters import CounterEngine
    from linkerd_amd.telemetry import MetricsTree, MetricsTreeStatsReceiver, StatEngine
    se = StatEngine(capacity=64)
    try:
        ce = CounterEngine(se, 128, batch=4096)
        sr = MetricsTreeStatsReceiver(MetricsTree(se, ce))
        counters = [sr.counter("rt", "http", "client", f"c{j}", "requests") for j in range(COUNTERS)]
        assert sorted(m.counter_id for m in counters) == list(range(COUNTERS))
        plan = [np.random.default_rng(t).integers(0, COUNTERS, CALLS) for t in range(THREADS)]
        deltas = [np.random.default_rng(100 + t).integers(-3, 1000, CALLS) for t in range(THREADS)]

        def work(t):
            for j, d in zip(plan[t].tolist(), deltas[t].tolist()):
                counters[j].incr(d)
        threads = [threading.Thread(target=work, args=(t,)) for t in range(THREADS)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        want = np.zeros(COUNTERS, np.int64)
        for t in range(THREADS):
            np.add.at(want, plan[t], deltas[t])
        assert [m.get() for m in counters] == want.tolist()
        assert ce.info()["adds"] == THREADS * CALLS and ce.info()["dropped"] == 0

        # StatEngine.grow hands the counters to its new engine
        stat = sr.stat("rt", "http", "request_latency_ms")
        stat.add(5.0)
        counters[0].incr(7)  # (staged across the swap)
        old = se.engine
        se.grow(256)
        assert se.engine is not old and ce.engine is se.engine and se.counters is ce
        want[0] += 7
        assert [m.get() for m in counters] == want.tolist()
        counters[1].incr(-1)
        want[1] -= 1
        np.testing.assert_array_equal(ce.values()[:COUNTERS], want)
        assert stat.summary.count == 1
    finally:
        se.engine.close()


def test_checkpoint_and_restore_on_a_fresh_engine(gpu_available):
    from linkerd_amd.counters import CounterEngine
    from linkerd_amd.engine import HistogramEngine
    from linkerd_amd.telemetry import MetricsTree
    with HistogramEngine(64) as a, HistogramEngine(64) as b:
        ce = CounterEngine(a, 50)
        tree = MetricsTree(counters=ce)
        ms = [tree.resolve([f"c{j}"]).mk_counter() for j in range(20)]
        for j, m in enumerate(ms):
            m.incr(j * 1_000_003 - 7)
        ce.write(ms[19].counter_id, np.array([(1 << 63) - 1], np.int64))
        ms[19].incr(1)  # wraps
        for j in (3, 11):
            tree.resolve([f"c{j}"]).prune()
        ms[5].incr(1)  # staged when the checkpoint is taken
        ck = ce.checkpoint()
        fresh = CounterEngine(b, 64)
        fresh.restore({k: np.array(v) for k, v in ck.items()})
        np.testing.assert_array_equal(fresh.values()[:20], ce.values()[:20])
        assert fresh.get(19) == -(1 << 63) and fresh.get(3) == 0 and fresh.get(5) == 5 * 1_000_003 - 6
        assert fresh.registered == ce.registered == 18
        assert [fresh.register() for _ in range(3)] == [ce.register() for _ in range(3)] == [11, 3, 20]
        assert not np.any(fresh.values()[20:])
