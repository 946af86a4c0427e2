"""GPU label rollups (l5dh_rollup, l5dh_rollup_dense) against the CPU oracle.

The truth everywhere: the members' oracle bucket counts and totals summed per group
(np.add.at over int64) and summarized by the oracle -- what ONE Stat fed every
member's samples reports.  Counts, totals and all 11 summary fields are compared
bytewise.
"""
import numpy as np
import pytest

from linkerd_amd import _native as N

pytestmark = pytest.mark.gpu

S, G = 257, 6          # tiles of 32 series + a remainder of 1: series 256 sits alone in its tile
QUIET = range(96, 128)  # tile 3 receives no sample
ITEMS = [None, 1, 3]    # PARAM_ROLLUP_ITEM: default (one item per group), one item per member, a remainder


def _assert_summaries_equal(got, want, label=""):
    for f in N.SUMMARY_FIELDS:
        g, w = got[f], want[f]
        if f == "avg":
            bad = ~((g == w) | (np.isnan(g) & np.isnan(w)))
        else:
            bad = g != w
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise AssertionError(f"{label} field {f}: {int(bad.sum())} mismatches; first series {i}: "
                                 f"got {g[i]!r} want {w[i]!r}\n got={got[i]}\nwant={want[i]}")


def _truth(O, counts, totals, group, ngroups):
    group = np.asarray(group, np.uint32)
    m = group != N.NO_GROUP
    gc = np.zeros((ngroups, N.NBUCKETS), np.int64)
    gt = np.zeros(ngroups, np.int64)
    np.add.at(gc, group[m], counts[m])
    np.add.at(gt, group[m], totals[m])
    return O.summarize_counts(gc.astype(np.int32), gt), gc, gt


def _check(got, want, label=""):
    """got: (summaries, counts, totals) of a rollup; want: _truth's triple."""
    np.testing.assert_array_equal(got[1].astype(np.int64), want[1], err_msg=f"{label} counts")
    np.testing.assert_array_equal(got[2], want[2], err_msg=f"{label} totals")
    _assert_summaries_equal(got[0], want[0], label)


def _batch(seed, n):
    rng = np.random.default_rng(seed)
    live = np.array([s for s in range(S) if s not in QUIET], np.uint32)
    series = live[rng.integers(0, live.size, size=n)]
    vals = np.exp(3.0 + rng.standard_normal(n)).astype(np.float32)
    # bin 0 and bin 1797 (lane 63's extra groups) in play
    vals[:8] = np.array([0, 1, 2, 113, 3030, 1e9, 3e9, -5], dtype=np.float32)
    series[:8] = [256, 0, 31, 32, 255, 256, 200, 33]
    return series, vals


def _oracle_state(O, batches):
    ref = O.OracleHistograms(S)
    for s, v in batches:
        assert ref.ingest(s, v) == 0
    return ref.counts().copy(), ref.totals().copy()


@pytest.fixture(scope="module")
def case(oracle):
    """Three batches (~20 k samples), the group map and the truth, computed once."""
    batches = [_batch(1, 8000), _batch(2, 7000), _batch(3, 5000)]
    rng = np.random.default_rng(9)
    group = rng.integers(3, G, size=S).astype(np.uint32)   # groups 3..5: random
    group[::7] = N.NO_GROUP                                # every 7th series in no group
    group[list(QUIET)] = N.NO_GROUP
    group[[100, 101, 106]] = 2                             # members all in the tile without samples
    group[256] = 1                                         # a singleton; group 0 has no members
    assert (group == 1).sum() == 1 and not (group == 0).any()
    counts, totals = _oracle_state(oracle, batches)
    assert not counts[list(QUIET)].any() and counts[:, 0].any() and counts[:, 1797].any()
    want = _truth(oracle, counts, totals, group, G)
    assert want[0]["count"][0] == 0 and want[0]["count"][2] == 0 and want[0]["count"][1] > 0
    series_want = oracle.summarize_counts(counts, totals)
    return dict(batches=batches, group=group, counts=counts, totals=totals, want=want, series_want=series_want)


def _engine(case=None, item=None, stage=0):
    """stage=0: every ingest call is binned at once, so segments are pending at the
    rollup; stage=None keeps the default ring, so the samples are still staged."""
    from linkerd_amd.engine import HistogramEngine
    e = HistogramEngine(S)
    if stage is not None:
        e.set_param(N.PARAM_STAGE_SAMPLES, stage)
    if item is not None:
        e.set_param(N.PARAM_ROLLUP_ITEM, item)
    if case is not None:
        for s, v in case["batches"]:
            e.ingest(s, v)
    return e


@pytest.mark.parametrize("stage", [0, None])
@pytest.mark.parametrize("item", ITEMS)
def test_live_parity(case, item, stage):
    with _engine(case, item, stage) as e:
        got = e.rollup(case["group"], G, with_counts=True)
        _check(got, case["want"], f"item={item} stage={stage}")
        # summaries alone (no dense rows asked for) are the same
        _assert_summaries_equal(e.rollup(case["group"], G), case["want"][0], "summaries only")


@pytest.mark.parametrize("item", ITEMS)
def test_sub_range_does_not_leak_and_resets_only_itself(oracle, case, item):
    first, count = 33, 190  # starts and ends inside a tile
    sl = slice(first, first + count)
    gsub = case["group"][sl].copy()
    gsub[0] = 0  # series 33 (value -5 went there) and the range's last series, in group 0
    gsub[-1] = 0
    want = _truth(oracle, case["counts"][sl], case["totals"][sl], gsub, G)
    with _engine(case, item) as e:
        got = e.rollup(gsub, G, first=first, count=count, reset=True, with_counts=True, with_series=True)
        _check(got, want, "sub-range")
        _assert_summaries_equal(got[3], case["series_want"][sl], "series of the range")
        after, counts = e.snapshot(reset=False, with_counts=True)
        expect = case["counts"].copy()
        expect[sl] = 0
        np.testing.assert_array_equal(counts, expect)
        tot = case["totals"].copy()
        tot[sl] = 0
        _assert_summaries_equal(after, oracle.summarize_counts(expect, tot), "state after the sub-range reset")


def test_atomic_snapshot_reset_and_reingest(oracle, case):
    zero = _truth(oracle, np.zeros_like(case["counts"]), np.zeros_like(case["totals"]), case["group"], G)
    with _engine(case, 3) as e, _engine(case) as twin:
        got = e.rollup(case["group"], G, reset=True, with_counts=True, with_series=True)
        _check(got, case["want"], "rollup")
        _assert_summaries_equal(got[3], twin.snapshot(reset=True), "series vs twin snapshot")
        after, counts = e.snapshot(reset=False, with_counts=True)
        assert not counts.any() and not after["count"].any() and not after["sum"].any()
        _check(e.rollup(case["group"], G, with_counts=True), zero, "second rollup")
        # clean tiles that turn dirty again contribute only the new samples
        s, v = _batch(4, 3000)
        keep = s < 64  # two tiles
        s, v = s[keep], v[keep]
        e.ingest(s, v)
        c2, t2 = _oracle_state(oracle, [(s, v)])
        _check(e.rollup(case["group"], G, with_counts=True), _truth(oracle, c2, t2, case["group"], G), "re-ingest")


def test_non_resetting_is_repeatable_and_leaves_the_snapshot_alone(case):
    with _engine(case, None, None) as e:
        a = e.rollup(case["group"], G, with_counts=True, with_series=True)
        b = e.rollup(case["group"], G, with_counts=True, with_series=True)
        for x, y in zip(a, b):
            assert x.tobytes() == y.tobytes()
        _check(a, case["want"])
        got, counts = e.snapshot(reset=True, with_counts=True)
        np.testing.assert_array_equal(counts, case["counts"])
        _assert_summaries_equal(got, case["series_want"], "snapshot after rollups")


@pytest.mark.parametrize("item", ITEMS)
def test_dense_source_numpy_and_device(case, item):
    import torch
    with _engine(case, item) as e:
        summ, counts = e.snapshot(reset=False, with_counts=True)
        totals = summ["sum"].copy()
        _check(e.rollup_dense(counts, totals, case["group"], G, with_counts=True), case["want"], "dense numpy")
        # no totals: sums and averages of zero, the same counts and quantiles
        nt = e.rollup_dense(counts, None, case["group"], G, with_counts=True)
        np.testing.assert_array_equal(nt[1].astype(np.int64), case["want"][1])
        assert not nt[2].any() and not nt[0]["sum"].any()
        for f in ("count", "min", "max", "p50", "p99", "p9999"):
            np.testing.assert_array_equal(nt[0][f], case["want"][0][f])
        dev = torch.device("cuda", e.device)
        d_counts = torch.from_numpy(counts).to(dev)
        d_totals = torch.from_numpy(totals).to(dev)
        d_group = torch.from_numpy(case["group"]).to(dev)
        o_summ = torch.full((G * 11,), -1, dtype=torch.int64, device=dev)
        o_counts = torch.full((G, N.NBUCKETS), -1, dtype=torch.int32, device=dev)
        o_totals = torch.full((G,), -1, dtype=torch.int64, device=dev)
        e.rollup_into(d_group, G, o_summ, o_counts, o_totals, dense=(d_counts, d_totals))
        got = (o_summ.cpu().numpy().view(N.SUMMARY_DTYPE), o_counts.cpu().numpy(), o_totals.cpu().numpy())
        _check(got, case["want"], "dense device")
        # the live rollup into device tensors, from a device map
        o_summ.fill_(-1)
        o_counts.fill_(-1)
        o_totals.fill_(-1)
        e.rollup_into(d_group, G, o_summ, o_counts, o_totals)
        got = (o_summ.cpu().numpy().view(N.SUMMARY_DTYPE), o_counts.cpu().numpy(), o_totals.cpu().numpy())
        _check(got, case["want"], "live device")


@pytest.mark.parametrize("item", [None, 1])
def test_range_is_detected_never_wrapped(oracle, case, item):
    B = 5  # bucket [5, 6): reported as 5
    rows = np.zeros((5, N.NBUCKETS), np.int32)
    rows[0, B], rows[1, B] = 2 ** 30, 2 ** 30 - 1          # group 0: exactly 2^31 - 1
    rows[2, 7] = 3                                          # group 1: small
    rows[3, 1797], rows[4, 1797] = 2 ** 31 - 1, 0           # group 2: the last bin at the limit
    totals = np.array([5 * 2 ** 30, 5 * (2 ** 30 - 1), 21, 2 ** 40, 0], np.int64)
    group = np.array([0, 0, 1, 2, 2], np.uint32)
    with _engine(case, item) as e:
        got = e.rollup_dense(rows, totals, group, 3, with_counts=True)
        _check(got, _truth(oracle, rows.astype(np.int64), totals, group, 3), "2^31 - 1")
        assert got[1][0, B] == 2 ** 31 - 1 and got[0]["count"][0] == 2 ** 31 - 1 and got[0]["p50"][0] == 5
        # 2^30 + 2^30 in group 1 of 2
        over = np.zeros((3, N.NBUCKETS), np.int32)
        over[0, 9] = 1
        over[1, B] = over[2, B] = 2 ** 30
        with pytest.raises(N.L5dhError, match="group 1") as ei:
            e.rollup_dense(over, None, np.array([0, 1, 1], np.uint32), 2)
        assert ei.value.code == -34
        # three members of 2^31 - 1 each: the sum passes 2^32 (one item, or one item per member)
        big = np.zeros((3, N.NBUCKETS), np.int32)
        big[:, 1000] = 2 ** 31 - 1
        with pytest.raises(N.L5dhError, match="group 0") as ei:
            e.rollup_dense(big, None, np.zeros(3, np.uint32), 1, with_counts=True)
        assert ei.value.code == -34
        # nine members: 9 (2^31 - 1) > 2^34; the two halves of u64 sums both matter
        big9 = np.zeros((9, N.NBUCKETS), np.int32)
        big9[:, 0] = 2 ** 31 - 1
        with pytest.raises(N.L5dhError) as ei:
            e.rollup_dense(big9, None, np.zeros(9, np.uint32), 1)
        assert ei.value.code == -34
        # a failing call resets nothing: the live state is what was ingested
        summ, counts = e.snapshot(reset=False, with_counts=True)
        np.testing.assert_array_equal(counts, case["counts"])
        _assert_summaries_equal(summ, case["series_want"], "state after -ERANGE")


def test_errors(case):
    with _engine(case) as e:
        bad = case["group"].copy()
        bad[77] = G  # neither < G nor NO_GROUP: found on the device, reported by this call
        with pytest.raises(N.L5dhError, match=r"group\[77\]") as ei:
            e.rollup(bad, G, reset=True, with_series=True)
        assert ei.value.code == -22
        summ, counts = e.snapshot(reset=False, with_counts=True)  # nothing was reset
        np.testing.assert_array_equal(counts, case["counts"])
        _assert_summaries_equal(summ, case["series_want"], "state after -EINVAL")
        e.sync()  # and nothing is left for l5dh_sync to report
        with pytest.raises(ValueError, match="ngroups"):
            e.rollup(case["group"], 0)
        with pytest.raises(ValueError, match="entries for 257 series"):
            e.rollup(case["group"][:-1], G)
        with pytest.raises(ValueError, match="dtype"):
            e.rollup(case["group"].astype(np.float32), G)
        # an empty range still writes ngroups empty results
        got = e.rollup(np.zeros(0, np.uint32), 3, first=5, count=0, with_counts=True)
        assert got[0].shape == (3,) and not got[0]["count"].any() and not got[1].any() and not got[2].any()
        assert not got[0]["avg"].any() and not got[0]["max"].any()
        # an int64 map with -1 for no group
        g64 = case["group"].astype(np.int64)
        g64[case["group"] == N.NO_GROUP] = -1
        _check(e.rollup(g64, G, with_counts=True), case["want"], "int64 map")


def test_end_to_end_tree_to_prometheus(oracle):
    from linkerd_amd.prometheus import PrometheusTelemeter, line_multiset, write_metrics
    from linkerd_amd.rollup import RollupPlan, plan_rollup, snapshot_histograms_rollup, write_rollup_metrics
    from linkerd_amd.telemetry import (HistogramSummary, MetricsTree, MetricsTreeStatsReceiver, StatEngine,
                                       snapshot_histograms)

    def build():
        eng = StatEngine(capacity=64, device=0, batch=128)
        tree = MetricsTree(eng)
        stats = MetricsTreeStatsReceiver(tree)
        rng = np.random.default_rng(21)
        fed = {}
        for r in ("http", "h2"):
            for c in ("a", "b", "c"):
                st = stats.scope("rt", r, "client", c).stat("request_latency_ms")
                vals = np.exp(3.0 + 1.5 * rng.standard_normal(70)).astype(np.float32)
                for v in vals:
                    st.add(float(v))
                fed.setdefault(r, []).extend(float(v) for v in vals)
        srv = stats.scope("rt", "http", "server", "x").stat("request_latency_ms")
        for v in (1.0, 20.0, 300.0):
            srv.add(v)
        return eng, tree, fed, srv

    eng, tree, fed, srv = build()
    plan = plan_rollup(tree, without=("client",), capacity=eng.capacity)
    assert plan.ngroups == 2 and plan.group_of[srv.series_id] == N.NO_GROUP
    summaries = snapshot_histograms_rollup(tree, eng, plan)
    text = PrometheusTelemeter(tree, rollups=(plan, summaries)).render()
    lines = line_multiset(text)
    for r in ("http", "h2"):
        one = oracle.PyStat()  # ONE oracle Stat fed the union of the router's samples
        for v in fed[r]:
            one.add(v)
        w = one.summary()
        hs = HistogramSummary(*[int(w[f]) for f in N.SUMMARY_FIELDS[:-1]], float(w["avg"]))
        want = []
        write_rollup_metrics(RollupPlan(plan.group_of, [("rt:client:request_latency_ms", (("rt", r),))]), [hs], want)
        assert len(want) == 11
        for ln in want:
            assert lines[ln.rstrip("\n")] == 1, ln
    # the per-series lines are those of a plain snapshot_histograms run
    eng2, tree2, _, _ = build()
    snapshot_histograms(tree2, eng2)
    plain, mine = [], []
    write_metrics(tree2, plain)
    write_metrics(tree, mine)
    assert sorted(plain) == sorted(mine) and len(plain) == 7 * 11
    assert sum(lines.values()) == 7 * 11 + 2 * 11
    eng.engine.close()
    eng2.engine.close()
