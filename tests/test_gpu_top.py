"""GPU exact top-k (l5dh_top, l5dh_top_summaries) against Python's sorted().

The truth everywhere: sorted() over the candidates -- count >= min_count and (no map or
group[i] == g) -- with the key (ordered key descending or ascending, id ascending).  The
ordered key of an int64 field is the integer; the ordered key of avg is built here from the
double's bits (struct), IEEE total order, never from the library.  Live engines are checked
against the CPU oracle's summaries and l5do_percentile.
"""
import struct

import numpy as np
import pytest

from linkerd_amd import _native as N
from linkerd_amd.admin_metrics import STAT_FIELDS, json_string
from linkerd_amd.javafmt import double_to_string, long_to_string
from linkerd_amd.telemetry import HistogramSummary, MetricsTree, MetricsTreeStatsReceiver, StatEngine, top_stats
from linkerd_amd.top import TopStatsHandler

from tests.test_gpu_quantiles import truth as q_truth

pytestmark = pytest.mark.gpu

CHUNK, LIMIT = N.TOP_CHUNK, N.TOP_LIMIT
I64_MIN, I64_MAX = -2 ** 63, 2 ** 63 - 1
GUARD32, GUARD64 = 0xA5A5A5A5, 0x5A5A5A5A5A5A5A5A
EINVAL = -22


# ---- the truth ---------------------------------------------------------------------------
def avg_key(x: float) -> int:
    """IEEE total order of the double's bits as an unsigned integer."""
    (bits,) = struct.unpack("<Q", struct.pack("<d", x))
    return bits ^ (0xFFFFFFFFFFFFFFFF if bits >> 63 else 1 << 63)


def keys_of(values, by):
    if by == "avg":
        raw = values["avg"].view(np.uint64).tolist()  # (the bits, whatever NaN payload)
        return [b ^ (0xFFFFFFFFFFFFFFFF if b >> 63 else 1 << 63) for b in raw]
    return values[by].tolist()


def top_truth(keys, counts, k, order="largest", min_count=1, group=None, g=0, first=0):
    cand = [i for i in range(len(keys)) if counts[i] >= min_count and (group is None or group[i] == g)]
    sign = -1 if order == "largest" else 1
    return [first + i for i in sorted(cand, key=lambda i: (sign * keys[i], i))[:k]]


def test_avg_key_is_the_total_order():
    nan = struct.unpack("<d", struct.pack("<Q", 0x7FF8000000000000))[0]
    nnan = struct.unpack("<d", struct.pack("<Q", 0xFFF8000000000000))[0]
    seq = [nnan, -np.inf, -1.7976931348623157e308, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, 1.7976931348623157e308, np.inf,
           nan]
    ks = [avg_key(x) for x in seq]
    assert ks == sorted(ks) and len(set(ks)) == len(ks)


# ---- running a selection behind guards ------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _host(x):
    return x if isinstance(x, np.ndarray) else x.cpu().numpy()


def select(e, values, k, by, order="largest", min_count=1, group=None, g=0, device=False):
    """(ids, summaries, n) of top_into over external summaries, the outputs behind guard
    words: nothing past n entries may change.  device: every buffer is a torch tensor."""
    ids = np.full(k + 4, GUARD32, np.uint32).view(np.int32)
    top = np.full((k + 2) * 11, GUARD64, np.int64)
    n_out = np.full(2, GUARD32, np.uint32).view(np.int32)
    vals = values
    if device:
        ids, top, n_out = _dev(ids), _dev(top), _dev(n_out)
        vals = _dev(values.view(np.int64).reshape(-1))
        group = None if group is None else _dev(group.view(np.int32))
    e.top_into(k, by, ids, n_out, top, order=order, min_count=min_count, group=group, g=g, values=vals)
    ids, top, n_out = (_host(x) for x in (ids, top, n_out))
    n = int(n_out.view(np.uint32)[0])
    assert n_out.view(np.uint32)[1] == GUARD32
    assert 0 <= n <= k
    assert (ids.view(np.uint32)[n:] == GUARD32).all(), "ids written past n_out"
    assert (top[n * 11:] == GUARD64).all(), "summaries written past n_out"
    return ids.view(np.uint32)[:n].copy(), top[:n * 11].view(N.SUMMARY_DTYPE).copy(), n


def check(e, values, k, by, want=None, **kw):
    ids, top, n = select(e, values, k, by, **{x: kw[x] for x in kw if x != "first"})
    if want is None:
        want = top_truth(keys_of(values, by), values["count"].tolist(), k, **kw)
    assert n == len(want)
    assert ids.tolist() == want, (by, k, kw.get("order"), ids[:8], want[:8])
    assert top.tobytes() == values[ids].tobytes()
    return ids


@pytest.fixture(scope="module")
def eng(gpu_available):
    from linkerd_amd.engine import HistogramEngine
    with HistogramEngine(32) as e:
        yield e


_CRAFTED = {}


def crafted(n):
    """n summaries with many equal p99 keys and counts 0..2 (a third are no candidates)."""
    if n not in _CRAFTED:
        rng = np.random.default_rng(n)
        v = np.zeros(n, N.SUMMARY_DTYPE)
        for f in N.SUMMARY_FIELDS[:-1]:
            v[f] = rng.integers(-50, 50, n)
        v["count"] = rng.integers(0, 3, n)
        v["p99"] = rng.integers(0, max(2, n // 7), n)
        v["avg"] = rng.standard_normal(n)
        _CRAFTED[n] = (v, keys_of(v, "p99"), v["count"].tolist())
    return _CRAFTED[n]


# ---- shapes of the tournament ---------------------------------------------------------------
SHAPE_N = [1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1, 17 * CHUNK + 5]
SHAPE_K = [1, 2, 63, 64, 65, 1000, 1024]


def test_constants():
    assert CHUNK == 4096 and LIMIT == 1024 and SHAPE_K[-1] == LIMIT
    # 17 chunks + 5 rows at k = 1024 (fan-in 4): 18 lists -> 5 -> 2 -> 1, three merge levels
    assert -(-SHAPE_N[-1] // CHUNK) > (CHUNK // LIMIT) ** 2


@pytest.mark.parametrize("n", SHAPE_N)
@pytest.mark.parametrize("k", SHAPE_K)
def test_shapes(eng, n, k):
    v, keys, counts = crafted(n)
    order = "largest" if (n + k) % 2 else "smallest"
    want = top_truth(keys, counts, k, order=order)
    check(eng, v, k, "p99", want=want, order=order)


def test_fewer_candidates_than_k_and_none(eng):
    n = 2 * CHUNK + 1
    v, keys, counts = crafted(n)
    group = np.full(n, N.NO_GROUP, np.uint32)
    members = [5, CHUNK - 1, CHUNK, 2 * CHUNK]
    group[members] = 3
    v = v.copy()
    v["count"][members] = 1
    for k in (1, 3, 4, 5, 64, 1024):
        ids = check(eng, v, k, "p99", group=group, g=3)
        assert len(ids) == min(k, 4)
    # zero candidates: n_out = 0 and nothing is written (the guards in select())
    ids, top, n0 = select(eng, v, 7, "p99", min_count=10 ** 12)
    assert n0 == 0 and ids.size == 0
    ids, top, n0 = select(eng, v, 1024, "count", group=group, g=4)
    assert n0 == 0


# ---- ties -----------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["largest", "smallest"])
def test_ties_all_equal(eng, order):
    n = 2 * CHUNK + 1
    v = np.zeros(n, N.SUMMARY_DTYPE)
    v["count"], v["p99"] = 1, 77
    for k in (1, 65, 1024):
        ids, _, _ = select(eng, v, k, "p99", order=order)
        assert ids.tolist() == list(range(k))


@pytest.mark.parametrize("order", ["largest", "smallest"])
def test_ties_kth_place_inside_a_run_across_a_chunk_boundary(eng, order):
    n = 2 * CHUNK + 1
    v = np.zeros(n, N.SUMMARY_DTYPE)
    v["count"], v["max"] = 1, 10
    run = np.arange(CHUNK - 30, CHUNK + 30)
    v["max"][run] = 20 if order == "largest" else 5   # the run of winners straddles chunks 0 | 1
    for k in (29, 30, 31, 40, 60, 61):
        ids = check(eng, v, k, "max", order=order)
        assert ids.tolist() == (run.tolist() + list(range(n)))[:k] if k <= 60 else ids[:60].tolist() == run.tolist()
    # and the k-th place inside the run of the OTHER value, which starts before the boundary
    ids = check(eng, v, 100, "max", order=order)
    assert ids[60:].tolist() == list(range(40))


def test_winners_only_in_the_last_chunk_and_one_per_chunk(eng):
    n = 17 * CHUNK + 5
    v = np.zeros(n, N.SUMMARY_DTYPE)
    v["count"] = 1
    v["sum"] = np.arange(n) % 1000
    last = np.arange(17 * CHUNK, n)
    v["sum"][last] = 10 ** 9 + np.arange(5)
    ids = check(eng, v, 5, "sum")
    assert ids.tolist() == last[::-1].tolist()
    check(eng, v, 1024, "sum")
    w = np.zeros(n, N.SUMMARY_DTYPE)
    w["count"] = 1
    one = np.array([c * CHUNK + (c * 37) % CHUNK for c in range(18) if c * CHUNK + (c * 37) % CHUNK < n])
    w["p50"][one] = 1000 + np.arange(one.size)
    for k in (one.size, 64, 1024):
        ids = check(eng, w, k, "p50")
        assert ids[:one.size].tolist() == one[::-1].tolist()


# ---- key domains ------------------------------------------------------------------------------
def domain_values():
    edges = np.array([I64_MIN, -1, 0, I64_MAX, 1, I64_MIN + 1, I64_MAX - 1, -2 ** 31, 2 ** 31, 12345], np.int64)
    bits = np.array([0x0000000000000000, 0x8000000000000000, 0x7FF0000000000000, 0xFFF0000000000000,
                     0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001, 0xFFFFFFFFFFFFFFFF,
                     0x0000000000000001, 0x8000000000000001, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF,
                     0x3FF8000000000000, 0xBFF8000000000000], np.uint64)  # +-0, +-Inf, +-NaN, payloads, denormals, max, 1.5
    n = 3 * edges.size * bits.size // 2
    v = np.zeros(n, N.SUMMARY_DTYPE)
    i = np.arange(n)
    mults = (1, 3, 7, 9, 11, 13, 17, 19, 21, 23)  # coprime with the 10 edges: every field holds every edge
    for f, name in enumerate(N.SUMMARY_FIELDS[:-1]):
        v[name] = edges[(i * mults[f] + f) % edges.size]
    v["avg"] = bits[(i * 5) % bits.size].view(np.float64)
    return v


@pytest.mark.parametrize("order", ["largest", "smallest"])
@pytest.mark.parametrize("by", N.SUMMARY_FIELDS)
def test_key_domains(eng, by, order):
    v = domain_values()
    assert {I64_MIN, -1, 0, I64_MAX} <= set(v[by].tolist()) or by == "avg"
    # min_count at INT64_MIN is illegal; 0 drops the negative counts, which is a filter test
    # of its own -- so rank rows of every count with the filter wide open through a copy
    w = v.copy()
    if by != "count":
        w["count"] = 1
    for k in (1, 7, v.size, 1024):
        check(eng, w, k, by, order=order, min_count=0 if by == "count" else 1)


# ---- filters ----------------------------------------------------------------------------------
def test_min_count_boundary_and_empty_rows(eng):
    n = 100
    v = np.zeros(n, N.SUMMARY_DTYPE)
    v["count"] = np.arange(n) % 10
    v["p99"] = (np.arange(n) * 7) % 13
    for mc in (0, 1, 5, 9, 10):
        ids = check(eng, v, 1024, "p99", min_count=mc)
        assert set(ids.tolist()) == {i for i in range(n) if i % 10 >= mc}  # == min_count in, one less out
    ids = check(eng, np.zeros(10, N.SUMMARY_DTYPE), 4, "max", min_count=0)
    assert ids.tolist() == [0, 1, 2, 3]                                  # empty rows admitted, ties by id
    _, _, n0 = select(eng, np.zeros(10, N.SUMMARY_DTYPE), 4, "max", min_count=1)
    assert n0 == 0


def test_group_members_only(eng):
    n = CHUNK + 77
    v, _, _ = crafted(CHUNK + 1)
    v = np.concatenate([v, v[:76]])
    rng = np.random.default_rng(5)
    group = rng.integers(0, 4, n).astype(np.uint32)
    group[::5] = N.NO_GROUP
    group[1::7] = 10 ** 6       # beyond any group count: simply not a member
    group[2::11] = 0xFFFFFFFE
    for g in (0, 3, 10 ** 6, N.NO_GROUP):   # (NO_GROUP as g selects the rows that carry it: a value like any other)
        check(eng, v, 200, "p99", group=group, g=g)
    _, _, n0 = select(eng, v, 200, "p99", group=group, g=17)  # g has no member
    assert n0 == 0
    # an int64 map with -1 for "no group" is converted
    gi = np.where(group == N.NO_GROUP, -1, group.astype(np.int64))
    ids, _, _ = select(eng, v, 50, "p99", group=gi, g=3)
    assert ids.tolist() == top_truth(keys_of(v, "p99"), v["count"].tolist(), 50, group=group, g=3)


# ---- outputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,k", [(CHUNK + 1, 65), (17 * CHUNK + 5, 1024), (3, 8)])
def test_host_and_device_buffers_agree(eng, n, k):
    v, _, _ = crafted(n)
    group = (np.arange(n) % 3).astype(np.uint32)
    for by, order in (("p99", "largest"), ("avg", "smallest")):
        h = select(eng, v, k, by, order=order, group=group, g=1)
        d = select(eng, v, k, by, order=order, group=group, g=1, device=True)
        assert h[2] == d[2] and h[0].tobytes() == d[0].tobytes() and h[1].tobytes() == d[1].tobytes()
        assert h[1].tobytes() == v[h[0]].tobytes()
        again = select(eng, v, k, by, order=order, group=group, g=1)
        assert again[0].tobytes() == h[0].tobytes()  # the same on every run


def test_top_summaries_wrapper(eng):
    v, keys, counts = crafted(CHUNK + 1)
    ids, summ = eng.top_summaries(v, 20, "p99")
    assert ids.dtype == np.uint32 and summ.dtype == N.SUMMARY_DTYPE
    assert ids.tolist() == top_truth(keys, counts, 20) and summ.tobytes() == v[ids].tobytes()
    ids, summ = eng.top_summaries(np.zeros(0, N.SUMMARY_DTYPE), 20, "p99")
    assert ids.size == 0 and summ.size == 0
    with pytest.raises(ValueError):
        eng.top_summaries(v, 20, 0.5)  # a quantile needs buckets: live state only


# ---- live engines -------------------------------------------------------------------------------
def samples(S, n, seed):
    rng = np.random.default_rng(seed)
    series = rng.integers(0, S, size=n, dtype=np.uint32)
    # a third of the series stay empty, so min_count and clean tiles matter
    series = np.where(series % 3 == 1, (series + 1) % S, series).astype(np.uint32)
    vals = np.exp(3.0 + 2.0 * rng.standard_normal(n)).astype(np.float32)
    vals[:12] = np.array([0, 113, 3030, 1e9, 3e9, -5, 0, 113, 3030, 1e9, 3e9, -5], np.float32)
    return series, vals


class Live:
    def __init__(self, oracle, S, seed):
        from linkerd_amd.engine import HistogramEngine
        self.S = S
        self.e = HistogramEngine(S)
        self.e.set_param(N.PARAM_STAGE_SAMPLES, 8192)
        self.ref = oracle.OracleHistograms(S)
        self.feed(20_000, seed)       # binned at once
        self.feed(1_500, seed + 1)    # stays in the staging ring until the query

    def feed(self, n, seed):
        s, v = samples(self.S, n, seed)
        self.e.ingest(s, v)
        self.ref.ingest(s, v)


@pytest.fixture(scope="module", params=[257, 2049])
def live(request, oracle, gpu_available):
    L = Live(oracle, request.param, 11)
    yield L
    L.e.close()


def test_live_fields(oracle, live):
    want = live.ref.snapshot(reset=False)
    counts = want["count"].tolist()
    assert 0 in counts and max(counts) > 1
    for by, order, k in (("p99", "largest", 20), ("count", "smallest", 64), ("sum", "largest", 5),
                         ("avg", "largest", 100), ("avg", "smallest", 1024)):
        ids, summ = live.e.top(k, by, order=order)
        truth_ids = top_truth(keys_of(want, by), counts, k, order=order)
        assert ids.tolist() == truth_ids, (by, order)
        assert summ.tobytes() == want[ids].tobytes()
    # min_count = 0: the empty series rank too (count ascending: they come first, by id)
    ids, summ = live.e.top(10, "count", order="smallest", min_count=0)
    assert ids.tolist() == top_truth(counts, counts, 10, order="smallest", min_count=0)
    assert not summ["count"].any()


@pytest.mark.parametrize("q", [0.0, 0.25, 0.995, 1.0])
def test_live_quantile(oracle, live, q):
    want = live.ref.snapshot(reset=False)
    qv = q_truth(oracle, live.ref.h, [q])[:, 0]
    for order in ("largest", "smallest"):
        ids, summ, qvals = live.e.top(33, q, order=order)
        assert ids.tolist() == top_truth(qv.tolist(), want["count"].tolist(), 33, order=order)
        assert qvals.dtype == np.int64 and qvals.tolist() == qv[ids].tolist()
        assert summ.tobytes() == want[ids].tobytes()
    if q == 1.0:  # percentile(1) of a non-empty row is its max
        assert live.e.top(33, q)[0].tolist() == live.e.top(33, "max")[0].tolist()


def test_live_unaligned_range_series_and_group(oracle, live):
    want = live.ref.snapshot(reset=False)
    first, count = 33, 100
    ids, summ, series = live.e.top(7, "p99", first=first, count=count, with_series=True)
    sub = want[first:first + count]
    assert ids.tolist() == top_truth(keys_of(sub, "p99"), sub["count"].tolist(), 7, first=first)  # absolute ids
    assert summ.tobytes() == want[ids].tobytes()
    assert series.tobytes() == live.e.snapshot(first=first, count=count, reset=False).tobytes() == sub.tobytes()
    group = (np.arange(count) % 4).astype(np.uint32)
    ids, _ = live.e.top(50, "max", first=first, count=count, group=group, g=2)
    assert ids.tolist() == top_truth(keys_of(sub, "max"), sub["count"].tolist(), 50, group=group, g=2, first=first)
    # device buffers, the quantile values included
    import torch
    d_ids, d_n = torch.zeros(16, dtype=torch.int32, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0")
    d_top = torch.zeros(16 * 11, dtype=torch.int64, device="cuda:0")
    d_q = torch.zeros(16, dtype=torch.int64, device="cuda:0")
    live.e.top_into(16, 0.995, d_ids, d_n, d_top, d_q, first=first, count=count)
    h = live.e.top(16, 0.995, first=first, count=count)
    m = int(d_n.cpu()[0])
    assert m == len(h[0]) and d_ids.cpu().numpy()[:m].tolist() == h[0].tolist()
    assert d_top.cpu().numpy()[:m * 11].tobytes() == h[1].tobytes() and d_q.cpu().numpy()[:m].tolist() == h[2].tolist()


def test_live_reset_sees_the_same_samples(oracle, gpu_available):
    L = Live(oracle, 2049, 23)
    try:
        want = L.ref.snapshot(reset=False)
        before = L.e.top(40, "p99")
        ids, summ, qv, series = L.e.top(40, 0.25, reset=True, with_series=True)
        assert series.tobytes() == want.tobytes()
        qt = q_truth(oracle, L.ref.h, [0.25])[:, 0]
        assert ids.tolist() == top_truth(qt.tolist(), want["count"].tolist(), 40) and qv.tolist() == qt[ids].tolist()
        assert before[0].tolist() == top_truth(keys_of(want, "p99"), want["count"].tolist(), 40)
        assert not L.e.snapshot(reset=False).view(np.uint8).any()  # the range was cleared
        L.ref.snapshot(reset=True)
        # clean tiles rank as count 0
        assert L.e.top(5, "p99")[0].size == 0
        ids, summ = L.e.top(5, "count", min_count=0)
        assert ids.tolist() == [0, 1, 2, 3, 4] and not summ.view(np.uint8).any()
        # a ranking by a field resets too, and returns the ranking of what it cleared
        L.feed(3_000, 31)
        want = L.ref.snapshot(reset=False)
        ids, summ = L.e.top(12, "sum", reset=True)
        assert summ.tobytes() == want[ids].tobytes()
        assert not L.e.snapshot(reset=False).view(np.uint8).any()
    finally:
        L.e.close()


def test_one_tile_engine(oracle, gpu_available):
    from linkerd_amd.engine import HistogramEngine
    S = 32
    s, v = samples(S, 5_000, 3)
    ref = oracle.OracleHistograms(S)
    ref.ingest(s, v)
    want = ref.snapshot(reset=False)
    with HistogramEngine(S) as e:
        e.ingest(s, v)
        for by in ("p99", "count", "avg"):
            ids, summ = e.top(5, by)
            assert ids.tolist() == top_truth(keys_of(want, by), want["count"].tolist(), 5)
            assert summ.tobytes() == want[ids].tobytes()
        ids, summ, qv = e.top(5, 0.75, order="smallest")
        qt = q_truth(oracle, ref.h, [0.75])[:, 0]
        assert ids.tolist() == top_truth(qt.tolist(), want["count"].tolist(), 5, order="smallest")


# ---- errors ---------------------------------------------------------------------------------------
def test_errors_write_and_reset_nothing(oracle, gpu_available):
    L = Live(oracle, 257, 41)
    try:
        e, lib, ctx, S = L.e, L.e._lib, L.e._ctx, 257
        e.sync()
        before = e.export_state(reset=False)
        ids = np.full(LIMIT + 1, GUARD32, np.uint32)
        top = np.full((LIMIT + 1) * 11, GUARD64, np.int64)
        qo = np.full(LIMIT + 1, GUARD64, np.int64)
        n_out = np.full(1, GUARD32, np.uint32)
        series = np.full(S * 11, GUARD64, np.int64)
        group = np.zeros(S, np.uint32)
        I, T, Q, NO, SE, G = (a.ctypes.data for a in (ids, top, qo, n_out, series, group))
        vals = np.zeros(4, N.SUMMARY_DTYPE)
        V = vals.ctypes.data
        nan = float("nan")

        def live_call(first=0, count=S, by=N.BY_P99, q=0.5, order=0, min_count=1, k=5, ids_p=I, n_p=NO):
            return lib.l5dh_top(ctx, first, count, by, q, order, min_count, G, 0, k, ids_p, T, Q, n_p, SE, 1)

        def ext_call(values=V, n=4, by=N.BY_P99, order=0, min_count=1, k=5, ids_p=I, n_p=NO):
            return lib.l5dh_top_summaries(ctx, values, n, by, order, min_count, G, 0, k, ids_p, T, n_p)

        bad_live = [dict(k=0), dict(k=LIMIT + 1), dict(by=-1), dict(by=12), dict(order=2), dict(order=-1),
                    dict(min_count=-1), dict(by=N.BY_QUANTILE, q=nan), dict(by=N.BY_QUANTILE, q=-0.001),
                    dict(by=N.BY_QUANTILE, q=1.001), dict(first=1, count=S), dict(first=S + 1, count=0),
                    dict(ids_p=None), dict(n_p=None), dict(count=0, k=0)]
        for kw in bad_live:
            assert live_call(**kw) == EINVAL, kw
        bad_ext = [dict(k=0), dict(k=LIMIT + 1), dict(by=-1), dict(by=N.BY_QUANTILE), dict(by=12), dict(order=2),
                   dict(min_count=-1), dict(n=(1 << 24) + 1), dict(ids_p=None), dict(n_p=None), dict(values=None)]
        for kw in bad_ext:
            assert ext_call(**kw) == EINVAL, kw
        for a, guard in ((ids, GUARD32), (top, GUARD64), (qo, GUARD64), (n_out, GUARD32), (series, GUARD64)):
            assert (a == guard).all()
        assert e.export_state(reset=False)[0].tobytes() == before[0].tobytes()
        assert e.export_state(reset=False)[1].tobytes() == before[1].tobytes()
        # q is ignored unless by == BY_QUANTILE; count == 0 / n == 0 set n_out = 0
        assert lib.l5dh_top(ctx, 0, S, N.BY_P99, nan, 0, 1, None, 0, 5, I, None, None, NO, None, 0) == 0
        assert n_out[0] == 5
        assert live_call(first=S, count=0) == 0 and n_out[0] == 0
        n_out[0] = GUARD32
        assert ext_call(values=None, n=0) == 0 and n_out[0] == 0
        # the Python face reports its own argument errors before the library is called
        for kw in (dict(k=0), dict(k=LIMIT + 1), dict(by="p98"), dict(order="biggest"), dict(first=200, count=100)):
            with pytest.raises(ValueError):
                e.top(**{"k": 5, **kw})
        with pytest.raises(N.L5dhError):
            e.top(5, 1.5)
    finally:
        L.e.close()


# ---- StatEngine, telemetry and the admin handler ------------------------------------------------
def small_tree(engine):
    """A tree of the shape tests/test_gpu_render.stat_tree builds: bare keys, then labelled
    Stats under rt/<router>/client/<client>."""
    tree = MetricsTree(engine)
    stats = MetricsTreeStatsReceiver(tree)
    out = []
    for j in range(60):
        if j < 8:
            out.append(stats.stat(("abcdefghij" * 4)[:j + 1]))
        elif j == 8:
            out.append(stats.scope("rt", "http", "client", 'é√日本"\\\n').stat("request_latency_ms"))
        else:
            out.append(stats.scope("rt", f"router{j % 7}", "client", f"$inet$10.0.0.{j}$8080").stat(
                "request_latency_ms"))
    return tree, out


def expected_json(items):
    parts = []
    for path, s, *rest in items:
        fields = [("name", json_string("/".join(path))), ("count", long_to_string(int(s["count"])))]
        fields += [(f, long_to_string(int(s[f]))) for f in STAT_FIELDS]
        fields += [("avg", double_to_string(float(s["avg"])))]
        fields += [("quantile", long_to_string(int(x))) for x in rest]
        parts.append("{" + ",".join(f'"{k}":{v}' for k, v in fields) + "}")
    return "[" + ",".join(parts) + "]"


def test_stat_engine_top_stats_and_handler(oracle, gpu_available):
    se = StatEngine(capacity=256, batch=1 << 12)
    try:
        tree, stats = small_tree(se)
        ref = oracle.OracleHistograms(256)
        rng = np.random.default_rng(9)
        path_of = {m.series_id: p for p, t in tree.walk() for m in [t.metric] if hasattr(m, "series_id")}
        assert len(path_of) == 60
        for j, m in enumerate(stats):
            if j % 4 == 3:
                continue  # empty Stats never rank with min_count >= 1
            vals = np.exp(2.0 + 0.05 * j + rng.standard_normal(50)).astype(np.float32)
            for x in vals:
                m.add(float(x))
            ref.ingest(np.full(vals.size, m.series_id, np.uint32), vals)
        # a released id has a zero row
        gone = stats[20]
        gone_id = gone.series_id
        tree.resolve(("rt", "router6", "client", "$inet$10.0.0.20$8080")).prune()
        ref.h[gone_id] = np.zeros((), oracle.HIST_DTYPE)
        del path_of[gone_id]
        want = ref.snapshot(reset=False)
        counts = want["count"].tolist()

        ids, summ = se.top(10, "p99")
        truth_ids = top_truth(keys_of(want, "p99"), counts, 10)
        assert ids.tolist() == truth_ids and gone_id not in truth_ids and summ.tobytes() == want[ids].tobytes()

        got = top_stats(tree, se, 10, by="p99")
        assert [p for p, _ in got] == [path_of[i] for i in truth_ids]
        assert [s for _, s in got] == [HistogramSummary.from_record(want[i]) for i in truth_ids]

        # scope restricts the candidates
        scope = ("rt", "router3")
        member = np.array([1 if path_of.get(i, ())[:2] == scope else 0 for i in range(256)])
        scoped = top_truth(keys_of(want, "max"), counts, 100, order="smallest", group=member, g=1)
        got = top_stats(tree, se, 100, by="max", order="smallest", scope=scope)
        assert 0 < len(scoped) < 10 and [p for p, _ in got] == [path_of[i] for i in scoped]
        assert top_stats(tree, se, 5, scope=("no", "such")) == []
        # min_count = 0: the empty Stats rank, rows no Stat owns never do
        owned = np.array([1 if i in path_of else 0 for i in range(256)])
        got = top_stats(tree, se, 1024, by="count", order="smallest", min_count=0)
        assert [p for p, _ in got] == [path_of[i] for i in top_truth(counts, counts, 1024, order="smallest", min_count=0,
                                                                      group=owned, g=1)]
        assert len(got) == 59
        # by a quantile: the value rides along
        qt = q_truth(oracle, ref.h, [0.995])[:, 0]
        got = top_stats(tree, se, 6, by=0.995)
        q_ids = top_truth(qt.tolist(), counts, 6)
        assert [(p, q) for p, _, q in got] == [(path_of[i], int(qt[i])) for i in q_ids]

        h = TopStatsHandler(tree, se)
        assert h.path == "/admin/metrics/top.json"
        status, media, body = h.handle("/admin/metrics/top.json")
        top20 = top_truth(keys_of(want, "p99"), counts, 20)
        assert (status, media) == (200, "application/json")
        assert body == expected_json([(path_of[i], want[i]) for i in top20])
        status, _, body = h.handle("/admin/metrics/top.json?by=max&order=smallest&k=100&q=rt/router3")
        assert status == 200 and body == expected_json([(path_of[i], want[i]) for i in scoped])
        status, _, body = h.handle("/admin/metrics/top.json?by=q0.995&k=6")
        assert status == 200 and body == expected_json([(path_of[i], want[i], qt[i]) for i in q_ids])
        status, _, body = h.handle("/admin/metrics/top.json?by=count&min_count=0&order=smallest&k=3&q=rt/http")
        assert status == 200 and body == expected_json([(path_of[stats[8].series_id], want[stats[8].series_id])])
        assert h.handle("/admin/metrics/top.json?q=rt/nope") == (404, "application/json",
                                                                 '{"error": "No such subtree: rt/nope"}')
        for bad in ("by=p98", "by=q1.5", "by=qx", "k=0", "k=1025", "k=ten", "order=up", "min_count=-1"):
            status, media, body = h.handle("/admin/metrics/top.json?" + bad)
            assert status == 400 and media == "application/json" and body.startswith('{"error": "'), bad
    finally:
        se.engine.close()
