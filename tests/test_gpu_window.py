"""GPU sliding windows (l5dh_window_*, linkerd_amd.window.Window) and what StatEngine builds
on them (push_window, window_summaries, release, grow).

Truth is the oracle throughout: per interval an oracle.OracleHistograms receives the
interval's samples; the expected window is oracle.summarize_counts of the summed rows and
totals of the last w intervals and, once per test, the summary of ONE oracle that received
all of those samples.  Summaries, rows and totals are compared as bytes.
"""
import numpy as np
import pytest

from linkerd_amd import _native as N

pytestmark = pytest.mark.gpu

NB = N.NBUCKETS
INT_MAX = 2 ** 31 - 1
EINVAL, ERANGE, EEXIST = -22, -34, -17
EDGE = np.array([0, 1, 2, 113, 3030, 1e9, 3e9, -5], np.float32)  # smoke()'s edge values (escapes: sumfix)


def _engine(n, stage=None):
    from linkerd_amd.engine import HistogramEngine
    e = HistogramEngine(n)
    if stage is not None:
        e.set_param(N.PARAM_STAGE_SAMPLES, stage)
    return e


def _window(e, slots):
    from linkerd_amd.window import Window
    return Window(e, slots)


def _batch(seed, S, n, quiet=()):
    rng = np.random.default_rng(seed)
    live = np.array([s for s in range(S) if s not in quiet], np.uint32)
    series = live[rng.integers(0, live.size, size=n)]
    vals = np.exp(3.0 + 1.5 * rng.standard_normal(n)).astype(np.float32)
    vals[:8] = EDGE
    return series, vals


def _bucket_values(buckets):
    """One float32 per bucket that lands in it: the middle of its limits from N.limits() (0 for
    bucket 0, 3e9 for the overflow bucket)."""
    L = N.limits().astype(np.int64)
    b = np.asarray(buckets, np.int64)
    lo = np.where(b == 0, 0, L[np.clip(b - 1, 0, 1796)])
    hi = L[np.clip(b, 0, 1796)]
    v = ((lo + hi) // 2).astype(np.float32)
    v[b == 0] = 0.0
    v[b == 1797] = 3e9
    return v


class Truth:
    """The oracle's rows and totals of every pushed interval."""

    def __init__(self, oracle, S):
        self.O, self.S, self.rows, self.totals, self.samples = oracle, S, [], [], []

    def interval(self, series, vals):
        ref = self.O.OracleHistograms(self.S)
        assert ref.ingest(series, vals) == 0
        self.rows.append(ref.counts().astype(np.int64))
        self.totals.append(ref.totals().copy())
        self.samples.append((series, vals))
        return ref

    def window(self, last, extra=None, mask=None):
        """(rows int32, totals int64, summaries) of the last ``last`` intervals (+ extra =
        (rows, totals)); mask [interval][S] bool: the rows that count."""
        rows, tot = np.zeros((self.S, NB), np.int64), np.zeros(self.S, np.int64)
        n = len(self.rows)
        for k in range(n - last, n):
            keep = np.ones(self.S, bool) if mask is None else mask[k]
            rows += self.rows[k] * keep[:, None]
            tot += self.totals[k] * keep
        if extra is not None:
            rows, tot = rows + extra[0], tot + extra[1]
        assert rows.max(initial=0) <= INT_MAX
        rows = rows.astype(np.int32)
        return rows, tot, self.O.summarize_counts(rows, tot)

    def one_oracle(self, last, more=()):
        ref = self.O.OracleHistograms(self.S)
        for s, v in self.samples[len(self.samples) - last:] + list(more):
            assert ref.ingest(s, v) == 0
        return ref.snapshot(reset=False)


def _check(win, truth, last, what="", first=0, count=None, **kw):
    count = truth.S - first if count is None else count
    got, rows, tot = win.summaries(last, first=first, count=count, with_counts=True, with_totals=True,
                                   include_open=kw.get("include_open", False))
    w_rows, w_tot, w_summ = truth.window(last, kw.get("extra"), kw.get("mask"))
    sl = slice(first, first + count)
    if rows.tobytes() != w_rows[sl].tobytes():
        s, b = np.argwhere(rows != w_rows[sl])[0]
        raise AssertionError(f"{what} last={last}: series {first + s} bucket {b}: "
                             f"got {rows[s, b]} want {w_rows[sl][s, b]}")
    assert tot.tobytes() == w_tot[sl].tobytes(), f"{what} last={last}: totals"
    assert got.tobytes() == w_summ[sl].tobytes(), f"{what} last={last}: summaries"
    return got


# ---- 1. ring order and wrap --------------------------------------------------------------------------
@pytest.mark.parametrize("S", [70, 20])  # three tiles, the last partial; the one-tile path with its sumfix
def test_ring_order_and_wrap(oracle, gpu_available, S):
    e, twin = _engine(S), _engine(S)
    win, truth = _window(e, 3), Truth(oracle, S)
    for i in range(5):
        s, v = _batch(10 + i, S, 3000 + 500 * i, quiet=range(32, 64) if i == 1 else ())
        e.ingest(s, v)
        twin.ingest(s, v)
        truth.interval(s, v)
        got = win.push(with_series=True)
        assert got.tobytes() == twin.snapshot(reset=True).tobytes(), f"push {i + 1}"
        filled = min(i + 1, 3)
        assert win.info()["filled"] == filled and win.info()["pushes"] == i + 1
        for last in range(1, filled + 1):
            _check(win, truth, last, f"S={S} after push {i + 1}")
        # (the class refuses it first; the library does too)
        assert e._lib.l5dh_window_query(e._ctx, 0, S, filled + 1, 0, None, None, None) == EINVAL
        assert e._lib.l5dh_window_query(e._ctx, 0, S, 0, 0, None, None, None) == EINVAL
        assert e._lib.l5dh_window_query(e._ctx, 1, S, 1, 0, None, None, None) == EINVAL
        with pytest.raises(ValueError):
            win.summaries(filled + 1)
    assert win.summaries(3).tobytes() == truth.one_oracle(3).tobytes()
    assert win.summaries(1).tobytes() == truth.one_oracle(1).tobytes()
    e.close()
    twin.close()


# ---- 2. row shapes ---------------------------------------------------------------------------------
def _shaped(rows_of):
    """Samples that give series s one sample in each bucket of rows_of[s]."""
    series = np.concatenate([np.full(len(b), s, np.uint32) for s, b in rows_of.items()])
    vals = np.concatenate([_bucket_values(b) for b in rows_of.values()])
    return series, vals


def test_row_shapes(oracle, gpu_available):
    S = 70
    rng = np.random.default_rng(5)
    pick = lambda n: np.sort(rng.choice(NB, size=n, replace=False))  # noqa: E731
    # interval A: tile 1 (series 32..63) stays clean; series 0 empty
    a = {1: [900], 2: pick(65), 3: pick(200), 4: np.arange(NB), 5: [0, 1797], 69: pick(64)}
    # interval B: the shapes move; series 4, 5 and tile 2 are empty, tile 1 is not
    b = {0: [1797], 2: pick(200), 3: pick(65), 40: np.arange(NB), 33: [0], 6: pick(129)}
    e = _engine(S)
    win, truth = _window(e, 2), Truth(oracle, S)
    for rows_of in (a, b):
        s, v = _shaped(rows_of)
        ref = truth.interval(s, v)
        for sid, bs in rows_of.items():  # every sample landed where it was aimed
            assert np.array_equal(np.flatnonzero(ref.counts()[sid]), np.asarray(bs)) and ref.counts()[sid].max() == 1
        e.ingest(s, v)
        win.push()
    assert (truth.rows[0][4] == 1).all() and not truth.rows[0][32:64].any() and not truth.rows[1][64:].any()
    for last in (1, 2):
        _check(win, truth, last, "shapes")
        _check(win, truth, last, "shapes sub-range", first=5, count=40)
    got = _check(win, truth, 2, "shapes")
    assert got["count"][4] == NB and got["count"][1] == 1 and got["count"][0] == 1 and got["count"][7] == 0
    assert win.summaries(2).tobytes() == truth.one_oracle(2).tobytes()
    e.close()


# ---- 3. the open interval ----------------------------------------------------------------------------
def test_include_open(oracle, gpu_available):
    S = 70
    e = _engine(S, stage=0)  # every batch is binned at once: a pending segment
    win, truth = _window(e, 3), Truth(oracle, S)
    for i in range(2):
        s, v = _batch(30 + i, S, 4000, quiet=range(64, 70))  # (tile 2 never receives a sample: it stays clean)
        e.ingest(s, v)
        truth.interval(s, v)
        win.push()
    opened = oracle.OracleHistograms(S)
    more = []

    def add(seed, n, quiet=()):
        s, v = _batch(seed, S, n, quiet)
        e.ingest(s, v)
        assert opened.ingest(s, v) == 0
        more.append((s, v))

    add(40, 3000, quiet=range(32, 70))  # a segment ...
    e.snapshot(first=0, count=1, reset=False)  # ... folded into the state rows; tile 1 holds zero rows
    add(41, 2000, quiet=range(32, 70))  # a pending segment
    e.set_param(N.PARAM_STAGE_SAMPLES, 1 << 20)
    add(42, 1000, quiet=range(32, 70))  # samples in the staging ring
    extra = (opened.counts().astype(np.int64), opened.totals())
    for last in (2, 1):
        _check(win, truth, last, "open", include_open=True, extra=extra)
    _check(win, truth, 2, "open sub-range", first=5, count=40, include_open=True, extra=extra)
    assert win.summaries(2, include_open=True).tobytes() == truth.one_oracle(2, more).tobytes()
    # the open interval alone: a snapshot that resets nothing
    assert win.summaries(0, include_open=True).tobytes() == e.snapshot(reset=False).tobytes()
    assert win.summaries(0, include_open=True).tobytes() == opened.snapshot(reset=False).tobytes()
    # ... and it is still all there, byte for byte
    before = e.export_state()
    assert before[0].tobytes() == opened.counts().tobytes() and before[1].tobytes() == opened.totals().tobytes()
    _check(win, truth, 2, "open, folded", include_open=True, extra=extra)
    after = e.export_state()
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    _check(win, truth, 2, "closed intervals alone")  # (the slots never saw the open rows)
    e.close()


# ---- 4. range ----------------------------------------------------------------------------------------
def _one_hot_csr(S, cells):
    """CSR over S rows of {series: (bucket, count)}."""
    rows = np.zeros((S, NB), np.int64)
    for s, (b, c) in cells.items():
        rows[s, b] = c
    r, b = np.nonzero(rows)
    row_off = np.zeros(S + 1, np.uint64)
    row_off[1:] = np.cumsum(np.bincount(r, minlength=S))
    entries = np.zeros(r.size, N.BUCKET_ENTRY_DTYPE)
    entries["bucket"], entries["count"] = b, rows[r, b]
    return rows, row_off, entries


def test_range(oracle, gpu_available):
    S = 40
    e = _engine(S)
    win, truth = _window(e, 4), Truth(oracle, S)

    def push(cells, seed):
        rows, row_off, entries = _one_hot_csr(S, cells)
        totals = np.arange(S, dtype=np.int64) * seed
        e.import_sparse(row_off, entries, totals)
        s, v = _batch(seed, S, 500, quiet=cells.keys())
        e.ingest(s, v)
        ref = truth.interval(s, v)
        truth.rows[-1] = ref.counts().astype(np.int64) + rows
        truth.totals[-1] = ref.totals() + totals
        win.push()

    def refused(last, series):
        info = win.info()
        with pytest.raises(N.L5dhError) as ex:
            win.summaries(last)
        assert ex.value.code == ERANGE and f"series {series} " in str(ex.value), str(ex.value)
        assert win.info() == info
        _check(win, truth, 1, f"after the refusal of last={last}")

    push({7: (11, 2 ** 30 + 1), 3: (1797, 2 ** 30 + 1)}, 50)
    _check(win, truth, 1, "one large interval")
    push({7: (11, 2 ** 30 + 1), 3: (1797, 2 ** 30 + 1)}, 51)
    refused(2, 3)
    for k in range(3):  # 3 (2^31 - 1) passes 2^32: still found, never a small number
        push({9: (5, INT_MAX)}, 52 + k)
    refused(3, 9)
    refused(2, 9)
    e.close()


# ---- 5. forget ---------------------------------------------------------------------------------------
def test_forget(oracle, gpu_available):
    S = 70
    e = _engine(S)
    win, truth = _window(e, 3), Truth(oracle, S)
    mask = np.ones((3, S), bool)
    for i in range(3):
        s, v = _batch(60 + i, S, 3000)
        e.ingest(s, v)
        truth.interval(s, v)
        win.push()
        if i == 0:
            win.forget(2, 3)  # series 2..4 start after push 1
            mask[0, 2:5] = False
        if i == 1:
            win.forget(69)  # the last series after push 2
            mask[:2, 69] = False
    for last in (1, 2, 3):
        _check(win, truth, last, "forget", mask=mask)
    got = win.summaries(3)
    assert got["count"][69] == truth.rows[2][69].sum()
    assert got["count"][2] == (truth.rows[1][2] + truth.rows[2][2]).sum()
    e.close()


def test_release_then_register_starts_the_id_anew(oracle, gpu_available):
    from linkerd_amd.telemetry import StatEngine
    S = 40
    se = StatEngine(capacity=S)
    se.enable_window(3)
    ids = [se.register() for _ in range(10)]
    truth = Truth(oracle, S)
    mask = np.ones((2, S), bool)

    def interval(seed):
        s, v = _batch(seed, len(ids), 2000)
        for sid, val in zip(s.tolist(), v.tolist()):
            se.add(sid, val)
        truth.interval(s, v)
        return se.push_window()

    first = interval(70)
    assert first.tobytes() == oracle.summarize_counts(truth.rows[0].astype(np.int32), truth.totals[0]).tobytes()
    se.release(4)
    assert se.register() == 4
    mask[0, 4] = False
    interval(71)
    rows, tot, want = truth.window(2, mask=mask)
    got = se.window_summaries(2)
    assert got.tobytes() == want.tobytes()
    assert got["count"][4] == truth.rows[1][4].sum() and got["count"][3] == (truth.rows[0][3] + truth.rows[1][3]).sum()
    se.engine.close()


# ---- 6. grow -------------------------------------------------------------------------------------------
def test_grow_keeps_the_window(oracle, gpu_available):
    from linkerd_amd.telemetry import StatEngine
    S0, S1 = 40, 100
    se = StatEngine(capacity=S0)
    se.enable_window(3)
    for _ in range(S0):
        se.register()
    small, big = Truth(oracle, S0), Truth(oracle, S1)
    for i in range(2):
        s, v = _batch(80 + i, S0, 3000)
        se.engine.ingest(s, v)
        small.interval(s, v)
        big.interval(s, v)
        se.push_window()
    s, v = _batch(82, S0, 1000)  # the open interval moves too
    se.engine.ingest(s, v)
    before = [se.window_summaries(last) for last in (1, 2)]
    before_open = se.window_summaries(2, include_open=True)
    assert before[1].tobytes() == small.window(2)[2].tobytes()
    se.grow(S1)
    assert se.capacity == S1 and se.window.engine is se.engine and se.window.info()["filled"] == 2
    for last, b in zip((1, 2), before):
        got = se.window_summaries(last)
        assert got[:S0].tobytes() == b.tobytes()
        assert got[S0:].tobytes() == np.zeros(S1 - S0, N.SUMMARY_DTYPE).tobytes()
    assert se.window_summaries(2, include_open=True)[:S0].tobytes() == before_open.tobytes()
    s2, v2 = _batch(83, S1, 3000)
    se.engine.ingest(s2, v2)
    big.interval(np.concatenate([s, s2]), np.concatenate([v, v2]))
    se.push_window()
    for last in (1, 2, 3):
        assert se.window_summaries(last).tobytes() == big.window(last)[2].tobytes(), last
    se.engine.close()


# ---- 7. composition --------------------------------------------------------------------------------------
def test_top_of_device_resident_window_summaries(oracle, gpu_available):
    import torch
    S = 70
    e = _engine(S)
    win, truth = _window(e, 2), Truth(oracle, S)
    for i in range(2):
        s, v = _batch(90 + i, S, 2500, quiet=range(10, 20))
        e.ingest(s, v)
        truth.interval(s, v)
        win.push()
    dev = torch.zeros(S * 11, dtype=torch.int64, device="cuda:0")
    rows = torch.zeros((S, NB), dtype=torch.int32, device="cuda:0")
    win.summaries_into(2, dev, rows)
    w_rows, _, want = truth.window(2)
    assert dev.cpu().numpy().tobytes() == want.tobytes() and rows.cpu().numpy().tobytes() == w_rows.tobytes()
    ids, summ = e.top_summaries(dev, 7, by="p99")
    cand = [i for i in range(S) if want["count"][i] >= 1]
    order = sorted(cand, key=lambda i: (-int(want["p99"][i]), i))[:7]
    assert ids.tolist() == order and summ.tobytes() == want[order].tobytes()
    # the summed rows feed the dense queries unchanged
    q = e.quantiles_dense(rows, [0.5, 0.99])
    assert np.array_equal(q[:, 0], want["p50"]) and np.array_equal(q[:, 1], want["p99"])
    e.close()


# ---- 8. lifecycle ------------------------------------------------------------------------------------------
def test_lifecycle(oracle, gpu_available):
    S = 70
    e, twin = _engine(S), _engine(S)
    lib, ctx = e._lib, e._ctx
    # without a window
    assert lib.l5dh_window_push(ctx, S, None) == EINVAL
    assert lib.l5dh_window_query(ctx, 0, S, 0, 1, None, None, None) == EINVAL
    assert lib.l5dh_window_forget(ctx, 0, 1) == EINVAL and lib.l5dh_window_close(ctx) == EINVAL
    assert lib.l5dh_window_info(ctx, None, None, None, None, None) == EINVAL
    assert lib.l5dh_window_open(ctx, 0) == EINVAL and lib.l5dh_window_open(ctx, 65) == EINVAL
    win = _window(e, 2)
    with pytest.raises(N.L5dhError) as ex:
        _window(e, 2)
    assert ex.value.code == EEXIST
    assert lib.l5dh_window_push(ctx, S + 1, None) == EINVAL
    assert win.info()["filled"] == 0 and win.info()["pushes"] == 0 and win.info()["entries"] == 0
    sizes = []
    for i in range(3):
        s, v = _batch(100 + i, S, 1500)
        e.ingest(s, v)
        twin.ingest(s, v)
        sizes.append(twin.export_sparse_size())
        twin.snapshot(reset=True)
        win.push()
        info = win.info()
        assert info["slots"] == 2 and info["pushes"] == i + 1 and info["filled"] == min(i + 1, 2)
        assert info["entries"] == sum(sizes[-2:]) and info["bytes"] >= 8 * info["entries"] + 8 * S
    # a move needs a target without a window, on at least as many series
    small = _engine(S - 1)
    assert lib.l5dh_window_move(ctx, small._ctx) == EINVAL and lib.l5dh_window_move(ctx, ctx) == EINVAL
    assert lib.l5dh_window_move(twin._ctx, ctx) == EINVAL  # (nothing to move)
    small.close()
    win.close()
    assert lib.l5dh_window_query(ctx, 0, S, 1, 0, None, None, None) == EINVAL
    win = _window(e, 2)
    assert win.info() == dict(win.info(), filled=0, pushes=0, entries=0)
    assert lib.l5dh_window_query(ctx, 0, S, 1, 0, None, None, None) == EINVAL  # (starts empty)
    assert win.summaries(0, include_open=True).tobytes() == np.zeros(S, N.SUMMARY_DTYPE).tobytes()
    e.close()  # (frees the ring too)
    twin.close()


# ---- the tick ------------------------------------------------------------------------------------------------
def test_push_window_is_the_tick(oracle, gpu_available):
    """push_window beside snapshot_all_quantiles of a twin fed the same samples: the summaries,
    the lifetime `le` counters and the quantiles agree; the telemetry drivers on top of it."""
    from linkerd_amd.telemetry import MetricsTree, StatEngine, snapshot_histograms_window, window_stats
    S = 40
    se, twin = StatEngine(capacity=S), StatEngine(capacity=S)
    for x in (se, twin):
        x.enable_le([10, 100, 1000])
        x.enable_quantiles([0.25, 0.75])
    se.enable_window(2)
    tree = MetricsTree(se)
    stats = [tree.resolve(["rt", f"s{i}"]).mk_stat() for i in range(5)]
    assert [m.series_id for m in stats] == list(range(5))
    truth = Truth(oracle, S)
    for i in range(2):
        s, v = _batch(110 + i, 5, 1500)
        for sid, val in zip(s.tolist(), v.tolist()):
            stats[sid].add(val)
            twin.add(sid, val)
        truth.interval(s, v)
        if i == 0:
            got = se.push_window()
        else:
            assert snapshot_histograms_window(tree, se) == 5
            got = None
        want = twin.snapshot_all_quantiles()
        if got is not None:
            assert got.tobytes() == want.tobytes()
        assert se.le_buckets.tobytes() == twin.le_buckets.tobytes() and se.le_sums.tobytes() == twin.le_sums.tobytes()
        assert se.quantile_values.tobytes() == twin.quantile_values.tobytes()
    from linkerd_amd.telemetry import HistogramSummary
    assert stats[3].snapshotted_summary == HistogramSummary.from_record(want[3])
    both = truth.window(2)[2]
    ws = window_stats(tree, se, 2)
    assert set(ws) == set(stats) and all(ws[m] == HistogramSummary.from_record(both[m.series_id]) for m in stats)
    assert window_stats(tree, se, 1)[stats[0]] == HistogramSummary.from_record(want[0])
    se.engine.close()
    twin.engine.close()
