"""GPU state import and sparse export (l5dh_import_state, l5dh_import_sparse,
l5dh_export_sparse) and what StatEngine builds on them (grow, checkpoint / restore).

The truth everywhere: the numpy integer sum of bucket rows and totals (rows from the CPU
oracle or from the crafted rows of tests/summary_rows.py), and oracle.summarize_counts of
those sums.  Rows, totals and summaries are compared as bytes.
"""
import numpy as np
import pytest

from linkerd_amd import _native as N

from tests import summary_rows as SR

pytestmark = pytest.mark.gpu

NB = N.NBUCKETS
INT_MAX = SR.INT_MAX
S, QUIET = 257, range(96, 128)  # 9 tiles, the last of one series; tile 3 receives no sample
FIRST, COUNT = 5, 200  # starts and ends inside a tile
SL = slice(FIRST, FIRST + COUNT)
ERANGE, EINVAL = -34, -22


def _engine(n, stage=None):
    from linkerd_amd.engine import HistogramEngine
    e = HistogramEngine(n)
    if stage is not None:
        e.set_param(N.PARAM_STAGE_SAMPLES, stage)
    return e


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _raw(x):
    return (x if isinstance(x, np.ndarray) else x.cpu().numpy()).tobytes()


def _batch(seed, n):
    rng = np.random.default_rng(seed)
    live = np.array([s for s in range(S) if s not in QUIET], np.uint32)
    series = live[rng.integers(0, live.size, size=n)]
    vals = np.exp(3.0 + 1.5 * rng.standard_normal(n)).astype(np.float32)
    vals[:8] = np.array([0, 1, 2, 113, 3030, 1e9, 3e9, -5], dtype=np.float32)  # smoke()'s edge values
    series[:8] = [256, 6, 31, 32, 204, 150, 200, 33]
    return series, vals


def _crafted_rows():
    """37 rows: 29 staircases over the lane and group edges (the last with all 1798 buckets
    non-zero), every bucket at 2^31 - 1, one-hot rows at the first / last bins of lanes 0, 1
    and 63 and of lane 63's extra groups, and the empty row."""
    stairs = SR.staircase_rows()[np.array(SR.FOLD_ROWS[:28] + (1798,)) - 1]
    hot = np.zeros((6, NB), np.int32)
    hot[np.arange(6), [0, 27, 28, 1791, 1792, 1797]] = [1, 2, 3, 4, INT_MAX, 6]
    rows = np.ascontiguousarray(np.concatenate([stairs, np.full((1, NB), INT_MAX, np.int32), hot,
                                                np.zeros((1, NB), np.int32)]))
    assert rows.shape == (37, NB)
    return rows, np.resize(np.array(SR.SPECIAL_TOTALS, np.int64), 37)


@pytest.fixture(scope="module")
def case(oracle, gpu_available):
    """Two batches (50 k samples), the oracle's rows of each and of both."""
    batches = [_batch(1, 30_000), _batch(2, 20_000)]
    each = []
    for s, v in batches:
        ref = oracle.OracleHistograms(S)
        assert ref.ingest(s, v) == 0
        each.append((ref.counts().copy(), ref.totals().copy()))
    counts, totals = each[0][0] + each[1][0], each[0][1] + each[1][1]
    assert not counts[list(QUIET)].any() and counts[:, 0].any() and counts[:, 1797].any()
    rows, rtot = _crafted_rows()
    return dict(batches=batches, each=each, counts=counts, totals=totals, rows=rows, rtot=rtot)


def _padded(rows, totals, first, n=S):
    c, t = np.zeros((n, NB), np.int32), np.zeros(n, np.int64)
    c[first:first + len(rows)], t[first:first + len(rows)] = rows, totals
    return c, t


def _csr(rows, totals=None):
    """(row_off, entries, totals) of dense rows: np.nonzero, row by row."""
    r, b = np.nonzero(rows)
    row_off = np.zeros(len(rows) + 1, np.uint64)
    row_off[1:] = np.cumsum(np.bincount(r, minlength=len(rows)))
    entries = np.zeros(r.size, N.BUCKET_ENTRY_DTYPE)
    entries["bucket"], entries["count"] = b, np.asarray(rows)[r, b]
    return row_off, entries, totals


def _state(e):
    counts, totals = e.export_state()
    return counts.tobytes() + totals.tobytes()


def _expect(e, oracle, counts, totals, what=""):
    """The whole engine reads as (counts, totals): rows, totals and summaries, as bytes."""
    got_c, got_t = e.export_state()
    if got_c.tobytes() != counts.tobytes():
        s, b = np.argwhere(got_c != counts)[0]
        raise AssertionError(f"{what}: series {s} bucket {b}: got {got_c[s, b]} want {counts[s, b]}")
    assert got_t.tobytes() == np.asarray(totals, np.int64).tobytes(), what
    assert e.snapshot(reset=False).tobytes() == oracle.summarize_counts(counts, totals).tobytes(), what


# ---- 1. round trip, dense --------------------------------------------------------------
@pytest.mark.parametrize("kind", ["host", "device"])
def test_dense_round_trip(oracle, case, kind):
    put = (lambda a: a) if kind == "host" else _dev
    with _engine(S) as a, _engine(S) as b:
        for s, v in case["batches"]:
            a.ingest(s, v)
        counts, totals = a.export_state()
        assert counts.tobytes() == case["counts"].tobytes() and totals.tobytes() == case["totals"].tobytes()
        b.import_state(put(counts), put(totals))
        _expect(b, oracle, case["counts"], case["totals"], kind)
        assert a.snapshot(reset=False).tobytes() == b.snapshot(reset=False).tobytes()
    # the crafted rows into a range inside a clean engine (no totals: zeros), then once more with totals
    with _engine(S) as b:
        small = case["rows"].copy()
        small[29] = INT_MAX // 2  # (imported twice below)
        small[34, 1792] = 5
        b.import_state(put(small), first=FIRST)
        _expect(b, oracle, *_padded(small, 0, FIRST), kind)
        b.import_state(put(small), put(case["rtot"]), first=FIRST)
        _expect(b, oracle, *_padded(2 * small, case["rtot"], FIRST), kind)


# ---- 2. stale clean tiles --------------------------------------------------------------
def _stale(case):
    e = _engine(S)
    for s, v in case["batches"]:
        e.ingest(s, v)
    assert e.snapshot(reset=True)["count"].sum() == 50_000  # every tile clean, its rows stale
    return e


def test_stale_clean_tiles_dense(oracle, case):
    c1, t1 = case["each"][1]
    with _stale(case) as e:
        e.import_state(c1[SL], t1[SL], first=FIRST)
        _expect(e, oracle, *_padded(c1[SL], t1[SL], FIRST), "dense range over stale tiles")


def test_stale_clean_tiles_sparse(oracle, case):
    c1, t1 = case["each"][1]
    series = np.array([3, 40, 95, 130, 159, 160, 200, 255, 256], np.uint32)  # one series of 8 tiles (not tile 3)
    assert len(set((series >> 5).tolist())) == 8
    want_c, want_t = np.zeros((S, NB), np.int32), np.zeros(S, np.int64)
    want_c[series], want_t[series] = c1[series], t1[series]
    with _stale(case) as e:
        e.import_sparse(*_csr(c1[series], t1[series]), series=series)
        _expect(e, oracle, want_c, want_t, "sparse rows over stale tiles")


# ---- 3. union with live samples ----------------------------------------------------------
@pytest.mark.parametrize("stage", [None, 0])  # the samples still staged / a binned, unfolded batch
def test_union_with_live_samples(oracle, case, stage):
    (c0, t0), (c1, t1) = case["each"]
    rows, rtot = c1[SL], t1[SL]
    with _engine(S, stage) as e:
        e.ingest(*case["batches"][0])
        e.import_state(rows, rtot, first=FIRST)
        add_c, add_t = _padded(rows, rtot, FIRST)
        want_c, want_t = c0 + add_c, t0 + add_t
        _expect(e, oracle, want_c, want_t, "import beside staged / pending samples")
        # the tiles are dirty now: read-add-write, dense and sparse
        e.import_state(rows, rtot, first=FIRST)
        e.import_sparse(*_csr(rows, rtot), first=FIRST)
        want_c, want_t = want_c + 2 * add_c, want_t + 2 * add_t
        _expect(e, oracle, want_c, want_t, "import into dirty tiles")
        # samples after the import, and an import beside them
        e.ingest(*case["batches"][1])
        e.import_sparse(*_csr(rows, rtot), first=FIRST)
        want_c, want_t = want_c + c1 + add_c, want_t + t1 + add_t
        summ, counts = e.snapshot(reset=True, with_counts=True)
        assert counts.tobytes() == want_c.tobytes()
        assert summ.tobytes() == oracle.summarize_counts(want_c, want_t).tobytes()
        # the next interval is empty
        _expect(e, oracle, np.zeros((S, NB), np.int32), np.zeros(S, np.int64), "after the reset")


def test_union_one_tile_space_with_sumfix(oracle, gpu_available):
    S1 = 20  # one tile: every batch is folded at ingest, escaped samples' sums stay in sumfix
    rng = np.random.default_rng(5)
    series = rng.integers(0, S1, size=4000, dtype=np.uint32)
    vals = np.exp(3.0 + 2.0 * rng.standard_normal(4000)).astype(np.float32)
    vals[:40] = np.resize(np.array([1e9, 3e9, -5, 2.5e6, 2 ** 21, 2 ** 21 - 2048, 4e6, 1e7], np.float32), 40)
    ref = oracle.OracleHistograms(S1)
    assert ref.ingest(series, vals) == 0
    c, t = ref.counts().copy(), ref.totals().copy()
    rows, rtot = c[3:17], t[3:17]
    with _engine(S1) as e:
        e.import_state(rows, rtot, first=3)  # into the clean tile
        _expect(e, oracle, *_padded(rows, rtot, 3, S1), "clean one-tile space")
        e.ingest(series, vals)
        e.import_sparse(*_csr(rows, rtot), first=3)  # beside a non-zero sumfix
        add_c, add_t = _padded(rows, rtot, 3, S1)
        _expect(e, oracle, c + 2 * add_c, t + 2 * add_t, "one-tile union")
        e.ingest(series, vals)
        summ = e.snapshot(reset=True)
        assert summ.tobytes() == oracle.summarize_counts(2 * c + 2 * add_c, 2 * t + 2 * add_t).tobytes()
        assert not e.snapshot(reset=False)["count"].any()


# ---- 4. range ------------------------------------------------------------------------------
def test_range_int_max_accepted_one_more_rejected(oracle, case):
    c1, t1 = case["each"][1]
    one = np.zeros((1, NB), np.int32)
    with _engine(S) as e:
        one[0, 7] = INT_MAX - 5
        e.import_state(one, np.array([2 ** 63 - 1], np.int64), first=40)
        one[0, 7] = 5
        e.import_state(one, np.array([2], np.int64), first=40)  # exactly INT_MAX; the total wraps
        want_c, want_t = np.zeros((S, NB), np.int32), np.zeros(S, np.int64)
        want_c[40, 7], want_t[40] = INT_MAX, -(2 ** 63) + 1
        _expect(e, oracle, want_c, want_t, "a bucket at INT_MAX, a wrapped total")
        before = _state(e)
        # valid rows, rows of clean tiles (all but tile 1) and the one bucket too many
        rows, rtot = c1[SL].copy(), t1[SL].copy()
        rows[40 - FIRST, 7] = 1
        rows[41 - FIRST, 9] = 3
        with pytest.raises(N.L5dhError) as ei:
            e.import_state(rows, rtot, first=FIRST)
        assert ei.value.code == ERANGE and "series 40 " in str(ei.value)
        assert _state(e) == before
        # the same through sparse rows (host and device), an empty row among them
        series = np.array([3, 40, 100, 200, 256], np.uint32)
        srows = c1[series].copy()
        srows[1, 7] = 1
        srows[3, :] = 0
        for put in (lambda a: a, _dev):
            ro, en, _ = _csr(srows)
            with pytest.raises(N.L5dhError) as ei:
                e.import_sparse(put(ro.view(np.int64)), put(en.view(np.uint32)), put(t1[series]), series=put(series))
            assert ei.value.code == ERANGE and "series 40 " in str(ei.value)
            assert _state(e) == before
        # without the offending bucket the same calls go through
        rows[40 - FIRST, 7] = 0
        e.import_state(rows, rtot, first=FIRST)
        add_c, add_t = _padded(rows, rtot, FIRST)
        _expect(e, oracle, want_c + add_c, (want_t + add_t), "after the accepted import")


# ---- 5. invalid input writes nothing -----------------------------------------------------
def test_invalid_input_writes_nothing(case):
    c1, t1 = case["each"][1]
    lib = N.load()
    with _engine(S, 0) as e:
        e.ingest(*case["batches"][0])
        before = _state(e)
        rows = c1[SL].copy()
        rows[77 - FIRST, 1797] = -1
        rows[150 - FIRST, 0] = -(2 ** 31)
        for put in (lambda a: a, _dev):
            with pytest.raises(N.L5dhError) as ei:
                e.import_state(put(rows), put(t1[SL]), first=FIRST)
            assert ei.value.code == EINVAL and "series 77" in str(ei.value)
            assert _state(e) == before
        # ranges out of bounds: found on the host
        assert lib.l5dh_import_state(e._ctx, S - 1, 2, c1.ctypes.data, None) == EINVAL
        assert lib.l5dh_import_state(e._ctx, 2 ** 32 - 1, 2, c1.ctypes.data, None) == EINVAL
        ro, en, tt = _csr(c1[:4], t1[:4])
        assert lib.l5dh_import_sparse(e._ctx, None, S - 3, 4, ro.ctypes.data, en.ctypes.data, tt.ctypes.data) == EINVAL
        assert lib.l5dh_export_sparse(e._ctx, S - 1, 2, None, None, 0, None, None, 1) == EINVAL
        assert _state(e) == before
        # sparse defects, one at a time: (name, the least offending row, the edit)
        series = np.array([3, 40, 100, 250], np.uint32)
        good = c1[series].copy()
        good[:, 10:14] = [[1, 2, 3, 4]] * 4  # every row holds >= 4 entries
        ro0, en0, tt0 = _csr(good, t1[series])

        def edit(**kw):
            ro, en, se = ro0.copy(), en0.copy(), series.copy()
            for k, (i, v) in kw.items():
                {"ro": ro, "bucket": en["bucket"], "count": en["count"], "se": se}[k][i] = v
            return ro, en, se

        r1, r2, r3 = int(ro0[1]), int(ro0[2]), int(ro0[3])
        defects = [
            ("row_off[0] != 0", 0, edit(ro=(0, 1))),
            ("row_off descends", 1, edit(ro=(2, r1 - 1))),
            ("row_off past the entries", 2, edit(ro=(3, int(ro0[4]) + 1))),
            ("bucket >= 1798", 2, edit(bucket=(r3 - 1, 1798))),
            ("buckets equal", 1, edit(bucket=(r1 + 1, int(en0["bucket"][r1])))),
            ("buckets descend", 3, edit(bucket=(r3, int(en0["bucket"][r3 + 1]) + 1))),
            ("count above INT_MAX", 3, edit(count=(r3 + 2, 2 ** 31))),
            ("series not ascending", 2, edit(se=(1, 100))),
            ("series descends", 1, edit(se=(0, 41))),
            ("series >= max_series", 3, edit(se=(3, S))),
        ]
        for name, row, (ro, en, se) in defects:
            for put in (lambda a: a, _dev):
                with pytest.raises(N.L5dhError) as ei:
                    e.import_sparse(put(ro.view(np.int64)), put(en.view(np.uint32)), put(tt0), series=put(se))
                assert ei.value.code == EINVAL and f"row {row} " in str(ei.value), (name, str(ei.value))
                assert _state(e) == before, name
        # two defects: the least row is named
        ro, en, se = edit(count=(r3 + 2, 2 ** 31), bucket=(r2, 4000))
        with pytest.raises(N.L5dhError) as ei:
            e.import_sparse(ro, en, tt0, series=se)
        assert "row 2 " in str(ei.value) and _state(e) == before
        # and the rows as they were are accepted
        e.import_sparse(ro0, en0, tt0, series=series)
        assert _state(e) != before


# ---- 6. sparse export ----------------------------------------------------------------------
def test_sparse_export(case):
    lib = N.load()
    rows, rtot = case["rows"], case["rtot"]
    with _engine(S) as e:
        e.import_state(rows, rtot, first=FIRST)  # tiles 0 and 1; the others stay clean
        e.ingest(np.array([250, 250, 256], np.uint32), np.array([7.0, 7.0, 3e9], np.float32))  # staged samples
        dense_c, dense_t = e.export_state()
        assert (dense_c[FIRST + 28] != 0).all() and not dense_c[FIRST + 36].any()  # all 1798 buckets / the empty row
        want_ro, want_en, _ = _csr(dense_c)
        n = e.export_sparse_size()
        assert n == want_en.size == int(want_ro[-1])
        row_off, entries, totals = e.export_sparse()
        assert entries.dtype == N.BUCKET_ENTRY_DTYPE and row_off.dtype == np.uint64
        assert row_off.tobytes() == want_ro.tobytes() and entries.tobytes() == want_en.tobytes()
        assert totals.tobytes() == dense_t.tobytes()
        # a range, and device buffers
        sub = e.export_sparse(first=FIRST, count=COUNT)
        w = _csr(dense_c[SL])
        assert sub[0].tobytes() == w[0].tobytes() and sub[1].tobytes() == w[1].tobytes()
        assert sub[2].tobytes() == dense_t[SL].tobytes()
        d_ro, d_en, d_t = _dev(np.zeros(S + 1, np.int64)), _dev(np.zeros((n + 3, 2), np.uint32)), _dev(np.zeros(S, np.int64))
        assert e.export_sparse_into(d_ro, d_en, d_t) == n
        assert _raw(d_ro) == want_ro.tobytes() and _raw(d_en)[:8 * n] == want_en.tobytes() and _raw(d_t) == dense_t.tobytes()
        # one entry short: -ERANGE, the count reported, nothing written, nothing reset
        before = _state(e)
        for put in (lambda a: a, _dev):
            ro = put(np.full(S + 1, 0x5A5A5A5A5A5A5A5A, np.int64))
            en = put(np.full((n - 1, 2), 0xABABABAB, np.uint32))
            tt = put(np.full(S, -77, np.int64))
            with pytest.raises(N.L5dhError) as ei:
                e.export_sparse_into(ro, en, tt, reset=True)
            assert ei.value.code == ERANGE
            assert (np.frombuffer(_raw(ro), np.int64) == 0x5A5A5A5A5A5A5A5A).all()
            assert (np.frombuffer(_raw(en), np.uint32) == 0xABABABAB).all()
            assert (np.frombuffer(_raw(tt), np.int64) == -77).all()
        got = N.ctypes.c_size_t(0)
        ro = np.zeros(S + 1, np.uint64)
        assert lib.l5dh_export_sparse(e._ctx, 0, S, ro.ctypes.data, want_en.ctypes.data, n - 1, N.ctypes.byref(got),
                                      None, 1) == ERANGE and got.value == n
        # the size query with reset = 1 resets nothing either
        assert lib.l5dh_export_sparse(e._ctx, 0, S, None, None, 0, N.ctypes.byref(got), None, 1) == 0 and got.value == n
        assert _state(e) == before
        # reset=True clears exactly the range
        cut = slice(FIRST + 3, FIRST + 33)
        part = e.export_sparse(first=cut.start, count=30, reset=True)
        w = _csr(dense_c[cut])
        assert part[0].tobytes() == w[0].tobytes() and part[1].tobytes() == w[1].tobytes()
        assert part[2].tobytes() == dense_t[cut].tobytes()
        left_c, left_t = dense_c.copy(), dense_t.copy()
        left_c[cut], left_t[cut] = 0, 0
        got_c, got_t = e.export_state()
        assert got_c.tobytes() == left_c.tobytes() and got_t.tobytes() == left_t.tobytes()
        # an empty range
        ro, en, tt = e.export_sparse(first=7, count=0)
        assert ro.tolist() == [0] and en.size == 0 and tt.size == 0


# ---- 7. round trip, sparse -------------------------------------------------------------------
def test_sparse_round_trip_into_another_size(oracle, case):
    S2 = 600
    target = (2 * np.arange(S) + 1).astype(np.uint32)
    with _engine(S) as a, _engine(S2) as b:
        for s, v in case["batches"]:
            a.ingest(s, v)
        row_off, entries, totals = a.export_sparse()
        b.import_sparse(row_off, entries, totals, series=target)
        want_c, want_t = np.zeros((S2, NB), np.int32), np.zeros(S2, np.int64)
        want_c[target], want_t[target] = case["counts"], case["totals"]
        _expect(b, oracle, want_c, want_t, "series map into a larger engine")
        # only the non-empty rows, as an aggregator would receive them
        keep = np.flatnonzero(np.diff(row_off.astype(np.int64)) > 0)
        assert 0 < keep.size < S
        b.import_sparse(*_csr(case["counts"][keep], totals[keep]), series=_dev(target[keep]))
        _expect(b, oracle, 2 * want_c, 2 * want_t, "the non-empty rows once more")


def test_two_sources_equal_their_union(oracle, case):
    exports = []
    for s, v in case["batches"]:
        with _engine(S, 0) as src:
            src.ingest(s, v)
            exports.append(src.export_sparse(reset=True))
            assert src.export_sparse_size() == 0
    with _engine(S) as agg:
        for row_off, entries, totals in exports:
            agg.import_sparse(row_off, entries, totals)
        _expect(agg, oracle, case["counts"], case["totals"], "two sources")


# ---- 8. StatEngine.grow, checkpoint / restore --------------------------------------------------
def test_stat_engine_grow_checkpoint_restore(oracle, gpu_available):
    from linkerd_amd.telemetry import Metric, StatEngine
    eng = StatEngine(capacity=64, device=0, batch=128)
    eng.enable_le([1, 250, 500, float("inf")])
    stats = [Metric.Stat(eng) for _ in range(64)]
    with pytest.raises(RuntimeError, match="histogram engine full"):
        eng.register()
    rng = np.random.default_rng(8)

    def interval(n_stats, per):
        """`per` samples to each of the first n_stats Stats; returns (ids, values)."""
        ids = np.repeat(np.arange(n_stats, dtype=np.uint32), per)
        vals = np.exp(3.0 + 2.0 * rng.standard_normal(ids.size)).astype(np.float32)
        vals[:4] = [0.5, 250.0, 3e9, 2.5e6]
        for i, v in zip(ids, vals):
            stats[i].add(float(v))
        return ids, vals

    def rows_of(n, *ivs):
        ref = oracle.OracleHistograms(n)
        for ids, vals in ivs:
            assert ref.ingest(ids, vals) == 0
        return ref.counts().copy(), ref.totals().copy()

    def le_truth(counts):
        cum = np.cumsum(counts.astype(np.uint64), axis=1)
        return np.concatenate([cum[:, eng.le_cuts.astype(np.int64) - 1], cum[:, -1:]], axis=1)

    iv1 = interval(64, 3)
    eng.snapshot_all_le()  # interval 1 ends: it lives on in the lifetime counters only
    iv2 = interval(64, 3)  # 192 adds: 128 went to the device (its staging ring), 64 wait on the host
    ids_before = [s.series_id for s in stats]
    eng.grow(256)
    assert eng.capacity == 256 and eng.engine.max_series == 256
    assert [s.series_id for s in stats] == ids_before
    stats += [Metric.Stat(eng) for _ in range(100)]
    assert [s.series_id for s in stats[64:]] == list(range(64, 164))
    assert eng.le_buckets.shape == (256, len(eng.le_cuts) + 1) and eng.le_sums.shape == (256,)
    iv3 = interval(164, 1)
    c_open, t_open = rows_of(256, iv2, iv3)
    assert eng.snapshot_all(reset=False).tobytes() == oracle.summarize_counts(c_open, t_open).tobytes()
    # checkpoint the open interval, restore it into a fresh engine
    ckpt = eng.checkpoint()
    assert all(isinstance(v, np.ndarray) for v in ckpt.values())
    eng2 = StatEngine(capacity=256, device=0, batch=128)
    eng2.restore(ckpt)
    assert eng2.register() == 164 and eng2.registered == 165
    with pytest.raises(RuntimeError):
        eng2.restore(ckpt)
    c_all, t_all = rows_of(256, iv1, iv2, iv3)
    for e in (eng, eng2):
        assert e.snapshot_all(reset=False).tobytes() == oracle.summarize_counts(c_open, t_open).tobytes()
        summ = e.snapshot_all_le()  # the open interval joins the lifetime counters
        assert summ.tobytes() == oracle.summarize_counts(c_open, t_open).tobytes()
        assert e.le_buckets.tobytes() == le_truth(c_all).tobytes() and e.le_sums.tobytes() == t_all.tobytes()
        assert not e.snapshot_all(reset=False)["count"].any()
        e.engine.close()
