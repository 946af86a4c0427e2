"""The fleet merge's sparse encoding pinned with the crafted rows of tests/merge_rows.py,
through loopback groups on one device: the export's encoders (row_encode / row_words
over dirty rows, the record paths of test (e)), k_mpack, and k_mdecode.

Rows enter each engine with import_state, which leaves the tiles dirty, so the export
takes the whole-row encode path; test (e) enters them by ingest.  Every rank's slice is
compared with the int64 sum of the ranks' rows: (first, count), the counts, the totals
and the summaries bytewise against oracle.summarize_counts.  In reduce-scatter mode the
encoded and sent bytes of merge_bytes() are compared with the word counts of the format
(fleet.sparse_encode), which pins the encoders' word counts exactly.
tests/test_merge_rows_host.py shows on the CPU what the rows expose.
"""
import numpy as np
import pytest

from linkerd_amd import _native as N
from tests import merge_rows as M
from tests import summary_rows as SR

pytestmark = pytest.mark.gpu

NB, CMAX, INT_MAX = M.NB, M.CMAX, M.INT_MAX
RS, AR = N.MERGE_REDUCE_SCATTER, N.MERGE_ALL_REDUCE
MODES = pytest.mark.parametrize("mode", [RS, AR], ids=["reduce_scatter", "all_reduce"])


@pytest.fixture(scope="module")
def cat():
    rows = M.catalogue()
    rows.setflags(write=False)
    return rows


class _Group:
    """W engines of S series as one loopback group; closed on exit."""

    def __init__(self, S, W):
        from linkerd_amd.engine import HistogramEngine
        self.cls, self.S, self.W, self.engines = HistogramEngine, S, W, []
        try:
            for _ in range(W):
                self.engines.append(HistogramEngine(S))
            HistogramEngine.comm_init_loopback(self.engines)
        except BaseException:
            self.close()
            raise

    def close(self):
        for e in self.engines:
            e.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def merge(self, mode, want_c, want_t, want_s, rank_rows=None, label=""):
        """One merge, every rank's outputs compared; rank_rows (the dense rows each rank
        holds) also pins merge_bytes in reduce-scatter mode.  Returns the results."""
        S, W = self.S, self.W
        per = -(-S // W)
        res = self.cls.merge_all(self.engines, mode, with_counts=True)
        for r, (first, count, summ, cnt, tot) in enumerate(res):
            what = f"{label} W={W} rank {r}"
            if mode == RS:
                assert (first, count) == (min(r * per, S), max(0, min(per, S - r * per))), what
            else:
                assert (first, count) == (0, S), what
            sl = slice(first, first + count)
            if want_c is not None:
                bad = np.argwhere(cnt != want_c[sl])
                if bad.size:
                    i, b = bad[0]
                    raise AssertionError(f"{what}: {len(bad)} buckets differ; first series {first + i} bucket {b}: "
                                         f"got {cnt[i, b]} want {want_c[sl][i, b]}")
                np.testing.assert_array_equal(cnt, want_c[sl], err_msg=what)
            np.testing.assert_array_equal(tot, want_t[sl], err_msg=what)
            if want_s is not None:
                bad = np.flatnonzero((summ.view(np.uint8).reshape(-1, 88) !=
                                      want_s[sl].view(np.uint8).reshape(-1, 88)).any(axis=1))
                assert bad.size == 0, f"{what}: {bad.size} summaries differ; first series {first + bad[0]}: " \
                                      f"got {summ[bad[0]]} want {want_s[sl][bad[0]]}"
                assert summ.tobytes() == want_s[sl].tobytes(), what
        if mode == RS and rank_rows is not None:
            for r, e in enumerate(self.engines):
                total, to = M.slice_words(rank_rows[r], W)
                mb = e.merge_bytes()
                assert mb["dense"] == per * W * (NB * 4 + 8), label
                assert mb["encoded"] == 4 * total + 12 * per * W, f"{label} W={W} rank {r}: encoded bytes"
                assert mb["sent"] == sum(4 * int(to[q]) + 12 * per for q in range(W) if q != r), \
                    f"{label} W={W} rank {r}: sent bytes"
        return res

    def import_all(self, rank_rows, rank_totals):
        for e, rr, tt in zip(self.engines, rank_rows, rank_totals):
            e.import_state(np.ascontiguousarray(rr, np.int32), np.ascontiguousarray(tt, np.int64))


def _summ(oracle, want_c, want_t):
    assert want_c.min() >= 0 and want_c.max() <= INT_MAX
    return oracle.summarize_counts(want_c.astype(np.int32), want_t, threads=8)


# ---- (a) the position and run catalogue ----------------------------------------------------
@MODES
@pytest.mark.parametrize("W", [2, 3])
def test_catalogue_merges_exactly(oracle, cat, W, mode):
    """S = the catalogue (261 rows: odd, so W = 2 has a short last slice); two merges
    through the same engines and buffers, the second with the rows dealt one rank on, so
    stale received encodings or word counts would show."""
    S = cat.shape[0]
    assert S % 2 == 1
    with _Group(S, W) as g:
        for rot in (0, 1):
            ranks, totals, want, want_t = M.split(cat, W, rot)
            g.import_all(ranks, totals)
            g.merge(mode, want, want_t, _summ(oracle, want, want_t), ranks, f"catalogue rot={rot}")


# ---- (b) every source escaped in one bucket ------------------------------------------------
def _shares(total, W, shift):
    q, r = divmod(total, W)
    a = np.full(W, q, np.int64)
    a[(np.arange(r) + shift) % W] += 1
    assert a.sum() == total
    return a


@MODES
@pytest.mark.parametrize("W", [2, 8])
def test_every_source_escaped_in_one_bucket(oracle, W, mode):
    """Buckets 0, 899 and 1797 sum to exactly 2^31 - 1 from W escaped counts; bucket 900
    reaches the escape (MERGE_CMAX) only across ranks, every source's count plain."""
    S = 2 * W + 1
    ranks = [np.zeros((S, NB), np.int32) for _ in range(W)]
    for i in range(S):
        big, plain = _shares(INT_MAX, W, i), _shares(CMAX, W, i + 1)
        assert big.min() >= CMAX and plain.max() < CMAX
        for q in range(W):
            ranks[q][i, [0, 899, NB - 1]] = big[q]
            ranks[q][i, 900] = plain[q]
            ranks[q][i, 898] = 1 + q
    totals = [M.totals_of(q, S) for q in range(W)]
    want = sum(r.astype(np.int64) for r in ranks)
    assert (want[:, [0, 899, NB - 1]] == INT_MAX).all() and (want[:, 900] == CMAX).all()
    want_t = M.wrap_sum(totals)
    with _Group(S, W) as g:
        g.import_all(ranks, totals)
        g.merge(mode, want, want_t, _summ(oracle, want, want_t), ranks, "all escaped")


# ---- (c) more than eight sources ---------------------------------------------------------------
SPECIAL_SOURCES = (7, 8, 15, 16, 63)
# (five of them may meet in one bucket: 5 * 2^28 stays below 2^31)
MANY_CYCLE = (2 ** 21 - 1, 2 ** 21, 2 ** 22 - 1, (5 << 21) | CMAX, 2 ** 28 - 1, 2 ** 28)


def _many_source_rows(W, S):
    ranks = []
    for q in range(W):
        rr = np.zeros((S, NB), np.int32)
        for i in range(S):
            if q in SPECIAL_SOURCES:  # 63 single samples, the first header on word 63, a run of escapes
                n = 1 + (5 * i + q) % 70
                rr[i, :63] = 1
                rr[i, 63:63 + n] = np.array(MANY_CYCLE, np.int64)[(np.arange(n) + q + i) % len(MANY_CYCLE)]
            else:  # a few single samples in buckets of its own
                rr[i, 28 * q + i % 27] = 1
                rr[i, 28 * q + 27] = 2
        ranks.append(rr)
    return ranks


@pytest.mark.parametrize("W", [9, 16, 64])
def test_more_than_eight_sources(oracle, W):
    """The second and later turns of k_mdecode's source batches (MDEC_BATCH = 8), up to
    MERGE_MAX_RANKS = 64 sources: every source holds words for every row, sources 7, 8,
    15, 16 and 63 a header on word 63 and a run of escapes.  S = 4 W + 3 (W = 64: the last
    ranks' slices are empty)."""
    S = 4 * W + 3
    ranks = _many_source_rows(W, S)
    assert all(r.any(axis=1).all() for r in ranks)
    assert any(q < W for q in SPECIAL_SOURCES)
    totals = [M.totals_of(q, S) for q in range(W)]
    want = sum(r.astype(np.int64) for r in ranks)
    assert want.max() <= INT_MAX
    want_t = M.wrap_sum(totals)
    with _Group(S, W) as g:
        g.import_all(ranks, totals)
        g.merge(RS, want, want_t, _summ(oracle, want, want_t), ranks, "many sources")


# ---- (d) a wave's second row ------------------------------------------------------------------------
def test_second_row_of_a_wave_starts_from_a_clean_lds_row(oracle, cat):
    """k_mdecode runs at most MDEC_GRID x MDEC_WAVES = 1280 x 4 = 5120 waves; with 6000
    rows per slice the wave that decoded row r < 880 decodes row r + 5120 into the LDS row
    it has just cleared, from word counts and offsets it loaded ahead.  Rows r < 880 of each
    slice are the catalogue's longest rows (the whole-row runs first), rows r + 5120
    alternate between the empty row and a single bucket (held by one rank, nothing on the
    other), the rows between are the catalogue cycled: a leaked LDS word or a wrong
    prefetch lands in a row that should be empty."""
    W, per = 2, 6000
    S = W * per
    assert per - 5120 == 880
    longest = cat[np.argsort(-M.row_words(cat), kind="stable")[:40]]
    assert (longest[0] >= CMAX).all() and M.row_words(longest).min() > 300
    r = np.arange(S) % per
    own = cat[r % cat.shape[0]].copy()
    own[r < 880] = longest[r[r < 880] % 40]
    tail = r >= 5120
    own[tail] = 0
    single = np.flatnonzero(tail & (r % 2 == 1))
    own[single, (7 * r[single]) % NB] = 1 + r[single] % 3
    owner = (np.arange(S) // 3) % W
    bg = M.background(own, W)
    bg[tail] = 0
    ranks = [np.where((owner == q)[:, None], own, bg).astype(np.int32) for q in range(W)]
    totals = [M.totals_of(q, S) for q in range(W)]
    want = own.astype(np.int64) + bg
    want_t = M.wrap_sum(totals)
    assert not want[tail & (r % 2 == 0)].any() and (want[single].sum(axis=1) <= 3).all()
    with _Group(S, W) as g:
        g.import_all(ranks, totals)
        g.merge(RS, want, want_t, _summ(oracle, want, want_t), ranks, "second row")


# ---- (e) the record paths ----------------------------------------------------------------------------
def test_record_paths_put_headers_on_words_63_and_65(oracle):
    """By ingest on a one-rank-heavy group: series 0 of a big tile receives one sample in
    each of buckets 0..62 and 2 200 000 in each of buckets 63 and 64 (a header on word 63,
    the next right after its count), series 16 -- the other half of the tile -- 62 leading
    single samples and the same two counts.  By import plus ingest (a dirty state row
    summed with new records): a bucket imported at MERGE_CMAX - 1 with one sample ingested
    into it (escaped only in the sum, with a look-alike count word), the same with the
    sample in the next bucket (stays plain), and a bucket imported at 2^31 - 2 with one
    sample ingested."""
    W, S, heavy = 2, 96, 2_200_000
    BV = SR.BUCKET_VALUES
    parts = []
    for s, lead in ((0, 63), (16, 62)):
        parts.append((np.full(lead, s, np.uint32), BV[:lead]))
        for b in (lead, lead + 1):
            parts.append((np.full(heavy, s, np.uint32), np.full(heavy, BV[b], np.float32)))
    b0 = 100
    parts.append((np.array([64, 65, 66], np.uint32), BV[[b0, b0 + 1, b0]]))
    series = np.concatenate([p[0] for p in parts])
    values = np.concatenate([p[1] for p in parts]).astype(np.float32)
    perm = np.random.default_rng(63).permutation(series.size)
    series, values = series[perm], values[perm]
    imp = np.zeros((3, NB), np.int32)
    imp[0, b0], imp[1, b0], imp[2, b0] = CMAX - 1, CMAX - 1, INT_MAX - 1
    imp_t = np.array([2 ** 53 + 1, -5, 12345], np.int64)
    light = (np.arange(S, dtype=np.uint32), np.full(S, BV[5], np.float32))  # rank 1: one sample per series
    held = []
    for batch in ((series, values), light):
        o = oracle.OracleHistograms(S)
        assert o.ingest(*batch, threads=8) == 0
        held.append((o.counts().astype(np.int64), o.totals().copy()))
    held[0][0][64:67] += imp
    held[0][1][64:67] += imp_t
    want, want_t = held[0][0] + held[1][0], held[0][1] + held[1][1]
    assert want[0, 63] == want[0, 64] == heavy and (want[0, :63] >= 1).all() and want[16, 62] == heavy
    assert want[64, b0] == CMAX and want[65, b0] == CMAX - 1 and want[66, b0] == INT_MAX
    with _Group(S, W) as g:
        g.engines[0].import_state(imp, imp_t, first=64)
        g.engines[0].ingest(series, values)
        g.engines[1].ingest(*light)
        g.merge(RS, want, want_t, _summ(oracle, want, want_t), [h[0] for h in held], "record paths")


# ---- (f) the worst case of the half-tile's encoding bound -----------------------------------------------
@pytest.mark.parametrize("how", ["import", "import_plus_ingest"])
def test_half_tile_of_rows_at_the_encoding_bound(oracle, cat, how):
    """Series 0..15 (one half-tile) with all 1798 buckets at MERGE_CMAX: 16 rows of 3596
    words, the most a half-tile's encoding can hold (ENC_HALF_CAP).  Once imported as they
    are, once imported at MERGE_CMAX - 1 with one sample ingested per bucket and series
    (28 768 records over dirty rows: the bound's 2 words per record exceed the cap).  Series
    16..31 hold single samples; all 32 rows and the rest of the slice must arrive whole."""
    W, S = 2, 70
    BV = SR.BUCKET_VALUES
    own = np.zeros((S, NB), np.int64)
    own_t = M.totals_of(0, S).copy()
    own[32:] = cat[20:20 + S - 32]
    if how == "import":
        own[:16] = CMAX
        for j in range(16):
            own[16 + j, :100 * j + 1] = 1
        batch = None
    else:
        own[:16] = CMAX - 1
        series = np.concatenate([np.repeat(np.arange(16, dtype=np.uint32), NB)] +
                                [np.full(50 * (j + 1), 16 + j, np.uint32) for j in range(16)])
        values = np.concatenate([np.tile(BV, 16)] + [BV[:50 * (j + 1)] for j in range(16)])
        perm = np.random.default_rng(16).permutation(series.size)
        batch = (series[perm], values[perm].astype(np.float32))
        assert (batch[0] < 16).sum() == 28768
    imported = own.astype(np.int32)
    if batch is not None:
        o = oracle.OracleHistograms(S)
        assert o.ingest(*batch) == 0
        own += o.counts()
        own_t = own_t + o.totals()
    assert (own[:16] == CMAX).all() and (M.row_words(own[:16]) == 3596).all() and own[16:32].any(axis=1).all()
    bg = M.background(own, W)
    bg_t = M.totals_of(1, S)
    want, want_t = own + bg, M.wrap_sum([own_t, bg_t])
    with _Group(S, W) as g:
        g.engines[0].import_state(imported, M.totals_of(0, S))
        if batch is not None:
            g.engines[0].ingest(*batch)
        g.engines[1].import_state(bg, bg_t)
        g.merge(RS, want, want_t, _summ(oracle, want, want_t), [own, bg], f"half-tile bound, {how}")


# ---- (g) empty slices ----------------------------------------------------------------------------------
@MODES
def test_empty_slices(oracle, cat, mode):
    """S = 5 < W = 8: ranks 5..7 own no row and report (5, 0)."""
    W = 8
    words = M.row_words(cat)
    rows = cat[[0, int(np.flatnonzero(words == 0)[0]), 25, 60, cat.shape[0] - 1]]
    S = rows.shape[0]
    ranks, totals, want, want_t = M.split(rows, W, rot=2)
    with _Group(S, W) as g:
        g.import_all(ranks, totals)
        res = g.merge(mode, want, want_t, _summ(oracle, want, want_t), ranks, "empty slices")
        if mode == RS:
            assert [(f, c) for f, c, *_ in res] == [(0, 1), (1, 1), (2, 1), (3, 1), (4, 1), (5, 0), (5, 0), (5, 0)]


# ---- (h) the documented wrap -----------------------------------------------------------------------------
@MODES
def test_merge_checks_no_range_and_wraps_in_32_bits(oracle, mode):
    """include/l5dhist.h: the merge adds the ranks' bucket counts in 32 bits and checks no
    range; the merged row's count is exact for the buckets as merged.  2^31 - 1 and 2 in
    one bucket: counts_out holds 2^31 + 1 as uint32, the summary's count is the sum of the
    row's buckets as uint32.  (Nothing above 2^32 is pinned.)"""
    W, S, b = 2, 3, 500
    ranks = [np.zeros((S, NB), np.int32) for _ in range(W)]
    ranks[0][:, 10], ranks[1][:, 1000] = 4, 6
    ranks[0][1, b], ranks[1][1, b] = INT_MAX, 2
    totals = [np.array([5, 7, -9], np.int64), np.array([1, 2, 3], np.int64)]
    want = ranks[0].astype(np.int64) + ranks[1]
    want_t = totals[0] + totals[1]
    keep = np.array([0, 2])
    want_s = oracle.summarize_counts(want[keep].astype(np.int32), want_t[keep])
    with _Group(S, W) as g:
        g.import_all(ranks, totals)
        res = g.merge(mode, None, want_t, None, ranks, "wrap")
        for first, count, summ, cnt, tot in res:
            got = cnt.view(np.uint32).astype(np.int64)
            np.testing.assert_array_equal(got, want[first:first + count])
            for i in range(count):
                s = first + i
                if s == 1:
                    assert got[i, b] == 2 ** 31 + 1 and int(summ["count"][i]) == 2 ** 31 + 1 + 10
                else:
                    assert summ[i].tobytes() == want_s[list(keep).index(s)].tobytes()
