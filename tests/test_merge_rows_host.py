"""The crafted merge rows (tests/merge_rows.py) checked on the CPU: the catalogue puts
escape headers where it claims, round-trips through the format's restatement
(fleet.sparse_encode / sparse_decode) and through the 64-word-chunk model of k_mdecode's
parse -- and each of the model's three defects gets catalogue rows wrong, so the GPU test
that feeds these rows to the kernel would notice the same slip."""
import numpy as np
import pytest

from linkerd_amd import fleet
from tests import merge_rows as M


@pytest.fixture(scope="module")
def cat():
    rows = M.catalogue()
    enc, words = fleet.sparse_encode(rows)
    rows.setflags(write=False)
    return rows, enc, words


def test_catalogue_is_legal_and_holds_the_named_rows(cat):
    rows, enc, words = cat
    assert rows.dtype == np.int32 and rows.shape[1] == M.NB and rows.flags["C_CONTIGUOUS"]
    assert rows.min() == 0 and rows.max() == M.INT_MAX
    assert rows.shape[0] % 6 != 0  # not a multiple of both 2 and 3: a short last slice
    np.testing.assert_array_equal(words, M.row_words(rows))
    assert words.max() == 2 * M.NB == 3596 and (rows[0] >= M.CMAX).all()  # the whole-row run comes first
    assert (words == 0).any()
    nz = rows != 0
    alone = nz.sum(axis=1) == 1
    for b in (0, M.NB - 1):
        c = rows[alone & nz[:, b], b]
        assert (c < M.CMAX).any() and (c >= M.CMAX).any(), b
    # the sweep: the header of bucket p is word p, a second one follows at word p + 3
    sweep = M.position_rows()
    e2, w2 = fleet.sparse_encode(sweep)
    got = {}
    for r, i, c in M.headers(e2, w2):
        got.setdefault(r, []).append((i, c))
    k = len(M.LOOKALIKE)
    for n, p in enumerate(M.POSITIONS):
        for j, c in enumerate(M.LOOKALIKE):
            h = got[n * k + j]
            assert h[0] == (p, c)
            if p + 2 < M.NB and c != M.INT_MAX:
                assert h[1][0] == p + 3 and h[1][1] >= M.CMAX
    both = lambda *ws: all(w in M.POSITIONS for w in ws)  # noqa: E731
    assert both(61, 62, 63, 64, 65) and both(127, 128) and both(191, 192) and both(255, 256)
    assert both(319, 320, 321) and both(575, 576) and both(1795, 1796)
    for n in (1, 2, 31, 32, 33, 64, 65, 160, 899, M.NB):
        assert n in M.RUNS


def test_headers_cover_every_lane_and_the_prefetch_groups(cat):
    rows, enc, words = cat
    hs = M.headers(enc, words)
    assert {i % M.CHUNK for _, i, _ in hs} == set(range(64))
    chunks = {i // M.CHUNK for _, i, _ in hs}
    assert chunks >= {0, 1, 4, 5, 8, 9} and max(chunks) == 3595 // M.CHUNK
    # a header on lane 63 in chunk 0, in a group's last chunk and in a later group's
    last = {i // M.CHUNK for _, i, _ in hs if i % M.CHUNK == 63}
    assert last >= {0, 4, 8}
    # two escapes in one row, back to back and apart
    per_row = np.bincount([r for r, _, _ in hs], minlength=rows.shape[0])
    assert (per_row >= 2).sum() > 100 and per_row.max() == M.NB


def test_every_lookalike_count_follows_a_header(cat):
    rows, enc, words = cat
    counts = {c for _, _, c in M.headers(enc, words)}
    assert counts >= set(M.LOOKALIKE)
    for c in (2 ** 21 - 1, 2 ** 22 - 1, (5 << 21) | M.CMAX, 2 ** 31 - 1):
        assert c & M.CMAX == M.CMAX and c in counts  # a count word that looks like a header
    # ... also as the first word of a chunk, behind a header on lane 63
    first = {c for _, i, c in M.headers(enc, words) if i % M.CHUNK == 63}
    assert first >= set(M.LOOKALIKE)


def test_format_round_trip(cat):
    rows, enc, words = cat
    assert enc.size == int(words.sum())
    np.testing.assert_array_equal(fleet.sparse_decode([(enc, words)], rows.shape[0]), rows)


def test_chunk_model_decodes_the_catalogue(cat):
    rows, enc, words = cat
    got = M.chunk_decode(enc, words)
    assert not got[:, M.NB:].any()
    np.testing.assert_array_equal(got[:, :M.NB], rows)


@pytest.mark.parametrize("defect", M.DEFECTS)
def test_each_defect_gets_catalogue_rows_wrong(cat, defect):
    rows, enc, words = cat
    got = M.chunk_decode(enc, words, defect=defect)
    bad = np.flatnonzero((got[:, :M.NB] != rows).any(axis=1) | got[:, M.NB:].any(axis=1))
    assert bad.size >= 1, defect
    # and the sweep alone (what tests (a) and (d) of the GPU suite merge) shows it too
    n_runs = 2 * len(M.RUNS)
    assert (bad >= n_runs).any(), defect


@pytest.mark.parametrize("W", [2, 3, 8, 9, 16, 64])
def test_split_keeps_every_sum_in_range(cat, W):
    rows = cat[0]
    for rot in (0, 1):
        ranks, totals, want, want_t = M.split(rows, W, rot)
        assert len(ranks) == len(totals) == W
        acc = np.zeros(rows.shape, np.int64)
        for q, rr in enumerate(ranks):
            assert rr.dtype == np.int32 and rr.min() >= 0
            own = (np.arange(rows.shape[0]) + rot) % W == q
            # every source has words for every row (but the owner of the empty row)
            assert ((rr != 0).any(axis=1) | (own & ~rows.any(axis=1))).all()
            np.testing.assert_array_equal(rr[own], rows[own])
            acc += rr
        assert acc.max() <= M.INT_MAX == want.max()
        np.testing.assert_array_equal(acc, want)
        # escaped and plain adds meet in one bucket
        assert ((rows >= M.CMAX) & (want > rows)).any()
        py = [sum(int(t[i]) for t in totals) for i in range(8)]
        assert [((v + 2 ** 63) % 2 ** 64) - 2 ** 63 for v in py] == want_t[:8].tolist()
        assert set(M.SPECIAL_TOTALS) == set(totals[0].tolist())


def test_slice_words_match_the_encoding(cat):
    rows = cat[0]
    for W in (2, 3):
        ranks, _, _, _ = M.split(rows, W)
        per = -(-rows.shape[0] // W)
        for rr in ranks:
            total, per_slice = M.slice_words(rr, W)
            assert total == fleet.sparse_encode(rr)[0].size == int(per_slice.sum())
            for q in range(W):
                assert per_slice[q] == fleet.sparse_encode(rr[q * per:(q + 1) * per])[0].size
