"""Crafted bucket-count rows that pin the fleet merge's sparse encoding: the encoders
(row_encode / row_words, the export's first-touch lists, k_mpack) and the decoder
(k_mdecode, which parses 64 words per step).

A random Zipf sample puts an escaped count (>= 2^21 - 1, which takes a second word)
in a row of a handful of words, if anywhere.  The rows here put escape headers on every
lane of the decoder's 64-word chunk, on both sides of every chunk edge and of every
four-chunk prefetch group, back to back, and give them counts whose own low 21 bits are
all ones, so a count word looks like a header to a decoder that does not resolve
headers in order:

* position sweep: row (p, k) holds one sample in each of buckets 0..p-1, bucket p at
  the escaped count k, bucket p + 1 at 3 and bucket p + 2 escaped again -- the header of
  bucket p is word p of the row;
* runs: n consecutive escaped buckets (counts cycling through the look-alike values)
  behind 0 or 1 single sample, n up to the whole row (3596 words);
* ends: the empty row, bucket 0 alone and bucket 1797 alone, plain and escaped.

split() deals the catalogue to W ranks over background rows, so that escaped and plain
adds of different sources meet in the same bucket; chunk_decode() restates k_mdecode's
chunked parse in plain Python and can switch on three defects, which
tests/test_merge_rows_host.py shows the catalogue catches.

Counts stay in [0, 2^31 - 1].  Everything is built on the CPU with numpy;
linkerd_amd.fleet.sparse_encode / sparse_decode restate the format and the oracle is the
only reference for the summaries.
"""
import numpy as np

from tests.summary_rows import INT_MAX, NB, SPECIAL_TOTALS

CMAX = 0x1FFFFF  # the count field of an entry; a count >= CMAX is escaped (MERGE_CMAX)
CHUNK = 64       # words k_mdecode parses per step
AHEAD = 4        # chunks it loads together after the first (MDEC_AHEAD)

# Escaped counts: the least one (its count word is 0x1FFFFF: a header of bucket 0), the
# next (low bits zero), and counts whose low 21 bits are all ones up to a saturated bucket.
LOOKALIKE = (2 ** 21 - 1, 2 ** 21, 2 ** 22 - 1, (5 << 21) | CMAX, 2 ** 30, INT_MAX)
# word of the first header: lanes 61..65 of chunk 0 / 1, the chunk edges, the edges of the
# prefetch groups (chunks 1..4 = words 64..319, chunks 5..8 = 320..575) and the row's end
POSITIONS = (0, 1, 2, 59, 60, 61, 62, 63, 64, 65, 124, 126, 127, 128, 129, 188, 190, 191, 192, 193, 252, 254, 255,
             256, 257, 316, 318, 319, 320, 321, 322, 572, 574, 575, 576, 577, 1795, 1796, 1797)
RUNS = (1, 2, 31, 32, 33, 64, 65, 160, 899, NB)
SMALL = 7  # bucket p + 2 beside a saturated bucket p


def position_rows() -> np.ndarray:
    rows = np.zeros((len(POSITIONS) * len(LOOKALIKE), NB), np.int32)
    i = 0
    for p in POSITIONS:
        for j, k in enumerate(LOOKALIKE):
            r = rows[i]
            r[:p] = 1
            r[p] = k
            if p + 1 < NB:
                r[p + 1] = 3
            if p + 2 < NB:
                r[p + 2] = SMALL if k == INT_MAX else LOOKALIKE[(j + 1) % len(LOOKALIKE)]
            i += 1
    return rows


def run_rows() -> np.ndarray:
    """The longest run first."""
    rows = np.zeros((2 * len(RUNS), NB), np.int32)
    cyc = np.resize(np.array(LOOKALIKE, np.int64), NB)
    for i, n in enumerate(reversed(RUNS)):
        for lead in (0, 1):  # headers on even words / on odd words
            r = rows[2 * i + lead]
            n1 = min(n, NB - lead)
            r[:lead] = 1
            r[lead:lead + n1] = cyc[:n1]
    return rows


def end_rows() -> np.ndarray:
    rows = np.zeros((7, NB), np.int32)  # row 0: empty
    rows[1, 0], rows[2, NB - 1] = 1, 1
    rows[3, 0], rows[4, NB - 1] = CMAX, INT_MAX
    rows[5, 0], rows[5, NB - 1] = INT_MAX, CMAX
    rows[6, 0], rows[6, NB - 1] = 2 ** 22 - 1, 1
    return rows


def catalogue() -> np.ndarray:
    """[R][1798] int32; the runs first (the longest rows), then the sweep and the ends."""
    rows = np.ascontiguousarray(np.concatenate([run_rows(), position_rows(), end_rows()]))
    assert rows.dtype == np.int32 and rows.min() >= 0
    return rows


def row_words(rows: np.ndarray) -> np.ndarray:
    """Encoding words per row: non-empty buckets + escaped counts."""
    u = np.asarray(rows).astype(np.int64)
    return ((u != 0).sum(axis=1) + (u >= CMAX).sum(axis=1)).astype(np.int64)


def headers(enc: np.ndarray, words: np.ndarray):
    """(row, word index within the row, count) of every escaped entry, by a sequential
    parse of each row."""
    out = []
    off = 0
    for r, nw in enumerate(np.asarray(words, np.int64)):
        i = 0
        while i < nw:
            if int(enc[off + i]) & CMAX == CMAX:
                out.append((r, i, int(enc[off + i + 1])))
                i += 1
            i += 1
        off += int(nw)
    return out


def totals_of(rank: int, nrows: int) -> np.ndarray:
    """A rank's int64 totals: SPECIAL_TOTALS cycled, shifted by the rank."""
    return np.array(SPECIAL_TOTALS, np.int64)[(np.arange(nrows) + rank) % len(SPECIAL_TOTALS)]


def wrap_sum(totals) -> np.ndarray:
    """The int64 sum of the ranks' totals as the merge computes it (two's complement)."""
    acc = np.zeros(len(totals[0]), np.uint64)
    for t in totals:
        acc = acc + np.asarray(t, np.int64).view(np.uint64)
    return acc.view(np.int64)


def background(owner_rows: np.ndarray, W: int) -> np.ndarray:
    """The other ranks' row of each series: 1 in every bucket where the owner's count
    leaves room for W - 1 more, nothing elsewhere."""
    return (owner_rows.astype(np.int64) < INT_MAX - W).astype(np.int32)


def split(rows: np.ndarray, W: int, rot: int = 0):
    """(per-rank rows [W] of [R][1798] int32, per-rank totals [W] of [R] int64, expected
    rows [R][1798] int64, expected totals [R] int64): row i goes to rank (i + rot) % W,
    every other rank holds its background row."""
    R = rows.shape[0]
    owner = (np.arange(R) + rot) % W
    bg = background(rows, W)
    assert bg.any(axis=1).all()  # every source holds words for every row
    ranks = [np.ascontiguousarray(np.where((owner == q)[:, None], rows, bg)).astype(np.int32) for q in range(W)]
    want = rows.astype(np.int64) + (W - 1) * bg.astype(np.int64)
    assert sum(r.astype(np.int64) for r in ranks).tobytes() == want.tobytes()
    assert want.max() <= INT_MAX and want.min() >= 0
    totals = [totals_of(q, R) for q in range(W)]
    return ranks, totals, want, wrap_sum(totals)


def slice_words(rank_rows: np.ndarray, W: int):
    """(words of all the rank's rows, words per destination slice [W]) of the
    reduce-scatter's ceil(S / W)-row slices."""
    w = row_words(rank_rows)
    per = -(-rank_rows.shape[0] // W)
    padded = np.zeros(per * W, np.int64)
    padded[:w.size] = w
    return int(w.sum()), padded.reshape(W, per).sum(axis=1)


# ---- k_mdecode's parse, 64 words at a time ---------------------------------------------
DEFECTS = ("no_carry", "unordered_headers", "lane63_next_lane")


def chunk_decode(enc: np.ndarray, words: np.ndarray, defect=None) -> np.ndarray:
    """One source's rows decoded as k_mdecode's `parse` does: per 64-word chunk the
    ballot of the words that look like a header, the headers resolved in order (the word
    behind a header is its count, never a header), a header on lane 63 carried into the
    next chunk, whose first word is then a count, and that lane's count read from the
    next word.  Returns [rows][2048] int64 (a wrong parse can name buckets >= 1798).

    defect: "no_carry" forgets the carried header; "unordered_headers" takes every
    look-alike word as a header at once (payload = headers << 1); "lane63_next_lane"
    gives lane 63 what a shift from the next lane returns at the wave's end (its own
    word) instead of the next word."""
    assert defect is None or defect in DEFECTS
    words = np.asarray(words, np.int64)
    out = np.zeros((words.size, 2048), np.int64)
    off = 0
    for r, nw in enumerate(words):
        nw = int(nw)
        carry = False
        for base in range(0, nw, CHUNK):
            n = min(CHUNK, nw - base)
            x = [int(v) for v in enc[off + base:off + base + n]]
            hm = [(v & CMAX) == CMAX for v in x]
            pay = [False] * CHUNK
            if carry and defect != "no_carry":
                pay[0] = True
                hm[0] = False
            next_carry = False
            if defect == "unordered_headers":
                for h in range(n):
                    if hm[h]:
                        if h == CHUNK - 1:
                            next_carry = True
                        else:
                            pay[h + 1] = True
            else:
                for h in range(n):
                    if not hm[h]:
                        continue
                    if h == CHUNK - 1:
                        next_carry = True
                    else:
                        pay[h + 1] = True
                        if h + 1 < n:
                            hm[h + 1] = False
            for lane in range(n):
                if pay[lane]:
                    continue
                b, c = x[lane] >> 21, x[lane] & CMAX
                if c == CMAX:
                    if lane == CHUNK - 1:
                        c = x[lane] if defect == "lane63_next_lane" else int(enc[off + base + lane + 1])
                    else:
                        c = x[lane + 1] if lane + 1 < n else 0
                out[r, b] += c
            carry = next_carry
        off += nw
    return out
