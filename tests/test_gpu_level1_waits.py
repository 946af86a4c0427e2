"""Level 1 (k_rbin1w): every way a sub-chunk's sample loads are issued and waited for.

A full sub-chunk's first half is loaded while the sub-chunk before it is still being
partitioned and its arrival is forced before that one's write-out; the second half is
loaded during the first half's ranking; a load with nothing to fetch re-reads a table;
the ragged loader and the slow path's re-reads wait for their own loads where they are
issued.  None of this may change a result, so every case is bit-exact against the CPU
oracle: dense counts and all summary fields, compared as tests/test_gpu_level1_sums.py
does.  The shapes walk the prefetch's condition: per-slab sample counts around whole
sub-chunks (CHW = 16384 slots), so that a slab has no prefetch, a prefetch of its last
full sub-chunk, a ragged tail after a prefetched one, or a condition that flips on the
last iteration.
"""
import numpy as np
import pytest

from linkerd_amd import _native as N

from .test_gpu_level1_sums import _assert_equal, _engine, _skewed, _values

pytestmark = pytest.mark.gpu

CHW = 16384  # slots per sub-chunk
S = 4096


def _check(oracle, series, vals, params, label, S=S):
    o = oracle.OracleHistograms(S)
    o.ingest(series, vals)
    with _engine(S, params) as eng:
        eng.ingest(series, vals)
        _assert_equal(eng, o, True, label)


# (samples per slab, slabs): a count that is no multiple of 4 is one slab's (the host rounds
# a slab's length up to 4, so only the batch's last slab can have such a count)
PER_SLAB = [(CHW, 4), (CHW + 1, 1), (2 * CHW, 3), (2 * CHW + 4, 2), (3 * CHW - 4, 2), (3 * CHW, 2), (5 * CHW + 7, 1),
            (9000, 3), (5001, 1)]


@pytest.mark.parametrize("per,slabs", PER_SLAB, ids=[f"{p}x{g}" for p, g in PER_SLAB])
def test_samples_per_slab(oracle, per, slabs):
    """Each slab holds exactly `per` samples: no prefetch at all (one sub-chunk or less), a
    prefetch of the last full sub-chunk (2 CHW, 3 CHW), a ragged tail after a prefetched
    sub-chunk (CHW + 1 has none before it, 2 CHW + 4 and 5 CHW + 7 have), and 3 CHW - 4,
    whose last sub-chunk misses being full by one 16-B group."""
    rng = np.random.default_rng(1000 + per)
    n = per * slabs
    assert per % 4 == 0 or slabs == 1
    assert slabs == min(slabs, (n + 8191) // 8192)  # the host makes exactly `slabs` slabs of `per`
    series, vals = _skewed(rng, S, n, tile=77)
    _check(oracle, series, vals, [(N.PARAM_MAX_SLABS, slabs)], f"{per} samples x {slabs} slabs")


def test_last_slab_ragged(oracle):
    """Two slabs of 2 CHW + 4 and 2 CHW + 1 samples: the prefetch condition differs between
    the workgroups of one launch."""
    rng = np.random.default_rng(107)
    n = (2 * CHW + 4) + (2 * CHW + 1)
    series, vals = _skewed(rng, S, n, tile=11)
    _check(oracle, series, vals, [(N.PARAM_MAX_SLABS, 2)], "last slab ragged")


@pytest.mark.parametrize("n", [3 * CHW + 5, 2 * (2 * CHW) + 3], ids=["one_slab", "two_slabs"])
def test_batch_offset_by_one_element(oracle, n):
    """Device tensors that start one element past a 16-B boundary (vec == 0): the ragged
    loader in every sub-chunk, and every vector load re-reads the table."""
    import torch
    rng = np.random.default_rng(109)
    series, vals = _skewed(rng, S, n, tile=101)
    o = oracle.OracleHistograms(S)
    o.ingest(series, vals)
    ds = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    dv = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    ds[1:].copy_(torch.from_numpy(series.view(np.int32)))
    dv[1:].copy_(torch.from_numpy(vals))
    s1, v1 = ds[1:], dv[1:]
    assert s1.data_ptr() % 16 == 4 and v1.data_ptr() % 16 == 4
    with _engine(S, [(N.PARAM_MAX_SLABS, 1 if n < 4 * CHW else 2)]) as eng:
        eng.ingest(s1, v1)
        _assert_equal(eng, o, True, "offset by one element")


def _zipf(rng, S, n):
    """Zipf ranks over a shuffled id space: a head of a few very hot series, in tiles apart."""
    ranks = np.minimum(rng.zipf(1.2, size=n), S) - 1
    return rng.permutation(S).astype(np.uint32)[ranks]


@pytest.mark.parametrize("S,dmax", [(4096, 0), (1 << 20, None), (4096, 2), (100_000, 5), (4096, None)],
                         ids=["S4096-none", "S1M-uniform-none", "S4096-dmax2", "S100000-dmax5", "S4096-default"])
def test_direct_and_super_tile_runs(oracle, S, dmax):
    """No direct tile at all (u32 records only: the parameter at 0, or 2^20 series with less than
    one sample per tile), and a Zipf head with the number of direct tiles capped, so that a
    write-out group of 64 stage entries holds u32 and u16 records and one group straddles the
    boundary between the two widths."""
    rng = np.random.default_rng(113 + S % 1000)
    n = 3 * (2 * CHW + 4)
    if S == 1 << 20:
        series = rng.integers(0, S, size=n, dtype=np.uint32)
    else:
        series = _zipf(rng, S, n)
    vals = _values(rng, n)
    params = [(N.PARAM_MAX_SLABS, 3)] + ([] if dmax is None else [(N.PARAM_DIRECT_MAX, dmax)])
    if S == 1 << 20:
        touched = np.unique(series)
        o = oracle.OracleHistograms(touched.size)
        o.ingest(np.searchsorted(touched, series).astype(np.uint32), vals)
        with _engine(S, params) as eng:
            eng.ingest(series, vals)
            for first in (0, S // 2, S - 2048):  # bucket rows: three windows of 2048 series
                rows, counts = eng.snapshot(first=first, count=2048, reset=False, with_counts=True)
                t = touched[(touched >= first) & (touched < first + 2048)]
                at = np.searchsorted(touched, t)
                np.testing.assert_array_equal(counts[t - first], o.h["counts"][at])
                assert int(counts.sum()) == int(o.h["counts"][at].sum())
            got = eng.snapshot(reset=True)
            want = o.snapshot(reset=True)
            for f in N.SUMMARY_FIELDS:
                g, w = got[f][touched], want[f]
                same = (g == w) | (np.isnan(g) & np.isnan(w)) if f == "avg" else g == w
                assert same.all(), f"field {f}"
            rest = np.ones(S, bool)
            rest[touched] = False
            assert not got["count"][rest].any()
        return
    _check(oracle, series, vals, params, f"S={S} dmax={dmax}", S=S)


def test_invalid_ids_inside_a_full_subchunk(oracle):
    """Ids >= S in the middle of the second of three full sub-chunks only: their trash-bin
    records are dropped in the write-out, the error is reported once, the rest is exact."""
    rng = np.random.default_rng(127)
    n = 3 * CHW
    series, vals = _skewed(rng, S, n, tile=120)
    bad = np.zeros(n, bool)
    bad[CHW + 5000:CHW + 5300] = True
    bad[CHW + 9001] = True
    series[bad] = rng.choice(np.array([S, S + 1, 1 << 20, 0xFFFFFFFF], np.uint32), size=int(bad.sum()))
    o = oracle.OracleHistograms(S)
    o.ingest(series[~bad], vals[~bad])
    with _engine(S, [(N.PARAM_MAX_SLABS, 1)]) as eng:
        eng.ingest(series, vals)
        with pytest.raises(N.L5dhError, match="EINVAL"):
            eng.sync()
        eng.sync()  # reported once
        _assert_equal(eng, o, True, "invalid ids dropped")


def test_redo_pass_runs_the_same_loop(oracle):
    """Regions at 40 % of the plan: runs are dropped and the redo pass runs over the same
    sub-chunk loop; results stay exact and partition_redos increases."""
    rng = np.random.default_rng(131)
    n = 2 * (5 * CHW + 8)
    series, vals = _skewed(rng, S, n, tile=55)
    o = oracle.OracleHistograms(S)
    o.ingest(series, vals)
    with _engine(S, [(N.PARAM_MAX_SLABS, 2), (N.PARAM_REGION_PCT, 40)]) as eng:
        r0 = eng.partition_redos()[0]
        eng.ingest(series, vals)
        _assert_equal(eng, o, True, "redo")
        assert eng.partition_redos()[0] > r0


def test_two_ingests_before_one_snapshot(oracle):
    """The second call's first sub-chunk follows the first call's stores: two ingests (two
    segments) of one slab each, then one snapshot."""
    rng = np.random.default_rng(137)
    o = oracle.OracleHistograms(S)
    with _engine(S, [(N.PARAM_MAX_SLABS, 1), (N.PARAM_MAX_SEGMENTS, 2)]) as eng:
        for tile, n in ((5, 2 * CHW), (99, 3 * CHW + 9)):
            b = _skewed(rng, S, n, tile)
            eng.ingest(*b)
            o.ingest(*b)
        _assert_equal(eng, o, True, "two ingests")


def test_threshold_values_in_every_group(oracle):
    """0, the values just below and at 2^17 and around the escape bound, one of them in every
    group of four slots of three full sub-chunks and a ragged one: every group takes the slow
    path, whose re-reads share the wait counter with the loads in flight."""
    rng = np.random.default_rng(139)
    n = 3 * CHW + 1001
    series, vals = _skewed(rng, S, n, tile=33)
    v_esc = float((1 << 21) - 2048)
    edge = np.array([0.0, -0.0, 131071.0, 131071.5, 131072.0, v_esc - 1, v_esc - 0.5, v_esc, np.nan], np.float32)
    pos = np.arange(0, n, 4) + rng.integers(0, 4, size=(n + 3) // 4)
    pos = pos[pos < n]
    vals[pos] = edge[rng.integers(0, edge.size, size=pos.size)]
    _check(oracle, series, vals, [(N.PARAM_MAX_SLABS, 1)], "threshold values")
