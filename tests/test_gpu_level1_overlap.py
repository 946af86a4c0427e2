"""Level 1 (k_rbin1w) from one sub-chunk to the next: what a workgroup carries across its
16K-slot sub-chunks (the stage, the counts, the run-head bitmap, the direct sums and their
guard) and how its waves are ordered between them.  Written for the forms that overlap a
sub-chunk's write-out with the next one's ranking (measured, not kept: DESIGN 6c) and kept as
the net under any change to the sub-chunk loop's barriers, clears or wave scheduling.  What
such a change could break lies between consecutive sub-chunks of one workgroup, so the shapes
are about sub-chunks per slab (none after another, one, many, a ragged one after full ones,
every one ragged), not about size.  Everything is bit-exact against the CPU oracle: dense
counts and all summary fields.

No test can force an interleaving of waves: the ordering is argued at the kernel's barriers,
these cases are the net under the argument.
"""
import numpy as np
import pytest

from linkerd_amd import _native as N

pytestmark = pytest.mark.gpu

V_ESC = (1 << 21) - 2048
CHW = 16384  # slots per sub-chunk
S = 4096


def _assert_equal(eng, o, reset, label):
    got, counts = eng.snapshot(reset=reset, with_counts=True)
    np.testing.assert_array_equal(counts, o.counts(), err_msg=label)
    want = o.snapshot(reset=reset)
    for f in N.SUMMARY_FIELDS:
        g, w = got[f], want[f]
        same = (g == w) | (np.isnan(g) & np.isnan(w)) if f == "avg" else g == w
        assert same.all(), f"{label} field {f}: series {int(np.flatnonzero(~same)[0])}: " \
                           f"got {g[~same][0]!r} want {w[~same][0]!r}"


def _engine(params=()):
    from linkerd_amd.engine import HistogramEngine
    e = HistogramEngine(S)
    e.set_param(N.PARAM_STAGE_SAMPLES, 0)  # every ingest binned at once
    for k, v in params:
        e.set_param(k, v)
    return e


def _values(rng, n):
    """Lognormal values, an eighth of them replaced by the edges of level 1's value classes."""
    vals = np.exp(4.0 + 1.5 * rng.standard_normal(n)).astype(np.float32)
    edge = np.array([0.0, -0.0, -7.5, np.nan, np.inf, 131071.0, 131071.5, 131072.0, V_ESC - 1, V_ESC - 0.5, V_ESC,
                     2.0 ** 31], np.float32)
    pos = rng.choice(n, size=n // 8, replace=False)
    vals[pos] = edge[rng.integers(0, edge.size, size=pos.size)]
    return vals


def _skewed(rng, n, tile):
    """Three series of one tile hold ~60 % of the samples (a direct tile: two half-bins with
    u16 records and LDS value sums), the rest are uniform (super-tile bins, u32 records)."""
    hot = tile * 32 + np.array([1, 16, 31], np.uint32)
    series = rng.integers(0, S, size=n, dtype=np.uint32)
    m = rng.random(n) < 0.6
    series[m] = hot[rng.integers(0, 3, size=int(m.sum()))]
    return series, _values(rng, n)


def _check_one_ingest(oracle, series, vals, params, label):
    o = oracle.OracleHistograms(S)
    o.ingest(series, vals)
    with _engine(params) as eng:
        eng.ingest(series, vals)
        _assert_equal(eng, o, True, label)


@pytest.mark.parametrize("extra", [0, 1027], ids=["full", "ragged_tail"])
def test_one_slab_many_subchunks(oracle, extra):
    """One workgroup runs 128 sub-chunks back to back; with 1027 samples more, a ragged last
    sub-chunk whose length is no multiple of 4 follows the full ones (the staging's full ->
    ragged transition)."""
    rng = np.random.default_rng(71)
    n = (1 << 21) + extra
    series, vals = _skewed(rng, n, tile=77)
    _check_one_ingest(oracle, series, vals, [(N.PARAM_MAX_SLABS, 1)], f"one slab n={n}")


@pytest.mark.parametrize("subchunks", [1, 2], ids=["one", "two"])
def test_exact_subchunks_per_slab(oracle, subchunks):
    """Four slabs of exactly one sub-chunk (nothing overlaps) and of exactly two (one overlap,
    followed straight by the slab's flush of the direct sums)."""
    rng = np.random.default_rng(73)
    slabs = 4
    n = subchunks * CHW * slabs
    series, vals = _skewed(rng, n, tile=3)
    _check_one_ingest(oracle, series, vals, [(N.PARAM_MAX_SLABS, slabs)], f"{subchunks} sub-chunks per slab")


def test_unaligned_device_inputs(oracle):
    """Device tensors that start one element past a 16-B boundary: no vector loads, every
    sub-chunk takes the slot-by-slot load.  Two slabs, a ragged end."""
    import torch
    rng = np.random.default_rng(79)
    n = (1 << 19) + 5
    series, vals = _skewed(rng, n, tile=101)
    o = oracle.OracleHistograms(S)
    o.ingest(series, vals)
    ds = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    dv = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    ds[1:].copy_(torch.from_numpy(series.view(np.int32)))
    dv[1:].copy_(torch.from_numpy(vals))
    s1, v1 = ds[1:], dv[1:]
    assert s1.data_ptr() % 16 == 4 and v1.data_ptr() % 16 == 4
    with _engine([(N.PARAM_MAX_SLABS, 2)]) as eng:
        eng.ingest(s1, v1)
        _assert_equal(eng, o, True, "unaligned")


def test_redo_pass(oracle):
    """Regions at 40 % of the plan: runs overflow, level 1 is redone with exact regions -- the
    same sub-chunk loop with pass == 1, which adds nothing to any sum."""
    rng = np.random.default_rng(83)
    n = 1 << 21
    series, vals = _skewed(rng, n, tile=55)
    o = oracle.OracleHistograms(S)
    o.ingest(series, vals)
    with _engine([(N.PARAM_MAX_SLABS, 2), (N.PARAM_REGION_PCT, 40)]) as eng:
        r0 = eng.partition_redos()[0]
        eng.ingest(series, vals)
        _assert_equal(eng, o, True, "redo")
        assert eng.partition_redos()[0] > r0


def test_no_direct_tiles(oracle):
    """No direct tiles: super-tile bins only (nst = every run), no LDS sums."""
    rng = np.random.default_rng(89)
    n = 1 << 20
    series, vals = _skewed(rng, n, tile=9)
    _check_one_ingest(oracle, series, vals, [(N.PARAM_MAX_SLABS, 1), (N.PARAM_DIRECT_MAX, 0)], "no direct tiles")


def test_invalid_ids_in_every_subchunk(oracle):
    """1 % of the ids are >= S, so the trash bin has records in every sub-chunk: they are
    dropped and reported (-EINVAL at the next sync, once), the rest is exact."""
    rng = np.random.default_rng(97)
    n = 1 << 20
    series, vals = _skewed(rng, n, tile=120)
    bad = rng.random(n) < 0.01
    series[bad] = rng.choice(np.array([S, S + 1, 1 << 20, 0xFFFFFFFF], np.uint32), size=int(bad.sum()))
    per_chunk = np.add.reduceat(bad.astype(np.int64), np.arange(0, n, CHW))
    assert per_chunk.min() > 0
    o = oracle.OracleHistograms(S)
    o.ingest(series[~bad], vals[~bad])
    with _engine([(N.PARAM_MAX_SLABS, 1)]) as eng:
        eng.ingest(series, vals)
        with pytest.raises(N.L5dhError, match="EINVAL"):
            eng.sync()
        eng.sync()  # reported once
        _assert_equal(eng, o, True, "invalid ids dropped")


def test_two_ingests_before_one_snapshot(oracle):
    """Two ingests (two segments) of one slab each, a non-resetting snapshot, a third ingest
    and a resetting snapshot."""
    rng = np.random.default_rng(103)
    n = 1 << 19
    o = oracle.OracleHistograms(S)
    with _engine([(N.PARAM_MAX_SLABS, 1), (N.PARAM_MAX_SEGMENTS, 2)]) as eng:
        for tile in (5, 99):
            b = _skewed(rng, n, tile)
            eng.ingest(*b)
            o.ingest(*b)
        _assert_equal(eng, o, False, "two segments")
        b = _skewed(rng, n + 13, 127)
        eng.ingest(*b)
        o.ingest(*b)
        _assert_equal(eng, o, True, "third ingest")
