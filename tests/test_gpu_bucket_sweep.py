"""Every bucket edge through each device decoder, bit for bit against the CPU oracle.

The bucket of a sample is decided by five pieces of device code, by the route the sample takes:

  D1  lut2_decode in level 1's record build        samples of direct tiles, payload in [0, V_ESC)
  D2  lut3_byte / lut3_bucket, lean form (k_rbin2)  whole level-2 items, first pass, no escape in the wave
  D3  lut3_bucket, careful form (k_rbin2)           ragged item ends, waves with an escape, the redo pass
  D4  count_batch -> lut2_decode in k_fold1         a series space of one tile, vector and scalar loads
  D5  payload1_slow -> bucketize -> bucket_lut /    payloads outside [0, V_ESC)
      search_key / java_f2l

Each case steers tests/bucket_sweep.py's value set (every key below 2^21 + 2048, every limit from
both sides, the far ends of float -> long -> int) down one of these routes, compares the dense
count rows and every summary field with the oracle fed the same arrays, then ingests the same batch
again without a reset and compares again (sums exact at twice the load, nothing added twice by a
redo pass).  The samples lie on the 32 series of one tile as a comb -- sample k on series
tile * 32 + k mod 32 -- so the counts are small and one sample in a wrong bucket shows.

Which route a sample took cannot be observed from Python; each case asserts of its input what the
kernels' rules need to take the route it is about.
"""
import functools

import numpy as np
import pytest

from linkerd_amd import _native as N
from tests import bucket_sweep as BS
from tests.test_gpu_parity import REGIME_PARAMS

pytestmark = pytest.mark.gpu

S_TILES = 4096  # 128 tiles, two super-tiles
TILE = 77       # the hot tile (super-tile 1)
NBG = 1 << 13   # background samples on the other tiles


# ---------------------------------------------------------------- batches and their references
@functools.lru_cache(maxsize=None)
def _batch(name):
    """(S, series, values), built once and read-only."""
    sw = BS.sweep()
    if name in ("tile_in_range", "tile_mixed"):
        v = sw.subset(name[5:])
        S = S_TILES
        series, vals = BS.with_background(BS.tile_series(v.size, TILE), v, S, TILE, NBG, seed=7)
    elif name == "spread_in_range":
        S = S_TILES
        v = sw.in_range
        n = v.size
        while any(c % BS.ITEM2 == 0 for c in _spread_super_tiles(n)):
            n += 1  # (a few of the first values once more)
        vals = v[np.arange(n) % v.size]
        series = BS.spread_series(n, S)
    elif name.startswith("mod"):  # mod<S>_r<n mod 4>: the mixed set over a one-tile series space
        S, r = int(name[3:5]), int(name[-1])
        v = sw.mixed
        n = v.size + (r - v.size) % 4
        vals = v[np.arange(n) % v.size]
        series = BS.spread_series(n, S)
    elif name == "slow_only":
        S, n = 70, 1 << 18
        vals = sw.escaped[np.arange(n) % sw.escaped.size]
        series = BS.spread_series(n, S)
    else:
        raise KeyError(name)
    series = np.ascontiguousarray(series, np.uint32)
    vals = np.ascontiguousarray(vals, np.float32)
    for a in (series, vals):
        a.setflags(write=False)
    return S, series, vals


def _spread_super_tiles(n):
    """Records per 2048-series super-tile of spread_series(n, 4096)."""
    c0 = n // 4096 * 2048 + min(n % 4096, 2048)
    return c0, n - c0


_REF = {}


def _reference(oracle, name):
    """The oracle after one and after two ingests of the batch: [(counts, summaries)] * 2, shared
    by the cases that use the batch and left unchanged."""
    if name not in _REF:
        S, series, vals = _batch(name)
        o = oracle.OracleHistograms(S)
        out = []
        for _ in range(2):
            o.ingest(series, vals)
            out.append((o.counts(), o.snapshot(reset=False)))
        _REF[name] = out
    return _REF[name]


def _engine(S, regimes=(), params=()):
    from linkerd_amd.engine import HistogramEngine
    e = HistogramEngine(S)
    e.set_param(N.PARAM_STAGE_SAMPLES, 0)  # every ingest binned at once
    for r in regimes:
        for k, v in REGIME_PARAMS[r].items():
            e.set_param(k, v)
    for k, v in params:
        e.set_param(k, v)
    return e


# ---------------------------------------------------------------- comparison
def _compare(case, eng, ref, name):
    """Dense counts, then count / sum / min / max / the six percentiles / avg, all bitwise.  A
    mismatch names the case, the series, the bucket and the batch's values that belong there."""
    S, series, vals = _batch(name)
    want_counts, want = ref
    got, counts = eng.snapshot(reset=False, with_counts=True)
    bad = counts != want_counts
    if bad.any():
        # the first cell that lost a sample (else the first that gained one) and the values that belong there
        lost = counts < want_counts
        s, b = (int(x) for x in np.argwhere(lost if lost.any() else bad)[0])
        mine = series == s
        here = vals[mine][BS.expected_bucket(vals[mine]) == b]
        cells = ", ".join(f"bucket {int(c)}: got {int(counts[s, c])} want {int(want_counts[s, c])}"
                          for c in np.flatnonzero(bad[s])[:4])
        L = BS.limits()
        lo = int(L[b - 1]) if b > 0 else None
        hi = int(L[b]) if b < L.size else None
        raise AssertionError(
            f"{case}: {int(bad.sum())} count cells differ; series {s} bucket {b} [{lo}, {hi}): "
            f"got {int(counts[s, b])} want {int(want_counts[s, b])}; "
            + (f"the batch's values of this series that map there run from {here.min()!r} to {here.max()!r}"
               if here.size else "no value of the batch maps there")
            + f"; this series' differing cells: {cells}")
    for f in N.SUMMARY_FIELDS:
        g, w = got[f], want[f]
        same = (g == w) | (np.isnan(g) & np.isnan(w)) if f == "avg" else g == w
        if not same.all():
            s = int(np.flatnonzero(~same)[0])
            raise AssertionError(f"{case}: field {f}: {int((~same).sum())} series differ; first: series {s}: "
                                 f"got {g[s]!r} want {w[s]!r}")
    return got


def _ingest_twice(oracle, case, name, regimes=(), params=(), feed=None, expect_redo=False):
    """Ingest, compare, ingest the same batch again without a reset, compare."""
    S, series, vals = _batch(name)
    ref = _reference(oracle, name)
    s_in, v_in = feed(series, vals) if feed else (series, vals)
    with _engine(S, regimes, params) as eng:
        r0 = eng.partition_redos()[0]
        for k in range(2):
            eng.ingest(s_in, v_in)
            got = _compare(f"{case}, ingest {k + 1}", eng, ref[k], name)
            if expect_redo:
                assert eng.partition_redos()[0] > r0, f"{case}: level 1 was not redone"
                r0 = eng.partition_redos()[0]
        eng.sync()  # no invalid id was reported
    return got


# ---------------------------------------------------------------- input properties
def _assert_hot_tile_is_direct(series, S):
    """k_rplan1 makes a tile direct when its estimate -- its draws among the batch's 2^18 evenly
    spaced ones, scaled by n / 2^18 -- is at least thr = max(n // 8192, 2^k), 2^k the smallest
    power of two that keeps at most 255 such tiles.  Here the hot tile's estimate is above
    n // 8192 and every other tile's is below it: one candidate, so the power-of-two cut keeps it
    (k = 0), and it is the only direct tile."""
    est = BS.plan_sample_tiles(series, S)
    thr_min = max(1, series.size // 8192)
    assert est[TILE] >= thr_min, (int(est[TILE]), thr_min)
    others = np.delete(est, TILE)
    assert others.max() < thr_min, (int(others.max()), thr_min)


def _assert_no_escape(vals):
    assert not np.isnan(vals).any() and not np.signbit(vals).any() and (vals < np.float32(BS.V_ESC)).all()


def _super_tile_records(series):
    return np.bincount(series >> 11, minlength=S_TILES >> 11)


# ---------------------------------------------------------------- D1
@pytest.mark.parametrize("regime", ["default", "redo"])
@pytest.mark.parametrize("subset", ["in_range", "mixed"])
def test_d1_direct_tile(oracle, subset, regime):
    """D1: the sweep on one direct tile of S = 4096, over 2^13 uniform background samples.  Level 1
    decodes every payload below V_ESC of a direct tile itself (lut2_decode); with `mixed` the
    same sub-chunks also hold escaped samples (D5) and the payloads in [2^17, V_ESC) take the slow
    route's sumfix while their buckets still come from lut2_decode.  With regions at 40 % of
    the plan the pass is redone, and must add nothing to any sum.  The tile is direct by
    k_rplan1's rule: see _assert_hot_tile_is_direct."""
    name = f"tile_{subset}"
    S, series, vals = _batch(name)
    _assert_hot_tile_is_direct(series, S)
    assert (series >> 5 == TILE).sum() == BS.sweep().subset(subset).size and series.size - NBG == (series >> 5 == TILE).sum()
    if subset == "in_range":
        _assert_no_escape(vals)
    _ingest_twice(oracle, f"D1 {subset} {regime}", name, [regime], expect_redo=regime == "redo")


# ---------------------------------------------------------------- D2
def test_d2_level2_lean(oracle):
    """D2: no direct tiles, no escape anywhere: the hot tile's super-tile is hundreds of whole
    ITEM2-record items, and every item but the region's last takes k_rbin2's lean form."""
    name = "tile_in_range"
    S, series, vals = _batch(name)
    _assert_no_escape(vals)
    assert _super_tile_records(series)[TILE >> 6] > 10 * BS.ITEM2
    _ingest_twice(oracle, "D2 lean", name, ["nodirect"])


# ---------------------------------------------------------------- D3
def test_d3_careful_escape_in_every_wave(oracle):
    """D3 by escapes: no direct tiles, and among any 64 consecutive samples of the hot tile's
    stream one that leaves an escaped record -- a wave holds at least 64 records, so none is lean."""
    name = "tile_mixed"
    S, series, vals = _batch(name)
    hot = series >> 5 == TILE
    t = BS.java_f2l(vals[hot])
    esc = ~((t >= 0) & (t < BS.V_ESC))
    gaps = np.diff(np.flatnonzero(np.concatenate([[True], esc, [True]])))
    assert gaps.max() < 64
    _ingest_twice(oracle, "D3 escapes", name, ["nodirect"])


def test_d3_careful_redo_pass(oracle):
    """D3 by the redo pass: no direct tiles, regions at 40 % of the plan; the second pass of
    k_rbin2 decodes in the careful form and adds nothing to a sum."""
    name = "tile_in_range"
    _assert_no_escape(_batch(name)[2])
    _ingest_twice(oracle, "D3 redo", name, ["nodirect", "redo"], expect_redo=True)


def test_d3_careful_ragged_items(oracle):
    """D3 by ragged items: the in-range values spread over all 4096 series (series k mod 4096),
    no direct tiles (spread evenly, all 128 tiles would be direct and nothing would reach level
    2), and n such that neither super-tile holds a multiple of ITEM2 records: each region ends in
    a short item, decoded in the careful form, after its whole ones."""
    name = "spread_in_range"
    S, series, vals = _batch(name)
    _assert_no_escape(vals)
    per = _super_tile_records(series)
    assert (per % BS.ITEM2 != 0).all() and (per > BS.ITEM2).all()
    _ingest_twice(oracle, "D3 ragged", name, ["nodirect"])


# ---------------------------------------------------------------- D4
def _aligned(series, vals):
    import torch
    ds = torch.from_numpy(series.view(np.int32).copy()).cuda()
    dv = torch.from_numpy(vals.copy()).cuda()
    assert ds.data_ptr() % 16 == 0 and dv.data_ptr() % 16 == 0
    return ds, dv


def _offset_by_one(series, vals):
    import torch
    n = series.size
    ds = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
    dv = torch.zeros(n + 1, dtype=torch.float32, device="cuda")
    ds[1:].copy_(torch.from_numpy(series.view(np.int32).copy()))
    dv[1:].copy_(torch.from_numpy(vals.copy()))
    assert ds[1:].data_ptr() % 16 == 4 and dv[1:].data_ptr() % 16 == 4
    return ds[1:], dv[1:]


@pytest.mark.parametrize("load", ["vector", "vector_tail", "scalar"])
@pytest.mark.parametrize("S,variant", [(16, 0), (32, 0), (16, 1)], ids=["S16-u32", "S32-u16", "S16-u16"])
def test_d4_one_tile_fold(oracle, S, variant, load):
    """D4: a series space of one tile is folded at ingest by k_fold1 -- u32 bins up to 16 series,
    u16 bins for 32 series and, with variant bit 0, for 16 too -- whose count_batch decodes with
    lut2_decode.  The mixed set from device memory: 16-byte aligned with n a multiple of 4 (the
    vector loop), aligned with n mod 4 = 3 (its ragged tail), and one element past a 16-byte
    boundary (the scalar loop)."""
    name = f"mod{S}_r{3 if load == 'vector_tail' else 0}"
    n = _batch(name)[1].size
    assert n % 4 == (3 if load == "vector_tail" else 0)
    feed = _offset_by_one if load == "scalar" else _aligned
    _ingest_twice(oracle, f"D4 S={S} variant={variant} {load}", name, params=[(N.PARAM_VARIANT, variant)], feed=feed)


# ---------------------------------------------------------------- D5
@pytest.mark.parametrize("regime", ["default", "redo", "nodirect"])
def test_d5_slow_route_alone(oracle, regime):
    """D5: only values outside [0, V_ESC) -- the limits' neighbourhoods from V_ESC up, negatives,
    NaN, +-Inf, beyond 2^31 and 2^63 -- cycled to 2^18 samples over S = 70 (no tile multiple).
    Every sample goes through payload1_slow: bucketize's three branches, bucket_lut's limit
    compares, search_key for the keys that wrap negative.  No id is reported invalid, and the
    sums equal the contributions added in numpy (a long's wrap-around), negative ones and
    Int.MaxValue among them."""
    name = "slow_only"
    S, series, vals = _batch(name)
    fast = (vals >= 0) & (vals < np.float32(BS.V_ESC))
    assert (~fast | ((vals == 0) & np.signbit(vals))).all()  # (-0.0 alone passes level 1's range test)
    c = BS.expected_contribution(vals)
    assert (c < 0).any() and (c == BS.INT_MAX).any()
    got = _ingest_twice(oracle, f"D5 {regime}", name, [regime])
    total = np.zeros(S, np.uint64)
    np.add.at(total, series, c.astype(np.uint64))
    np.testing.assert_array_equal(got["sum"], (total * np.uint64(2)).view(np.int64))
    np.testing.assert_array_equal(got["count"], 2 * np.bincount(series, minlength=S))
