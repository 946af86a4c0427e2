"""The counter space on the GPU (l5dh_counters_*): k_cnt_add under both variants (the LDS claim
table and, L5DH_PARAM_VARIANT bit 3, one global atomic per add), the range calls and
k_cnt_rollup, against numpy on the CPU: np.add.at into an int64 array, which wraps as a Java
long does.
"""
import errno

import numpy as np
import pytest

from linkerd_amd import _native as N

pytestmark = pytest.mark.gpu

VARIANTS = [0, N.VARIANT_COUNTERS_PLAIN]
C = 8192  # slots of a workgroup's claim table; an id's home slot is id mod C, with 4 probes
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


@pytest.fixture(scope="module")
def engine(gpu_available):
    from linkerd_amd.engine import HistogramEngine
    with HistogramEngine(1024) as e:
        yield e


@pytest.fixture
def space(engine):
    """open(capacity, variant) -> a CounterEngine of the shared engine, closed after the test."""
    from linkerd_amd.counters import CounterEngine
    made = []

    def open_(capacity, variant=0):
        engine.set_param(N.PARAM_VARIANT, variant)
        ce = CounterEngine(engine, capacity)
        made.append(ce)
        return ce
    yield open_
    for ce in made:
        ce.close()
    engine.set_param(N.PARAM_VARIANT, 0)


def truth(capacity, batches):
    want = np.zeros(capacity, np.int64)
    for ids, deltas in batches:
        ok = ids < capacity
        np.add.at(want, ids[ok], 1 if deltas is None else deltas[ok].astype(np.int64))
    return want


def on_device(a, offset):
    """``a`` in device memory, ``offset`` elements (4 bytes each) past a 16-byte boundary."""
    import torch
    t = torch.zeros(a.size + 4, dtype=torch.int32, device="cuda")
    assert t.data_ptr() % 16 == 0
    v = t[offset:offset + a.size]
    v.copy_(torch.from_numpy(a.view(np.int32)))
    return v


@pytest.mark.parametrize("variant", VARIANTS)
def test_lengths_and_alignment(space, variant):
    cap = 1000
    ce = space(cap, variant)
    rng = np.random.default_rng(11)
    want = np.zeros(cap, np.int64)
    adds = 0
    for n in (0, 1, 2, 3, 4, 5, 63, 64, 65, 255, 257, 4 * 1024 * 3 + 1):
        for offset in (0, 1, 2, 3):  # 0, 4, 8 and 12 bytes
            for with_deltas in (False, True):
                ids = rng.integers(0, cap, n).astype(np.uint32)
                deltas = rng.integers(-1000, 1000, n).astype(np.int32) if with_deltas else None
                # ids and deltas at different offsets: the vector path of one, the element path of the other
                d_off = (offset + 1) % 4 if n % 2 else offset
                ce.add(on_device(ids, offset), None if deltas is None else on_device(deltas, d_off))
                if offset == 0:
                    ce.add(ids, deltas)  # host memory
                    want += truth(cap, [(ids, deltas)])
                    adds += n
                want += truth(cap, [(ids, deltas)])
                adds += n
        np.testing.assert_array_equal(ce.values(), want, err_msg=f"n={n}")
    info = ce.info()
    assert info["adds"] == adds and info["dropped"] == 0 and info["lds_adds"] + info["global_adds"] == adds
    assert (info["lds_adds"] == 0) == (variant != 0)


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("slabs", [1, 2, 512])
def test_slabs_and_workgroups(gpu_available, variant, slabs):
    """n = 3 * 2^18 + 5: with 1 or 2 workgroups each takes several slabs of 2^18 (and the last
    one a short one); with 512 there are fewer slabs than workgroups."""
    from linkerd_amd.counters import CounterEngine
    from linkerd_amd.engine import HistogramEngine
    n, cap = 3 * (1 << 18) + 5, 50_021
    rng = np.random.default_rng(slabs)
    ids = rng.integers(0, cap, n).astype(np.uint32)
    deltas = rng.integers(I32_MIN, I32_MAX, n, endpoint=True).astype(np.int32)
    with HistogramEngine(64) as e:
        e.set_param(N.PARAM_MAX_SLABS, slabs)
        e.set_param(N.PARAM_VARIANT, variant)
        ce = CounterEngine(e, cap)
        ce.add(on_device(ids, 0), on_device(deltas, 0))
        np.testing.assert_array_equal(ce.values(), truth(cap, [(ids, deltas)]))
        assert ce.info()["adds"] == n


@pytest.mark.parametrize("variant", VARIANTS)
def test_one_address(space, variant):
    cap, n = 70_001, 1 << 18
    ce = space(cap, variant)
    for cid in (0, cap - 1):
        before = ce.info()
        ce.add(np.full(n, cid, np.uint32))
        assert ce.get(cid) == n
        after = ce.info()
        if variant == 0:
            # the table took them: at most one global add per workgroup (64 slabs of 4096 here)
            assert after["global_adds"] - before["global_adds"] <= 64
            assert after["lds_adds"] - before["lds_adds"] >= n - 64
        else:
            assert after["global_adds"] - before["global_adds"] == n
    want = np.zeros(cap, np.int64)
    want[[0, cap - 1]] = n
    np.testing.assert_array_equal(ce.values(), want)


def test_table_overflow(gpu_available):
    from linkerd_amd.counters import CounterEngine
    from linkerd_amd.engine import HistogramEngine
    with HistogramEngine(64) as e:
        e.set_param(N.PARAM_MAX_SLABS, 1)  # one workgroup, one table: a batch below 2^18 adds is one slab
        _table_overflow(CounterEngine(e, 8 * C), 8 * C)


def _table_overflow(ce, cap):
    # one home slot, probe depth 4: four of the eight ids get slots, the others go to global memory
    ids = np.tile(np.arange(8, dtype=np.uint32) * C, 500)
    deltas = np.arange(ids.size, dtype=np.int32) - 1234
    ce.add(ids, deltas)
    a = ce.info()
    assert a["lds_adds"] > 0 and a["global_adds"] > 0 and a["lds_adds"] + a["global_adds"] == a["adds"] == ids.size
    # 3 C distinct ids once each in one slab: the table holds at most C of them
    once = np.arange(3 * C, dtype=np.uint32)
    ce.add(once)
    b = ce.info()
    assert b["lds_adds"] - a["lds_adds"] > 0 and b["global_adds"] - a["global_adds"] >= 2 * C
    assert b["lds_adds"] + b["global_adds"] == b["adds"] == ids.size + once.size
    np.testing.assert_array_equal(ce.values(), truth(cap, [(ids, deltas), (once, None)]))


@pytest.mark.parametrize("variant", VARIANTS)
def test_arithmetic_wraps_like_a_java_long(space, variant):
    ce = space(8, variant)
    ce.add(np.array([0, 1, 2, 0, 1, 2], np.uint32), np.array([I32_MIN, I32_MAX, -1, I32_MIN, I32_MAX, -1], np.int32))
    np.testing.assert_array_equal(ce.values()[:3], [2 * I32_MIN, 2 * I32_MAX, -2])
    ce.write(3, np.array([I64_MAX, I64_MIN], np.int64))
    ce.add(np.array([3, 4], np.uint32), np.array([1, -1], np.int32))
    assert ce.get(3) == I64_MIN and ce.get(4) == I64_MAX
    ce.add(np.array([3], np.uint32))  # deltas null: 1
    assert ce.get(3) == I64_MIN + 1


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("cap", [1, 33, 100_003])
def test_invalid_ids_are_dropped_counted_and_reported_once(space, engine, variant, cap):
    ce = space(cap, variant)
    rng = np.random.default_rng(cap)
    ids = rng.integers(0, cap, 5000).astype(np.uint32)
    bad = rng.choice(ids.size, 300, replace=False)
    ids[bad] = rng.choice(np.array([cap, cap + 1, 0xFFFFFFFF], np.uint32), bad.size)
    deltas = rng.integers(-5, 6, ids.size).astype(np.int32)
    ce.add(ids, deltas)
    ce.add(on_device(ids, 1), None)
    np.testing.assert_array_equal(ce.values(), truth(cap, [(ids, deltas), (ids, None)]))
    info = ce.info()
    assert info["dropped"] == 2 * bad.size and info["adds"] == 2 * (ids.size - bad.size)
    with pytest.raises(N.L5dhError, match="counter") as ei:
        engine.sync()
    assert ei.value.code == -errno.EINVAL
    engine.sync()  # (reported once)


@pytest.mark.parametrize("variant", VARIANTS)
def test_skewed_and_uniform_load(space, variant):
    from linkerd_amd import synth
    cap, n = 100_003, 1 << 20
    ce = space(cap, variant)
    rng = np.random.default_rng(5)
    cdf = synth.zipf_cdf(100_000)
    batches = []
    for k in range(3):
        zipf = np.minimum(np.searchsorted(cdf, rng.random(n), side="right"), 99_999).astype(np.uint32)
        unif = rng.integers(0, cap, n).astype(np.uint32)
        deltas = rng.integers(-1000, 1000, n).astype(np.int32) if k else None
        batches += [(zipf, deltas), (unif, None)]
        ce.add(on_device(zipf, 0), None if deltas is None else on_device(deltas, 0))
        ce.add(unif)
    np.testing.assert_array_equal(ce.values(), truth(cap, batches))
    info = ce.info()
    assert info["adds"] == 6 * n
    if variant == 0:
        assert info["lds_adds"] > info["global_adds"]  # (the Zipf head and most else stay in LDS)


# ---- range calls ------------------------------------------------------------------------------
def test_read_write_edges(space):
    cap = 257
    ce = space(cap)
    vals = np.arange(cap, dtype=np.int64) * 1_000_000_007 - 5
    ce.write(0, vals)
    np.testing.assert_array_equal(ce.values(), vals)
    for first, count in ((0, 0), (0, 1), (1, 1), (cap - 1, 1), (cap, 0), (0, cap), (100, 57)):
        np.testing.assert_array_equal(ce.read(first, count), vals[first:first + count])
    ce.write(cap - 1, np.array([7], np.int64))
    ce.write(0, np.array([-7], np.int64))
    ce.write(5, None, count=10)  # a null write clears
    ce.write(cap, None, count=0)
    vals[cap - 1], vals[0], vals[5:15] = 7, -7, 0
    np.testing.assert_array_equal(ce.values(), vals)
    import torch
    ce.write(20, torch.arange(3, dtype=torch.int64, device="cuda"))  # device values
    vals[20:23] = [0, 1, 2]
    np.testing.assert_array_equal(ce.values(), vals)


def _rc(engine, name, *args):
    return getattr(engine._lib, name)(engine._ctx, *args)


def test_failing_calls_change_nothing(space, engine):
    cap = 100
    ce = space(cap)
    vals = np.arange(cap, dtype=np.int64) - 50
    ce.write(0, vals)
    out = np.zeros(cap + 1, np.int64)
    group = np.zeros(cap + 1, np.uint32)
    E = -errno.EINVAL
    assert _rc(engine, "l5dh_counters_open", 10) == -errno.EEXIST
    assert _rc(engine, "l5dh_counters_read", 1, cap, out.ctypes.data) == E
    assert _rc(engine, "l5dh_counters_read", 0xFFFFFFFF, 2, out.ctypes.data) == E
    assert _rc(engine, "l5dh_counters_write", cap, 1, out.ctypes.data) == E
    assert _rc(engine, "l5dh_counters_write", 50, cap, None) == E
    assert _rc(engine, "l5dh_counters_resize", cap - 1) == E  # grow only
    assert _rc(engine, "l5dh_counters_resize", N.MAX_COUNTERS + 1) == E
    assert _rc(engine, "l5dh_counters_add", group.ctypes.data, None, (1 << 30) + 1) == E
    assert _rc(engine, "l5dh_counters_rollup", 0, cap + 1, group.ctypes.data, 1, out.ctypes.data) == E
    assert _rc(engine, "l5dh_counters_rollup", 0, cap, group.ctypes.data, 0, out.ctypes.data) == E
    assert _rc(engine, "l5dh_counters_rollup", 0, cap, group.ctypes.data, N.MAX_COUNTERS + 1, out.ctypes.data) == E
    assert engine._lib.l5dh_counters_read(None, 0, 1, out.ctypes.data) == E
    np.testing.assert_array_equal(ce.values(), vals)
    assert ce.info()["max_counters"] == cap


def test_calls_without_counters_are_refused(gpu_available):
    from linkerd_amd.engine import HistogramEngine
    out = np.zeros(4, np.int64)
    with HistogramEngine(64) as e:
        E = -errno.EINVAL
        assert _rc(e, "l5dh_counters_close") == E
        assert _rc(e, "l5dh_counters_add", out.ctypes.data, None, 1) == E
        assert _rc(e, "l5dh_counters_read", 0, 1, out.ctypes.data) == E
        assert _rc(e, "l5dh_counters_info", None, None, None, None, None) == E
        assert _rc(e, "l5dh_counters_open", 0) == E and _rc(e, "l5dh_counters_open", N.MAX_COUNTERS + 1) == E
        assert b"counters" in e._lib.l5dh_last_error(e._ctx)
        e.sync()


def test_resize_keeps_values_and_zeroes_the_new(space):
    ce = space(33)
    vals = np.arange(33, dtype=np.int64) * -3
    ce.write(0, vals)
    ce.incr(32, 5)  # (staged: grow flushes it)
    ce.grow(100_003)
    vals[32] += 5
    np.testing.assert_array_equal(ce.values(), np.concatenate([vals, np.zeros(100_003 - 33, np.int64)]))
    ce.add(np.array([100_002, 33], np.uint32))
    assert ce.get(100_002) == 1 and ce.get(33) == 1 and ce.info()["max_counters"] == 100_003
    with pytest.raises(ValueError):
        ce.grow(100)


def test_move_hands_the_space_over(gpu_available):
    from linkerd_amd.counters import CounterEngine
    from linkerd_amd.engine import HistogramEngine
    with HistogramEngine(64) as a, HistogramEngine(128) as b:
        ce = CounterEngine(a, 1000)
        ids = np.arange(1000, dtype=np.uint32)
        ce.add(ids, (ids.astype(np.int32) - 500))
        ce.incr(7, 100)  # staged
        ce.move_to(b)
        assert ce.engine is b
        assert _rc(a, "l5dh_counters_info", None, None, None, None, None) == -errno.EINVAL  # the old context has none
        want = ids.astype(np.int64) - 500
        want[7] += 100
        np.testing.assert_array_equal(ce.values(), want)
        other = CounterEngine(a, 10)
        with pytest.raises(N.L5dhError) as ei:
            other.move_to(b)  # the target has counters
        assert ei.value.code == -errno.EEXIST
        np.testing.assert_array_equal(ce.values(), want)


def test_device_values_is_the_live_array(space):
    ce = space(500)
    ce.incr(3, -9)
    t = ce.device_values()
    assert t.is_cuda and str(t.dtype) == "torch.int64" and t.numel() == 500
    ce.engine.sync()  # (the view is ordered on the engine's stream, torch reads on its own)
    assert int(t[3]) == -9
    ce.incr(3, 10)
    assert ce.device_values().data_ptr() == t.data_ptr()
    ce.engine.sync()
    assert int(t[3]) == 1  # a view: nothing was copied


# ---- rollup -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ngroups", [1, 7, 8192, 8193, 100_000])
def test_rollup(space, ngroups):
    cap = 150_001
    ce = space(cap)
    rng = np.random.default_rng(ngroups)
    vals = rng.integers(I64_MIN, I64_MAX, cap, endpoint=True)  # sums that wrap
    ce.write(0, vals)
    group = rng.integers(0, ngroups, cap).astype(np.uint32)
    group[rng.choice(cap, cap // 10, replace=False)] = N.NO_GROUP
    if ngroups > 1:
        group[group == ngroups - 1] = N.NO_GROUP  # an empty group
    for first, count in ((0, cap), (17, cap - 1000), (cap - 1, 1), (5, 0)):
        g = group[first:first + count]
        want = np.zeros(ngroups, np.int64)
        member = g != N.NO_GROUP
        np.add.at(want, g[member], vals[first:first + count][member])
        got = ce.rollup(g, ngroups, first, count)
        np.testing.assert_array_equal(got, want)
        if ngroups > 1:
            assert got[ngroups - 1] == 0
    # the map in device memory, at a 4-byte offset
    got = ce.rollup(on_device(group, 1), ngroups)
    want = np.zeros(ngroups, np.int64)
    np.add.at(want, group[group != N.NO_GROUP], vals[group != N.NO_GROUP])
    np.testing.assert_array_equal(got, want)


@pytest.mark.parametrize("ngroups", [7, 8193])
def test_rollup_invalid_entry_names_the_least_index(space, ngroups):
    cap = 20_000
    ce = space(cap)
    vals = np.arange(cap, dtype=np.int64)
    ce.write(0, vals)
    group = (np.arange(cap) % ngroups).astype(np.uint32)
    group[[4321, 15_000, 19_999]] = [ngroups, ngroups + 5, 0xFFFFFFFE]
    with pytest.raises(N.L5dhError, match=r"group\[4321\]") as ei:
        ce.rollup(group, ngroups)
    assert ei.value.code == -errno.EINVAL
    np.testing.assert_array_equal(ce.values(), vals)  # nothing changed
